"""CPU: the planted worst-case rounding pairs of tests/f16_margin_ref.py are what they claim to be, and the NumPy model of the
filter decision ("kept iff s16 >= bound - f M") keeps the true neighbour at f = 1 and loses it at f = 0.5, family by family.
So a one-sided margin (E where 2 E is needed) is inside what tests/test_f16_margin_gpu.py sees.  The floors are conditions
on the inputs: 0.55 M (K8), 0.50 M (K14), 0.85 M (radius)."""
import numpy as np
import pytest

import f16_margin_ref as R

K8_SETS = [(128, None), (61, None), (128, "q3"), (128, "t"), (61, "t")]
K14_SETS = [(129, None), (160, None), (256, None), (160, "q8"), (160, "q9"), (160, "t")]


def _model(rep):
    for r in rep:
        assert R.kept(r["s1"], r["bound"], r["M"], 1.0), r["fraction"]
        assert not R.kept(r["s1"], r["bound"], r["M"], 0.5), r["fraction"]


@pytest.mark.parametrize("dim,decoy", K8_SETS)
def test_k8_competitor_sets(dim, decoy):
    p = R.pair_set(dim, decoy)
    fr = R.check_competitor(p, R.EPS_K8, R.FLOOR_K8)
    assert len(fr) == len(R.PLACES) + len(R.PLACES_T3) and min(fr) >= 0.55
    _model(R.competitor_report(p, R.EPS_K8))
    dk = R.kscale(p.Q) - R.kscale(p.T)
    assert dk == {None: 0, "q3": -3, "t": 2 if dim >= 128 else 1}[decoy]      # the output side's power of two minus the streamed side's


@pytest.mark.parametrize("dim,decoy", K14_SETS)
def test_k14_competitor_sets(dim, decoy):
    p = R.pair_set(dim, decoy)
    fr = R.check_competitor(p, R.EPS_K14, R.FLOOR_K14)
    assert min(fr) >= 0.50
    _model(R.competitor_report(p, R.EPS_K14))
    assert R.kscale(p.Q) - R.kscale(p.T) == {None: 0, "q8": -8, "q9": -9, "t": 2}[decoy]


@pytest.mark.parametrize("dim", [128, 160])
def test_sets_with_rows_stacked_in_front(dim):
    """A grown bank and a collection put small-norm rows in front of the planted ones: nothing about the pin changes."""
    p = R.stacked(R.doubled_set(dim), R.small_rows(224, dim, 1))
    assert R.kscale(p.Q) - R.kscale(p.T) == 1
    eps, floor = (R.EPS_K8, R.FLOOR_K8) if dim <= 128 else (R.EPS_K14, R.FLOOR_K14)
    R.check_competitor(p, eps, floor)
    _model(R.competitor_report(p, eps))
    # with the small rows' own maximum in the margin's place the planted row is lost: what a stale or per-image maximum does
    small_max = R._sq(R.small_rows(224, dim, 1)).max()
    for r, f in zip(R.competitor_report(p, eps), p.fams):
        stale = R.margin(eps, R._sq(p.Q[f["q"]]), small_max)
        assert stale < r["M"] and not R.kept(r["s1"], r["bound"], stale)


@pytest.mark.parametrize("n", sorted(R.SELF_PLACES))
def test_self_bank(n):
    rep = R.check_self(R.self_bank(n))
    assert len(rep) == len(R.SELF_PLACES[n])
    _model(rep)


def test_radius_set():
    p = R.radius_set()
    r, fr = R.check_threshold(p)
    assert min(fr) >= 0.85 and sum(f["kind"] == "hit" for f in p.fams) == len(fr) == 9
    for f, h in zip(p.fams, R.threshold_report(p, R.EPS_K8)):
        if f["kind"] == "hit":
            r2 = float(r) ** 2
            assert R.within(h["A16"], r2, h["M"], 1.0) and not R.within(h["A16"], r2, h["M"], 0.5)


def test_the_shared_support_form_stays_under_one_half():
    """q_k = g_k, t1 = q (1 + u (1 - delta)), t2 = q (1 + u (1 + delta)): 0.45 M at best, no pin for a one-sided margin -- the
    reason for the split form."""
    g = np.ldexp(1.0, R._exps(128))
    q = g.astype(np.float32)
    t1 = (g * (1.0 + R.U * (1.0 - R.DELTA))).astype(np.float32)
    t2 = (g * (1.0 + R.U * (1.0 + R.DELTA))).astype(np.float32)
    Q16, qn = R.plane(q[None])
    T16, tn = R.plane(np.stack([t1, t2]))
    s = R.scores(Q16[0], T16, tn)
    assert 0.40 < (s[1] - s[0]) / R.margin(R.EPS_K8, qn[0], tn.max()) < 0.5
