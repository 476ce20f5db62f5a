"""Planted worst-case rounding pairs for the fp16 matrix-core filters (K8 filter_f16.hip, the float32 route of radius.hip, K14
wide_f32.hip), their host-side checks and a NumPy model of the filter decision.  Nothing here touches the GPU.

Every float32 answer rests on "scores off by at most E, margin M >= 2 E": M = eps (|c|^2 + max |m|^2) with eps = 1.1 * 2^-10
(K8, radius) or 1.25 * 2^-10 (K14), c the output row and m the streamed rows.  Random data realises a small part of E, because
its rounding errors have random signs.  The rows below make every rounding error of a pair point the same way.

Notation: u = 2^-11 (fp16's unit roundoff), delta = 2^-9, g = +-2^e with e in 0 .. -9 (scaled into [2^13, 2^14) the smallest is
2^4, and 2^-4 beside a decoy of 2^8: never an fp16 subnormal).  g (1 + u (1 - delta)) lies just under the midpoint of two fp16
values and rounds DOWN to g, g (1 + u (1 + delta)) just above it and rounds UP to g (1 + 2 u).

Competitor form (top-K filters).  q = [a ; b] with a_k = g_k (1 + u (1 - delta)), b_k = g'_k (1 + u (1 + delta)); t1 = [a ; 0] is
the true nearest row, t2 = [0 ; b] the competitor.  D(q, t1) = |b|^2 and D(q, t2) = |a|^2; g' starts as g and single values of
it are halved (largest amount that still fits first) until |b|^2 <= |a|^2 (1 - 1.02 * 2^-13), so the oracle's float32 chain
separates the two rows.  Both operands of q.t1 lose u, both of q.t2 gain u: s16(t2) - s16(t1) ~ 2^-10 |q|^2 (1 - delta) minus
the exact gap, against the exact order.  With |t|^2 = |q|^2 / 2 that is 1 / 1.65 = 0.606 of K8's M and 0.533 of K14's at best.
Top-2: the issue's second competitor t3 needs a second D gap of 2^-13, which costs another 0.017 M and leaves K14 at 0.49 M, under
one half, where a one-sided margin is no longer seen.  So the top-2 families put the planted pair in SECOND place instead: a row
t0 = 0.6875 q (|t0|^2 < |t1|^2, D = 0.098 |q|^2) is every filter's best row, the exact top-2 is (t0, t1), the second-best bound
is s16(t2) and a filter that loses t1 returns (t0, t2).  Same inversion as top-1, one gap.  Up to 128 values two families carry
the issue's t3 as well (PLACES_T3; 0.56 of K8's M): the exact top-2 is (t1, t2), a filter that loses t1 returns (t2, t3).

Threshold form (float32 radiusMatch).  q_k = g_k (1 + u (1 - delta)), t_k = g_k (1 + u (1 - 2 delta)): both round down to g, the
exact D = u^2 delta^2 sum g^2 is tiny and A16 = |q|^2 + |t|^2 - 2 q16.t16 exceeds it by ~ 2^-10 (|q|^2 + |t|^2): 0.9 M.  The radius
is the float32 after the pair's exact distance.  The mirror pair rounds UP (1 + u (1 + delta)) / (1 + u (1 + 2 delta)), with one
coordinate of 2^-3 at 3 delta: its exact distance is 0.1 % larger, above the radius, and it must be absent.  (The issue writes t =
q (1 + u (1 - delta)) with q under a midpoint as well; such a t lies past the midpoint and rounds up.  This is the same idea with
both rows under it.)  Pairs of one data set share the magnitudes and differ in signs, so one scalar radius serves them all.

Background rows are N(0, sigma^2) with |row|^2 ~ 0.4 |t1|^2, clipped into the planted rows' binade: no row exceeds a planted row's
norm (max |m|^2 stays the planted rows' own) and every one is far beyond 4 M from every planted q.  Families differ in their
random signs, so another family's rows are background to a q as well.  check_competitor / check_threshold assert all of it,
the exact order through the oracle's order-1 chain, and the emulated inversion / excess against the floors.

The fp16 plane is emulated as bank_prep_f16_kernel builds it: times the bank's power of two (largest magnitude into
[2^13, 2^14)), astype(float16), norms of the unrounded rows in float64; s16 = c16.m16 - |m|^2 / 2 in float64, with 2^-16 |q||t|
taken off an inversion for the matrix core's float32 accumulation."""
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle           # noqa: E402

U = 2.0 ** -11
DELTA = 2.0 ** -9
GAP = 2.0 ** -13
EPS_K8 = 1.1 * 2.0 ** -10
EPS_K14 = 1.25 * 2.0 ** -10
FLOOR_K8, FLOOR_K14, FLOOR_RADIUS = 0.55, 0.50, 0.85
T0_SCALE = 0.6875
MIN_EXP = -9


def _exps(n):
    """The exponents of n planted values: 0 .. -3 in turn, the last twelve -4 .. -7 (small values to balance with)."""
    e = -(np.arange(n) % 4)
    e[-12:] = [-4, -4, -4, -4, -5, -5, -5, -5, -6, -6, -7, -7]
    return e


def _sq(a):
    a = np.asarray(a, np.float64)
    return (a * a).sum(-1)


# ---- constructions ---------------------------------------------------------------------------------------------------------
def competitor(dim, rng):
    """(q, t1, t2, t0, t3) float32 [dim] of one family with its own random signs."""
    na = dim // 2
    nb = dim - na                                            # the longer half is the one that is cut down
    ea, eb = _exps(na), _exps(nb).copy()
    a = (np.ldexp(1.0, ea) * (1.0 + U * (1.0 - DELTA))).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), np.ldexp(1.0, ea) * (1.0 + U * (1.0 - DELTA)))       # exact in float32
    up = 1.0 + U * (1.0 + DELTA)
    target = _sq(a) * (1.0 - 1.02 * GAP)
    while True:
        R = _sq(np.ldexp(up, eb)) - target
        if R <= 0:
            break
        amount = np.where(eb > MIN_EXP, 0.75 * np.ldexp(up, eb) ** 2, np.inf)       # what halving value k takes off |b|^2
        fits = np.where(amount <= R, amount, -np.inf)
        k = int(np.argmax(fits)) if np.isfinite(fits.max()) else int(np.argmin(amount))
        assert np.isfinite(amount[k])
        eb[k] -= 1
    b = np.ldexp(up, eb).astype(np.float32)
    assert np.array_equal(b.astype(np.float64), np.ldexp(up, eb))
    sa, sb = rng.choice([-1.0, 1.0], na).astype(np.float32), rng.choice([-1.0, 1.0], nb).astype(np.float32)
    a, b = a * sa, b * sb
    zero_a, zero_b = np.zeros(na, np.float32), np.zeros(nb, np.float32)
    q = np.concatenate([a, b])
    t1, t2 = np.concatenate([a, zero_b]), np.concatenate([zero_a, b])
    t0 = (np.float32(T0_SCALE) * q).astype(np.float32)
    # t3: t2 with a few small values halved, (b_k / 2)^2 each farther from q: of the 16 smallest values the subset whose sum
    # is the least one that reaches 1.02 * 2^-13 |a|^2
    mag = np.abs(b).astype(np.float64)
    small = np.argsort(mag, kind="stable")[:16]
    small = small[eb[small] > MIN_EXP]
    pick = (np.arange(1 << len(small))[:, None] >> np.arange(len(small))[None, :]) & 1
    sums = pick @ (0.25 * mag[small] ** 2)
    best = int(np.argmin(np.where(sums >= 1.02 * GAP * _sq(a), sums, np.inf)))
    half = np.ones(nb)
    half[small[pick[best] == 1]] = 0.5
    t3 = np.concatenate([zero_a, (b * half).astype(np.float32)])
    return q, t1, t2, t0, t3


def threshold_pair(dim, rng):
    """(q, t, q', t') float32 [dim]: the hit that rounds down and the mirror pair that rounds up, under one set of signs."""
    g = np.ldexp(1.0, _exps(dim))
    s = rng.choice([-1.0, 1.0], dim)
    j = int(np.nonzero(_exps(dim) == -3)[0][0])
    e2 = np.full(dim, 2.0)
    e2[j] = 3.0
    rows = [g * (1.0 + U * (1.0 - DELTA)), g * (1.0 + U * (1.0 - 2.0 * DELTA)),
            g * (1.0 + U * (1.0 + DELTA)), g * (1.0 + U * (1.0 + e2 * DELTA))]
    out = []
    for r in rows:
        f = (s * r).astype(np.float32)
        assert np.array_equal(f.astype(np.float64), s * r)
        out.append(f)
    return tuple(out)


def background(n, dim, rng, t1_norm, part=0.4):
    """n rows of N(0, sigma^2), |row|^2 ~ part * t1_norm, clipped into [-1.9, 1.9] (the planted rows' largest values lie in
    [1, 2): the bank's power of two is the planted rows')."""
    sigma = np.sqrt(part * t1_norm / dim)
    return np.clip(rng.standard_normal((n, dim)) * sigma, -1.9, 1.9).astype(np.float32)


class Planted(object):
    """Two row sets and the places of their planted rows.  fams: dicts q, t1, t2, t0 (None: a top-1 family) -- or q, t, kind
    ("hit" / "mirror") for the threshold form."""

    def __init__(self, Q, T, fams):
        self.Q, self.T, self.fams = Q, T, fams
        Q.setflags(write=False)
        T.setflags(write=False)


def competitor_set(dim, nq, nt, places, seed, q_decoy=None, t_decoy=None, doubled=False):
    """places: (q row, t1 row, t2 row, t0 row or None) per family.  doubled: self_competitor's rows (below), whose margin is
    two thirds max |m|^2 -- the form that feels a stale maximum.  q_decoy (row, magnitude): a query row of +-1.25 *
    magnitude -- the output side's own norm alone feels it.  t_decoy (row, value): a train row with ONE value, whose norm
    stays under the planted rows' (checked)."""
    rng = np.random.default_rng(seed)
    if doubled:
        rows = [self_competitor(dim, rng) for _ in places]
        # (t0 = 1.25 q here, still under the planted rows' 2 |q|^2: its own ratio over the query rows stays well under q's 0.25)
        rows = [r + ((np.float32(1.25) * r[0]).astype(np.float32),) for r in rows]
    else:
        rows = [competitor(dim, rng) for _ in places]
    t1n = min(_sq(r[1]) for r in rows)
    # (the query background has 0.9 |q|^2: the output side's norms are no part of a planted q's margin, and with the banks
    # exchanged the planted t rows are query rows whose own ratios d(t, q) / d(t, background) must pass the ratio test -- t1's --
    # and stay under q's d(q, t0) / d(q, t1) -- t0's, which a symmetric mutual ratio test then reports)
    Q = background(nq, dim, rng, min(_sq(r[0]) for r in rows), 0.9)
    T = background(nt, dim, rng, t1n / 4.0) * np.float32(2.0) if doubled else background(nt, dim, rng, t1n)
    fams = []
    for place, row in zip(places, rows):
        rq, r1, r2, r0 = place[:4]
        r3 = place[4] if len(place) > 4 else None
        Q[rq], T[r1], T[r2] = row[0], row[1], row[2]
        if r0 is not None:
            T[r0] = row[3]
        if r3 is not None:
            T[r3] = row[4]
        fams.append({"q": rq, "t1": r1, "t2": r2, "t0": r0, "t3": r3})
    if q_decoy is not None:
        Q[q_decoy[0]] = 1.25 * q_decoy[1] * rng.choice([-1.0, 1.0], dim)
    if t_decoy is not None:
        T[t_decoy[0]] = 0.0
        T[t_decoy[0], 0] = t_decoy[1]
    used = [f[k] for f in fams for k in ("t1", "t2", "t0", "t3") if f[k] is not None]
    assert len(set(used)) == len(used) and len(set(f["q"] for f in fams)) == len(fams)
    return Planted(Q, T, fams)


def threshold_set(dim, nq, nt, places, seed):
    """places: (q row, t row, "hit" or "mirror")."""
    rng = np.random.default_rng(seed)
    Q = T = None
    fams = []
    for rq, rt, kind in places:
        q, t, qm, tm = threshold_pair(dim, rng)
        if Q is None:
            Q, T = background(nq, dim, rng, _sq(t)), background(nt, dim, rng, _sq(t))
        Q[rq], T[rt] = (q, t) if kind == "hit" else (qm, tm)
        fams.append({"q": rq, "t": rt, "kind": kind})
    return Planted(Q, T, fams)


# ---- the fp16 planes and the filter's decision -------------------------------------------------------------------------------
def kscale(X):
    """The bank's power of two: its largest magnitude times 2^k lies in [2^13, 2^14)."""
    vmax = float(np.abs(X).max())
    return 14 - int(np.frexp(vmax)[1]) if vmax > 0 else 0


def plane(X, k=None):
    """(the fp16 image of the rows, back in the rows' own units, float64; |row|^2 of the unrounded rows, float64)."""
    k = kscale(X) if k is None else k
    scaled = np.ldexp(np.asarray(X, np.float64), k)
    assert np.abs(scaled).max() < 65504.0
    return np.ldexp(scaled.astype(np.float16).astype(np.float64), -k), _sq(X)


def scores(c16, M16, mnorm):
    """s16 of every streamed row against one output row: c16.m16 - |m|^2 / 2."""
    return M16 @ c16 - 0.5 * mnorm


def margin(eps, cnorm, mnorm_max):
    return eps * (cnorm + mnorm_max)


def kept(s16_row, bound, M, f=1.0):
    """The filter's decision: a row is examined iff its score reaches the K-th best score minus f * M."""
    return s16_row >= bound - f * M


def within(A16, r2, M, f=1.0):
    """The radius sweep's decision: a row is a candidate iff A16 <= r^2 + f * M."""
    return A16 <= r2 + f * M


def competitor_report(p, eps, c_bank="Q"):
    """Per family: dict with M, the K-th best score (bound), s16 of t1 and t2, the inversion (s16(t2) - s16(t1) - 2^-16 |q||t1|)
    and `fraction` = inversion / M.  c_bank "Q": the query rows are the output rows (the forward sweep); the planes are the
    two banks' own."""
    Q16, qn = plane(p.Q)
    T16, tn = plane(p.T)
    out = []
    for f in p.fams:
        s = scores(Q16[f["q"]], T16, tn)
        M = margin(eps, qn[f["q"]], tn.max())
        ktop = 1 if f["t0"] is None and f.get("t3") is None else 2
        bound = np.sort(s)[-ktop]
        rival = f["t2"] if f.get("t3") is None else f["t3"]                  # the row whose score is the K-th best
        inv = s[rival] - s[f["t1"]] - 2.0 ** -16 * np.sqrt(qn[f["q"]] * tn[f["t1"]])
        out.append({"M": M, "bound": bound, "s1": s[f["t1"]], "s2": s[rival], "scores": s, "inversion": inv, "fraction": inv / M})
    return out


def check_competitor(p, eps, floor):
    """The conditions of the module docstring, for a competitor set; returns the fractions of M reached."""
    k = 3 if any(f["t0"] is not None or f.get("t3") is not None for f in p.fams) else 2
    rows = np.array([f["q"] for f in p.fams])
    idx, dist = oracle.bf_knn(np.ascontiguousarray(p.Q[rows]), np.ascontiguousarray(p.T), k, order=1)
    tn, qn = _sq(p.T), _sq(p.Q)
    D = qn[rows][:, None] + tn[None, :] - 2.0 * p.Q[rows].astype(np.float64) @ p.T.astype(np.float64).T
    rep = competitor_report(p, eps)
    fr = []
    for i, (f, r) in enumerate(zip(p.fams, rep)):
        want = [f["t1"], f["t2"]] if f["t0"] is None else [f["t0"], f["t1"], f["t2"]]
        if f.get("t3") is not None:
            want = want + [f["t3"]]
        assert idx[i, :len(want)].tolist() == want, (f, idx[i])
        assert (np.diff(dist[i, :len(want)].astype(np.float64)) > 0).all(), (f, dist[i])              # the chain separates them
        d1, d2 = D[i, f["t1"]], D[i, f["t2"]]
        assert (d2 - d1) / d1 >= GAP, (f, (d2 - d1) / d1)
        if f.get("t3") is not None:
            assert (D[i, f["t3"]] - d2) / d2 >= GAP and tn[f["t3"]] < tn[f["t2"]], f
            d2 = D[i, f["t3"]]
        planted = np.zeros(len(p.T), bool)
        planted[want] = True
        top = max(tn[f["t1"]], tn[f["t2"]])
        assert tn[~planted].max() <= top, f                                               # max |m|^2 is a planted row's own
        if f["t0"] is not None:
            assert tn[f["t0"]] < top
        assert (D[i, ~planted] > d2 + 8.0 * r["M"]).all(), f                              # (D = |q|^2 - 2 s: 8 M in D is 4 M in s)
        assert (r["scores"][~planted] < r["s1"] - 4.0 * r["M"]).all(), f
        assert r["bound"] == r["s2"], f                                                   # the K-th best score is the competitor's
        assert r["fraction"] >= floor, (f, r["fraction"])
        fr.append(r["fraction"])
    return fr


def threshold_report(p, eps):
    """Per family: M, r^2 (r = the float32 after the hit's exact distance; the mirror's own for a mirror), A16 and `fraction` =
    (A16 - r^2 - 2^-15 |q||t|) / M."""
    Q16, qn = plane(p.Q)
    T16, tn = plane(p.T)
    out = []
    for f in p.fams:
        q, t = f["q"], f["t"]
        _, d = oracle.bf_knn(np.ascontiguousarray(p.Q[q:q + 1]), np.ascontiguousarray(p.T[t:t + 1]), 1, order=1)
        r = np.nextafter(d[0, 0], np.float32(np.inf))
        A16 = qn[q] + tn[t] - 2.0 * float(Q16[q] @ T16[t])
        M = margin(eps, qn[q], tn.max())
        exc = A16 - float(r) ** 2 - 2.0 ** -15 * np.sqrt(qn[q] * tn[t])
        out.append({"M": M, "r": r, "dist": d[0, 0], "A16": A16, "fraction": exc / M})
    return out


def check_threshold(p, eps=EPS_K8, floor=FLOOR_RADIUS):
    """The conditions for a threshold set.  Returns (the scalar radius, the hits' fractions of M)."""
    rep = threshold_report(p, eps)
    hits = [r for f, r in zip(p.fams, rep) if f["kind"] == "hit"]
    mirrors = [r for f, r in zip(p.fams, rep) if f["kind"] == "mirror"]
    r = hits[0]["r"]
    assert all(h["r"] == r and h["dist"] < r for h in hits)                # one distance, bit for bit, under the radius
    assert all(m["dist"] >= r for m in mirrors)                            # the mirror is no hit
    tn, qn = _sq(p.T), _sq(p.Q)
    planted_t = np.zeros(len(p.T), bool)
    planted_t[[f["t"] for f in p.fams]] = True
    hit_norm = min(tn[f["t"]] for f in p.fams if f["kind"] == "hit")
    assert tn[~planted_t].max() < hit_norm
    for f, h in zip(p.fams, rep):
        if f["kind"] != "hit":
            continue
        assert tn.max() <= tn[f["t"]] * (1.0 + 2.0 ** -9), f               # (the mirror rows are 2^-10 larger: M grows by 2^-11)
        d = qn[f["q"]] + tn - 2.0 * p.T.astype(np.float64) @ p.Q[f["q"]].astype(np.float64)
        d[[g["t"] for g in p.fams if g["q"] == f["q"]]] = np.inf
        assert (d > float(r) ** 2 + 8.0 * h["M"]).all(), f                 # every other row is far beyond the threshold
        assert h["fraction"] >= floor, (f, h["fraction"])
    return r, [h["fraction"] for h in hits]


# ---- self distances: the output row is a row of the streamed bank -------------------------------------------------------------
def self_competitor(dim, rng):
    """(c, m1, m2) for fm_self_dist.  In a self sweep max |m|^2 >= |c|^2, which leaves the split form above at 0.45 M.  Doubling
    the streamed rows wins it back: c = [a ; b], m1 = [2 a ; 0], m2 = [0 ; 2 b] keep every rounding direction (2 g is a power of
    two), c.m doubles, and M = eps (|c|^2 + 4 |b|^2) = 3 eps |c|^2: 2 / 3.3 = 0.606 again.  D(c, m1) = D(c, m2) = |c|^2 as they
    stand; a few small values of m1 stay at a_k, which takes a_k^2 each off D(c, m1), 1.02 * 2^-13 |c|^2 in all."""
    na = dim // 2
    nb = dim - na
    ea, eb = _exps(na), _exps(nb)
    a = np.ldexp(1.0 + U * (1.0 - DELTA), ea)
    b = np.ldexp(1.0 + U * (1.0 + DELTA), eb)
    R = 1.02 * GAP * (_sq(a) + _sq(b))
    lam = np.full(na, 2.0)
    for k in np.argsort(-a, kind="stable"):
        if a[k] * a[k] <= R:
            lam[k] = 1.0
            R -= a[k] * a[k]
    if R > 0:
        lam[int(np.argmin(np.where(lam == 2.0, a, np.inf)))] = 1.0
    sa, sb = rng.choice([-1.0, 1.0], na), rng.choice([-1.0, 1.0], nb)
    c = np.concatenate([a * sa, b * sb]).astype(np.float32)
    m1 = np.concatenate([lam * a * sa, np.zeros(nb)]).astype(np.float32)
    m2 = np.concatenate([np.zeros(na), 2.0 * b * sb]).astype(np.float32)
    return c, m1, m2


def self_set(dim, n, places, seed):
    """places: (c row, m1 row, m2 row) per family, all in ONE bank.  The background's values stay in the planted rows' binade
    [2, 4) and its norms under theirs."""
    rng = np.random.default_rng(seed)
    rows = [self_competitor(dim, rng) for _ in places]
    X = 2.0 * background(n, dim, rng, min(_sq(r[1]) for r in rows) / 4.0)
    fams = []
    for (rc, r1, r2), (c, m1, m2) in zip(places, rows):
        X[rc], X[r1], X[r2] = c, m1, m2
        fams.append({"q": rc, "t1": r1, "t2": r2, "t0": None, "t3": None})
    return Planted(X, X, fams)


def check_self(p, eps=EPS_K8, floor=FLOOR_K8):
    """check_competitor's conditions inside one bank: the row itself is no candidate."""
    X = p.Q
    rows = np.array([f["q"] for f in p.fams])
    idx, dist = oracle.bf_knn(np.ascontiguousarray(X[rows]), np.ascontiguousarray(X), 3, order=1)
    X16, xn = plane(X)
    fr = []
    for i, f in enumerate(p.fams):
        assert idx[i].tolist() == [f["q"], f["t1"], f["t2"]] and dist[i, 0] == 0 and dist[i, 1] < dist[i, 2], (f, idx[i], dist[i])
        s = scores(X16[f["q"]], X16, xn)
        D = xn[f["q"]] + xn - 2.0 * X.astype(np.float64) @ X[f["q"]].astype(np.float64)
        M = margin(eps, xn[f["q"]], xn.max())
        other = np.ones(len(X), bool)
        other[[f["q"], f["t1"], f["t2"]]] = False
        assert (D[f["t2"]] - D[f["t1"]]) / D[f["t1"]] >= GAP
        assert xn[other].max() <= max(xn[f["t1"]], xn[f["t2"]])
        assert (D[other] > D[f["t2"]] + 8.0 * M).all() and (s[other] < s[f["t1"]] - 4.0 * M).all(), f
        s_others = np.where(np.arange(len(X)) == f["q"], -np.inf, s)
        assert s_others.max() == s[f["t2"]]
        inv = s[f["t2"]] - s[f["t1"]] - 2.0 ** -16 * np.sqrt(xn[f["q"]] * xn[f["t1"]])
        assert inv / M >= floor, (f, inv / M)
        fr.append({"M": M, "bound": s[f["t2"]], "s1": s[f["t1"]], "fraction": inv / M})
    return fr


# ---- the data sets of the two test files (computed once, read-only) ------------------------------------------------------------
NQ, NT = 300, 1100          # query rows: an output chunk of 256 rows and 44 more; train rows: 8 stages of 128 and a partial one
# (q row, t1 row, t2 row, t0 row or None).  The q rows lie on the first and last row of an output chunk, on the first row of
# the next and on the last real row, on four waves (64 rows each); t1 comes before t2 in stream order (it sits in a lane's
# entries when the competitor raises the bound: rescore_kernel's thr) or after it (the stream test against a raised bound),
# in one 128-row stage or in two, which "f32_nsplit" 3 and 7 put into different splits.
# t0 lies in t2's group of 4 rows: K14's bound is the best KTOP-th best of the four lanes that share an output row, and a lane
# sees 4 rows of every 16-row tile, so only a lane that has met t0 AND t2 has s16(t2) for its second best.
PLACES = [(0, 5, 77, None), (255, 100, 20, None), (256, 130, 900, None), (299, 1099, 3, None),
          (70, 300, 301, 303), (133, 640, 511, 509), (200, 1024, 1023, 1021), (17, 700, 200, 202)]
# The issue's form for top-2, at up to 128 values (0.56 of K8's M; K14 would be at 0.49): (q row, t1 row, t2 row, None, t3 row)
# with a second competitor t3 behind t2.  The exact top-2 is (t1, t2), the second-best bound is s16(t3), and a filter that loses
# t1 returns (t2, t3): the one way fm_knn's k = 1 -- the first column of the top-2 sweep -- can show a lost row.
PLACES_T3 = [(40, 820, 350, None, 60), (230, 150, 760, None, 980)]
DECOYS = {None: {}, "q3": {"q_decoy": (150, 8.0)}, "q8": {"q_decoy": (150, 256.0)}, "q9": {"q_decoy": (150, 512.0)},
          "t": {"t_decoy": (600, None)}}
# (c row, m1 row, m2 row) in a self bank of 600 rows (n_pad 640: the smallest size with a piece off the diagonal) and of 1100:
# everything inside the first 512-row chunk (the masked block on the diagonal); c in the chunk and m1, m2 in a later stage (c
# is an output row of the piece: the row direction); c in a later stage and m1, m2 in the chunk (c is a streamed row there:
# the column direction, tri_rescore_kernel)
SELF_PLACES = {600: [(100, 200, 300), (10, 520, 599), (590, 30, 500)],
               1100: [(100, 300, 200), (10, 520, 1099), (1090, 30, 500), (600, 700, 1000), (1023, 640, 513)]}
# (q row, t row, kind): the hits on all four waves of a workgroup, on both workgroups, on the first and last lane of a block,
# in the first and last 64-row stage (the last one partial: 1088 .. 1099), on both sides of a stage boundary
RADIUS_PLACES = [(0, 3, "hit"), (15, 64, "hit"), (16, 127, "hit"), (63, 500, "hit"), (64, 1023, "hit"), (130, 1024, "hit"),
                 (255, 1090, "hit"), (256, 63, "hit"), (299, 1099, "hit"), (100, 700, "mirror"), (201, 1095, "mirror"),
                 (298, 1, "mirror")]


@functools.lru_cache(maxsize=None)
def pair_set(dim, decoy=None, shift=0):
    """The competitor set of a width.  decoy: a key of DECOYS -- "q3" / "q8" / "q9": a query row of magnitude 2^3 / 2^8 / 2^9
    (the output side's power of two drops by 3 / 8 / 9), "t": one train row with a single value of 4.0625 (2.25 under 128
    values), which raises the train side's power of two by 2 (1) and stays under the planted rows' norm."""
    kw = dict(DECOYS[decoy])
    if decoy == "t":
        kw["t_decoy"] = (600, 4.0625 if dim >= 128 else 2.25)
    return competitor_set(dim, NQ, NT, PLACES + (PLACES_T3 if dim <= 128 else []), 4100 + dim, **kw)


@functools.lru_cache(maxsize=None)
def doubled_set(dim):
    """The competitor set in self_competitor's form (t1 = [2 a ; 0], t2 = [0 ; 2 b]): M = eps (|q|^2 + 2 |q|^2), so a margin made
    from a smaller max |m|^2 -- a maximum left over from before an append or an add, one image's own -- loses t1."""
    return competitor_set(dim, NQ, NT, PLACES, 4400 + dim, doubled=True)


def small_rows(n, dim, seed, scale=1.0):
    """n rows of small norm whose largest values still lie in the doubled set's binade [2, 4): 3 values of +-(2 .. 2.5) per row
    (|row|^2 <= 18.75 against the planted rows' 80 at 128 values); `scale` moves them to another binade."""
    rng = np.random.default_rng(seed)
    X = np.zeros((n, dim), np.float32)
    # (where the planted rows' values are 2^-2 and less: q.row stays small and the row far from every q)
    allowed = np.nonzero(np.concatenate([_exps(dim // 2), _exps(dim - dim // 2)]) <= -2)[0]
    for i in range(n):
        k = rng.choice(allowed, 3, replace=False)
        X[i, k] = rng.uniform(2.0, 2.5, 3) * rng.choice([-1.0, 1.0], 3)
    return (X * np.float32(scale)).astype(np.float32)


def stacked(p, rows_in_front):
    """The set with `rows_in_front` stacked in front of its train rows (a bank that grew, the images of a collection)."""
    n = len(rows_in_front)
    T = np.concatenate([rows_in_front, p.T]).astype(np.float32)
    fams = [{k: (v + n if k != "q" and v is not None else v) for k, v in f.items()} for f in p.fams]
    return Planted(np.array(p.Q), T, fams)


def swapped(p):
    """The train rows as the query bank: the planted q is then an output row of the REVERSE sweep."""
    return Planted(np.array(p.T), np.array(p.Q), [])


@functools.lru_cache(maxsize=None)
def radius_set(dim=128):
    return threshold_set(dim, NQ, NT, RADIUS_PLACES, 4300 + dim)


@functools.lru_cache(maxsize=None)
def self_bank(n, dim=128):
    return self_set(dim, n, SELF_PLACES[n], 4200 + n)
