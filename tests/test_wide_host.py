"""Wide float banks (FM_BANK_F32W), everything that needs no GPU: header and binding, the refusals of matchutil / torchmatch
before anything is uploaded, the reference's own composition, the clustered data set's margin census."""
import os
import re
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil, torchmatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                   # noqa: E402
import wide_ref as ref          # noqa: E402


def _header_text():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


def test_header_and_binding():
    hdr = _header_text()
    assert int(re.search(r"#define\s+FM_BANK_F32W\s+(\d+)", hdr).group(1)) == 4 and _ffi.FM_BANK_F32W == 4
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    comment = " ".join(hdr.split("#define FM_ABI_VERSION")[0].split()).replace(" * ", " ")
    assert "still revision 12, additions only -- FM_BANK_F32W" in comment
    sect = hdr.split("---- K14: wide float banks")[1].split("int  fm_bank_destroy")[0]
    flat = " ".join(sect.replace("\n *", " ").split())
    for phrase in ("129 <= dim <= 256", "s = fmaf(v_k, v_k, s)", "bit-identical", "v_mfma_f32_16x16x32_f16", '"f32_filter"',
                   "fm_f32_filter_stats", "FM_EINVAL, even when one of them is empty", '"wide"'):
        assert phrase in flat, phrase
    not_built = flat.split("Not built for wide float banks:")[1]
    for name in ("k >= 3", "fm_radius_match(_dev)", "fm_self_dist(_batch)", "fm_bank_set_selfdist", "fm_match_accepted*",
                 "fm_xcheck1_keys*", "fm_xcheck1_batched", "fm_knn_masked(_dev)", "fm_bank_refill_u8_async", "fm_bank_append_*",
                 "fm_expand_create", "fm_collection_*"):
        assert name in not_built, name


class _NoContext(object):
    handle = None

    def __init__(self):
        self._children = set()


def _wide_bank(n=4, dim=256):
    return _ffi.Bank(_NoContext(), None, n, dim, _ffi.FM_BANK_F32W)


def test_matchutil_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    monkeypatch.setattr(_ffi, "default_context", no_device)
    q = np.zeros((4, 256), np.float32)
    t = np.zeros((5, 256), np.float32)
    for a, b in ((q, t), (_wide_bank(4), _wide_bank(5)), (q.astype(np.float64)[:, :129], t[:, :129])):
        with pytest.raises(ValueError, match="wide"):
            matchutil.bf_radius_match(a, b, 1.0)
        with pytest.raises(ValueError, match="wide"):
            matchutil.bf_radius_match_arrays(a, b, np.ones(4, np.float32))
        with pytest.raises(ValueError, match="wide"):
            matchutil.bf_match(a, b, k=3)
        with pytest.raises(ValueError, match="wide"):
            matchutil.flann_match_arrays(a, b, k=8)
        with pytest.raises(ValueError, match="wide"):
            matchutil.bf_match(a, b, k=2, options={"mask": np.ones((4, 5), np.uint8)})
    m = matchutil.BFMatcher()
    with pytest.raises(ValueError, match="wide"):
        m.add([np.zeros((3, 128), np.float32), q])
    assert m.empty()
    # what is served reaches the device: these get as far as the context
    for call in (lambda: matchutil.bf_match(q, t, k=2), lambda: matchutil.bf_match(q, t, k=1, options={"crossCheck": True}),
                 lambda: matchutil.ratio_match_arrays(q, t, 0.8), lambda: matchutil.mutual_ratio_match_arrays(q, t, 0.8, True)):
        with pytest.raises(AssertionError, match="touched the device"):
            call()
    # uint8 rows wider than 128 are not wide float descriptors: they go on to the library, which refuses them
    with pytest.raises(AssertionError, match="touched the device"):
        matchutil.bf_radius_match(np.zeros((4, 200), np.uint8), np.zeros((4, 200), np.uint8), 1.0)


def test_torchmatch_refusals_come_before_the_library(monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the library")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(torchmatch, "_ctx_for", no_device)
    qb, tb = _wide_bank(4), _wide_bank(5)
    with pytest.raises(ValueError, match="wide"):
        torchmatch.radius_match(qb, tb, 1.0)
    with pytest.raises(ValueError, match="wide"):
        torchmatch.knn(qb, tb, 2, mask=torch.ones((4, 5), dtype=torch.bool))
    with pytest.raises(ValueError, match="wide"):
        torchmatch.knn(qb, tb, 3)
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        x = torch.zeros((4, 256), dtype=dt)
        with pytest.raises(ValueError, match="wide"):
            torchmatch.radius_match(x, x, 1.0)
        coll = torchmatch.Collection()
        with pytest.raises(ValueError, match="wide"):
            coll.add(x)
        with pytest.raises(ValueError, match="wide"):
            coll.knn(x, 2)
        with pytest.raises(ValueError, match="wide"):
            coll.ratio_match(qb, 0.8)
        assert coll._coll is None
    # uint8 rows are not wide float descriptors: the usual refusal of a host tensor
    with pytest.raises(ValueError, match="CUDA tensor"):
        torchmatch.Collection().add(torch.zeros((4, 200), dtype=torch.uint8))


def test_reference_composition_equals_the_oracle():
    Q, T = ref.clustered(300, 257, 161, seed=5)
    idx, dist = ref.knn(Q, T, 2)
    # the oracle's chain, restated: s = fmaf(v, v, s) over k ascending is float32(float64(s) + float64(v) * float64(v)) -- the
    # float64 product of two float32 values and its sum with a float32 are rounded once
    for i in (0, 17, 299):
        s = np.zeros(len(T), np.float32)
        for k in range(161):
            v = (Q[i, k] - T[:, k]).astype(np.float32)
            s = (s.astype(np.float64) + v.astype(np.float64) * v.astype(np.float64)).astype(np.float32)
        d = np.sqrt(s)
        order = np.lexsort((np.arange(len(T)), d))[:2]
        assert np.array_equal(idx[i], order) and np.array_equal(dist[i].view(np.uint32), d[order].view(np.uint32))
    o_idx, o_dist = oracle.bf_knn(Q, T, 2, order=1)
    assert np.array_equal(idx, o_idx) and np.array_equal(dist.view(np.uint32), o_dist.view(np.uint32))
    # k = 1 is the first column; crossCheck is the mutual 1-NN of the two directions
    i1, d1 = ref.knn(Q, T, 1)
    assert np.array_equal(i1[:, 0], idx[:, 0]) and np.array_equal(d1[:, 0], dist[:, 0])
    x_idx, x_dist = ref.xcheck1(Q, T)
    r1, rd = ref.knn(T, Q, 1)
    elected = np.full(len(Q), -1, np.int32)
    e_dist = np.full(len(Q), np.inf, np.float32)
    for t in range(len(T)):                       # every train row elects its nearest query row; a query row keeps the closest
        q = r1[t, 0]                              # electing train row, the lowest index on ties
        if rd[t, 0] < e_dist[q]:
            elected[q], e_dist[q] = t, rd[t, 0]
    assert np.array_equal(x_idx, elected) and np.array_equal(x_dist.view(np.uint32), e_dist.view(np.uint32))
    # the ratio match at tau = +inf keeps every row with a second neighbour; the mutual form is a subset of it, and of crossCheck
    q_all, t_all, d_all, r_all = ref.ratio_match(Q, T, np.inf)
    assert np.array_equal(q_all, np.arange(300)) and np.array_equal(t_all, idx[:, 0]) and np.array_equal(d_all, dist[:, 0])
    assert np.array_equal(r_all, dist[:, 0].astype(np.float64) / dist[:, 1].astype(np.float64))
    for sym in (False, True):
        mq, mt, md, mr = ref.mutual_ratio(Q, T, 0.8, sym)
        fq, ft, fd, fr = ref.ratio_match(Q, T, 0.8)
        assert len(mq) > 0 and set(mq) <= set(fq)
        assert np.array_equal(mt, x_idx[mq]) and np.array_equal(md.view(np.uint32), x_dist[mq].view(np.uint32))
        assert (mr < 0.8).all() and (mr >= fr[np.searchsorted(fq, mq)]).all()


@pytest.mark.parametrize("shape", [(300, 257), (1000, 4099), (4099, 1000)])
@pytest.mark.parametrize("dim", [129, 160, 256])
def test_clustered_set_stays_inside_the_margin(shape, dim):
    """What the GPU test's "no whole-call fallback" assertion relies on: few train rows sit within the filter's margin of a
    query row's second neighbour, so the record list of a working filter stays far below its capacity."""
    for seed in (7, 8):
        Q, T = ref.clustered(shape[0], shape[1], dim, seed)
        c = ref.margin_census(Q, T)
        print("clustered", shape, dim, seed, "max", int(c.max()), "share above 2: %.3f" % (c > 2).mean())
        assert c.max() <= 6, (seed, int(c.max()))
