"""CPU: the host side of the mutual nearest-neighbour ratio match (fm_mutual_ratio, fm_collection_mutual_ratio_each and their
device forms) -- the NumPy reference (tests/mutual_ratio_ref.py) on hand-made cases, the four prototypes against the ctypes
binding, the ABI revision they leave alone, what the header still lists as not built, and the refusals of matchutil and
torchmatch, which touch no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil, torchmatch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutual_ratio_ref as ref        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fm_mutual_ratio", "fm_mutual_ratio_dev", "fm_collection_mutual_ratio_each", "fm_collection_mutual_ratio_each_dev")
INF = float("inf")


def _rows(*vals):
    a = np.zeros((len(vals), 128), np.uint8)
    a[:, 0] = vals
    return a


def _bits(*vals):
    """One-byte binary rows whose Hamming distances are |a - b| for values written in unary (a ones in the low bits)."""
    return np.array([(1 << v) - 1 for v in vals], np.uint8)[:, None]


def _q(res):
    return res[0].tolist(), res[1].tolist()


# ---- the reference on hand-made cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [False, True])
def test_two_queries_share_a_first_neighbour(binary):
    mk = _bits if binary else _rows
    T = mk(0, 8)                                   # (the second train row is far from everything: ratios are small)
    # q0 at 2 and q1 at 1 from train row 0: both pass the ratio test, only the nearer (q1) is mutual
    q, t, d, r = ref.mutual_ratio(mk(2, 1), T, 0.8, binary=binary)
    assert (q.tolist(), t.tolist(), d.tolist()) == ([1], [0], [1.0]) and r[0] == 1.0 / 7.0
    # at equal distance only the lower query index
    assert _q(ref.mutual_ratio(mk(1, 1), T, 0.8, binary=binary)) == ([0], [0])
    t0, d0, fwd, ok, mutual, rev = ref.classes(mk(2, 1), T, 0.8, binary)
    assert ok.tolist() == [True, True] and mutual.tolist() == [False, True]


@pytest.mark.parametrize("binary", [False, True])
def test_duplicates_one_row_banks_and_the_reverse_ratio(binary):
    mk = _bits if binary else _rows
    # duplicate train rows: d0 = d1 = 0 is 0 / 0 = NaN (rejected), d0 = d1 > 0 gives ratio 1: kept by tau = inf only
    assert _q(ref.mutual_ratio(mk(3), mk(3, 3), INF, binary=binary)) == ([], [])
    assert _q(ref.mutual_ratio(mk(4), mk(3, 3), 1.0, binary=binary)) == ([], [])
    assert _q(ref.mutual_ratio(mk(4), mk(3, 3), INF, binary=binary)) == ([0], [0])          # ... at the lower train row
    # nt == 1: no second neighbour, no ratio
    assert _q(ref.mutual_ratio(mk(1, 2), mk(1), INF, binary=binary)) == ([], [])
    # nq == 1: accepted without `symmetric`, never with it (the train row has no second query neighbour)
    assert _q(ref.mutual_ratio(mk(1), mk(0, 8), 0.8, binary=binary)) == ([0], [0])
    assert _q(ref.mutual_ratio(mk(1), mk(0, 8), INF, symmetric=True, binary=binary)) == ([], [])
    # forward passes (1 / 7), mutual, but the train row's second query neighbour is as close as the first but one: 1 / 2
    Q, T = mk(1, 2), mk(0, 8)
    assert _q(ref.mutual_ratio(Q, T, 0.4, binary=binary)) == ([0], [0])
    assert _q(ref.mutual_ratio(Q, T, 0.4, symmetric=True, binary=binary)) == ([], [])
    q, t, d, r = ref.mutual_ratio(Q, T, 0.6, symmetric=True, binary=binary)
    assert _q((q, t)) == ([0], [0]) and r[0] == 0.5                                        # the larger of 1 / 7 and 1 / 2
    # empty banks accept nothing
    assert _q(ref.mutual_ratio(mk(), mk(1, 2), INF, binary=binary)) == ([], [])
    assert _q(ref.mutual_ratio(mk(1, 2), mk(), INF, binary=binary)) == ([], [])


def test_structured_construction_has_every_class():
    for binary in (False, True):
        Q, T = ref.structured(1, binary)
        t0, d0, fwd, ok, mutual, rev = ref.classes(Q, T, 0.8, binary)
        acc = ok & mutual
        with np.errstate(invalid="ignore"):
            sym = acc & (rev < 0.8)
        assert min((ok & ~mutual).sum(), (mutual & ~ok).sum(), acc.sum(), (acc & ~sym).sum()) >= 10


# ---- header and binding -----------------------------------------------------------------------------------------------------
def _header_text():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


def _klass_of_text(p):
    p = " ".join(p.split())
    if "*" in p or "[" in p:
        return "ptr"
    for word, k in (("double", "f64"), ("float", "f32"), ("int64_t", "i64"), ("int32_t", "i32")):
        if re.search(r"\b%s\b" % word, p):
            return k
    raise AssertionError("unclassified parameter: " + p)


def _klass_of_ctype(t):
    if t is ctypes.c_void_p or hasattr(t, "contents"):
        return "ptr"
    return {ctypes.c_double: "f64", ctypes.c_float: "f32", ctypes.c_int64: "i64", ctypes.c_int32: "i32"}[t]


@pytest.mark.parametrize("name", NEW)
def test_new_prototypes_match_the_binding(name):
    hdr = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(fm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    assert name in protos, "the header does not declare %s" % name
    res, argtypes = _ffi.SYMBOLS[name]
    assert res is ctypes.c_int
    got = [_klass_of_text(p) for p in protos[name].split(",")]
    assert got == [_klass_of_ctype(t) for t in argtypes]
    # (ctx, [collection,] q, [t,] tau, symmetric, cap, ...): four arrays + count | d_rows, d_count(s), host count(s), stream
    want = ["ptr"] * 3 + ["f64", "i32", "i64"] + ["ptr"] * (4 if name.endswith("_dev") else 5)
    assert got == want
    assert hasattr(_ffi.load_library(), name)
    for method in ("mutual_ratio", "mutual_ratio_dev"):
        assert callable(getattr(_ffi.Context, method))
    for method in ("mutual_ratio_each", "mutual_ratio_votes", "mutual_ratio_each_dev"):
        assert callable(getattr(_ffi.Collection, method))


def test_abi_revision_is_still_12():
    hdr = _header_text()
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    comment = " ".join(hdr.split("#define FM_ABI_VERSION")[0].split()).replace(" * ", " ")
    for name in NEW:
        assert name in comment
    assert "still revision 12, additions only -- fm_mutual_ratio, fm_mutual_ratio_dev" in comment
    assert "still revision 12, additions only -- fm_collection_xcheck1_each, fm_collection_xcheck1_each_dev" in comment


def test_header_phrases():
    hdr = _header_text()
    sect = hdr.split("---- train collections")[1].split("typedef struct fm_collection")[0]
    not_built = " ".join(sect.split("Not built:")[1].replace("\n *", " ").split())
    assert "mutual nearest neighbours combined with the per-image ratio test" not in not_built
    for still in ("the STACKED crossCheck on a collection", "the per-image form is built: fm_collection_xcheck1_each",
                  "a single reverse K8 sweep over a float32-route stack", "Hamming radiusMatch (for pairs or collections)",
                  "an _each form", "skipping the second count sweep", "expansion loop on a collection", "per-image sweep",
                  "binary collections in the self-distance test", "sharding a collection across GPUs"):
        assert still in not_built, still
    # the option's description keeps its sentences and states the bytes per candidate of the gathered bank
    opt = " ".join(hdr.split('"coll_ws_bytes" 0..2^31-1')[1].split("Unknown names")[0].replace("\n *", " ").split())
    assert "25 bytes per entry" in opt and "17 in the cross-check" in opt
    assert "fm_collection_mutual_ratio_each" in opt and "132 bytes per candidate" in opt and "776" in opt and "80 per 16 bytes" in opt
    # the device form says how often it waits for the host
    flat = " ".join(hdr.replace("\n *", " ").split())
    assert "fm_mutual_ratio_dev" in flat and "ONE on every route, the 8-byte candidate count" in flat


# ---- refusals that touch no device --------------------------------------------------------------------------------------------
def test_matchutil_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    monkeypatch.setattr(_ffi, "default_context", no_device)
    q = np.zeros((4, 128), np.uint8)
    with pytest.raises(ValueError, match="NORM_HAMMING"):
        matchutil.mutual_ratio_match_arrays(q.astype(np.float32), q, 0.8, options={"normType": matchutil.NORM_HAMMING})
    with pytest.raises(ValueError, match="normType"):
        matchutil.mutual_ratio_match_arrays(q, q, 0.8, options={"normType": 7})
    for norm in (matchutil.NORM_L2, matchutil.NORM_HAMMING):
        with pytest.raises(ValueError, match="no train descriptors"):
            matchutil.BFMatcher(norm).mutualRatioMatchEach(q, 0.8)                     # an empty collection
        with pytest.raises(ValueError, match="no train descriptors"):
            matchutil.BFMatcher(norm).mutualRatioMatchEach_arrays(q, 0.8, symmetric=True)
    h = matchutil.BFMatcher(matchutil.NORM_HAMMING)
    h.add([np.zeros((2, 32), np.uint8)])
    with pytest.raises(ValueError, match="NORM_HAMMING"):
        h.mutualRatioMatchEach(np.zeros((4, 32), np.float32), 0.8)                     # a wrong dtype for NORM_HAMMING
    m = matchutil.BFMatcher()
    m.add([q])
    with pytest.raises(ValueError, match="2-D"):
        m.mutualRatioMatchEach_arrays(np.zeros(128, np.uint8), 0.8)


def test_torchmatch_refusals_come_before_the_library(monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the library")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    cpu = torch.zeros((4, 128), dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA tensor"):
        torchmatch.mutual_ratio_match(cpu, cpu, 0.8)
    with pytest.raises(ValueError, match="torch.Tensor"):
        torchmatch.mutual_ratio_match(np.zeros((4, 128), np.uint8), cpu, 0.8)
    coll = torchmatch.Collection()
    with pytest.raises(ValueError, match="CUDA tensor"):
        coll.mutual_ratio_each(cpu, 0.8)
    with pytest.raises(ValueError, match="torch.Tensor"):
        coll.mutual_ratio_each(np.zeros((4, 128), np.uint8), 0.8, symmetric=True)
    with pytest.raises(ValueError, match="cap"):
        coll.mutual_ratio_each(cpu, 0.8, cap=-1)
    assert coll._coll is None
    assert "mutual_ratio_match" in torchmatch.__doc__ and "mutual_ratio_each" in torchmatch.__doc__
