"""CPU: the host side of Fast-Match's self-distance test on binary descriptors -- hand-checked cases of the NumPy reference
(tests/hamming_fast_ref.py), the ValueErrors of matchutil / BFMatcher / torchmatch that are raised before anything is
uploaded, and the new prototypes of the header against the ctypes binding and the ABI revision they leave alone."""
import ctypes
import os
import re

import numpy as np
import pytest

import hamming_fast_ref as HF
from fastmatch_amd import _ffi, matchutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fm_hamming_self_dist", "fm_hamming_self_dist_batch", "fm_hamming_set_selfdist", "fm_hamming_match_ratio",
       "fm_hamming_match_accepted", "fm_hamming_match_accepted_dev", "fm_collection_hamming_match_accepted_each",
       "fm_collection_hamming_match_accepted_each_dev")
L2 = {"fm_hamming_self_dist": "fm_self_dist", "fm_hamming_self_dist_batch": "fm_self_dist_batch",
      "fm_hamming_set_selfdist": "fm_bank_set_selfdist", "fm_hamming_match_ratio": "fm_match_ratio",
      "fm_hamming_match_accepted": "fm_match_accepted", "fm_hamming_match_accepted_dev": "fm_match_accepted_dev",
      "fm_collection_hamming_match_accepted_each": "fm_collection_match_accepted_each",
      "fm_collection_hamming_match_accepted_each_dev": "fm_collection_match_accepted_each_dev"}


def _rows(*hexes):
    return np.array([list(bytes.fromhex(h)) for h in hexes], np.uint8)


# ---- the reference, by hand ------------------------------------------------------------------------------------------------
def test_self_dist_by_hand():
    B = _rows("00ff", "01ff", "00ff", "ff00")         # rows 0 and 2 are duplicates; row 1 is 1 bit from both; row 3 their complement
    assert HF.self_dist(B).tolist() == [0.0, 1.0, 0.0, 15.0]
    assert HF.self_dist(_rows("a5")).tolist() == [np.inf]                     # a bank of one row
    assert HF.self_dist(np.zeros((0, 4), np.uint8)).shape == (0,)
    x = _rows("0f3c", "f0c3")                                                 # complementary rows: every bit differs
    assert HF.self_dist(x).tolist() == [16.0, 16.0]
    assert HF.self_dist(_rows("0f", "0f", "0f")).tolist() == [0.0, 0.0, 0.0]  # an all-equal bank
    assert HF.self_dist(B).dtype == np.float64


def test_ratio_rules_by_hand():
    Q = _rows("00", "00", "0f", "f0")                 # rows 0 and 1 are duplicates (selfdist 0), rows 2 and 3 are 8 apart, 4 from them
    sd = HF.self_dist(Q)
    assert sd.tolist() == [0.0, 0.0, 4.0, 4.0]
    # train row 0 = query 0 exactly (elects row 0, the lower duplicate: 0 / 0), row 1 is 1 bit from query 2, row 2 is 3 bits from query 3
    T = _rows("00", "0e", "f7")
    tidx, dist, ratio, passed = HF.match_ratio(Q, T, sd, 0.5)
    assert tidx.tolist() == [0, -1, 1, 2] and dist[[0, 2, 3]].tolist() == [0.0, 1.0, 3.0] and np.isinf(dist[1])
    assert np.isnan(ratio[0]) and np.isnan(ratio[1]) and ratio[2] == 0.25 and ratio[3] == 0.75
    assert passed.tolist() == [False, False, True, False]                      # 0 / 0 rejected, 0.25 < 0.5, 0.75 not
    assert HF.match_ratio(Q, T, sd, np.inf)[3].tolist() == [False, False, True, True]      # NaN is not < inf either
    # d / 0: the duplicates' train row one bit away -> +inf, rejected at every tau
    tidx, dist, ratio, passed = HF.match_ratio(Q, _rows("01"), sd, np.inf)
    assert tidx[0] == 0 and dist[0] == 1.0 and ratio[0] == np.inf and not passed.any()
    # a bank of one query row: selfdist +inf, ratio 0, accepted for every tau > 0 and for none at tau = 0
    one = _rows("3c")
    assert HF.self_dist(one).tolist() == [np.inf]
    q, t, d, r = HF.match_accepted(one, _rows("ff", "00"), HF.self_dist(one), 1e-300)
    assert q.tolist() == [0] and t.tolist() == [0] and d.tolist() == [4.0] and r.tolist() == [0.0]               # (strict <: the lower train row on the tie at 4)
    assert len(HF.match_accepted(one, _rows("ff"), HF.self_dist(one), 0.0)[0]) == 0
    # accepted rows ascend in query index and carry float64 ratios
    q, t, d, r = HF.match_accepted(Q, T, sd, 0.9)
    assert q.tolist() == [2, 3] and t.tolist() == [1, 2] and r.dtype == np.float64 and d.dtype == np.float32
    assert HF.same_f64(np.array([np.nan, 1.0]), np.array([-np.nan, 1.0])) and not HF.same_f64(np.array([0.0]), np.array([-0.0]))


# ---- refusals that touch no device -----------------------------------------------------------------------------------------
def test_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    b32, b16 = np.zeros((4, 32), np.uint8), np.zeros((4, 16), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        matchutil.hamming_fast_match_arrays(b32.astype(np.float32), b32, 0.9)
    with pytest.raises(ValueError, match="32 bytes per query row, 16 per train row"):
        matchutil.hamming_fast_match(b32, b16, 0.9)
    with pytest.raises(ValueError, match="1 .. 64 bytes"):
        matchutil.hamming_fast_match_arrays(np.zeros((4, 65), np.uint8), np.zeros((4, 65), np.uint8), 0.9)
    with pytest.raises(ValueError, match="2-D"):
        matchutil.hamming_fast_match_arrays(np.zeros(32, np.uint8), b32, 0.9)
    with pytest.raises(ValueError, match="NORM_HAMMING matcher"):
        matchutil.BFMatcher().hammingFastMatchEach(b32, 0.9)                  # an L2 matcher
    l2 = matchutil.BFMatcher()
    l2.add([np.zeros((2, 128), np.uint8)])
    with pytest.raises(ValueError, match="NORM_HAMMING matcher"):
        l2.hammingFastMatchEach_arrays(np.zeros((4, 128), np.uint8), 0.9)
    h = matchutil.BFMatcher(matchutil.NORM_HAMMING)
    with pytest.raises(ValueError, match="no train descriptors"):
        h.hammingFastMatchEach(b32, 0.9)                                       # nothing added
    with pytest.raises(ValueError, match="no train descriptors"):
        h.hammingFastMatchEach_arrays(b32, 0.9)
    h.add([b32])
    with pytest.raises(ValueError, match="uint8"):
        h.hammingFastMatchEach(b32.astype(np.float32), 0.9)
    # fastMatchEach keeps refusing a NORM_HAMMING matcher, and says which method serves it
    with pytest.raises(ValueError, match="NORM_HAMMING") as e:
        h.fastMatchEach(b32, 0.9)
    assert "hammingFastMatchEach" in str(e.value)


# ---- header and binding ----------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


def _prose(comment):
    """A block comment's text on one line, without the ' * ' that starts its lines."""
    return " ".join(re.sub(r"\n\s*\*\s?", " ", comment).split())


def _klass_of_text(p):
    p = " ".join(p.split())
    if "*" in p or "[" in p:
        return "ptr"
    if re.search(r"\bdouble\b", p):
        return "f64"
    if re.search(r"\b(int64_t|uint64_t)\b", p):
        return "i64"
    if re.search(r"\b(int32_t|int)\b", p):
        return "i32"
    raise AssertionError("unclassified parameter: " + p)


def _klass_of_ctype(t):
    if t is ctypes.c_void_p or hasattr(t, "contents"):
        return "ptr"
    return {ctypes.c_double: "f64", ctypes.c_int64: "i64", ctypes.c_int: "i32", ctypes.c_int32: "i32"}[t]


@pytest.mark.parametrize("name", NEW)
def test_new_prototypes_match_the_binding_and_their_l2_namesakes(name):
    protos = dict(re.findall(r"\bint\s+(fm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S), flags=re.S))
    assert name in protos, "the header does not declare %s" % name
    texts = protos[name].split(",")
    res, argtypes = _ffi.SYMBOLS[name]
    assert res is ctypes.c_int and len(texts) == len(argtypes)
    assert [_klass_of_text(p) for p in texts] == [_klass_of_ctype(t) for t in argtypes]
    # the argument list is the L2 call's
    assert [_klass_of_text(p) for p in texts] == [_klass_of_text(p) for p in protos[L2[name]].split(",")]
    assert hasattr(_ffi.load_library(), name)


def test_abi_revision_and_not_built_lists():
    hdr = _header()
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    for name in NEW:                                  # the revision comment names the additions
        assert name in hdr.split("#define FM_ABI_VERSION")[0]
    k11 = _prose(hdr.split("int  fm_bank_create_bin")[0].split("Not built:")[-1])
    assert "self distances" not in k11 and "fm_expand_*" in k11 and "NORM_HAMMING2" in k11
    sect = _prose(hdr.split("---- Hamming Fast-Match")[1].split("int fm_hamming_self_dist")[0])
    for out_of_scope in ("triangular sweep", "ratio cut", "fm_expand_*", "async / batch / sharded-key", "NORM_HAMMING2"):
        assert out_of_scope in sect.split("Not built:")[1], out_of_scope
    for rule in ("0 / 0 = NaN", "d / 0 = +inf", "bank of one query row", "lowest index wins a tie", "no self distances"):
        assert rule in sect, rule


def test_python_layers_expose_the_calls():
    for k, names in ((_ffi.Context, ("hamming_self_dist", "hamming_self_dist_batch", "hamming_match_ratio", "hamming_match_accepted",
                                     "hamming_match_accepted_dev")),
                     (_ffi.Bank, ("set_hamming_selfdist",)),
                     (_ffi.Collection, ("hamming_match_accepted_each", "hamming_match_accepted_each_dev")),
                     (matchutil.BFMatcher, ("hammingFastMatchEach", "hammingFastMatchEach_arrays"))):
        for n in names:
            assert callable(getattr(k, n)), n
    assert callable(matchutil.hamming_fast_match) and callable(matchutil.hamming_fast_match_arrays)
    from fastmatch_amd import torchmatch
    assert callable(torchmatch.hamming_fast_match) and callable(torchmatch.Collection.hamming_fast_match_each)
