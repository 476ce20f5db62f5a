"""CPU: the host side of image-pair matching inside a train collection (fm_collection_pairs_mutual_ratio and its device
form) -- the two prototypes against the ctypes binding, the header sentences they leave alone and the ones they add, the NumPy
reference (tests/pairs_ref.py) on a hand-worked three-image case, and the refusals of _ffi, matchutil and torchmatch that
touch no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil, torchmatch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairs_ref as ref        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fm_collection_pairs_mutual_ratio", "fm_collection_pairs_mutual_ratio_dev")
INF = float("inf")


def _rows(*vals):
    a = np.zeros((len(vals), 128), np.uint8)
    a[:, 0] = vals
    return a


def _header_text():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


# ---- header and binding -----------------------------------------------------------------------------------------------------
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
    assert name in _ffi.SYMBOLS, "the binding does not declare %s" % name
    res, argtypes = _ffi.SYMBOLS[name]
    assert res is ctypes.c_int
    got = [_klass_of_text(p) for p in protos[name].split(",")]
    assert got == [_klass_of_ctype(t) for t in argtypes]
    # (ctx, collection, pairs, n_pairs, tau, symmetric, cap, ...): offsets + four arrays + total | d_offsets, d_rows, total, stream
    want = ["ptr"] * 3 + ["i64", "f64", "i32", "i64"] + ["ptr"] * (4 if name.endswith("_dev") else 6)
    assert got == want
    assert hasattr(_ffi.load_library(), name)
    for method in ("pairs_mutual_ratio", "pairs_mutual_ratio_counts", "pairs_mutual_ratio_dev"):
        assert callable(getattr(_ffi.Collection, method))
    assert callable(torchmatch.Collection.match_pairs)
    assert callable(matchutil.BFMatcher.matchPairs) and callable(matchutil.BFMatcher.matchPairs_arrays)


def test_abi_revision_is_still_12_and_names_the_additions():
    hdr = _header_text()
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    comment = " ".join(hdr.split("#define FM_ABI_VERSION")[0].split()).replace(" * ", " ")
    assert "still revision 12, additions only -- FM_BANK_F32W" in comment
    assert comment.index("FM_BANK_F32W") < comment.index(NEW[0]) < comment.index(NEW[1])
    assert "still revision 12, additions only -- fm_collection_pairs_mutual_ratio, fm_collection_pairs_mutual_ratio_dev" in comment


def test_header_keeps_its_sentences_and_lists_what_is_not_built():
    hdr = _header_text()
    sect = hdr.split("---- train collections")[1].split("typedef struct fm_collection")[0]
    not_built = " ".join(sect.split("Not built:")[1].replace("\n *", " ").split())
    for still in ("Hamming radiusMatch (for pairs or collections)", "an _each form", "skipping the second count sweep",
                  "sharding a collection across GPUs", "fm_collection_knn_masked is built", "the STACKED crossCheck on a collection",
                  "binary collections in the self-distance test"):
        assert still in not_built, still
    for new in ("a sweep that computes a pair's tiles once for both directions", "sharing sweeps between (a, b) and (b, a)"):
        assert new in not_built, new
    flat = " ".join(hdr.replace("\n *", " ").split())
    assert "Not built for wide float banks" in flat and 'Not built ("masks")' in flat
    opt = " ".join(hdr.split('"coll_ws_bytes" 0..2^31-1')[1].split("Unknown names")[0].replace("\n *", " ").split())
    assert "25 bytes per entry" in opt and "132 bytes per candidate" in opt
    assert "fm_collection_pairs_mutual_ratio" in opt and "at least one pair per chunk" in opt
    for phrase in ("longest prefix of whole pairs", "pair p = (a, b) is ORDERED", "n_images (n_images - 1) / 2",
                   "2 rows(a) rows(b) per pair"):
        assert phrase in flat, phrase


# ---- the reference on a hand-worked case -----------------------------------------------------------------------------------
def test_reference_on_three_images_worked_by_hand():
    A, B, C = _rows(0, 10), _rows(1, 20), _rows()
    images = [A, B, C]

    def lists(res):
        return [(q.tolist(), t.tolist(), d.tolist(), r.tolist()) for q, t, d, r in res]

    # (A, B): row 0 of A is at 1 and 20 from B's rows (ratio 1 / 20), B's row 0 is nearest to A's row 0: accepted; row 1 of
    # A is at 9 and 10 (ratio 0.9): fails at 0.8, and at +inf its first neighbour, B's row 0, prefers A's row 0
    for tau in (0.8, INF):
        assert lists(ref.pairs_mutual_ratio(images, [(0, 1)], tau)) == [([0], [0], [1.0], [1.0 / 20.0])]
    # (B, A) is another pair: row 0 of B at 1 and 9; row 1 of B at 10 (A's row 1) and 20 passes (0.5) but A's row 1 prefers B's row 0
    assert lists(ref.pairs_mutual_ratio(images, [(1, 0)], 0.8)) == [([0], [0], [1.0], [1.0 / 9.0])]
    # symmetric: the reverse ratio of B's row 0 over A is 1 / 9, the larger of the two is reported
    assert lists(ref.pairs_mutual_ratio(images, [(0, 1)], 0.8, True)) == [([0], [0], [1.0], [1.0 / 9.0])]
    assert lists(ref.pairs_mutual_ratio(images, [(0, 1)], 0.1, True)) == [([], [], [], [])]
    # a == b: every row is its own mutual neighbour at distance 0
    assert lists(ref.pairs_mutual_ratio(images, [(0, 0)], 0.8)) == [([0, 1], [0, 1], [0.0, 0.0], [0.0, 0.0])]
    # an empty image keeps its index and accepts nothing, on either side
    assert lists(ref.pairs_mutual_ratio(images, [(0, 2), (2, 0), (2, 2)], INF)) == [([], [], [], [])] * 3
    # pairs = None: every i < j in lexicographic order
    assert ref.all_pairs(3) == [(0, 1), (0, 2), (1, 2)] and ref.all_pairs(1) == [] and ref.all_pairs(0) == []
    assert [r[0].tolist() for r in ref.pairs_mutual_ratio(images, None, 0.8)] == [[0], [], []]
    # the packing rule: full counts always, rows for the longest prefix of whole pairs
    per = ref.pairs_mutual_ratio(images, [(0, 1), (0, 0), (2, 0), (1, 0), (0, 1)], 0.8)
    for cap, rows in ((0, 0), (1, 1), (2, 1), (3, 3), (4, 4), (5, 5), (99, 5)):
        offsets, n, cols = ref.pack(per, cap)
        assert offsets.tolist() == [0, 1, 3, 3, 4, 5] and n == rows and all(c.shape[0] == rows for c in cols)
    assert ref.pack(per, 4)[2][0].tolist() == [0, 0, 1, 0] and ref.pack(per, 4)[2][1].tolist() == [0, 0, 1, 0]
    assert ref.pack(per, 4)[2][3].tolist() == [1.0 / 20.0, 0.0, 0.0, 1.0 / 9.0]
    assert ref.pack([], 7)[0].tolist() == [0]


# ---- refusals that touch no device --------------------------------------------------------------------------------------------
def test_pairs_array_accepts_lists_and_arrays_and_refuses_the_rest():
    a = _ffi.pairs_array([(0, 1), (2, 0)])
    assert a.dtype == np.int32 and a.shape == (2, 2) and a.flags.c_contiguous and a.tolist() == [[0, 1], [2, 0]]
    same = np.array([[3, 4]], np.int32)
    assert _ffi.pairs_array(same) is same
    assert _ffi.pairs_array(np.array([[3, 4]], np.int64)).tolist() == [[3, 4]]
    empty = _ffi.pairs_array([])
    assert empty.shape == (0, 2) and empty.ctypes.data != 0          # (NULL would mean "every a < b")
    for bad in ([(0, 1, 2)], [0, 1], np.zeros((2, 2), np.float32), [(0.5, 1)], 7, [[(0, 1)]]):
        with pytest.raises(ValueError, match="pairs"):
            _ffi.pairs_array(bad)
    with pytest.raises(ValueError, match="outside"):
        _ffi.pairs_array([(0, 3)], 3)
    with pytest.raises(ValueError, match="outside"):
        _ffi.pairs_array([(-1, 0)], 3)
    with pytest.raises(ValueError, match="int32"):
        _ffi.pairs_array([(0, 2 ** 40)])


def test_matchutil_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "load_library", no_device)
    q = np.zeros((4, 128), np.uint8)
    for norm in (matchutil.NORM_L2, matchutil.NORM_HAMMING):
        with pytest.raises(ValueError, match="no train descriptors"):
            matchutil.BFMatcher(norm).matchPairs()                                  # an empty collection
        x = matchutil.BFMatcher(norm, crossCheck=True)
        x.add([q[:, :32], q[:, :32]])
        with pytest.raises(ValueError, match="mutual by itself"):
            x.matchPairs()
        with pytest.raises(ValueError, match="mutual by itself"):
            x.matchPairs_arrays([(0, 1)])
        m = matchutil.BFMatcher(norm)
        m.add([q[:, :32], q[:, :32], q[:0, :32]])
        for bad in ([(0, 1, 2)], [0, 1], np.zeros((2, 2), np.float32), [(0, 3)], [(-1, 0)], [(0, 1), (3, 0)]):
            with pytest.raises(ValueError, match="pairs"):
                m.matchPairs(bad)
            with pytest.raises(ValueError, match="pairs"):
                m.matchPairs_arrays(bad, ratio=0.7, symmetric=True)
        assert m._coll is None and m._uploaded == 0


def test_torchmatch_refusals_come_before_the_library(monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the library")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "load_library", no_device)
    coll = torchmatch.Collection()
    with pytest.raises(ValueError, match="cap"):
        coll.match_pairs(cap=-1)
    with pytest.raises(ValueError, match="pairs"):
        coll.match_pairs([(0, 1, 2)])
    with pytest.raises(ValueError, match="int32 CPU tensor"):
        coll.match_pairs(torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="pairs"):
        coll.match_pairs(torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="outside"):
        coll.match_pairs([(0, 1)])                                    # no image has been added
    with pytest.raises(ValueError, match="outside"):
        coll.match_pairs(torch.tensor([[0, 1]], dtype=torch.int32), tau=0.7, symmetric=True, cap=10)
    assert coll._coll is None
    assert "match_pairs" in torchmatch.__doc__ and "fm_collection_pairs_mutual_ratio_dev" in torchmatch.__doc__
