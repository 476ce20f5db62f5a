"""A wide query against a wide collection (fm_collection_wide_knn2_each, fm_collection_wide_mutual_ratio_each and its device
form), everything that needs no GPU: the three prototypes against the ctypes binding, the header's new paragraph and the
sentences the earlier host tests quote, the refusals of matchutil and torchmatch that touch no device, and the NumPy reference
(tests/wide_query_ref.py) on a hand-worked case."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_query_ref as ref                    # noqa: E402

from fastmatch_amd import _ffi, matchutil, torchmatch      # noqa: E402

NEW = ("fm_collection_wide_knn2_each", "fm_collection_wide_mutual_ratio_each", "fm_collection_wide_mutual_ratio_each_dev")
WANT = {
    # (ctx, collection, q, idx, dist)
    NEW[0]: ["ptr"] * 5,
    # (ctx, collection, q, tau, symmetric, cap, offsets, qidx, tidx, dist, ratio, n_total)
    NEW[1]: ["ptr"] * 3 + ["f64", "i32", "i64"] + ["ptr"] * 6,
    # (ctx, collection, q, tau, symmetric, cap, d_offsets, d_rows, n_total, consumer_stream)
    NEW[2]: ["ptr"] * 3 + ["f64", "i32", "i64"] + ["ptr"] * 4,
}


def _header_text():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


def _klass_of_text(p):
    p = " ".join(p.split())
    if "*" in p or "[" in p:
        return "ptr"
    for word, k in (("double", "f64"), ("int64_t", "i64"), ("int32_t", "i32"), ("int", "int")):
        if re.search(r"\b%s\b" % word, p):
            return k
    raise AssertionError("unclassified parameter: %r" % p)


@pytest.mark.parametrize("name", NEW)
def test_prototypes_match_the_binding(name):
    hdr = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(fm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    assert name in protos, "the header does not declare %s" % name
    assert name in _ffi.SYMBOLS, "the binding does not declare %s" % name
    res, argtypes = _ffi.SYMBOLS[name]
    assert res is ctypes.c_int
    assert [_klass_of_text(p) for p in protos[name].split(",")] == WANT[name]
    assert len(argtypes) == len(WANT[name])
    for t, k in zip(argtypes, WANT[name]):
        if k == "ptr":
            assert t not in (ctypes.c_int32, ctypes.c_int64, ctypes.c_int, ctypes.c_double)
        elif k == "f64":
            assert t is ctypes.c_double
        else:
            assert t is not ctypes.c_double and ctypes.sizeof(t) == (8 if k == "i64" else 4)
    assert hasattr(_ffi.load_library(), name)
    for method in ("wide_knn2_each", "wide_mutual_ratio_each", "wide_mutual_ratio_each_counts", "wide_mutual_ratio_each_dev"):
        assert callable(getattr(_ffi.Collection, method))
    assert callable(torchmatch.Collection.wide_mutual_ratio_each)
    for method in ("mutualRatioMatchWideEach", "mutualRatioMatchWideEach_arrays", "knnMatchWideEach_arrays"):
        assert callable(getattr(matchutil.BFMatcher, method))


def test_abi_comment_appends_the_three_symbols():
    hdr = _header_text()
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    comment = " ".join(hdr.split("#define FM_ABI_VERSION")[0].split()).replace(" * ", " ")
    mine = "still revision 12, additions only -- " + ", ".join(NEW)
    earlier = "still revision 12, additions only -- fm_collection_add_wide, fm_collection_add_wide_dev"
    assert mine in comment and earlier in comment and comment.index(earlier) < comment.index(mine)


def test_header_paragraph():
    hdr = _header_text()
    sect = hdr.split("---- K14: wide float banks")[1].split("int  fm_bank_destroy")[0]
    flat = " ".join(sect.replace("\n *", " ").split())
    # the headings stand once each, in their order, and the new paragraph comes last
    for heading in ("Not built for wide float banks:", "Wide COLLECTIONS:", "Not built for wide collections:", "Wide QUERIES:"):
        assert flat.count(heading) == 1, heading
    assert (flat.index("Not built for wide float banks:") < flat.index("Wide COLLECTIONS:") < flat.index("Not built for wide collections:")
            < flat.index("Wide QUERIES:"))
    # what the earlier host tests quote is still found by their own splits
    old = flat.split("Not built for wide float banks:")[1]
    assert "and every fm_collection_* call -- a wide query bank, and fm_collection_add_f32 / fm_collection_add_dev with more than 128 values per row." in old
    for name in ("k >= 3", "fm_radius_match(_dev)", "fm_self_dist(_batch)", "fm_knn_masked(_dev)", "fm_expand_create", "fm_collection_*"):
        assert name in old, name
    coll = flat.split("Wide COLLECTIONS:")[1]
    for phrase in ("129 <= dim <= 256", "even with n = 0", "never lowered again", "fm_collection_pairs_mutual_ratio(_dev)",
                   "one launch per filtered chunk and one fallback per chunk redone", "PER CHUNK", "straight after the NULL-handle checks"):
        assert phrase in coll, phrase
    not_built = coll.split("Not built for wide collections:")[1].split("Wide QUERIES:")[0]
    assert "every other fm_collection_* call" in not_built
    for name in ("fm_collection_knn(_dev)", "fm_collection_knn2_each", "fm_collection_votes", "fm_collection_xcheck1_each(_dev)",
                 "fm_collection_mutual_ratio_each(_dev)", "fm_mask_create_coll", "k >= 3", "LDS staging", "once for both directions"):
        assert name in not_built, name
    new = flat.split("Wide QUERIES:")[1]
    for phrase in NEW[:2] + ("fm_collection_wide_mutual_ratio_each_dev", "fm_knn2(q, B_i)", "fm_mutual_ratio(q, B_i, tau, symmetric)",
                             "bit for bit", "qidx is the query row", "the row inside image i", "An empty image keeps its slot".lower(),
                             "longest prefix of whole images", "cap = 0 is counts only", "12-byte rows", "not accounted in fm_stats",
                             "2 nq sum rows_i", "offsets[0] = 0", "even for an empty query", "ONE OPERAND OUTSIDE THE STACK",
                             "ONE filter launch", "no host wait between the sweeps", "differ by more than 8", '"f32_nsplit"',
                             "one launch per filtered chunk and one fallback per chunk redone", "pad128(nq) + pad128(rows_i)",
                             "Out of scope here", "votes mode 0", "masks", "radius queries", "one resident copy of the query's B operand",
                             "LDS staging of the streamed operand", "once for both directions"):
        assert phrase in new, phrase


def test_matchutil_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    monkeypatch.setattr(_ffi, "default_context", no_device)
    w = [np.zeros((4, 256), np.float32), np.zeros((0, 256), np.float32), np.zeros((5, 256), np.float32)]
    q = np.zeros((3, 256), np.float32)
    wide_calls = (lambda m, x: m.mutualRatioMatchWideEach(x, 0.8), lambda m, x: m.mutualRatioMatchWideEach_arrays(x, 0.8, True),
                  lambda m, x: m.knnMatchWideEach_arrays(x))
    # a collection that is not wide, an empty one, another norm
    narrow = matchutil.BFMatcher()
    narrow.add([np.zeros((3, 128), np.float32)])
    for call in wide_calls:
        with pytest.raises(ValueError, match="not a wide one"):
            call(narrow, q)
        with pytest.raises(ValueError, match="no train descriptors"):
            call(matchutil.BFMatcher(), q)
        with pytest.raises(ValueError, match="NORM_L2"):
            call(matchutil.BFMatcher(matchutil.NORM_HAMMING), q)
    m = matchutil.BFMatcher()
    m.add_wide(w)
    # a query that is not a float array [nq, the collection's width]
    for bad in (np.zeros((3, 200), np.float32), np.zeros((3, 256), np.uint8), np.zeros(256, np.float32), np.zeros((3, 128), np.float32),
                np.zeros((3, 256), np.int32)):
        for call in wide_calls:
            with pytest.raises(ValueError, match="float array"):
                call(m, bad)
    # the old methods still say "wide"
    for call in (lambda: m.knnMatch(q, k=2), lambda: m.match(q), lambda: m.knnMatchEach_arrays(q), lambda: m.votes(q, 0.8),
                 lambda: m.matchEach(q), lambda: m.mutualRatioMatchEach(q, 0.8), lambda: m.mutualRatioMatchEach_arrays(q, 0.8),
                 lambda: m.fastMatchEach(q, 0.8)):
        with pytest.raises(ValueError, match="wide"):
            call()
    # what is served reaches the device
    for x in (q, q.astype(np.float64)):
        for call in wide_calls:
            with pytest.raises(AssertionError, match="touched the device"):
                call(m, x)
    with pytest.raises(AssertionError, match="touched the device"):
        m.matchPairs()


def test_torchmatch_refusals_come_before_the_library(monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the library")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(torchmatch, "_ctx_for", no_device)
    coll = torchmatch.Collection()
    x = torch.zeros((4, 256))
    with pytest.raises(ValueError, match="not a wide one"):
        coll.wide_mutual_ratio_each(x, 0.8)
    assert coll._coll is None
    coll._wide = True                                 # what the first add_wide leaves behind
    with pytest.raises(ValueError, match="CUDA tensor"):
        coll.wide_mutual_ratio_each(x, 0.8)
    with pytest.raises(ValueError, match="negative"):
        coll.wide_mutual_ratio_each(x, 0.8, cap=-1)
    # the old methods still say "wide"
    for call in (lambda: coll.knn(x, 2), lambda: coll.ratio_match(x, 0.8), lambda: coll.mutual_ratio_each(x, 0.8),
                 lambda: coll.mutual_nn_each(x), lambda: coll.fast_match_each(x, 0.8)):
        with pytest.raises(ValueError, match="wide"):
            call()
    assert coll._coll is None


def test_reference_on_a_hand_worked_case():
    dim = 129

    def rows(*specs):
        a = np.zeros((len(specs), dim), np.float32)
        for i, spec in enumerate(specs):
            for k, v in spec:
                a[i, k] = v
        return a
    # q0 is the nearest query row of a row of A AND of a row of B: the images are independent, it matches in both
    Q = rows([(0, 1.0)], [(1, 1.0)], [(128, 1.0)], [(128, 1.0)])
    A = rows([(0, 1.0)], [(1, 1.0), (2, 0.1)], [(5, 4.0)])
    B = rows([(9, 3.0)], [(0, 1.0), (3, 0.2)], [(128, 1.0), (4, 0.1)], [(7, 3.0)])
    E = np.zeros((0, dim), np.float32)
    One = rows([(0, 1.0)])
    images = [A, E, B, One]
    for sym in (False, True):
        per = ref.mutual_ratio_each(Q, images, 0.8, sym)
        # A: q0 = a0 exactly (ratio 0), q1 has a1 at 0.1 (second neighbour a0 at sqrt(2)); q2, q3 are sqrt(2) from a0 and
        # sqrt(2.01) from a1: ratio 0.9975 fails
        assert per[0][0].tolist() == [0, 1] and per[0][1].tolist() == [0, 1]
        assert per[0][2][0] == 0 and abs(float(per[0][2][1]) - 0.1) < 1e-7
        assert per[0][3][0] == 0 and abs(per[0][3][1] - 0.1 / np.sqrt(2.0)) < 1e-6
        # the empty image and the one-row image (no second neighbour: no ratio) accept nothing
        assert per[1][0].shape[0] == 0 and per[3][0].shape[0] == 0
        # B: q0 has b1 at 0.2 (second: b2 at sqrt(2.01)); q2 and q3 are both 0.1 from b2, whose nearest query row is the
        # LOWER index q2 -- q3 is not mutual -- and whose own ratio over the query rows is 0.1 / 0.1 = 1: symmetric drops q2
        assert per[2][0].tolist() == ([0] if sym else [0, 2]) and per[2][1].tolist() == ([1] if sym else [1, 2])
        assert abs(float(per[2][2][0]) - 0.2) < 1e-7
    # tau = +inf keeps every mutual row with a second neighbour: q2 passes in symmetric mode too (1 < inf), q3 never
    per = ref.mutual_ratio_each(Q, images, float("inf"), True)
    assert per[2][0].tolist() == [0, 2] and per[2][3][1] == 1.0
    assert per[3][0].shape[0] == 0                    # one row: the ratio is NaN, and NaN < inf is false
    # the knn2 form: -1 / +inf where an image has fewer than two rows
    idx, dist = ref.knn2_each(Q, images)
    assert idx.shape == (4, 4, 2) and (idx[1] == -1).all() and np.isinf(dist[1]).all()
    assert idx[3, :, 0].tolist() == [0, 0, 0, 0] and (idx[3, :, 1] == -1).all() and np.isinf(dist[3, :, 1]).all()
    assert idx[0, 0].tolist() == [0, 1] and idx[2, 2].tolist() == [2, 1]
    # the packed output: full counts in the offsets, the longest prefix of whole images in the rows
    per = ref.mutual_ratio_each(Q, images, 0.8)
    offsets, written, cols = ref.pack(per, 3)
    assert offsets.tolist() == [0, 2, 2, 4, 4] and written == 2 and cols[0].tolist() == [0, 1]
    offsets, written, cols = ref.pack(per, 4)
    assert written == 4 and cols[0].tolist() == [0, 1, 0, 2] and cols[1].tolist() == [0, 1, 1, 2]


def test_planted_views_are_found_by_the_reference():
    """The data of the GPU test: every second query row is a view of a row of image 5; images 2 .. 6 accept rows, the empty
    images and the one-row image none; with one query row times 8 (another fp16 scale) the reference still accepts rows."""
    for dim in (129, 256):
        images, Q = ref.data(dim)
        assert np.array_equal(Q[6], Q[7])
        for tau, sym in ((0.8, False), (0.8, True), (float("inf"), False)):
            counts = [r[0].shape[0] for r in ref.mutual_ratio_each(Q, images, tau, sym)]
            assert all(c > 0 for c in counts[2:7]) and counts[0] == counts[1] == counts[7] == 0, counts
            assert counts[5] >= 100
        Q8 = Q.copy()
        Q8[11] *= 8
        counts = [r[0].shape[0] for r in ref.mutual_ratio_each(Q8, images, 0.8, True)]
        assert all(c > 0 for c in counts[2:7])
