"""Wide collections (fm_collection_add_wide, fm_collection_add_wide_dev; the match graph on 129 .. 256-D images), everything
that needs no GPU: the header's sentences and the ABI comment, the two prototypes against the ctypes binding, the refusals of
matchutil and torchmatch that touch no device, and the NumPy reference (tests/wide_pairs_ref.py) on a hand-worked case."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_pairs_ref as ref                    # noqa: E402

from fastmatch_amd import _ffi, matchutil, torchmatch      # noqa: E402

NEW = ("fm_collection_add_wide", "fm_collection_add_wide_dev")


def _header_text():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


def test_abi_comment_appends_the_two_symbols():
    hdr = _header_text()
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    comment = " ".join(hdr.split("#define FM_ABI_VERSION")[0].split()).replace(" * ", " ")
    assert "still revision 12, additions only -- fm_collection_add_wide, fm_collection_add_wide_dev" in comment
    # appended: the earlier sentences stand in front of it, unchanged
    earlier = "still revision 12, additions only -- fm_collection_pairs_mutual_ratio, fm_collection_pairs_mutual_ratio_dev"
    assert earlier in comment and comment.index(earlier) < comment.index("-- fm_collection_add_wide,")
    assert "still revision 12, additions only -- FM_BANK_F32W" in comment


def _klass_of_text(p):
    p = " ".join(p.split())
    if "*" in p or "[" in p:
        return "ptr"
    for word, k in (("int64_t", "i64"), ("int32_t", "i32"), ("int", "int")):
        if re.search(r"\b%s\b" % word, p):
            return k
    raise AssertionError("unclassified parameter: %r" % p)


def _klass_of_ctype(t):
    if t is ctypes.c_int64:
        return "i64"
    if t is ctypes.c_int32 and t is not ctypes.c_int:
        return "i32"
    if t is ctypes.c_int:
        return "int"
    return "ptr"


@pytest.mark.parametrize("name", NEW)
def test_prototypes_match_the_binding(name):
    hdr = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(fm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    assert name in protos, "the header does not declare %s" % name
    assert name in _ffi.SYMBOLS, "the binding does not declare %s" % name
    res, argtypes = _ffi.SYMBOLS[name]
    assert res is ctypes.c_int
    got = [_klass_of_text(p) for p in protos[name].split(",")]
    # (ctx, collection, rows, n, dim, img_idx) | (ctx, collection, d_rows, dtype, n, dim, row_pitch_bytes, producer_stream, img_idx)
    want = ["ptr"] * 3 + (["i64", "int", "ptr"] if name == NEW[0] else ["int", "i64", "int", "i64", "ptr", "ptr"])
    assert got == want
    assert len(argtypes) == len(want)
    for t, k in zip(argtypes, want):
        if k == "ptr":
            assert _klass_of_ctype(t) == "ptr"
        else:
            assert ctypes.sizeof(t) == (8 if k == "i64" else 4)
    assert hasattr(_ffi.load_library(), name)
    for method in ("add_wide", "add_wide_from_device"):
        assert callable(getattr(_ffi.Collection, method))
    assert callable(torchmatch.Collection.add_wide) and callable(matchutil.BFMatcher.add_wide)


def test_header_sentences():
    hdr = _header_text()
    sect = hdr.split("---- K14: wide float banks")[1].split("int  fm_bank_destroy")[0]
    flat = " ".join(sect.replace("\n *", " ").split())
    # what was there stays, word for word
    old = flat.split("Not built for wide float banks:")[1]
    assert "and every fm_collection_* call -- a wide query bank, and fm_collection_add_f32 / fm_collection_add_dev with more than 128 values per row." in old
    new = flat.split("Wide COLLECTIONS:")[1]
    for phrase in ("fm_collection_add_wide", "fm_collection_add_wide_dev", "129 <= dim <= 256", "dim <= 128 is FM_EINVAL",
                   "dim > 256 FM_EUNSUPPORTED", "even with n = 0", "Every refusal leaves the collection unchanged".lower(),
                   "fm_collection_clear resets kind and width", "no FM_COLLECTION_F32_MAX limit", "excluded by index, never by value",
                   "bit for bit", "may alternate", "never lowered again", "fm_collection_info (kind FM_BANK_F32W, the real dim)",
                   "fm_collection_image_rows", "fm_collection_train", "fm_collection_pairs_mutual_ratio(_dev)",
                   "one launch per filtered chunk and one fallback per chunk redone", "PER CHUNK", '"wide"',
                   "straight after the NULL-handle checks"):
        assert phrase in new, phrase
    not_built = new.split("Not built for wide collections:")[1]
    assert "every other fm_collection_* call" in not_built
    for name in ("fm_collection_knn(_dev)", "fm_collection_knn2_ratio(_dev)", "fm_collection_knn2_each", "fm_collection_votes",
                 "fm_collection_knn_masked(_dev)", "fm_collection_radius_match(_dev)", "fm_collection_match_accepted_each(_dev)",
                 "fm_collection_xcheck1_each(_dev)", "fm_collection_mutual_ratio_each(_dev)", "fm_mask_create_coll", "k >= 3",
                 "LDS staging", "once for both directions"):
        assert name in not_built, name
    opt = " ".join(hdr.split('"coll_ws_bytes" 0..2^31-1')[1].split("Unknown names")[0].replace("\n *", " ").split())
    assert "wide collection" in opt and "256 records of 12 bytes" in opt and "20 bytes per row" in opt


def test_matchutil_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    monkeypatch.setattr(_ffi, "default_context", no_device)
    w = [np.zeros((4, 256), np.float32), np.zeros((0, 256), np.float64), np.zeros((5, 256), np.float32)]
    q = np.zeros((3, 256), np.float32)
    m = matchutil.BFMatcher()
    # what add_wide does not take
    for bad in ([np.zeros((4, 128), np.float32)], [np.zeros((4, 257), np.float32)], [np.zeros((4, 200), np.uint8)],
                [np.zeros((4, 256), np.float32), np.zeros((4, 255), np.float32)], [np.zeros(256, np.float32)]):
        with pytest.raises(ValueError):
            m.add_wide(bad)
        assert m.empty()
    with pytest.raises(ValueError, match="NORM_L2"):
        matchutil.BFMatcher(matchutil.NORM_HAMMING).add_wide(w)
    narrow = matchutil.BFMatcher()
    narrow.add([np.zeros((3, 128), np.float32)])
    with pytest.raises(ValueError, match="do not mix"):
        narrow.add_wide(w)
    assert len(narrow.getTrainDescriptors()) == 1
    # add keeps refusing wide rows, and now names add_wide
    with pytest.raises(ValueError, match="wide.*add_wide"):
        matchutil.BFMatcher().add(w)
    m.add_wide(w)
    assert len(m.getTrainDescriptors()) == 3 and all(a.dtype == np.float32 for a in m.getTrainDescriptors())
    with pytest.raises(ValueError, match="wide"):
        m.add([np.zeros((3, 128), np.float32)])
    with pytest.raises(ValueError, match="share a width"):
        m.add_wide([np.zeros((3, 200), np.float32)])
    assert len(m.getTrainDescriptors()) == 3
    for call in (lambda: m.knnMatch(q, k=2), lambda: m.match(q), lambda: m.knnMatch_arrays(q, 1), lambda: m.knnMatchEach_arrays(q),
                 lambda: m.votes(q, 0.8), lambda: m.fastMatchEach(q, 0.8), lambda: m.fastMatchEach_arrays(q, 0.8),
                 lambda: m.matchEach(q), lambda: m.matchEach_arrays(q), lambda: m.mutualRatioMatchEach(q, 0.8),
                 lambda: m.mutualRatioMatchEach_arrays(q, 0.8), lambda: m.knnMatch(q, k=1, masks=[None, None, None])):
        with pytest.raises(ValueError, match="wide"):
            call()
    # what is served reaches the device
    for call in (lambda: m.matchPairs(), lambda: m.matchPairs_arrays([(0, 2)], 0.8, True), lambda: m.train()):
        with pytest.raises(AssertionError, match="touched the device"):
            call()
    m.clear()
    assert m.empty()
    m.add([np.zeros((3, 128), np.float32)])          # clear resets the kind
    assert len(m.getTrainDescriptors()) == 1


def test_torchmatch_refusals_come_before_the_library(monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the library")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(torchmatch, "_ctx_for", no_device)
    coll = torchmatch.Collection()
    with pytest.raises(ValueError, match="CUDA tensor"):
        coll.add_wide(torch.zeros((4, 256)))
    assert coll._coll is None and not coll._wide
    coll._wide = True                                 # what the first add_wide leaves behind
    x = torch.zeros((4, 128))
    for call in (lambda: coll.add(x), lambda: coll.knn(x, 2), lambda: coll.ratio_match(x, 0.8), lambda: coll.radius_match(x, 1.0),
                 lambda: coll.fast_match_each(x, 0.8), lambda: coll.mutual_nn_each(x), lambda: coll.mutual_ratio_each(x, 0.8),
                 lambda: coll.mask(4)):
        with pytest.raises(ValueError, match="wide"):
            call()
    assert coll._coll is None
    coll.clear()
    assert not coll._wide
    # add keeps refusing wide rows, and now names add_wide
    with pytest.raises(ValueError, match="wide.*add_wide"):
        torchmatch.Collection().add(torch.zeros((4, 256)))


def test_reference_on_a_hand_worked_case():
    dim = 129

    def rows(*specs):
        a = np.zeros((len(specs), dim), np.float32)
        for i, spec in enumerate(specs):
            for k, v in spec:
                a[i, k] = v
        return a
    A = rows([(0, 1.0)], [(1, 1.0)], [(128, 1.0)])
    B = rows([(1, 1.0), (2, 0.1)], [(0, 1.0)], [(7, 3.0)])
    E = np.zeros((0, dim), np.float32)
    images = [A, B, E]
    # a0 = b1 exactly; a1 has b0 at 0.1; a2 is sqrt(2) from b1 and sqrt(2.01) from b0: its ratio 0.9975 fails at 0.8, and at
    # tau = inf it is not mutual (b1's nearest row of A is a0)
    for tau in (0.8, float("inf")):
        for sym in (False, True):
            (q, t, d, r), = ref.pairs_mutual_ratio(images, [(0, 1)], tau, sym)
            assert q.tolist() == [0, 1] and t.tolist() == [1, 0]
            assert d[0] == 0 and abs(float(d[1]) - 0.1) < 1e-7
            # a1: second neighbour b1 at sqrt(2); b0's own second neighbour is at sqrt(2.01): the forward ratio is the larger
            assert r[0] == 0 and abs(r[1] - 0.1 / np.sqrt(2.0)) < 1e-6
    # the reverse pair: b0 -> a1, b1 -> a0; b2 is 3.16 from every row of A, ratio 1: never accepted below tau = 1
    (q, t, d, r), = ref.pairs_mutual_ratio(images, [(1, 0)], 0.8)
    assert q.tolist() == [0, 1] and t.tolist() == [1, 0]
    # a == b: every row is its own nearest neighbour at distance 0
    (q, t, d, r), = ref.pairs_mutual_ratio(images, [(0, 0)], 0.8, True)
    assert q.tolist() == t.tolist() == [0, 1, 2] and (d == 0).all()
    # empty images accept nothing, on either side; NULL pairs are every a < b
    per = ref.pairs_mutual_ratio(images, None, 0.8)
    assert [p[0].shape[0] for p in per] == [2, 0, 0] and ref.all_pairs(3) == [(0, 1), (0, 2), (1, 2)]
    memo = {}
    again = ref.pairs_mutual_ratio(images, [(0, 1), (0, 1)], 0.8, memo=memo)
    assert len(memo) == 1 and again[0] is again[1]
    offsets, rows_written, cols = ref.pack(per + per, 3)
    assert offsets.tolist() == [0, 2, 2, 2, 4, 4, 4] and rows_written == 2 and cols[0].tolist() == [0, 1]


def test_planted_views_are_found_by_the_reference():
    """The data of the GPU test: image 4 (129 rows) holds 43 views of rows of image 5 (1000 rows)."""
    for dim in (129, 256):
        images = ref.images([0, 1, 127, 128, 129, 1000, 5, 0], dim, 7100 + dim, big=5)
        (q, t, d, r), = ref.pairs_mutual_ratio(images, [(4, 5)], 0.8, True)
        assert q.shape[0] >= 10
        assert all(np.allclose(np.linalg.norm(im, axis=1), 1.0, atol=1e-5) for im in images if im.shape[0])
