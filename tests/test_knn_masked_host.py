"""CPU: the surface of knnMatch masks (fm_mask_*, fm_knn_masked, fm_knn_masked_dev, fm_collection_knn_masked,
fm_collection_knn_masked_dev -- additions to ABI revision 12): declared, exported and bound with matching prototypes; the
NumPy reference of tests/masked_ref.py packs and unpacks the bit layout and equals ``oracle.bf_knn`` under an all-ones mask;
the header's "Not built" lists say what is left; matchutil's mask checks fire before a context exists."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                       # noqa: E402
import masked_ref as R              # noqa: E402
import hamming_ref as H             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fm_mask_create": 4, "fm_mask_create_coll": 4, "fm_mask_set_u8": 5, "fm_mask_set_dev": 6, "fm_mask_set_all": 4,
       "fm_mask_destroy": 2, "fm_mask_info": 5, "fm_knn_masked": 7, "fm_knn_masked_dev": 8, "fm_collection_knn_masked": 8,
       "fm_collection_knn_masked_dev": 9}


def _header_text():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


def test_declared_exported_and_bound_at_revision_12():
    text = _header_text()
    head = text[:text.index("#define FM_ABI_VERSION")]
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", text).group(1)) == 12 == _ffi.FM_ABI_VERSION
    lib = _ffi.load_library()
    assert lib.fm_abi_version() == 12
    for name in NEW:
        assert name in head, "%s is not named in the revision comment" % name
        assert name in _ffi.SYMBOLS and hasattr(lib, name)
    for cls, names in ((_ffi.Mask, ("set", "set_dev", "set_all", "close", "__enter__", "__exit__")),
                       (_ffi.Context, ("mask", "knn_masked", "knn_masked_dev")),
                       (_ffi.Collection, ("mask", "knn_masked", "knn_masked_dev"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def test_prototypes_match_the_binding():
    hdr = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    want = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}
    for name, count in NEW.items():
        params = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1).split(",")
        argtypes = _ffi.SYMBOLS[name][1]
        assert _ffi.SYMBOLS[name][0] is ctypes.c_int
        assert len(params) == len(argtypes) == count, name
        for p, t in zip(params, argtypes):
            p = " ".join(p.split())
            if "*" in p:
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, p, t)
            else:
                assert t is want[p.replace("const ", "").split()[0]], (name, p, t)


def test_pack_unpack_round_trip_in_the_masks_layout():
    rng = np.random.default_rng(5)
    for nq, nt in [(1, 1), (3, 63), (3, 64), (3, 65), (2, 128), (2, 129), (5, 1100)]:
        m = (rng.random((nq, nt)) < 0.4).astype(np.uint8)
        w = R.pack(m)
        assert w.dtype == np.uint64 and w.shape == (nq, R.pad128(nt) // 64)
        assert np.array_equal(R.unpack(w, nt), m)
        assert np.array_equal(R.pack(m.astype(bool)), w)
        # bit b of word w is train row 64 w + b, and nothing is set at or beyond nt
        for i in range(nq):
            for j in range(nt):
                assert ((int(w[i, j >> 6]) >> (j & 63)) & 1) == m[i, j]
        total = sum(bin(int(x)).count("1") for x in w.reshape(-1))
        assert total == int(m.sum())
    one = np.zeros((1, 130), np.uint8)
    one[0, 129] = 1
    assert R.pack(one).tolist() == [[0, 0, 2, 0]]


def test_reference_under_an_all_ones_mask_is_the_oracle():
    rng = np.random.default_rng(6)
    Q, T = synth.synth_sift(37, rng), synth.synth_sift(301, rng)
    ones = np.ones((37, 301), np.uint8)
    for k in (1, 2, 5):
        ri, rd = R.knn_u8(Q, T, ones, k)
        oi, od = oracle.bf_knn(Q, T, k)
        assert np.array_equal(ri, oi) and np.array_equal(rd.view(np.uint32), od.view(np.uint32))
    Qf = (Q[:9] + rng.uniform(-0.5, 0.5, (9, 128))).astype(np.float32)
    Tf = (T + rng.uniform(-0.5, 0.5, T.shape)).astype(np.float32)
    ri, rd = R.knn_f32(Qf, Tf, ones[:9], 3)
    oi, od = oracle.bf_knn(Qf, Tf, 3, order=1)
    assert np.array_equal(ri, oi) and np.array_equal(rd.view(np.uint32), od.view(np.uint32))
    Qb, Tb = rng.integers(0, 256, (11, 32), dtype=np.uint8), rng.integers(0, 256, (90, 32), dtype=np.uint8)
    ri, rd = R.knn_bin(Qb, Tb, np.ones((11, 90), np.uint8), 4)
    hi, hd = H.knn(Qb, Tb, 4)
    assert np.array_equal(ri, hi) and np.array_equal(rd.view(np.uint32), np.asarray(hd, np.float32).view(np.uint32))
    # fewer permitted rows than k: the tail is -1 / +inf; none: the whole row
    m = np.zeros((2, 301), np.uint8)
    m[0, 7] = 1
    ri, rd = R.knn_u8(Q[:2], T, m, 2)
    assert ri.tolist() == [[7, -1], [-1, -1]] and np.isinf(rd[0, 1]) and np.isinf(rd[1]).all()


def test_not_built_lists_name_what_is_left():
    text = " ".join(re.sub(r"\n \*", " ", _header_text()).split())
    for left in ("masks on the fp16-filter (K8) and FP4 (K11) matrix-core sweeps", "masked crossCheck", "masked radiusMatch",
                 "masked ratio / mutual-ratio / accepted-match calls", "masks in the _each forms"):
        assert left in text, left
    coll = text[text.index("Not built: the STACKED crossCheck on a collection"):text.index("typedef struct fm_collection fm_collection;")]
    assert "counts-then-fill pattern, masks, the expansion loop" not in coll          # plain `masks` is gone from the list
    assert "fm_collection_knn_masked is built" in coll
    for kept in ("Hamming radiusMatch (for pairs or collections)", "an _each form", "skipping the second count sweep",
                 "sharding a collection across GPUs"):
        assert kept in coll, kept
    assert "recalled, not verified" in text.lower() or "RECALLED, not verified" in text
    assert "NOT on the matrix cores" in text and "MATRIX CORES" in text


def _untouchable(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("a refusal reached the device")

    monkeypatch.setattr(matchutil, "_context", touched)
    monkeypatch.setattr(_ffi, "default_context", touched)
    monkeypatch.setattr(_ffi, "load_library", touched)


def test_matchutil_mask_checks_fire_before_a_context_exists(monkeypatch):
    _untouchable(monkeypatch)
    q, t = np.zeros((3, 128), np.uint8), np.zeros((5, 128), np.uint8)
    ok = np.ones((3, 5), np.uint8)
    for bad in (np.ones((3, 4), np.uint8), np.ones((5, 3), np.uint8), np.ones(15, np.uint8), np.ones((3, 5), np.float32)):
        for call in (matchutil.bf_match, matchutil.bf_match_arrays, matchutil.flann_match, matchutil.flann_match_arrays):
            with pytest.raises(ValueError, match="mask"):
                call(q, t, k=2, options={"mask": bad})
    with pytest.raises(ValueError, match="crossCheck"):
        matchutil.bf_match(q, t, k=1, options={"mask": ok, "crossCheck": True})
    with pytest.raises(ValueError, match="radiusMatch"):
        matchutil.bf_radius_match(q, t, 3.0, options={"mask": ok})
    with pytest.raises(ValueError, match="ratio"):
        matchutil.ratio_match_arrays(q, t, 0.8, options={"mask": ok})
    m = matchutil.BFMatcher()
    m.add([t, t[:2]])
    with pytest.raises(ValueError, match="2 images"):
        m.knnMatch(q, k=2, masks=[ok])
    with pytest.raises(ValueError, match=r"masks\[1\]"):
        m.knnMatch(q, k=2, masks=[None, ok])
    with pytest.raises(ValueError, match="train argument"):
        m.knnMatch(q, k=2, mask=ok)
    with pytest.raises(ValueError, match="train collection"):
        m.knnMatch(q, t, k=2, masks=[ok])
    x = matchutil.BFMatcher(crossCheck=True)
    x.add([t])
    with pytest.raises(ValueError, match="crossCheck"):
        x.match(q, masks=[ok])
    resident = _ffi.Mask.__new__(_ffi.Mask)              # a resident Mask is refused with crossCheck as an array is
    resident.ctx, resident.handle, resident.coll = None, None, None
    for k in (1, 2):
        with pytest.raises(ValueError, match="crossCheck"):
            x.knnMatch(q, k=k, masks=resident)
