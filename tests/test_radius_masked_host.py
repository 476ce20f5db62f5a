"""CPU: the surface of masked radiusMatch (fm_radius_match_masked, fm_radius_match_masked_dev,
fm_collection_radius_match_masked, fm_collection_radius_match_masked_dev -- additions to ABI revision 12): declared, exported
and bound with matching prototypes; the reference of tests/radius_masked_ref.py passes its own checks and the masks the GPU
tests use keep some, and not all, of the unmasked hits on every data set; the header's "Not built" sentences stand; matchutil's
refusals fire before a context exists; the Python layers expose the new names and keywords."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil, torchmatch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radius_masked_ref as M       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fm_radius_match_masked": 11, "fm_radius_match_masked_dev": 12, "fm_collection_radius_match_masked": 12,
       "fm_collection_radius_match_masked_dev": 13}


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


def test_prototypes_match_the_binding_and_their_unmasked_namesakes():
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
        # the unmasked namesake's list with `const fm_mask* mask` behind the train operand (the third handle)
        base = _ffi.SYMBOLS[name.replace("_masked", "")][1]
        assert argtypes[:3] + argtypes[4:] == base and argtypes[3] is ctypes.c_void_p, name
        assert " ".join(params[3].split()) == "const fm_mask* mask", name


def test_the_not_built_sentences_stand():
    text = " ".join(_header_text().replace("\n *", " ").split())
    for s in ("masked crossCheck", "masked radiusMatch", "masked Hamming radius queries", "radiusMatch, masks, k >= 3", "Not built: masks;"):
        assert s in text, s
    sec = text[text.index("---- Masked radiusMatch"):text.index("---- Wide stacked knnMatch")]
    tail = sec[sec.index("Not built:"):]
    for s in ("masks on a wide collection", "masked crossCheck, ratio, mutual-ratio and accepted-match calls", "compactResult in the C ABI"):
        assert s in tail, s
    assert "recalled, not verified" in sec and 'says "wide"' in sec


def test_the_reference_passes_its_own_checks():
    for name in ("i8", "ham32", "wide129"):
        ref = M.ref(name)
        for what, r in M.radii(name) + [("inf", np.float32(np.inf))]:
            cut = ref.cut(r)
            ones = M.filtered(cut, M.mask("ones"))
            for a, b in zip(ones, cut):
                assert np.array_equal(a, b, equal_nan=True), (name, what)
            zeros = M.filtered(cut, M.mask("zeros"))
            assert not zeros[0].any() and all(x.size == 0 for x in zeros[1:]), (name, what)
        # the bit walk at r = +inf: row i lists exactly the train rows congruent to i modulo 64
        off, _, _, dist, glob = M.want(name, np.float32(np.inf), M.mask("walk"))
        fin = np.isfinite(ref.sorted if M.kind(name) == "ham" else ref.dist).all()
        for i in (0, 1, 63, 64, 299):
            got = np.sort(glob[off[i]:off[i + 1]])
            assert (got % 64 == i % 64).all()
            if fin:
                assert np.array_equal(got, np.arange(i % 64, M.NT, 64))


@pytest.mark.parametrize("name", M.PAIR_SETS)
def test_the_masks_keep_some_and_not_all_of_the_hits(name):
    """0 < kept < unmasked hits for every data set x (random, band, third) mask and every radius the GPU tests use: no test
    passes on empty lists, and none on a mask that removes nothing."""
    ref = M.ref(name)
    for what, r in M.radii(name):
        cut = ref.cut(r)
        hits = int(cut[0][-1])
        for pattern in ("random", "band", "third"):
            kept = int(M.filtered(cut, M.mask(pattern))[0][-1])
            print(name, what, pattern, "kept", kept, "of", hits)
            assert 0 < kept < hits, (name, what, pattern, kept, hits)
        if name in M.COLL_SETS:
            for pattern in ("random", "band"):
                kept = int(M.filtered(cut, M.coll_mask(pattern))[0][-1])
                assert 0 < kept < hits, (name, what, pattern, "collection", kept, hits)


def test_mask_patterns():
    assert M.NT == sum(M.SIZES) == 32 * 64 + 52 and M.NQ % 64 and M.NQ % 128 and M.NQ % 256
    assert abs(M.mask("random").mean() - 0.5) < 0.01
    band = M.mask("band")
    assert (band.sum(axis=1) == M.BAND).all()
    words = np.add.reduceat(band, np.arange(0, M.NT, 64), axis=1) > 0
    assert words.sum(axis=1).max() <= 2 and words.shape[1] == 33          # at most two of 33 words per row are non-zero
    assert M.mask("first").sum() == M.NQ == M.mask("last").sum() and M.mask("last")[:, M.NT - 1].all()
    assert not M.mask("third")[0::3].any() and M.mask("third")[1::3].any()
    per = M.per_image(M.coll_mask("random"))
    assert per[M.IMG_ALL] is None and not per[M.IMG_NONE].any() and [p.shape[1] for p in per if p is not None] == [700, 1, 0, 1269]


def _untouchable(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("a refusal reached the device")

    monkeypatch.setattr(matchutil, "_context", touched)
    monkeypatch.setattr(_ffi, "default_context", touched)
    monkeypatch.setattr(_ffi, "load_library", touched)


class _CollMask(_ffi.Mask):
    """A resident collection Mask as matchutil sees one, without a device behind it."""
    def __init__(self, nq, nt):
        self.nq, self.nt, self.n_images, self.handle, self.ctx = nq, nt, 2, None, None

    def close(self):
        pass


def test_matchutil_refusals_fire_before_a_context_exists(monkeypatch):
    _untouchable(monkeypatch)
    ok = np.ones((3, 5), np.uint8)
    operands = [(np.zeros((3, 128), np.uint8), np.zeros((5, 128), np.uint8), {}),
                (np.zeros((3, 128), np.float32), np.zeros((5, 128), np.float32), {}),
                (np.zeros((3, 32), np.uint8), np.zeros((5, 32), np.uint8), {"normType": matchutil.NORM_HAMMING}),
                (np.zeros((3, 200), np.float32), np.zeros((5, 200), np.float32), {})]
    for q, t, opts in operands:
        for call in (matchutil.bf_radius_match_masked, matchutil.bf_radius_match_masked_arrays):
            for bad in (np.ones((3, 4), np.uint8), np.ones((5, 3), np.uint8), np.ones(15, np.uint8)):      # a wrong shape
                with pytest.raises(ValueError, match="mask"):
                    call(q, t, 3.0, bad, options=opts)
            with pytest.raises(ValueError, match="uint8 or bool"):                                          # a wrong dtype
                call(q, t, 3.0, np.ones((3, 5), np.float32), options=opts)
            with pytest.raises(ValueError, match="of a collection"):                                        # a collection's Mask
                call(q, t, 3.0, _CollMask(3, 5), options=opts)
            with pytest.raises(ValueError, match="mask is None"):
                call(q, t, 3.0, None, options=opts)
            with pytest.raises(ValueError, match="radii"):
                call(q, t, np.ones(4, np.float32), ok, options=opts)
    with pytest.raises(ValueError, match="values per query row"):
        matchutil.bf_radius_match_masked(np.zeros((3, 200), np.float32), np.zeros((5, 129), np.float32), 1.0, ok)
    with pytest.raises(ValueError, match="bytes per query row"):
        matchutil.bf_radius_match_masked(np.zeros((3, 32), np.uint8), np.zeros((5, 16), np.uint8), 1.0, ok,
                                         options={"normType": matchutil.NORM_HAMMING})
    # the old call keeps its refusal
    with pytest.raises(ValueError, match="radiusMatch"):
        matchutil.bf_radius_match(np.zeros((3, 128), np.uint8), np.zeros((5, 128), np.uint8), 3.0, options={"mask": ok})
    m = matchutil.BFMatcher()
    with pytest.raises(ValueError, match="collection"):
        m.radiusMatch(np.zeros((3, 128), np.uint8), 3.0, mask=ok)
    with pytest.raises(ValueError, match="mask"):
        m.radiusMatch(np.zeros((3, 128), np.uint8), np.zeros((5, 128), np.uint8), 3.0, mask=np.ones((3, 4), np.uint8), compactResult=True)


def test_the_python_layers_expose_the_new_names_and_keywords():
    for cls, names in ((_ffi.Context, ("radius_match_masked", "radius_match_masked_dev")),
                       (_ffi.Collection, ("radius_match_masked", "radius_match_masked_dev"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert list(inspect.signature(_ffi.Context.radius_match_masked).parameters)[1:] == ["q", "t", "mask", "r"]
    assert list(inspect.signature(_ffi.Collection.radius_match_masked).parameters)[1:] == ["q", "mask", "r"]
    assert callable(matchutil.bf_radius_match_masked) and callable(matchutil.bf_radius_match_masked_arrays)
    assert list(inspect.signature(matchutil.bf_radius_match_masked_arrays).parameters) == ["dt1", "dt2", "maxDistance", "mask", "options"]
    p = inspect.signature(matchutil.BFMatcher.radiusMatch).parameters
    assert p["mask"].default is None and p["compactResult"].default is False
    for f in (torchmatch.radius_match, torchmatch.hamming_radius_match, torchmatch.wide_radius_match):
        assert inspect.signature(f).parameters["mask"].default is None, f
    for f in (torchmatch.Collection.radius_match, torchmatch.Collection.hamming_radius_match):
        assert inspect.signature(f).parameters["masks"].default is None, f
