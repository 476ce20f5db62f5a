"""CPU: the host side of radiusMatch on wide float descriptors (FM_BANK_F32W) -- the four new prototypes of the header against
the ctypes binding and their L2 namesakes, the ABI revision they leave alone, the header's new section, the ValueErrors of
matchutil / torchmatch that are raised before anything is uploaded, the reference's cut rules by hand, the margin of the wide
threshold sweep on planted worst-case rounding pairs (tests/f16_margin_ref.py, no GPU) and (hipcc cross-compiles) the
registers and scratch of the eight instantiations of radius_wide_kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

import f16_margin_ref as F
import isa_read as R
import wide_radius_ref as WR
from fastmatch_amd import _ffi, matchutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fm_wide_radius_match", "fm_wide_radius_match_dev", "fm_collection_wide_radius_match",
       "fm_collection_wide_radius_match_dev")
L2 = {"fm_wide_radius_match": "fm_radius_match", "fm_wide_radius_match_dev": "fm_radius_match_dev",
      "fm_collection_wide_radius_match": "fm_collection_radius_match",
      "fm_collection_wide_radius_match_dev": "fm_collection_radius_match_dev"}


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
    if re.search(r"\bfloat\b", p):
        return "f32"
    if re.search(r"\b(int64_t|uint64_t)\b", p):
        return "i64"
    raise AssertionError("unclassified parameter: " + p)


def _klass_of_ctype(t):
    if t is ctypes.c_void_p or hasattr(t, "contents"):
        return "ptr"
    return {ctypes.c_float: "f32", ctypes.c_int64: "i64"}[t]


@pytest.mark.parametrize("name", NEW)
def test_new_prototypes_match_the_binding_and_their_l2_namesakes(name):
    protos = dict(re.findall(r"\bint\s+(fm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S), flags=re.S))
    assert name in protos, "the header does not declare %s" % name
    texts = protos[name].split(",")
    res, argtypes = _ffi.SYMBOLS[name]
    assert res is ctypes.c_int and len(texts) == len(argtypes)
    assert [_klass_of_text(p) for p in texts] == [_klass_of_ctype(t) for t in argtypes]
    # the argument list is the L2 call's, word for word, and so is the binding's
    norm = lambda p: " ".join(p.split())                  # noqa: E731
    assert [norm(p) for p in texts] == [norm(p) for p in protos[L2[name]].split(",")]
    assert _ffi.SYMBOLS[name] == _ffi.SYMBOLS[L2[name]]
    assert hasattr(_ffi.load_library(), name)


def test_abi_revision_and_header_section():
    hdr = _header()
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    comment = _prose(hdr.split("#define FM_ABI_VERSION")[0])
    assert "still revision 12, additions only -- " + ", ".join(NEW) in comment
    assert hdr.index("---- Wide Fast-Match") < hdr.index("---- Wide radiusMatch") < hdr.index("---- train collections")
    sect = _prose(hdr.split("---- Wide radiusMatch")[1].split("int fm_wide_radius_match")[0])
    for rule in ("fm_radius_match's contract applies word for word", "sqrtf(s), s = fmaf(v_k, v_k, s)", "k ascending over the real dim",
                 "dist(i, j) < r_i, a strict float32 compare", "A NaN or +inf distance is never listed, not even at r = +inf",
                 "r <= 0 or NaN gives an empty list", "(distance bits, train index)", "No option changes a result", '"radius_ws_bytes"',
                 "keep refusing wide banks and wide collections", "v_mfma_f32_16x16x32_f16", "two blocks of 16 query rows",
                 "1.25 * 2^-10", "kept out by INDEX", "read at the call", "fm_f32_filter_stats", "scale exponents differ by more than 8",
                 "FM_EINVAL, even when it is empty", "fm_radius_match or fm_hamming_radius_match", "all-zero offsets",
                 "nq * real rows", "the _dev forms are not accounted"):
        assert rule in sect, rule
    # the L2-named calls keep refusing: the earlier "Not built" sentences are still there, with a pointer to the new names
    k14 = _prose(hdr.split("---- K14: wide float banks")[1].split("int  fm_bank_destroy")[0])
    assert "fm_radius_match(_dev)" in k14.split("Not built for wide float banks:")[1]
    assert "fm_collection_radius_match(_dev)" in k14.split("Not built for wide collections:")[1]
    assert k14.count('"Wide radiusMatch" below') == 3
    fast = _prose(hdr.split("---- Wide Fast-Match")[1].split("int fm_wide_self_dist")[0])
    assert "radiusMatch, masks, k >= 3" in fast.split("Not built:")[1] and '"Wide radiusMatch" below' in fast


def test_python_layers_expose_the_calls():
    for k, names in ((_ffi.Context, ("wide_radius_match", "wide_radius_match_dev")),
                     (_ffi.Collection, ("wide_radius_match", "wide_radius_match_dev"))):
        for n in names:
            assert callable(getattr(k, n)), n
    assert callable(matchutil.wide_radius_match) and callable(matchutil.wide_radius_match_arrays)
    from fastmatch_amd import torchmatch
    assert callable(torchmatch.wide_radius_match) and callable(torchmatch.Collection.wide_radius_match)


# ---- refusals that touch no device -----------------------------------------------------------------------------------------
class _NoContext(object):
    handle = None

    def __init__(self):
        self._children = set()


def _bank(kind, n=4, dim=256):
    return _ffi.Bank(_NoContext(), None, n, dim, kind)


def test_matchutil_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    monkeypatch.setattr(_ffi, "default_context", no_device)
    w256, w200 = np.zeros((4, 256), np.float32), np.zeros((5, 200), np.float32)
    for fn in (matchutil.wide_radius_match_arrays, matchutil.wide_radius_match):
        for dim in (128, 257, 32):                                              # other widths
            with pytest.raises(ValueError, match="129 .. 256 values per row"):
                fn(np.zeros((4, dim), np.float32), np.zeros((4, dim), np.float32), 1.0)
        for bad in (w256.astype(np.uint8), np.zeros((4, 200), np.uint8), w256.astype(np.int32)):      # uint8 rows
            with pytest.raises(ValueError, match="float32 / float64"):
                fn(bad, w256, 1.0)
            with pytest.raises(ValueError, match="float32 / float64"):
                fn(w256, bad, 1.0)
        with pytest.raises(ValueError, match="256 values per query row, 200 per train row"):      # widths that differ
            fn(w256, w200, 1.0)
        with pytest.raises(ValueError, match="256 values per query row, 200 per train row"):
            fn(_bank(_ffi.FM_BANK_F32W, 4, 256), _bank(_ffi.FM_BANK_F32W, 5, 200), 1.0)
        with pytest.raises(ValueError, match="mask"):                            # a mask option
            fn(w256, w256, 1.0, options={"mask": np.ones((4, 4), np.uint8)})
        for radii in (np.ones(3, np.float32), np.ones(5, np.float32), np.ones((2, 4), np.float32)):    # a wrong number of radii
            with pytest.raises(ValueError, match="radii for 4 query rows"):
                fn(w256, w256, radii)
        with pytest.raises(ValueError, match="radii for 4 query rows"):
            fn(_bank(_ffi.FM_BANK_F32W), w256, np.ones(7, np.float32))
        with pytest.raises(ValueError, match="wide float banks"):                # resident banks of another kind
            fn(_bank(_ffi.FM_BANK_F32, 4, 128), w256, 1.0)
        with pytest.raises(ValueError, match="2-D"):
            fn(np.zeros(256, np.float32), w256, 1.0)
        # what is served reaches the device
        with pytest.raises(AssertionError, match="touched the device"):
            fn(w256, w256.astype(np.float64), np.ones(4, np.float32))
    # the L2-named calls keep refusing wide operands
    with pytest.raises(ValueError, match="wide"):
        matchutil.bf_radius_match(w256, w256, 1.0)


def test_torchmatch_refusals_come_before_the_library(monkeypatch):
    torch = pytest.importorskip("torch")
    from fastmatch_amd import torchmatch

    def no_library(*a, **k):
        raise AssertionError("a refusal touched the library")
    monkeypatch.setattr(torchmatch, "bank", no_library)
    monkeypatch.setattr(_ffi, "default_context", no_library)
    monkeypatch.setattr(torchmatch, "_ctx_for", no_library)
    w256, w200 = torch.zeros((4, 256)), torch.zeros((4, 200))
    with pytest.raises(ValueError):
        torchmatch.wide_radius_match(w256, w256, 1.0)                            # CPU tensors
    with pytest.raises(ValueError):
        torchmatch.wide_radius_match(torch.zeros((4, 256), dtype=torch.uint8), w256, 1.0)
    with pytest.raises(ValueError):
        torchmatch.wide_radius_match(w256, w200, 1.0)
    qb, tb = _bank(_ffi.FM_BANK_F32W, 4, 256), _bank(_ffi.FM_BANK_F32W, 5, 200)
    with pytest.raises(ValueError, match="256 values per query row, 200 per train row"):
        torchmatch.wide_radius_match(qb, tb, 1.0)
    with pytest.raises(ValueError, match="wide float banks"):
        torchmatch.wide_radius_match(_bank(_ffi.FM_BANK_F32, 4, 128), qb, 1.0)
    with pytest.raises(ValueError, match="not a wide one"):
        torchmatch.Collection().wide_radius_match(qb, 1.0)
    # the L2-named calls keep refusing wide operands
    with pytest.raises(ValueError, match="wide"):
        torchmatch.radius_match(qb, qb, 1.0)


# ---- the reference, by hand ------------------------------------------------------------------------------------------------
def _rows(*rows, dim=130):
    out = np.zeros((len(rows), dim), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def test_reference_cut_rules_by_hand():
    Q = _rows([0, 0], [np.nan, 0], [3.0e38, 0])
    T = _rows([3, 4], [0, 1], [0, 1], [np.inf, 0], [-1.0e18, 0], [0, 0])
    ref = WR.Ref(Q, [T])
    # row 0: distances 5, 1, 1, inf, 1e18, 0; the strict compare; ties by index; inf never listed
    off, _, _, dist, idx = ref.cut(np.float32(5.0))
    assert idx[off[0]:off[1]].tolist() == [5, 1, 2] and dist[off[0]:off[1]].tolist() == [0.0, 1.0, 1.0]
    off, _, _, dist, idx = ref.cut(np.nextafter(np.float32(5.0), np.float32(np.inf)))
    assert idx[off[0]:off[1]].tolist() == [5, 1, 2, 0]
    off, _, _, dist, idx = ref.cut(np.float32(np.inf))
    assert idx[off[0]:off[1]].tolist() == [5, 1, 2, 0, 4]                     # not row 3 (+inf), at r = +inf either
    assert off[2] == off[1]                                                     # a NaN query row lists nothing
    assert off[3] == off[2]                                                     # row 2: every squared difference overflows to +inf
    for r in (0.0, -1.0, np.nan):
        assert not ref.cut(np.float32(r))[0].any()
    off = ref.cut(np.array([1.0, np.inf, 0.0], np.float32))[0]
    assert off.tolist() == [0, 1, 1, 1]
    # a collection: global rows become (image, row inside the image), an empty image in between
    c = WR.Ref(Q, [T[:2], T[:0], T[2:]])
    off, img, loc, dist, idx = c.cut(np.float32(np.inf))
    assert img[off[0]:off[1]].tolist() == [2, 0, 2, 0, 2] and loc[off[0]:off[1]].tolist() == [3, 1, 0, 0, 2]
    assert WR.Ref(Q[:0], [T]).cut(1.0)[0].tolist() == [0] and WR.Ref(Q, [T[:0]]).cut(1.0)[0].tolist() == [0, 0, 0, 0]
    assert [(d + 31) // 32 for d in WR.DIMS] == [WR.KSTEPS[d] for d in WR.DIMS] and sorted(set(WR.KSTEPS.values())) == [5, 6, 7, 8]


# ---- the margin, from below ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [129, 160, 161, 192, 255, 256])
def test_planted_threshold_pairs_need_the_whole_margin(dim):
    """The planted hits (both rows round DOWN in fp16: A16 exceeds the exact d2 by ~2^-10 (|q|^2 + |t|^2)) sit at 0.78 of
    K14's M = 1.25 * 2^-10 (|q'|^2 + max |t'|^2): kept by the sweep's test A <= r^2 + M, lost under half the margin -- a
    sweep with too small a constant, or with K steps that drop products, fails the GPU test on these rows."""
    p = F.radius_set(dim)
    r, fractions = F.check_threshold(p, eps=F.EPS_K14, floor=0.75)
    rep = F.threshold_report(p, F.EPS_K14)
    hits = [h for f, h in zip(p.fams, rep) if f["kind"] == "hit"]
    print("dim", dim, "r", float(r), "fractions of M", ["%.4f" % x for x in fractions])
    assert len(hits) == 9 and all(0.75 <= x < 1.0 for x in fractions)
    for h in hits:
        assert F.within(h["A16"], float(r) ** 2, h["M"], 1.0)
        assert not F.within(h["A16"], float(r) ** 2, h["M"], 0.5)


# ---- the eight instantiations of the sweep -------------------------------------------------------------------------------
@pytest.mark.skipif(not R.have_hipcc(), reason="needs hipcc to cross-compile csrc/radius.hip")
def test_wide_sweep_instantiations_have_no_scratch_and_no_spills(tmp_path_factory):
    md = R.metadata(R.isa("radius", tmp_path_factory))
    wide = {n: m for n, m in md.items() if re.match(r"_ZN2fm\d+radius_wide_kernelI", n)}
    assert sorted(re.search(r"ILb([01])ELi(\d)E", n).groups() for n in wide) == sorted((f, str(k)) for f in "01" for k in (5, 6, 7, 8))
    for n, m in wide.items():
        print(n, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, n
        assert m["group_segment_fixed_size"] == 0, n             # the streamed rows come straight from memory: no LDS
        assert m["vgpr_count"] <= 256, n                          # two waves per SIMD
    for base in ("radius_wide_rescore_kernel", "radius_wide_limits_kernel"):
        (m,) = [m for n, m in md.items() if re.match(r"_ZN2fm\d+%sE" % base, n)]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0
    text = R.isa("radius", tmp_path_factory)
    body = text.split("_ZN2fm18radius_wide_kernelILb0ELi8EEEvNS_6RSweepE:")[1].split(".Lfunc_end")[0]
    assert body.count("v_mfma_f32_16x16x32_f16") >= 2 * 8 and "ds_read" not in body and "s_barrier" not in body
