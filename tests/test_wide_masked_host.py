"""CPU: the host side of knnMatch masks on wide float banks (fm_wide_knn_masked, fm_wide_knn_masked_dev -- additions to ABI
revision 12): the prototypes against the ctypes binding and against fm_knn_masked's, word for word; the header's new section
and every older "Not built" sentence; the ValueErrors of matchutil / torchmatch that are raised before anything reaches the
library; the NumPy reference (tests/wide_masked_ref.py) on a hand-worked case; and (hipcc cross-compiles) the registers,
scratch and instantiations of the new unit's kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

import isa_read as R
import wide_masked_ref as WM
from fastmatch_amd import _ffi, matchutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fm_wide_knn_masked", "fm_wide_knn_masked_dev")
NAMESAKE = {"fm_wide_knn_masked": "fm_knn_masked", "fm_wide_knn_masked_dev": "fm_knn_masked_dev"}


def _header():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


def _prose(comment):
    """A block comment's text on one line, without the ' * ' that starts its lines."""
    return " ".join(re.sub(r"\n\s*\*\s?", " ", comment).split())


def _klass_of_text(p):
    p = " ".join(p.split())
    if "*" in p:
        return "ptr"
    if re.search(r"\b(int64_t|uint64_t)\b", p):
        return "i64"
    if re.search(r"\b(int32_t|int)\b", p):
        return "i32"
    raise AssertionError("unclassified parameter: " + p)


def _klass_of_ctype(t):
    if t is ctypes.c_void_p or hasattr(t, "contents"):
        return "ptr"
    return {ctypes.c_int64: "i64", ctypes.c_int: "i32", ctypes.c_int32: "i32"}[t]


# ---- header and binding ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW)
def test_prototypes_match_the_binding_and_their_namesakes(name):
    bare = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(fm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", bare, flags=re.S))
    assert name in protos, "the header does not declare %s" % name
    texts = protos[name].split(",")
    res, argtypes = _ffi.SYMBOLS[name]
    assert res is ctypes.c_int and len(texts) == len(argtypes)
    assert [_klass_of_text(p) for p in texts] == [_klass_of_ctype(t) for t in argtypes]
    norm = lambda p: " ".join(p.split())                  # noqa: E731
    assert [norm(p) for p in texts] == [norm(p) for p in protos[NAMESAKE[name]].split(",")]      # word for word
    assert _ffi.SYMBOLS[name] == _ffi.SYMBOLS[NAMESAKE[name]]
    assert hasattr(_ffi.load_library(), name)


def test_abi_revision_and_header_section():
    hdr = _header()
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    head = _prose(hdr.split("#define FM_ABI_VERSION")[0])
    assert "still revision 12, additions only -- fm_wide_knn_masked, fm_wide_knn_masked_dev" in head
    # the section sits behind the last masked prototype and in front of the ratio calls
    assert hdr.index("int  fm_collection_knn_masked_dev(") < hdr.index("---- Wide knnMatch masks") < hdr.index("int  fm_wide_knn_masked(") \
        < hdr.index("int  fm_knn2_ratio(")
    sect = _prose(hdr.split("---- Wide knnMatch masks")[1].split("int  fm_wide_knn_masked(")[0])
    for rule in ("PERMITTED train rows of row i only", "sqrtf(s), s = fmaf(v_k, v_k, s)", "lowest permitted index wins a tie",
                 "-1 / +inf where fewer than k rows are permitted", "A NaN or +inf distance is never listed",
                 "An all-ones mask reproduces fm_knn bit for bit", "nq = 0, nt = 0 and an all-zero mask are valid",
                 "k >= 3 is FM_EUNSUPPORTED", "k < 1 is FM_EINVAL", "No option changes a result", "names fm_knn_masked",
                 "even when it is empty", "a collection's mask", "fm_knn_dev's pointer checks", "fm_f32_filter_stats",
                 "one launch per filtered call and one fallback per call that is redone", "v_mfma_f32_16x16x32_f16",
                 "one 8-byte word per four tiles", "dropped by INDEX", '"f32_filter" 0 / 1 / 2'):
        assert rule in sect, rule
    left = sect.split("Not built:")[1]
    for out_of_scope in ("wide mutual-ratio, ratio, self-distance, radius and collection calls", "k >= 3", "a masked K8 filter for 128-D float banks"):
        assert out_of_scope in left, out_of_scope


def test_every_older_not_built_sentence_is_still_there():
    hdr = _header()
    text = _prose(hdr)
    # K13's list: fm_knn_masked's own routes are what they were
    for kept in ("masks on the fp16-filter (K8) and FP4 (K11) matrix-core sweeps", "masked crossCheck", "masked radiusMatch",
                 "masked ratio / mutual-ratio / accepted-match calls", "masks in the _each forms", "NOT on the matrix cores"):
        assert kept in text, kept
    # K14's lists, the Wide Fast-Match and the Wide radiusMatch sections
    k14 = _prose(hdr.split("---- K14: wide float banks")[1].split("int  fm_bank_destroy")[0])
    assert "fm_knn_masked(_dev)" in k14.split("Not built for wide float banks:")[1]
    fast = _prose(hdr.split("---- Wide Fast-Match")[1].split("int fm_wide_self_dist")[0])
    assert "radiusMatch, masks, k >= 3" in fast.split("Not built:")[1]
    radius = _prose(hdr.split("---- Wide radiusMatch")[1].split("int fm_wide_radius_match(")[0])
    assert "masks" in radius.split("Not built:")[1]


def test_python_layers_expose_the_calls():
    assert callable(_ffi.Context.wide_knn_masked) and callable(_ffi.Context.wide_knn_masked_dev)
    assert callable(matchutil.wide_bf_match_masked) and callable(matchutil.wide_bf_match_masked_arrays)
    from fastmatch_amd import torchmatch
    assert callable(torchmatch.wide_knn_masked)


# ---- refusals that touch no device -----------------------------------------------------------------------------------------
def test_matchutil_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "load_library", no_device)
    q, t = np.zeros((3, 256), np.float32), np.zeros((5, 256), np.float32)
    ok = np.ones((3, 5), np.uint8)
    call = matchutil.wide_bf_match_masked
    for bad in (q.astype(np.uint8), q.astype(np.float16), q.astype(np.int32)):
        with pytest.raises(ValueError, match="float32 / float64"):
            call(bad, t, ok)
        with pytest.raises(ValueError, match="float32 / float64"):
            matchutil.wide_bf_match_masked_arrays(q, np.zeros((5, 256), bad.dtype), ok)
    for dim in (128, 257, 32):
        with pytest.raises(ValueError, match="129 .. 256 values per row"):
            call(np.zeros((3, dim), np.float32), np.zeros((5, dim), np.float32), ok)
    with pytest.raises(ValueError, match="256 values per query row, 200 per train row"):
        call(q, np.zeros((5, 200), np.float32), ok)
    with pytest.raises(ValueError, match="2-D"):
        call(np.zeros(256, np.float32), t, ok)
    for bad in (np.ones((3, 4), np.uint8), np.ones((5, 3), np.uint8), np.ones(15, np.uint8), np.ones((3, 5), np.float32)):
        with pytest.raises(ValueError, match="mask"):
            call(q, t, bad)
    with pytest.raises(ValueError, match="mask is None"):
        call(q, t, None)
    for k in (0, 3, 8):
        with pytest.raises(ValueError, match="k = 1 or 2"):
            call(q, t, ok, k=k)
    # the older entry points keep their refusals
    with pytest.raises(ValueError, match="a mask is not built for wide float descriptors"):
        matchutil.bf_match(q, t, k=2, options={"mask": ok})
    with pytest.raises(ValueError, match="a mask is not built for wide float descriptors"):
        matchutil.bf_match_arrays(q, t, k=1, options={"mask": ok})


def test_torchmatch_refusals_come_before_the_library():
    torch = pytest.importorskip("torch")
    from fastmatch_amd import torchmatch

    def no_library(*a, **k):
        raise AssertionError("a refusal touched the library")
    saved = torchmatch.bank
    torchmatch.bank = no_library
    try:
        w256, w200 = torch.zeros((4, 256)), torch.zeros((4, 200))
        ok = torch.ones((4, 4), dtype=torch.bool)
        with pytest.raises(ValueError, match="k = 1 or 2"):
            torchmatch.wide_knn_masked(w256, w256, 3, ok)
        with pytest.raises(ValueError, match="k = 1 or 2"):
            torchmatch.wide_knn_masked(w256, w256, 0, ok)
        with pytest.raises(ValueError):
            torchmatch.wide_knn_masked(w256, w200, 2, ok)                  # (CPU tensors, and widths that differ)
        with pytest.raises(ValueError):
            torchmatch.wide_knn_masked(torch.zeros((4, 256), dtype=torch.uint8), w256, 2, ok)
        with pytest.raises(ValueError, match="a mask is not built for wide float descriptors"):
            torchmatch.knn(w256, w256, 2, mask=ok)                         # knn keeps its refusal
    finally:
        torchmatch.bank = saved


# ---- the reference, by hand ------------------------------------------------------------------------------------------------
def _rows(*rows, dim=130):
    out = np.zeros((len(rows), dim), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def test_reference_by_hand_3_by_4():
    # distances: q0 -> (0, 5, 5, 1), q1 -> (5, 0, 0, 4), q2 -> (10, 5, 5, 9)
    Q = _rows([0, 0], [3, 4], [6, 8])
    T = _rows([0, 0], [3, 4], [3, 4], [0, 1])
    ones = np.ones((3, 4), np.uint8)
    idx, dist = WM.knn(Q, T, ones, 2)
    assert idx.tolist() == [[0, 3], [1, 2], [1, 2]] and dist.tolist() == [[0.0, 1.0], [0.0, 0.0], [5.0, 5.0]]
    assert idx.dtype == np.int32 and dist.dtype == np.float32
    mask = np.array([[0, 1, 1, 0],          # the two nearest rows forbidden: the tie at 5 goes to the lower index
                     [0, 0, 1, 0],          # one permitted row: the tail is -1 / +inf
                     [0, 0, 0, 0]], np.uint8)
    idx, dist = WM.knn(Q, T, mask, 2)
    assert idx.tolist() == [[1, 2], [2, -1], [-1, -1]]
    assert dist[0].tolist() == [5.0, 5.0] and dist[1, 0] == 0.0 and np.isinf(dist[1, 1]) and np.isinf(dist[2]).all()
    idx, dist = WM.knn(Q, T, mask, 1)
    assert idx.tolist() == [[1], [2], [-1]] and dist[:2, 0].tolist() == [5.0, 0.0] and np.isinf(dist[2, 0])
    # a NaN train row is never listed, permitted or not; the value is the float32 chain's
    N = _rows([np.nan, 0], [1, 1])
    idx, dist = WM.knn(Q[:1], N, np.ones((1, 2), np.uint8), 2)
    assert idx.tolist() == [[1, -1]] and dist[0, 0] == np.sqrt(np.float32(2.0)) and np.isinf(dist[0, 1])


def test_mask_generators():
    for name, f in WM.MASKS.items():
        for nq, nt in WM.SHAPES + [(40, 300)]:
            for k in (1, 2):
                m = f(nq, nt, k, 3)
                assert m.shape == (nq, nt) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}, name
    assert (WM.exactly_one(40, 300, 2, 3).sum(1) == 1).all()
    assert (WM.k_minus_one(40, 300, 2, 3).sum(1) == 1).all() and WM.k_minus_one(40, 300, 1, 3).sum() == 0
    assert WM.last_word(40, 300, 2, 3)[:, :256].sum() == 0 and WM.last_word(40, 300, 2, 3)[:, 256:].any()
    b = WM.band(40, 300, 2, 3)
    assert (b.sum(1) <= 64).all() and b[20, 150] == 1 and b[20, 150 - 33] == 0 and b[20, 150 + 32] == 0
    assert (WM.sparse(300, 257, 2, 3).sum(1) < 2).any()
    Q, T, mask, rows = WM.planted(50, 200, 129, 5)
    assert np.array_equal(T[rows], Q) and mask.sum() == 50 * 199 and (mask[np.arange(50), rows] == 0).all()
    Q, T, mask = WM.overflow_cluster()
    same = (T == T[np.nonzero(mask[0] == 0)[0][0]]).all(1)
    assert Q.shape == (600, 129) and T.shape == (2304, 129) and same.sum() == 2100 and (mask[:, same].sum(1) == 1890).all()


# ---- the new unit's kernels ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def masked_meta(tmp_path_factory):
    return R.metadata(R.isa("wide_masked", tmp_path_factory))


@pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")
def test_new_kernels_run_without_scratch(masked_meta):
    assert masked_meta, "no kernel in wide_masked.hip"
    for n, m in masked_meta.items():
        assert (m["vgpr_spill_count"], m["private_segment_fixed_size"]) == (0, 0), (n, m)
        assert m["vgpr_count"] <= 256, (n, m)               # two waves per SIMD, as K14's filter and exact kernel have


@pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")
def test_the_masked_filter_exists_at_every_k_step_count(masked_meta):
    filt = {n for n in masked_meta if re.match(r"_ZN2fm\d+wide_masked_filter_kernelI", n)}
    want = {"Li%dELi%dE" % (ks, ktop) for ks in (5, 6, 7, 8) for ktop in (1, 2)}
    assert {re.search(r"kernelI(Li\dELi\dE)", n).group(1) for n in filt} == want and len(filt) == 8, sorted(filt)
    exact = {n for n in masked_meta if re.match(r"_ZN2fm\d+wide_masked_exact_kernelI", n)}
    assert len(exact) == 2, sorted(exact)
    assert len(masked_meta) == 10, sorted(masked_meta)       # nothing else: the rescoring and the merge are reused


@pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")
def test_the_masked_filter_uses_the_matrix_cores(tmp_path_factory):
    text = R.isa("wide_masked", tmp_path_factory)
    for k in R.kernels(text):
        n_mfma = sum(1 for _, line in k.insns if line.startswith("v_mfma_f32_16x16x32_f16"))
        if "wide_masked_filter_kernel" in k.name:
            ks = int(re.search(r"kernelILi(\d)E", k.name).group(1))
            assert n_mfma >= 2 * ks, (k.name, n_mfma)        # two blocks of KS matrix instructions per tile
        else:
            assert n_mfma == 0, k.name
