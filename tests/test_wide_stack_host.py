"""CPU: the host side of the stacked knnMatch calls on a wide train collection (fm_collection_wide_knn, _wide_knn_dev,
_wide_knn2_ratio, _wide_knn2_ratio_dev, _wide_votes -- additions to ABI revision 12): the prototypes against the ctypes binding
and against their L2 namesakes', word for word; the header's new section, its place, and every older "Not built" sentence; the
ValueErrors of matchutil / torchmatch that are raised before anything reaches the library; the NumPy reference
(tests/wide_stack_ref.py) on a hand-worked collection; and (hipcc cross-compiles) the scratch, spills and instantiations of the
new unit's kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

import isa_read as R
import wide_stack_ref as WS
from fastmatch_amd import _ffi, matchutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMESAKE = {"fm_collection_wide_knn": "fm_collection_knn", "fm_collection_wide_knn_dev": "fm_collection_knn_dev",
            "fm_collection_wide_knn2_ratio": "fm_collection_knn2_ratio", "fm_collection_wide_knn2_ratio_dev": "fm_collection_knn2_ratio_dev",
            "fm_collection_wide_votes": "fm_collection_votes"}


def _header():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


def _prose(comment):
    """A block comment's text on one line, without the ' * ' that starts its lines."""
    return " ".join(re.sub(r"\n\s*\*\s?", " ", comment).split())


def _klass_of_text(p):
    p = " ".join(p.split())
    if "*" in p:
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
    return {ctypes.c_int64: "i64", ctypes.c_int: "i32", ctypes.c_int32: "i32", ctypes.c_double: "f64"}[t]


# ---- header and binding ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NAMESAKE))
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
    assert ("still revision 12, additions only -- fm_collection_wide_knn, fm_collection_wide_knn_dev, fm_collection_wide_knn2_ratio, "
            "fm_collection_wide_knn2_ratio_dev, fm_collection_wide_votes") in head
    # the section sits behind the wide masked prototypes and in front of the ratio calls
    assert hdr.index("int  fm_wide_knn_masked_dev(") < hdr.index("---- Wide stacked knnMatch") < hdr.index("int  fm_collection_wide_knn(") \
        < hdr.index("int  fm_collection_wide_votes(") < hdr.index("int  fm_knn2_ratio(")
    sect = _prose(hdr.split("---- Wide stacked knnMatch")[1].split("int  fm_collection_wide_knn(")[0])
    for rule in ("Let T be the real rows of the images concatenated in image order",
                 "equals fm_knn(q, bank(T), k) bit for bit", "(img, row inside the image)", "sqrtf(s), s = fmaf(v_k, v_k, s)",
                 "ascend strictly by (distance bits, img, row)", "fewer than k real rows the entry is -1 / -1 / +inf",
                 "a NaN or +inf distance is never listed", "k >= 3 is FM_EUNSUPPORTED", "k < 1 is FM_EINVAL",
                 "float64 d0 / d1 < tau", "d1 == 0 rejected", "the full count in *n_accepted",
                 "mode 0 is the same test counted at the first neighbour's image", "fm_collection_wide_knn2_each",
                 "Empty images keep their index", "no add has succeeded is valid", "No option changes a result",
                 "read at the call", "(row & 127) < real_rows[row >> 7]", "leaves by INDEX", "v_mfma_f32_16x16x32_f16",
                 "skips its matrix instructions and its operand fetch", '"f32_filter" 0 / 1 / 2', "4e6 real pairs",
                 "scale exponents more than 8 apart", "fm_f32_filter_stats",
                 "one launch per filtered call and one fallback per call that is redone",
                 "(1) NULL handles, or a collection of another context", "(2) a query that is not FM_BANK_F32W", "even when it is empty",
                 "(3) widths that differ", "(4) k, or for the votes the mode", "(5) the output pointers",
                 "fm_collection_knn_dev's", "order themselves against consumer_stream in both directions",
                 "not accounted in fm_stats", "the host forms add nq * real rows pairs"):
        assert rule in sect, rule
    left = sect.split("Not built:")[1]
    for out_of_scope in ("k >= 3", "masks on a wide collection (fm_mask_create_coll", "fm_collection_wide_xcheck1_each",
                         "a stacked sweep shared by several query banks"):
        assert out_of_scope in left, out_of_scope


def test_every_older_not_built_sentence_is_still_there():
    hdr = _header()
    k14 = _prose(hdr.split("---- K14: wide float banks")[1].split("int  fm_bank_destroy")[0])
    listed = k14.split("Not built for wide collections:")[1]
    assert listed.startswith(" every other fm_collection_* call -- fm_collection_knn(_dev), fm_collection_knn2_ratio(_dev), "
                             "fm_collection_knn2_each, fm_collection_votes, fm_collection_knn_masked(_dev), fm_collection_radius_match(_dev), "
                             "fm_collection_match_accepted_each(_dev), fm_collection_xcheck1_each(_dev), fm_collection_mutual_ratio_each(_dev) "
                             "-- and fm_mask_create_coll: FM_EUNSUPPORTED")
    assert '"Wide stacked knnMatch" below' in listed                 # the parenthesis that points to the new section
    assert "Also not built: k >= 3, LDS staging of the streamed operand, computing a pair's tiles once for both directions" in listed
    assert "Out of scope here: the stacked forms on a wide collection (knnMatch over all images, knn2_ratio, votes mode 0)" in k14
    assert "fm_knn_masked(_dev)" in k14.split("Not built for wide float banks:")[1]
    fast = _prose(hdr.split("---- Wide Fast-Match")[1].split("int fm_wide_self_dist")[0])
    assert "radiusMatch, masks, k >= 3" in fast.split("Not built:")[1]
    radius = _prose(hdr.split("---- Wide radiusMatch")[1].split("int fm_wide_radius_match(")[0])
    assert "k >= 3 and the stacked knn forms on a wide collection." in radius.split("Not built:")[1]
    masked = _prose(hdr.split("---- Wide knnMatch masks")[1].split("int  fm_wide_knn_masked(")[0])
    assert "fm_collection_wide_*); k >= 3; a masked K8 filter for 128-D float banks" in masked.split("Not built:")[1]
    text = _prose(hdr)
    for kept in ("masks on the fp16-filter (K8) and FP4 (K11) matrix-core sweeps", "masked crossCheck", "masked radiusMatch",
                 "Not built: the STACKED crossCheck on a collection"):
        assert kept in text, kept


def test_python_layers_expose_the_calls():
    for m in ("wide_knn", "wide_knn_dev", "wide_knn2_ratio", "wide_knn2_ratio_dev", "wide_votes"):
        assert callable(getattr(_ffi.Collection, m)), m
    for m in ("knnMatchWide_arrays", "knnMatchWide", "ratioMatchWide_arrays", "votesWide"):
        assert callable(getattr(matchutil.BFMatcher, m)), m
    from fastmatch_amd import torchmatch
    for m in ("wide_knn", "wide_ratio_match", "wide_votes"):
        assert callable(getattr(torchmatch.Collection, m)), m


# ---- refusals that touch no device -----------------------------------------------------------------------------------------
def test_matchutil_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    monkeypatch.setattr(_ffi, "default_context", no_device)
    monkeypatch.setattr(_ffi, "load_library", no_device)
    monkeypatch.setattr(matchutil.BFMatcher, "train", no_device)
    wide = matchutil.BFMatcher(matchutil.NORM_L2)
    wide.add_wide([np.zeros((5, 256), np.float32)])
    q = np.zeros((3, 256), np.float32)
    calls = {"knnMatchWide_arrays": lambda m, x: m.knnMatchWide_arrays(x, 2), "knnMatchWide": lambda m, x: m.knnMatchWide(x, 1),
             "ratioMatchWide_arrays": lambda m, x: m.ratioMatchWide_arrays(x, 0.8), "votesWide": lambda m, x: m.votesWide(x, 0.8)}
    for name, call in calls.items():
        for bad in (q.astype(np.uint8), np.zeros((3, 200), np.float32), np.zeros(256, np.float32)):
            with pytest.raises(ValueError, match="float array"):
                call(wide, bad)
        narrow = matchutil.BFMatcher(matchutil.NORM_L2)
        narrow.add([np.zeros((5, 128), np.float32)])
        with pytest.raises(ValueError, match="not a wide one"):
            call(narrow, q)
        with pytest.raises(ValueError):
            call(matchutil.BFMatcher(matchutil.NORM_L2), q)             # an empty collection
        ham = matchutil.BFMatcher(matchutil.NORM_HAMMING)
        with pytest.raises(ValueError, match="NORM_L2"):
            call(ham, q)
    for k in (0, 3, 8):
        with pytest.raises(ValueError, match="k = 1, 2"):
            wide.knnMatchWide_arrays(q, k)
        with pytest.raises(ValueError, match="k = 1, 2"):
            wide.knnMatchWide(q, k)
    with pytest.raises(ValueError, match="mode"):
        wide.votesWide(q, 0.8, mode=2)
    # the L2-named methods keep refusing a wide collection
    with pytest.raises(ValueError, match="wide"):
        wide.knnMatch(q, k=2)
    with pytest.raises(ValueError, match="wide"):
        wide.votes(q, 0.8)


def test_torchmatch_refusals_come_before_the_library():
    torch = pytest.importorskip("torch")
    from fastmatch_amd import torchmatch

    def no_library(*a, **k):
        raise AssertionError("a refusal touched the library")
    saved = torchmatch.bank, torchmatch.Collection._collection
    torchmatch.bank = no_library
    torchmatch.Collection._collection = no_library
    try:
        w256 = torch.zeros((4, 256))
        narrow = torchmatch.Collection()
        for call in (lambda c: c.wide_knn(w256, 2), lambda c: c.wide_ratio_match(w256, 0.8), lambda c: c.wide_votes(w256, 0.8)):
            with pytest.raises(ValueError, match="not a wide one"):
                call(narrow)
        wide = torchmatch.Collection()
        wide._wide = True
        for k in (0, 3, 8):
            with pytest.raises(ValueError, match="k = 1, 2"):
                wide.wide_knn(w256, k)
        with pytest.raises(ValueError, match="mode"):
            wide.wide_votes(w256, 0.8, mode=2)
        with pytest.raises(ValueError):
            wide.wide_knn(w256, 2)                                       # a CPU tensor
        with pytest.raises(ValueError):
            wide.wide_ratio_match(torch.zeros((4, 256), dtype=torch.uint8), 0.8)
        # the L2-named methods keep refusing a wide collection
        for call in (lambda: wide.knn(w256, 2), lambda: wide.ratio_match(w256, 0.8)):
            with pytest.raises(ValueError, match="wide collection"):
                call()
    finally:
        torchmatch.bank, torchmatch.Collection._collection = saved


# ---- the reference, by hand ------------------------------------------------------------------------------------------------
def _rows(*rows, dim=130):
    out = np.zeros((len(rows), dim), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def test_reference_by_hand_on_three_images():
    """Three images, the middle one empty.  Every real row lies at 5 or more from q0 = (3, 4) while the zero row -- what the
    stack's padding holds -- would lie at exactly 5 from it and at 1 from q1 = (0, 1): nearer than every real row of q1.  The
    reference works on the concatenation of the REAL rows, so it cannot return it."""
    Q = _rows([3, 4], [0, 1], [6, 8])
    images = [_rows([6, 8], [3, -1]), _rows(), _rows([6, 8], [0, 6], [3, 9])]
    # distances: q0 -> (5, 5 | 5, sqrt 13, 5), q1 -> (sqrt 85, sqrt 13 | sqrt 85, 5, sqrt 73), q2 -> (0, sqrt 90 | 0, sqrt 40, sqrt 10)
    assert WS.first_rows(images).tolist() == [0, 2, 2, 5]
    img, idx, dist = WS.knn(Q, images, 2)
    assert img.dtype == idx.dtype == np.int32 and dist.dtype == np.float32
    assert img.tolist() == [[2, 0], [0, 2], [0, 2]]
    assert idx.tolist() == [[1, 0], [1, 1], [0, 0]]                       # ties: the earlier image, then the earlier row
    s13 = float(np.sqrt(np.float32(13.0)))
    assert dist.tolist() == [[s13, 5.0], [s13, 5.0], [0.0, 0.0]]
    assert (dist[1] > 1.0).all()                                        # the zero row at 1.0 is in no list
    img1, idx1, dist1 = WS.knn(Q, images, 1)
    assert img1.tolist() == [[2], [0], [0]] and idx1.tolist() == [[1], [1], [0]] and dist1[:, 0].tolist() == [s13, s13, 0.0]
    # the ratio test: q0 13^.5 / 5 = 0.72, q1 the same, q2 0 / 0 (rejected: the second distance is 0)
    qi, im, ti, d, r = WS.ratio_match(Q, images, 0.8)
    assert qi.tolist() == [0, 1] and im.tolist() == [2, 0] and ti.tolist() == [1, 1] and d.tolist() == [s13, s13]
    assert np.allclose(r, s13 / 5.0) and WS.ratio_match(Q, images, 0.7)[0].size == 0
    assert WS.ratio_match(Q, images, np.inf)[0].tolist() == [0, 1]
    assert WS.votes(Q, images, 0.8, 0).tolist() == [1, 0, 1]
    # per image: image 0 alone q0 -> 5 / 5, q1 -> sqrt 13 / sqrt 85 = 0.39, q2 -> 0 / sqrt 90 = 0; image 2 alone q0 -> sqrt 13 / 5,
    # q1 -> 5 / sqrt 73 = 0.59, q2 -> 0 / sqrt 10 = 0
    assert WS.votes(Q, images, 0.8, 1).tolist() == [2, 0, 3]
    assert WS.votes(Q, images, 0.5, 1).tolist() == [2, 0, 1]
    # fewer than k real rows, no rows at all, no query rows
    img, idx, dist = WS.knn(Q, [_rows(), _rows([0, 1]), _rows()], 2)
    assert img.tolist() == [[1, -1]] * 3 and idx.tolist() == [[0, -1]] * 3 and np.isinf(dist[:, 1]).all()
    img, idx, dist = WS.knn(Q, [_rows(), _rows()], 2)
    assert (img == -1).all() and (idx == -1).all() and np.isinf(dist).all() and img.shape == (3, 2)
    assert WS.knn(Q[:0], images, 2)[0].shape == (0, 2) and WS.votes(Q[:0], images, 0.8, 1).tolist() == [0, 0, 0]
    # a NaN train row is never listed
    img, idx, dist = WS.knn(Q[:1], [_rows([np.nan, 0]), _rows([3, 5])], 2)
    assert img.tolist() == [[1, -1]] and idx.tolist() == [[0, -1]] and dist[0, 0] == 1.0 and np.isinf(dist[0, 1])


def test_data_makers():
    assert WS.SIZES == [300, 0, 128, 1, 65, 129, 700, 100] and WS.SIZES_EMPTY_ENDS[0] == WS.SIZES_EMPTY_ENDS[-1] == 0
    Q, images = WS.unit_images(50, WS.SIZES, 129, 3)
    assert [len(im) for im in images] == WS.SIZES and np.allclose(np.linalg.norm(Q, axis=1), 1.0, atol=1e-6)
    d = WS.knn(Q, images, 2)[2]
    assert (d > 1.0).all()                     # every real neighbour is farther than a zero row would be
    Q, images = WS.tied_images(129, 5)
    img, idx, dist = WS.knn(Q, images, 2)
    assert (dist[:10] == 0).all() and (img[:10] == 1).all() and (idx[:10, 0] < idx[:10, 1]).all() and (dist[10:, 0] > 0).all()
    assert idx[:10, 0].tolist() == [20 + j for j in range(10)] and idx[:10, 1].tolist() == [190 - 3 * j for j in range(10)]
    Q, images, fewer = WS.overflow_images()
    assert Q.shape == (600, 129) and [len(im) for im in images] == [1000, 1304] == [len(im) for im in fewer]


# ---- the new unit's kernels ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stack_text(tmp_path_factory):
    return R.isa("wide_stack", tmp_path_factory)


@pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")
def test_new_kernels_run_without_scratch(stack_text):
    meta = R.metadata(stack_text)
    assert meta, "no kernel in wide_stack.hip"
    for n, m in meta.items():
        assert (m["vgpr_spill_count"], m["private_segment_fixed_size"]) == (0, 0), (n, m)
        assert m["vgpr_count"] <= 256, (n, m)               # two waves per SIMD, as K14's filter and exact kernel have


@pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")
def test_the_stack_filter_exists_at_every_k_step_count(stack_text):
    meta = R.metadata(stack_text)
    filt = {n for n in meta if re.match(r"_ZN2fm\d+wide_stack_filter_kernelI", n)}
    assert {int(re.search(r"kernelILi(\d)E", n).group(1)) for n in filt} == {5, 6, 7, 8}, sorted(filt)
    assert all(re.search(r"kernelILi\dELi2EE", n) for n in filt) and len(filt) == 4, sorted(filt)      # top-2: k = 1 is its first column
    exact = {n for n in meta if re.match(r"_ZN2fm\d+wide_stack_exact_kernelI", n)}
    assert len(exact) == 1, sorted(exact)
    assert len(meta) == 5, sorted(meta)                      # nothing else: the rescoring, the merge and the tails are reused


@pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")
def test_the_stack_filter_uses_the_matrix_cores(stack_text):
    for k in R.kernels(stack_text):
        n_mfma = sum(1 for _, line in k.insns if line.startswith("v_mfma_f32_16x16x32_f16"))
        if "wide_stack_filter_kernel" in k.name:
            ks = int(re.search(r"kernelILi(\d)E", k.name).group(1))
            assert n_mfma >= 2 * ks, (k.name, n_mfma)        # two blocks of KS matrix instructions per tile
        else:
            assert n_mfma == 0, k.name
