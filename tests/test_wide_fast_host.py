"""CPU: the host side of Fast-Match's self-distance test on wide float descriptors (FM_BANK_F32W) -- hand-checked cases of the
NumPy reference (tests/wide_fast_ref.py), the ValueErrors of matchutil / BFMatcher / torchmatch that are raised before
anything is uploaded, the new prototypes of the header against the ctypes binding and the ABI revision they leave alone,
and (hipcc cross-compiles) the registers, scratch and instantiations of the SELF forms of K14's kernels."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import isa_read as R
import wide_fast_ref as WF
from fastmatch_amd import _ffi, matchutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fm_wide_self_dist", "fm_wide_self_dist_batch", "fm_wide_set_selfdist", "fm_wide_match_ratio",
       "fm_wide_match_accepted", "fm_wide_match_accepted_dev", "fm_collection_wide_match_accepted_each",
       "fm_collection_wide_match_accepted_each_dev")
L2 = {"fm_wide_self_dist": "fm_self_dist", "fm_wide_self_dist_batch": "fm_self_dist_batch",
      "fm_wide_set_selfdist": "fm_bank_set_selfdist", "fm_wide_match_ratio": "fm_match_ratio",
      "fm_wide_match_accepted": "fm_match_accepted", "fm_wide_match_accepted_dev": "fm_match_accepted_dev",
      "fm_collection_wide_match_accepted_each": "fm_collection_match_accepted_each",
      "fm_collection_wide_match_accepted_each_dev": "fm_collection_match_accepted_each_dev"}


def _rows(*rows, dim=130):
    """Rows of `dim` values: the given leading values, zeros behind them."""
    out = np.zeros((len(rows), dim), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


# ---- the reference, by hand ------------------------------------------------------------------------------------------------
def test_self_dist_by_hand():
    X = _rows([0, 0], [3, 4], [0, 0], [3, 0])             # rows 0 and 2 are duplicates; row 1 is 5 from them and 4 from row 3
    assert WF.self_dist(X).tolist() == [0.0, 4.0, 0.0, 3.0]
    assert WF.self_dist(X).dtype == np.float64
    assert WF.self_dist(_rows([1, 2])).tolist() == [np.inf]                   # a bank of one row
    assert WF.self_dist(np.zeros((0, 200), np.float32)).shape == (0,)
    assert WF.self_dist(_rows([7], [7], [7])).tolist() == [0.0, 0.0, 0.0]     # an all-equal bank: the third row's two nearest are both others
    # a NaN row and a row with an infinite value have no finite distance and are nobody's neighbour
    N = _rows([0, 0], [np.nan, 0], [0, 1], [np.inf, 0], [0, 3])
    assert WF.self_dist(N).tolist() == [1.0, np.inf, 1.0, np.inf, 2.0]
    # the value is the float32 chain's, widened: sqrtf(2) as a float32
    assert WF.self_dist(_rows([0, 0], [1, 1]))[0] == np.float64(np.sqrt(np.float32(2.0)))


def test_ratio_rules_by_hand():
    Q = _rows([0, 0], [0, 0], [10, 0], [10, 4])           # rows 0 and 1 are duplicates (selfdist 0), rows 2 and 3 are 4 apart
    sd = WF.self_dist(Q)
    assert sd.tolist() == [0.0, 0.0, 4.0, 4.0]
    # train row 0 = query 0 exactly (elects row 0, the lower duplicate: 0 / 0), row 1 is 1 from query 2, row 2 is 3 from query 3
    T = _rows([0, 0], [10, -1], [10, 7])
    tidx, dist, ratio, passed = WF.match_ratio(Q, T, sd, 0.5)
    assert tidx.tolist() == [0, -1, 1, 2] and dist[[0, 2, 3]].tolist() == [0.0, 1.0, 3.0] and np.isinf(dist[1])
    assert np.isnan(ratio[0]) and np.isnan(ratio[1]) and ratio[2] == 0.25 and ratio[3] == 0.75
    assert passed.tolist() == [False, False, True, False]                      # 0 / 0 rejected, 0.25 < 0.5, 0.75 not
    assert WF.match_ratio(Q, T, sd, np.inf)[3].tolist() == [False, False, True, True]      # NaN is not < inf either
    # d / 0: the duplicates' train row at distance 1 -> +inf, rejected at every tau
    tidx, dist, ratio, passed = WF.match_ratio(Q, _rows([0, 1]), sd, np.inf)
    assert tidx[0] == 0 and dist[0] == 1.0 and ratio[0] == np.inf and not passed.any()
    # a bank of one query row: selfdist +inf, ratio 0, accepted for every tau > 0 and for none at tau = 0
    one = _rows([1, 1])
    q, t, d, r = WF.fast_match(one, _rows([1, 3], [1, -1]), 1e-300)
    assert q.tolist() == [0] and t.tolist() == [0] and d.tolist() == [2.0] and r.tolist() == [0.0]   # (strict <: the lower train row on the tie)
    assert len(WF.fast_match(one, _rows([5]), 0.0)[0]) == 0
    # accepted rows ascend in query index and carry float64 ratios; the per-image form is a loop
    q, t, d, r = WF.fast_match(Q, T, 0.9)
    assert q.tolist() == [2, 3] and t.tolist() == [1, 2] and r.dtype == np.float64 and d.dtype == np.float32
    each = WF.fast_match_each(Q, [T, T[:0], T[1:]], 0.9)
    assert [e[0].tolist() for e in each] == [[2, 3], [], [2, 3]] and each[2][1].tolist() == [0, 1]
    assert WF.same_f64(np.array([np.nan, 1.0]), np.array([-np.nan, 1.0])) and not WF.same_f64(np.array([0.0]), np.array([-0.0]))


# ---- refusals that touch no device -----------------------------------------------------------------------------------------
def test_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    w256, w200 = np.zeros((4, 256), np.float32), np.zeros((4, 200), np.float32)
    for bad in (w256.astype(np.uint8), w256.astype(np.float16), w256.astype(np.int32)):
        with pytest.raises(ValueError, match="float32 / float64"):
            matchutil.wide_fast_match_arrays(bad, w256, 0.9)
        with pytest.raises(ValueError, match="float32 / float64"):
            matchutil.wide_fast_match(w256, bad, 0.9)
    for dim in (128, 257, 32):
        with pytest.raises(ValueError, match="129 .. 256 values per row"):
            matchutil.wide_fast_match_arrays(np.zeros((4, dim), np.float32), np.zeros((4, dim), np.float32), 0.9)
    with pytest.raises(ValueError, match="256 values per query row, 200 per train row"):
        matchutil.wide_fast_match(w256, w200, 0.9)
    with pytest.raises(ValueError, match="2-D"):
        matchutil.wide_fast_match_arrays(np.zeros(256, np.float32), w256, 0.9)
    # the matcher: nothing added, a collection that is not wide, a NORM_HAMMING matcher, a query of another width or dtype
    with pytest.raises(ValueError, match="no train descriptors"):
        matchutil.BFMatcher().wideFastMatchEach(w256, 0.9)
    with pytest.raises(ValueError, match="no train descriptors"):
        matchutil.BFMatcher().wideFastMatchEach_arrays(w256, 0.9)
    l2 = matchutil.BFMatcher()
    l2.add([np.zeros((2, 128), np.float32)])
    with pytest.raises(ValueError, match="not a wide one"):
        l2.wideFastMatchEach_arrays(w256, 0.9)
    with pytest.raises(ValueError, match="NORM_L2"):
        matchutil.BFMatcher(matchutil.NORM_HAMMING).wideFastMatchEach(w256, 0.9)
    w = matchutil.BFMatcher()
    w.add_wide([w256])
    with pytest.raises(ValueError, match="collection's width"):
        w.wideFastMatchEach_arrays(w200, 0.9)
    with pytest.raises(ValueError, match="float array"):
        w.wideFastMatchEach(w256.astype(np.uint8), 0.9)
    # fastMatchEach keeps refusing a wide collection, and says which method serves it
    with pytest.raises(ValueError, match="wide collection") as e:
        w.fastMatchEach(w256, 0.9)
    assert "wideFastMatchEach" in str(e.value)


def test_torchmatch_refusals_come_before_the_library():
    torch = pytest.importorskip("torch")
    from fastmatch_amd import torchmatch

    def no_library(*a, **k):
        raise AssertionError("a refusal touched the library")
    saved = torchmatch.bank
    torchmatch.bank = no_library
    try:
        w256, w200 = torch.zeros((4, 256)), torch.zeros((4, 200))
        with pytest.raises(ValueError):
            torchmatch.wide_fast_match(torch.zeros((4, 256), dtype=torch.uint8), w256, 0.9)      # (a CPU tensor, or its dtype)
        with pytest.raises(ValueError):
            torchmatch.wide_fast_match(w256, w200, 0.9)
        coll = torchmatch.Collection()
        with pytest.raises(ValueError, match="not a wide one"):
            coll.wide_fast_match_each(w256, 0.9)
    finally:
        torchmatch.bank = saved


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
    # the argument list is the L2 call's, word for word
    norm = lambda p: " ".join(p.split())                  # noqa: E731
    assert [norm(p) for p in texts] == [norm(p) for p in protos[L2[name]].split(",")]
    assert hasattr(_ffi.load_library(), name)


def test_abi_revision_and_header_section():
    hdr = _header()
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    comment = _prose(hdr.split("#define FM_ABI_VERSION")[0])
    assert "still revision 12, additions only -- " + ", ".join(NEW) in comment
    sect = _prose(hdr.split("---- Wide Fast-Match")[1].split("int fm_wide_self_dist")[0])
    assert hdr.index("---- Hamming Fast-Match") < hdr.index("---- Wide Fast-Match") < hdr.index("---- train collections")
    for out_of_scope in ("triangular sweep", "async / batch / sharded-key", "fm_expand_*", "radiusMatch, masks, k >= 3",
                         "shared launch for fm_wide_self_dist_batch"):
        assert out_of_scope in sect.split("Not built:")[1], out_of_scope
    for rule in ("min over j != i", "sqrtf(s), s = fmaf(v_k, v_k, s)", "strict <", "starting from +inf", "0 / 0 = NaN", "d / 0 = +inf",
                 "bank of one query row", "lowest index wins a tie", "NaN never beats anything", "no self distances",
                 "second column of fm_knn2(b, b)", "There is no ratio cut", "one sweep per bank", "do not share a stack",
                 "a bank listed twice is FM_EINVAL", "bit for bit, fm_wide_match_accepted(q, B_i, tau, cap)", '"coll_ws_bytes"',
                 "an empty image keeps its slot and accepts nothing", "dropped by INDEX", '"f32_filter" and "f32_nsplit"',
                 "fm_f32_filter_stats", "n * n pairs for a self sweep and nq * nt for a match",
                 "names the L2 or the Hamming call"):
        assert rule in sect, rule
    # the L2-named calls keep refusing: every earlier "Not built" sentence is still there
    k14 = _prose(hdr.split("---- K14: wide float banks")[1].split("int  fm_bank_destroy")[0])
    old = k14.split("Not built for wide float banks:")[1]
    for name in ("fm_self_dist(_batch)", "fm_bank_set_selfdist", "fm_match_ratio", "fm_match_accepted*"):
        assert name in old, name
    assert "fm_collection_match_accepted_each(_dev)" in k14.split("Not built for wide collections:")[1]


def test_python_layers_expose_the_calls():
    for k, names in ((_ffi.Context, ("wide_self_dist", "wide_self_dist_batch", "wide_match_ratio", "wide_match_accepted",
                                     "wide_match_accepted_dev")),
                     (_ffi.Bank, ("set_wide_selfdist",)),
                     (_ffi.Collection, ("wide_match_accepted_each", "wide_match_accepted_each_dev")),
                     (matchutil.BFMatcher, ("wideFastMatchEach", "wideFastMatchEach_arrays"))):
        for n in names:
            assert callable(getattr(k, n)), n
    assert callable(matchutil.wide_fast_match) and callable(matchutil.wide_fast_match_arrays)
    from fastmatch_amd import torchmatch
    assert callable(torchmatch.wide_fast_match) and callable(torchmatch.Collection.wide_fast_match_each)


# ---- the SELF forms of K14's kernels ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_meta(tmp_path_factory):
    return R.metadata(R.isa("wide_f32", tmp_path_factory))


def _instances(md, base):
    return {n: m for n, m in md.items() if re.match(r"_ZN2fm\d+%s(I|E)" % base, n)}


@pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")
def test_self_forms_run_without_scratch(wide_meta):
    """SELF is a template parameter (the trailing Lb1E of the mangled name): six new instantiations -- the filter at its four
    K-step counts with KTOP = 1, the rescoring and the exact kernel -- and six more of the table kernels (top-1, outside
    operand), none of which spills or takes scratch; the instantiations that were there keep their number and take no scratch
    either."""
    want = {"wide_filter_kernel": (4, 8), "wide_rescore_kernel": (1, 2), "wide_exact_kernel": (1, 2)}
    for base, (n_self, n_plain) in want.items():
        found = _instances(wide_meta, base)
        selfs = {n: m for n, m in found.items() if re.search(r"Lb1EEEv", n)}
        plain = {n: m for n, m in found.items() if n not in selfs}
        assert (len(selfs), len(plain)) == (n_self, n_plain), (base, sorted(found))
        for n in selfs:
            assert re.search(r"Li1ELb1EEEv", n), n                 # KTOP = 1
        for n, m in found.items():
            assert (m["vgpr_spill_count"], m["private_segment_fixed_size"]) == (0, 0), (n, m)
    # the collection form's top-1 table kernels with an outside operand: <KS, 1, true> x 4, <1, true>, <1, true>
    for base, total, top1 in (("wide_filter_table_kernel", 12, 4), ("wide_rescore_table_kernel", 3, 1), ("wide_exact_table_kernel", 3, 1)):
        found = _instances(wide_meta, base)
        assert len(found) == total and sum(1 for n in found if re.search(r"Li1ELb1EEEv", n)) == top1, (base, sorted(found))
        for n, m in found.items():
            assert (m["vgpr_spill_count"], m["private_segment_fixed_size"]) == (0, 0), (n, m)


# The 28 kernels of wide_f32.hip that existed before the SELF and the top-1 table forms, as the commit before them compiled
# (the product's flags): instructions, unified VGPRs, static LDS bytes, and the first 12 hex digits of the SHA-1 of the
# instruction stream with its branch labels normalised.  The new forms are template parameters of the same bodies; these
# kernels -- every existing wide sweep, the exact kernel behind "f32_filter" 0 and the filter's fallback among them -- must
# compile to the code they were.  (A co-compiled instantiation CAN move them: one wide_exact_body<1> shared by
# wide_exact_kernel<1> and wide_exact_table_kernel<1, true> did, see the OWN parameter.)  The values are this compiler's;
# another compiler, or a deliberate change of these kernels, must edit the table on purpose.
RECORDED_WITH = "AMD clang version 22.0.0git (https://github.com/RadeonOpenCompute/llvm-project roc-7.2.0 26014 7b800a19466229b8479a78de19143dc33c3ab9b5)"
UNCHANGED = {
    "_ZN2fm16wide_copy_kernelILi2EEEvPKhlliPflPi": (163, 14, 0, 'd0c090e43ca3'),
    "_ZN2fm16wide_copy_kernelILi3EEEvPKhlliPflPi": (165, 14, 0, 'ef617df16578'),
    "_ZN2fm16wide_copy_kernelILi4EEEvPKhlliPflPi": (165, 14, 0, 'd2ab4deabcbe'),
    "_ZN2fm17wide_exact_kernelILi1ELb0EEEvNS_15WideExactParamsE": (2384, 204, 104448, '1c5786c4d9ab'),
    "_ZN2fm17wide_exact_kernelILi2ELb0EEEvNS_15WideExactParamsE": (4046, 206, 104448, '3a071bf2bd05'),
    "_ZN2fm18wide_filter_kernelILi5ELi1ELb0EEEvNS_16WideFilterParamsE": (1004, 128, 0, '203e8c672938'),
    "_ZN2fm18wide_filter_kernelILi5ELi2ELb0EEEvNS_16WideFilterParamsE": (1108, 128, 0, 'f63d327bdf1a'),
    "_ZN2fm18wide_filter_kernelILi6ELi1ELb0EEEvNS_16WideFilterParamsE": (1016, 144, 0, '793852fb3565'),
    "_ZN2fm18wide_filter_kernelILi6ELi2ELb0EEEvNS_16WideFilterParamsE": (1128, 144, 0, 'fb853f7a2f5f'),
    "_ZN2fm18wide_filter_kernelILi7ELi1ELb0EEEvNS_16WideFilterParamsE": (1028, 160, 0, '3855e580f0b9'),
    "_ZN2fm18wide_filter_kernelILi7ELi2ELb0EEEvNS_16WideFilterParamsE": (1139, 160, 0, '0663f4037b4e'),
    "_ZN2fm18wide_filter_kernelILi8ELi1ELb0EEEvNS_16WideFilterParamsE": (1039, 176, 0, 'b0753f38a2e6'),
    "_ZN2fm18wide_filter_kernelILi8ELi2ELb0EEEvNS_16WideFilterParamsE": (1150, 176, 0, 'dc8efd74dda9'),
    "_ZN2fm18wide_planes_kernelEPKflliPtPfS3_Pi": (163, 38, 0, 'f395c0e6c49c'),
    "_ZN2fm19wide_rescore_kernelILi1ELb0EEEvNS_17WideRescoreParamsE": (140, 24, 0, 'a044d448a46b'),
    "_ZN2fm19wide_rescore_kernelILi2ELb0EEEvNS_17WideRescoreParamsE": (146, 24, 0, '526709819fa1'),
    "_ZN2fm23wide_exact_table_kernelILi2ELb0EEEvNS_15WideTableParamsE": (4012, 207, 104448, 'e877ce4e425a'),
    "_ZN2fm23wide_exact_table_kernelILi2ELb1EEEvNS_15WideTableParamsE": (4021, 206, 104448, 'e3b4d9c9e02c'),
    "_ZN2fm24wide_filter_table_kernelILi5ELi2ELb0EEEvNS_15WideTableParamsE": (1164, 128, 0, '48cc5b85734c'),
    "_ZN2fm24wide_filter_table_kernelILi5ELi2ELb1EEEvNS_15WideTableParamsE": (1179, 128, 0, 'f69eed3876a4'),
    "_ZN2fm24wide_filter_table_kernelILi6ELi2ELb0EEEvNS_15WideTableParamsE": (1185, 144, 0, '89e0cc692c7f'),
    "_ZN2fm24wide_filter_table_kernelILi6ELi2ELb1EEEvNS_15WideTableParamsE": (1200, 144, 0, 'fd4c2d51e36a'),
    "_ZN2fm24wide_filter_table_kernelILi7ELi2ELb0EEEvNS_15WideTableParamsE": (1197, 160, 0, '698ca1628f17'),
    "_ZN2fm24wide_filter_table_kernelILi7ELi2ELb1EEEvNS_15WideTableParamsE": (1212, 160, 0, 'c639da2c5a9e'),
    "_ZN2fm24wide_filter_table_kernelILi8ELi2ELb0EEEvNS_15WideTableParamsE": (1208, 176, 0, '1efe0e67f9c6'),
    "_ZN2fm24wide_filter_table_kernelILi8ELi2ELb1EEEvNS_15WideTableParamsE": (1223, 176, 0, '4270431abd41'),
    "_ZN2fm25wide_rescore_table_kernelILi2ELb0EEEvNS_15WideTableParamsE": (182, 22, 0, '036f00145812'),
    "_ZN2fm25wide_rescore_table_kernelILi2ELb1EEEvNS_15WideTableParamsE": (206, 28, 0, 'c04cb7d3f9ad'),
}


@pytest.mark.skipif(not R.have_hipcc(), reason="no hipcc")
def test_existing_kernels_compile_to_the_code_they_were(tmp_path_factory, wide_meta):
    text = R.isa("wide_f32", tmp_path_factory)
    found = {}
    for k in R.kernels(text):
        body = [re.sub(r"\.LBB\d+_\d+", "L", line) for _, line in k.insns[1:]]
        found[k.name] = (len(body), wide_meta[k.name]["vgpr_count"], wide_meta[k.name]["group_segment_fixed_size"],
                         hashlib.sha1("\n".join(body).encode()).hexdigest()[:12])
    assert len(UNCHANGED) == 28 and set(UNCHANGED) <= set(found), sorted(set(UNCHANGED) - set(found))
    moved = {n: (found[n], want) for n, want in UNCHANGED.items() if found[n] != want}
    assert not moved, "kernels that no longer compile to what they were (recorded with %s): %r" % (RECORDED_WITH, moved)
    # and nothing else came into the unit but the forms this file names: 6 SELF forms, 6 top-1 table forms
    assert len(found) == 28 + 12, sorted(set(found) - set(UNCHANGED))
