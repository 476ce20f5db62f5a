"""CPU: the host side of crossCheck on a train collection (fm_collection_xcheck1_each, its device form) -- the two new
prototypes against the ctypes binding, the ABI revision they leave alone, what the header still lists as not built, the
refusals of BFMatcher.matchEach and torchmatch.Collection.mutual_nn_each, which touch no device, and the NumPy reference
(tests/xcheck_each_ref.py) on hand-made cases."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil, torchmatch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xcheck_each_ref as ref        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fm_collection_xcheck1_each", "fm_collection_xcheck1_each_dev")
INF = np.float32(np.inf)


def _header_text():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


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
def test_new_prototypes_match_the_binding(name):
    hdr = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(fm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    assert name in protos, "the header does not declare %s" % name
    texts = protos[name].split(",")
    res, argtypes = _ffi.SYMBOLS[name]
    assert res is ctypes.c_int
    got = [_klass_of_text(p) for p in texts]
    assert got == [_klass_of_ctype(t) for t in argtypes]
    # (ctx, collection, query, max_dist, ...): tidx, dist, n_matched | cap, d_rows, d_counts, h_counts, consumer_stream
    want = ["ptr", "ptr", "ptr", "f32"] + (["ptr"] * 3 if name == NEW[0] else ["i64"] + ["ptr"] * 4)
    assert got == want
    assert hasattr(_ffi.load_library(), name)
    for method in ("xcheck1_each", "mutual_votes", "xcheck1_each_dev"):
        assert callable(getattr(_ffi.Collection, method))


def test_abi_revision_is_still_12():
    hdr = _header_text()
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    comment = " ".join(hdr.split("#define FM_ABI_VERSION")[0].split())
    for name in NEW:                         # ... and the revision comment names the additions
        assert name in comment
    assert "still revision 12, additions only -- fm_collection_xcheck1_each, fm_collection_xcheck1_each_dev" in comment.replace(" * ", " ")


def test_header_phrases():
    hdr = _header_text()
    sect = hdr.split("---- train collections")[1].split("typedef struct fm_collection")[0]
    not_built = " ".join(sect.split("Not built:")[1].replace("\n *", " ").split())
    for still in ("expansion loop on a collection", "per-image sweep", "binary collections in the self-distance test",
                  "sharding a collection", "Hamming radiusMatch (for pairs or collections)", "an _each form",
                  "skipping the second count sweep", "sharding a collection across GPUs"):
        assert still in not_built, still
    assert "self-distance test and" not in not_built
    # the stacked form is not built, the per-image form is; the single float32 sweep over the stack is not
    assert "Not built: the STACKED crossCheck on a collection" in " ".join(sect.replace("\n *", " ").split())
    assert "the per-image form is built: fm_collection_xcheck1_each" in not_built
    assert "a single reverse K8 sweep over a float32-route stack" in not_built
    dev = hdr.split("---- descriptors already on the GPU")[1]
    assert " ".join(dev.split("Not built:")[1].replace("\n *", " ").split()).startswith(
        "device sources for fm_bank_refill_u8_async and fm_bank_append_*")
    # the option's description states the bytes per entry of both calls
    opt = " ".join(hdr.split('"coll_ws_bytes" 0..2^31-1')[1].split("Unknown names")[0].replace("\n *", " ").split())
    assert "25 bytes per entry" in opt and "17 in the cross-check" in opt and "fm_collection_xcheck1_each" in opt


def test_match_each_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    monkeypatch.setattr(_ffi, "default_context", no_device)
    q = np.zeros((4, 128), np.uint8)
    for cross in (False, True):
        with pytest.raises(ValueError, match="no train descriptors"):
            matchutil.BFMatcher(crossCheck=cross).matchEach(q)                # an empty collection
        with pytest.raises(ValueError, match="no train descriptors"):
            matchutil.BFMatcher(matchutil.NORM_HAMMING, crossCheck=cross).matchEach_arrays(q)
        h = matchutil.BFMatcher(matchutil.NORM_HAMMING, crossCheck=cross)
        h.add([np.zeros((2, 32), np.uint8)])
        with pytest.raises(ValueError, match="NORM_HAMMING"):
            h.matchEach(np.zeros((4, 32), np.float32))                        # a wrong dtype for NORM_HAMMING
        with pytest.raises(ValueError, match="NORM_HAMMING"):
            h.matchEach_arrays(np.zeros((4, 32), np.int32))
    # match / knnMatch keep refusing crossCheck on more than one image, and say where the per-image form is
    m = matchutil.BFMatcher(crossCheck=True)
    m.add([q, q])
    with pytest.raises(ValueError, match="crossCheck") as e:
        m.match(q)
    assert "matchEach" in str(e.value)


def test_mutual_nn_each_refusals_come_before_the_library(monkeypatch):
    import torch

    def no_device(*a, **k):
        raise AssertionError("a refusal touched the library")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    coll = torchmatch.Collection()
    with pytest.raises(ValueError, match="CUDA tensor"):
        coll.mutual_nn_each(torch.zeros((4, 128), dtype=torch.uint8))         # a CPU tensor
    with pytest.raises(ValueError, match="torch.Tensor"):
        coll.mutual_nn_each(np.zeros((4, 128), np.uint8))
    with pytest.raises(ValueError, match="cap"):
        coll.mutual_nn_each(torch.zeros((4, 128), dtype=torch.uint8), cap=-1)
    assert coll._coll is None


# ---- the reference on hand-made cases ---------------------------------------------------------------------------------------
def _rows(*vals):
    a = np.zeros((len(vals), 128), np.uint8)
    a[:, 0] = vals
    return a


def _bits(*vals):
    return np.array(vals, np.uint8)[:, None]


@pytest.mark.parametrize("binary", [False, True])
def test_reference_ties(binary):
    mk = _bits if binary else _rows
    # a train row elects the lowest query index on a tie: queries 0 and 1 are equal
    Q = mk(1, 1, 7)
    tidx, dist = ref.xcheck_each(Q, [mk(1)], binary)
    assert tidx.tolist() == [[0, -1, -1]] and dist[0, 0] == 0 and dist[0, 1] == INF
    # a query keeps the lowest train row on a tie: train rows 1 and 2 are equal, both elect query 0
    tidx, dist = ref.xcheck_each(mk(3), [mk(0, 3, 3)], binary)
    assert tidx.tolist() == [[1]] and dist[0, 0] == 0
    # one row present in two images matches in both; an empty image keeps its slot
    A, B, E = mk(1, 15), mk(15), mk()
    tidx, dist = ref.xcheck_each(mk(15, 1), [A, E, B], binary)
    assert tidx.tolist() == [[1, 0], [-1, -1], [0, -1]]
    assert dist[1].tolist() == [INF, INF] and dist[2, 0] == 0
    assert ref.counts(tidx).tolist() == [2, 0, 1]


def test_reference_max_dist_and_compaction():
    Q = _rows(0, 10, 20)
    images = [_rows(3, 14), _rows(20)]            # distances: image 0: q0 - t0 = 3, q1 - t1 = 4 (q2 elected by nobody); image 1: q2 - t0 = 0
    tidx, dist = ref.xcheck_each(Q, images)
    assert tidx.tolist() == [[0, 1, -1], [-1, -1, 0]] and dist[0, :2].tolist() == [3.0, 4.0]
    for md, want in ((np.inf, [[0, 1, -1], [-1, -1, 0]]), (4.0, [[0, -1, -1], [-1, -1, 0]]),          # equal to a distance: strict <
                     (np.nextafter(np.float32(4), INF), [[0, 1, -1], [-1, -1, 0]]),
                     (0.0, [[-1] * 3] * 2), (-1.0, [[-1] * 3] * 2), (np.nan, [[-1] * 3] * 2)):
        t, d = ref.xcheck_each(Q, images, max_dist=md)
        assert t.tolist() == want, md
        assert np.array_equal(d == INF, t < 0)
    rows, cnt, full = ref.compact(tidx, dist, cap=1)
    assert cnt.tolist() == [1, 1] and full.tolist() == [2, 1]
    assert rows[0, 0].tolist() == [0, 0, int(np.float32(3).view(np.int32))] and rows[1, 0].tolist() == [2, 0, 0]
    rows, cnt, full = ref.compact(tidx, dist)
    assert rows.shape == (2, 3, 3) and rows[0, 1].tolist() == [1, 1, int(np.float32(4).view(np.int32))] and (rows[0, 2] == -7).all()
    rows, cnt, full = ref.compact(tidx, dist, cap=0)
    assert rows.shape == (2, 0, 3) and cnt.tolist() == [0, 0] and full.tolist() == [2, 1]
