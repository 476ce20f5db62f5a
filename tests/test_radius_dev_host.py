"""CPU: the surface of radiusMatch on train collections and of its device forms (fm_collection_radius_match,
fm_radius_match_dev, fm_collection_radius_match_dev -- additions to ABI revision 12): declared, exported and bound; the
``torchmatch`` radius calls refuse a bad radius tensor with ValueError before a context or the library is touched; and
``BFMatcher.radiusMatch`` on a collection still refuses, naming the array-form route."""
import ctypes
import os
import re

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fm_collection_radius_match", "fm_radius_match_dev", "fm_collection_radius_match_dev"]


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
    assert callable(_ffi.Collection.radius_match) and callable(_ffi.Collection.radius_match_dev)
    assert callable(_ffi.Context.radius_match_dev)


def test_prototypes_match_the_binding():
    hdr = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    want = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}
    counts = {"fm_collection_radius_match": 11, "fm_radius_match_dev": 11, "fm_collection_radius_match_dev": 12}
    for name in NEW:
        params = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1).split(",")
        argtypes = _ffi.SYMBOLS[name][1]
        assert _ffi.SYMBOLS[name][0] is ctypes.c_int
        assert len(params) == len(argtypes) == counts[name], name
        for p, t in zip(params, argtypes):
            p = " ".join(p.split())
            if "*" in p:
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, p, t)
            else:
                assert t is want[p.replace("const ", "").split()[0]], (name, p, t)


def test_not_built_lists_name_what_is_left():
    text = " ".join(re.sub(r"\n \*", " ", _header_text()).split())
    assert "device results for fm_radius_match" not in text
    assert "Appendix A; neither cv2 nor its source was at hand), radiusMatch, masks" not in text
    for left in ("Hamming radiusMatch (for pairs or collections)", "an _each form", "skipping the second count sweep",
                 "sharding a collection across GPUs"):
        assert left in text, left
    assert "28 in the collection forms" in text                 # the chunk budget per candidate
    assert "the call DOES synchronise" in text


class _FakeCtx(object):
    device = 0


def _fake_bank(n):
    b = _ffi.Bank.__new__(_ffi.Bank)
    b.ctx, b.handle, b.n, b.dim, b.kind = _FakeCtx(), None, n, 128, _ffi.FM_BANK_I8
    return b


def test_torchmatch_radius_refusals_fire_before_the_library_is_touched(monkeypatch):
    import torch
    from fastmatch_amd import torchmatch

    def touched(*a, **k):
        raise AssertionError("a refusal reached the library")

    monkeypatch.setattr(_ffi, "default_context", touched)
    monkeypatch.setattr(_ffi, "load_library", touched)
    monkeypatch.setattr(_ffi, "Context", touched)
    monkeypatch.setattr(torchmatch, "_ctx_for", touched)
    monkeypatch.setattr(torchmatch, "_pair", touched)
    monkeypatch.setattr(torchmatch, "bank", touched)
    monkeypatch.setattr(_ffi.Context, "radius_match_dev", touched, raising=False)
    monkeypatch.setattr(_ffi.Collection, "radius_match_dev", touched)
    q, t = _fake_bank(6), _fake_bank(9)
    coll = torchmatch.Collection()
    monkeypatch.setattr(coll, "_query", touched)
    bad = [("a CPU tensor", torch.ones(6, dtype=torch.float32)),
           ("float64", torch.ones(6, dtype=torch.float64, device="meta")),
           ("float64 on the host", torch.ones(6, dtype=torch.float64)),
           ("the wrong length", torch.ones(7, dtype=torch.float32, device="meta")),
           ("2-D", torch.ones((6, 1), dtype=torch.float32, device="meta")),
           ("a host array of radii", np.ones(6, np.float32))]
    for what, r in bad:
        with pytest.raises(ValueError):
            torchmatch.radius_match(q, t, r)
        with pytest.raises(ValueError):
            coll.radius_match(q, r)
    # a query tensor that is refused is refused first, and as a ValueError too
    with pytest.raises(ValueError):
        torchmatch.radius_match(torch.zeros(4, 128, dtype=torch.uint8), t, 1.0)
    with pytest.raises(ValueError):
        coll.radius_match(torch.zeros(4, 128, dtype=torch.int16, device="meta"), 1.0)


def test_the_messages_say_which_rule():
    import torch
    from fastmatch_amd import torchmatch
    with pytest.raises(ValueError, match="float32"):
        torchmatch._radius(torch.ones(6, dtype=torch.float64, device="meta"), 6, 0)
    with pytest.raises(ValueError, match="1-D"):
        torchmatch._radius(torch.ones((6, 1), dtype=torch.float32, device="meta"), 6, 0)
    with pytest.raises(ValueError, match="7 radii for 6"):
        torchmatch._radius(torch.ones(7, dtype=torch.float32, device="meta"), 6, 0)
    with pytest.raises(ValueError, match="CUDA"):
        torchmatch._radius(torch.ones(6, dtype=torch.float32), 6, 0)
    assert torchmatch._radius(np.float32(2.5), 6, 0) == (None, 2.5) and torchmatch._radius(3, 6, 0) == (None, 3.0)


def test_bfmatcher_radius_match_on_a_collection_still_refuses_without_touching_the_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the refusal reached the device")

    monkeypatch.setattr(matchutil, "_context", touched)
    monkeypatch.setattr(_ffi, "default_context", touched)
    monkeypatch.setattr(_ffi, "load_library", touched)
    m = matchutil.BFMatcher()
    q = np.zeros((3, 128), np.uint8)
    for call in (lambda: m.radiusMatch(q, maxDistance=3.0), lambda: m.radiusMatch(q, 3.0)):
        with pytest.raises(ValueError, match="radiusMatch") as e:
            call()
        assert "Collection.radius_match" in str(e.value)         # the array-form route
