"""CPU: the surface of the device forms of the train collection (fm_collection_add_dev, fm_collection_knn_dev,
fm_collection_knn2_ratio_dev) -- additions to ABI revision 12: declared, exported and bound; and ``torchmatch.Collection.add``
refuses what it cannot take with ValueError before a context or the library is touched."""
import ctypes
import os
import re

import pytest

from fastmatch_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fm_collection_add_dev", "fm_collection_knn_dev", "fm_collection_knn2_ratio_dev"]


def _header_text():
    return open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()


def test_names_in_the_revision_comment_and_the_binding_table():
    text = _header_text()
    head = text[:text.index("#define FM_ABI_VERSION")]
    assert "still revision 12, additions only" in " ".join(head.split())
    for name in NEW:
        assert name in head, "%s is not named in the revision comment" % name
        assert name in _ffi.SYMBOLS
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", text).group(1)) == 12


def test_library_exports_them_and_the_version_stays_12():
    lib = _ffi.load_library()
    assert _ffi.FM_ABI_VERSION == 12 == lib.fm_abi_version()
    for name in NEW:
        assert hasattr(lib, name)
    for meth in ("add_from_device", "knn_dev", "knn2_ratio_dev"):
        assert callable(getattr(_ffi.Collection, meth))


def test_prototypes_match_the_binding():
    hdr = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    want = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name in NEW:
        params = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S).group(1).split(",")
        argtypes = _ffi.SYMBOLS[name][1]
        assert _ffi.SYMBOLS[name][0] is ctypes.c_int
        assert len(params) == len(argtypes), name
        for p, t in zip(params, argtypes):
            p = " ".join(p.split())
            if "*" in p:
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, p, t)
            else:
                assert t is want[p.replace("const ", "").split()[0]], (name, p, t)


def test_not_built_list_no_longer_names_collection_adds():
    text = " ".join(_header_text().split())
    assert "device sources for collection adds" not in text
    assert "Not built: device sources for fm_bank_refill_u8_async and fm_bank_append_*" in text


def test_torchmatch_collection_add_refuses_before_the_library_is_touched(monkeypatch):
    import torch
    from fastmatch_amd import torchmatch

    def touched(*a, **k):
        raise AssertionError("a refusal reached the library")

    monkeypatch.setattr(_ffi, "default_context", touched)
    monkeypatch.setattr(_ffi, "load_library", touched)
    monkeypatch.setattr(_ffi, "Context", touched)
    monkeypatch.setattr(torchmatch, "_ctx_for", touched)
    coll = torchmatch.Collection()
    bad = [(torch.zeros(4, 128, dtype=torch.uint8), False),                        # a CPU tensor
           (torch.zeros(128, dtype=torch.uint8, device="meta"), False),            # 1-D
           (torch.zeros(4, 128, dtype=torch.int16, device="meta"), False),         # a dtype that is not taken
           (torch.zeros(4, 32, dtype=torch.float32, device="meta"), True)]         # binary rows must be uint8
    for x, binary in bad:
        with pytest.raises(ValueError):
            coll.add(x, binary=binary)
    with pytest.raises(ValueError):
        coll.add(torch.zeros(4, 32, dtype=torch.float32), binary=True)
    with pytest.raises(ValueError):
        coll.knn(torch.zeros(4, 128, dtype=torch.uint8), 2)
    with pytest.raises(ValueError):
        coll.knn(torch.zeros(4, 128, dtype=torch.uint8), 0)
    assert coll.info() == (0, 0, 0, 0)
    coll.clear()
    coll.close()
