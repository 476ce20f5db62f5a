"""CPU: the host side of Fast-Match's accepted-match test on a train collection -- the two new prototypes of the header
against the ctypes binding, the ABI revision they leave alone, and BFMatcher.fastMatchEach's refusals, which touch no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from fastmatch_amd import _ffi, matchutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fm_collection_match_accepted_each", "fm_collection_match_accepted_each_dev")


def _header():
    """The header without its comments, as tests/test_abi.py reads it."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read(), flags=re.S)


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
def test_new_prototypes_match_the_binding(name):
    protos = dict(re.findall(r"\bint\s+(fm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S))
    assert name in protos, "the header does not declare %s" % name
    texts = protos[name].split(",")
    res, argtypes = _ffi.SYMBOLS[name]
    assert res is ctypes.c_int
    assert len(texts) == len(argtypes)
    assert [_klass_of_text(p) for p in texts] == [_klass_of_ctype(t) for t in argtypes]
    # what the issue fixes: (ctx, collection, query, tau, cap, ...)
    assert [_klass_of_text(p) for p in texts][:5] == ["ptr", "ptr", "ptr", "f64", "i64"]
    assert len(texts) == (10 if name == NEW[0] else 9)
    assert hasattr(_ffi.load_library(), name)


def test_abi_revision_is_still_12():
    hdr = open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()
    assert int(re.search(r"#define\s+FM_ABI_VERSION\s+(\d+)", hdr).group(1)) == 12
    assert _ffi.FM_ABI_VERSION == 12 and _ffi.load_library().fm_abi_version() == 12
    for name in NEW:                         # ... and the revision comment names the additions
        assert name in hdr.split("#define FM_ABI_VERSION")[0]


def test_not_built_list_of_the_collection_section():
    hdr = open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read()
    sect = hdr.split("---- train collections")[1].split("typedef struct fm_collection")[0]
    not_built = " ".join(sect.split("Not built:")[1].split())
    assert "self-distance test and" not in not_built
    for still in ("expansion loop on a collection", "per-image sweep", "binary collections in the self-distance test", "sharding a collection"):
        assert still in not_built, still


def test_fast_match_each_refusals_come_before_any_upload(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a refusal touched the device")
    monkeypatch.setattr(matchutil, "_context", no_device)
    q = np.zeros((4, 128), np.uint8)
    with pytest.raises(ValueError, match="no train descriptors"):
        matchutil.BFMatcher().fastMatchEach(q, 0.9)                       # nothing added
    with pytest.raises(ValueError, match="no train descriptors"):
        matchutil.BFMatcher(crossCheck=True).fastMatchEach_arrays(q, 0.9)
    h = matchutil.BFMatcher(matchutil.NORM_HAMMING)
    with pytest.raises(ValueError, match="NORM_HAMMING"):
        h.fastMatchEach(np.zeros((4, 32), np.uint8), 0.9)                 # (nothing added either: the norm is refused first)
    h.add([np.zeros((2, 32), np.uint8)])
    with pytest.raises(ValueError, match="NORM_HAMMING"):
        h.fastMatchEach(np.zeros((4, 32), np.uint8), 0.9)
    with pytest.raises(ValueError, match="NORM_HAMMING"):
        h.fastMatchEach_arrays(np.zeros((4, 32), np.uint8), 0.9)
