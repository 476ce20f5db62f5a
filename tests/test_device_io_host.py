"""CPU: the surface of ABI revision 12 (device sources, device results) -- the symbols exist and are bound as the header
declares them, and ``torchmatch`` refuses what it cannot take with ValueError before the library is loaded."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from fastmatch_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fm_bank_create_dev", "fm_knn_dev", "fm_xcheck1_dev", "fm_knn2_ratio_dev"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fastmatch_hip.h")).read(), flags=re.S)


def test_new_symbols_are_exported_and_bound():
    lib = _ffi.load_library()
    assert _ffi.FM_ABI_VERSION == 12 == lib.fm_abi_version()
    for name in NEW:
        assert name in _ffi.SYMBOLS
        assert hasattr(lib, name)
    for meth in ("bank_from_device", "knn_dev", "xcheck1_dev", "knn2_ratio_dev"):
        assert callable(getattr(_ffi.Context, meth))


def test_new_prototypes_match_the_binding():
    """Parameter by parameter, by the C type written in the header (stricter than the class check of test_abi.py)."""
    hdr = _header()
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


def test_dtype_codes_of_header_and_binding_agree():
    hdr = _header()
    for name in ("FM_DT_U8", "FM_DT_F32", "FM_DT_F16", "FM_DT_BF16", "FM_DT_BIN"):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == getattr(_ffi, name)


_REFUSALS = r"""
import sys
sys.path.insert(0, %r)
import fastmatch_amd
assert "torch" not in sys.modules, "importing the package pulled torch in"
from fastmatch_amd import torchmatch, _ffi
assert "torch" not in sys.modules, "importing torchmatch pulled torch in"
import numpy as np
import torch
bad = [torch.zeros(4, 128, dtype=torch.uint8),             # a CPU tensor
       torch.zeros(4, 128, dtype=torch.float32),
       np.zeros((4, 128), np.uint8),                        # not a tensor at all
       torch.zeros(4, 128, dtype=torch.float64),            # (CPU and the wrong dtype)
       torch.zeros(128, dtype=torch.uint8),                 # wrong rank
       torch.zeros(2, 4, 128, dtype=torch.float32)]
for x in bad:
    for call in (lambda: torchmatch.bank(x), lambda: torchmatch.knn(x, x, 2), lambda: torchmatch.mutual_nn(x, x),
                 lambda: torchmatch.ratio_match(x, x, 0.8), lambda: torchmatch.bank(x, binary=True)):
        try:
            call()
        except ValueError:
            continue
        raise SystemExit("no ValueError for %%r" %% (x,))
# dtype and rank are checked on their own, device or not: the meta device has shapes and dtypes and no memory
for x in (torch.zeros(4, 128, dtype=torch.float64, device="meta"), torch.zeros(4, 128, dtype=torch.int32, device="meta"),
          torch.zeros(128, dtype=torch.uint8, device="meta")):
    try:
        torchmatch._checked(x)
    except ValueError:
        continue
    raise SystemExit("no ValueError for %%r" %% (x,))
try:
    torchmatch.knn(torch.zeros(4, 128), torch.zeros(4, 128), 0)
except ValueError:
    pass
else:
    raise SystemExit("k = 0 accepted")
assert _ffi._lib is None, "a refusal loaded the library"
print("refused")
"""


def test_torchmatch_refuses_before_the_library_is_touched():
    """In a process of its own: the library must not have been loaded by the time every refusal has been raised, and
    neither the package nor torchmatch imports torch at import time."""
    r = subprocess.run([sys.executable, "-c", _REFUSALS % ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr


def test_torchmatch_has_no_import_time_torch():
    src = open(os.path.join(ROOT, "fast-match_amd", "torchmatch.py")).read()
    assert not re.search(r"^(import|from)\s+torch\b", src, flags=re.M)
