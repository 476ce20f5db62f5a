"""ctypes binding of libfastmatch_hip.so (C-ABI: include/fastmatch_hip.h).

This is the only bridge between the Python surface (fastmatch / cache / matchutil) and
the HIP kernels.  There is no CPU fallback: if the library is missing, or no gfx950
device is present, every compute entry point raises ``FastMatchHipError``.
"""
import ctypes
import weakref
import importlib.util
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfastmatch_hip.so")

FM_BANK_I8 = 1
FM_BANK_F32 = 2
FM_BANK_BIN = 3             # binary descriptors (Context.bank_binary): NORM_HAMMING
FM_BANK_F32W = 4            # float rows of 129 .. 256 values (Context.bank / bank_from_device make it for every such width)
# element types of rows in device memory (Context.bank_from_device)
FM_DT_U8, FM_DT_F32, FM_DT_F16, FM_DT_BF16, FM_DT_BIN = 1, 2, 3, 4, 5
FM_BANK_BIN2 = 5            # binary descriptors of 2-bit cells (Context.bank_binary2): NORM_HAMMING2
FM_DT_BIN2 = 6              # ... their rows in device memory (Context.bank_from_device; banks only)


class FastMatchHipError(RuntimeError):
    """Raised for every failure of the HIP path (the analogue of cv2.error).  ``code`` = the FM_E* status
    (-3 = FM_ENOMEM) when the library returned one."""
    code = None


class fm_stats(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("kernel_launches", ctypes.c_int64), ("pairs", ctypes.c_int64),
                ("calls", ctypes.c_int64)]


class fm_stats_ex(ctypes.Structure):
    _fields_ = [("struct_bytes", ctypes.c_int64), ("kernel_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("kernel_launches", ctypes.c_int64), ("pairs", ctypes.c_int64), ("calls", ctypes.c_int64),
                ("bytes_moved", ctypes.c_int64)]


FM_ABI_VERSION = 12         # include/fastmatch_hip.h: the revision this binding was written against


class fm_expand_desc(ctypes.Structure):
    _fields_ = [("query", ctypes.c_void_p), ("query_pos", ctypes.c_void_p),
                ("index_bucket", ctypes.c_double), ("index_x0", ctypes.c_double), ("index_y0", ctypes.c_double),
                ("index_nbx", ctypes.c_int32), ("index_nby", ctypes.c_int32),
                ("index_order", ctypes.c_void_p), ("index_start", ctypes.c_void_p),
                ("target", ctypes.c_void_p), ("cell_off", ctypes.c_void_p), ("target_pos", ctypes.c_void_p),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("cell_w", ctypes.c_int32), ("cell_h", ctypes.c_int32),
                ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("margin", ctypes.c_int32), ("radius", ctypes.c_int32),
                ("match_cap", ctypes.c_int64), ("stack_cap", ctypes.c_int64), ("metric", ctypes.c_int32),
                ("lazy", ctypes.c_int32)]


EXPAND_STATUS = {0: "ok", 1: "pending stack full", 2: "a radius subset the device could not take (see FM_EXPAND_SUBSET_FULL)",
                 3: "target position outside the image", 4: "result list full", 5: "hash table full",
                 6: "float32 round: candidate list full", 7: "lazy target: a cell is wanted", 9: "per-round log full"}
FM_EXPAND_NEED_CELL = 7     # include/fastmatch_hip.h

# name -> (restype, argtypes); every symbol include/fastmatch_hip.h declares
_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_INT = ctypes.c_int
_I32 = ctypes.c_int32
SYMBOLS = {
    "fm_ctx_create": (_INT, [_INT, ctypes.POINTER(_P)]),
    "fm_ctx_destroy": (_INT, [_P]),
    "fm_ctx_set_option": (_INT, [_P, ctypes.c_char_p, _I64]),
    "fm_ctx_get_option": (_INT, [_P, ctypes.c_char_p, ctypes.POINTER(_I64)]),
    "fm_last_error": (ctypes.c_char_p, [_P]),
    "fm_sync": (_INT, [_P]),
    "fm_abi_version": (_INT, []),
    "fm_get_stats": (_INT, [_P, ctypes.POINTER(fm_stats)]),
    "fm_get_stats_ex": (_INT, [_P, ctypes.POINTER(fm_stats_ex), _I64]),
    "fm_reset_stats": (_INT, [_P]),
    "fm_device_name": (_INT, [_P, ctypes.c_char_p, _INT]),
    "fm_f32_filter_stats": (_INT, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "fm_host_alloc": (_INT, [_P, _I64, ctypes.POINTER(_P)]),
    "fm_host_free": (_INT, [_P, _P]),
    "fm_bank_create_u8": (_INT, [_P, _P, _I64, _INT, ctypes.POINTER(_P)]),
    "fm_bank_create_f32": (_INT, [_P, _P, _I64, _INT, ctypes.POINTER(_P)]),
    "fm_bank_create_f32_route": (_INT, [_P, _P, _I64, _INT, ctypes.POINTER(_P)]),
    "fm_bank_create_bin": (_INT, [_P, _P, _I64, _INT, ctypes.POINTER(_P)]),
    "fm_bank_create_bin2": (_INT, [_P, _P, _I64, _INT, ctypes.POINTER(_P)]),
    "fm_bank_create_dev": (_INT, [_P, _P, _INT, _I64, _INT, _I64, _INT, _P, ctypes.POINTER(_P)]),
    "fm_knn_dev": (_INT, [_P, _P, _P, _I32, _P, _P, _P]),
    "fm_xcheck1_dev": (_INT, [_P, _P, _P, _P, _P, _P]),
    "fm_knn2_ratio_dev": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, ctypes.POINTER(_I64), _P]),
    "fm_bank_destroy": (_INT, [_P, _P]),
    "fm_bank_info": (_INT, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_INT), ctypes.POINTER(_INT)]),
    "fm_bank_set_selfdist": (_INT, [_P, _P, _P]),
    "fm_bank_refill_u8_async": (_INT, [_P, _P, _P, _I64]),
    "fm_bank_create_u8_cap": (_INT, [_P, _P, _I64, _INT, _I64, ctypes.POINTER(_P)]),
    "fm_grid_pack_cells": (_INT, [_P, _I64, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I64, _P, ctypes.POINTER(_I64), _P, _P]),
    "fm_bank_create_u8_gather": (_INT, [_P, _P, _I64, _INT, _P, _I64, ctypes.POINTER(_P)]),
    "fm_bank_create_f32_gather": (_INT, [_P, _P, _I64, _INT, _INT, _P, _I64, ctypes.POINTER(_P)]),
    "fm_bank_append_u8": (_INT, [_P, _P, _P, _I64, ctypes.POINTER(_I64)]),
    "fm_bank_create_f32_cap": (_INT, [_P, _INT, _I64, _P, ctypes.POINTER(_P)]),
    "fm_bank_append_f32": (_INT, [_P, _P, _P, _I64, ctypes.POINTER(_I64)]),
    "fm_expand_set_cell": (_INT, [_P, _P, ctypes.c_int32, _I64, _I64, _P]),
    "fm_expand_run_lazy": (_INT, [_P, _P, _P, _I64, ctypes.c_double, ctypes.c_int32, ctypes.POINTER(_I64), ctypes.POINTER(_I64),
                           ctypes.POINTER(_I64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "fm_upload_fence": (_INT, [_P]),
    "fm_self_dist_batch": (_INT, [_P, ctypes.c_int32, _P, _P]),
    "fm_knn2": (_INT, [_P, _P, _P, _P, _P]),
    "fm_knn": (_INT, [_P, _P, _P, ctypes.c_int32, _P, _P]),
    "fm_radius_match": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_xcheck1_keys": (_INT, [_P, _P, _P, _I64, _P]),
    "fm_xcheck1_keys_dev": (_INT, [_P, _P, _P, _I64, _P]),
    "fm_mutual_ratio": (_INT, [_P, _P, _P, ctypes.c_double, ctypes.c_int32, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_mutual_ratio_dev": (_INT, [_P, _P, _P, ctypes.c_double, ctypes.c_int32, _I64, _P, _P, ctypes.POINTER(_I64), _P]),
    "fm_knn2_ratio": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_self_dist": (_INT, [_P, _P, _P]),
    "fm_self_dist_plan": (_INT, [_I64, _I32, _P, _I64, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
    "fm_xcheck1": (_INT, [_P, _P, _P, _P, _P]),
    "fm_ratio_filter": (_INT, [_P, _P, _P, _P, _I64, ctypes.c_double, _P, _P, ctypes.POINTER(_I64)]),
    "fm_match_ratio": (_INT, [_P, _P, _P, ctypes.c_double, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_match_accepted": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_match_accepted_async": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, _P]),
    "fm_mark": (_INT, [_P, ctypes.POINTER(_I64)]),
    "fm_wait": (_INT, [_P, _I64]),
    "fm_expand_fetch_many": (_INT, [_P, ctypes.c_int32, _P, _P, ctypes.POINTER(_I64), _P, _P, _P]),
    "fm_match_accepted_batch": (_INT, [_P, ctypes.c_int32, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, _P]),
    "fm_match_accepted_dev_batch": (_INT, [_P, ctypes.c_int32, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P]),
    "fm_match_accepted_dev": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, ctypes.POINTER(_I64)]),
    "fm_match_accepted_dev_async": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P]),
    "fm_xcheck1_batched": (_INT, [_P, _P, _P, _P, _P, _P, _I64, _P, _P, _P]),
    "fm_expand_create": (_INT, [_P, ctypes.POINTER(fm_expand_desc), ctypes.POINTER(_P)]),
    "fm_expand_destroy": (_INT, [_P, _P]),
    "fm_expand_run": (_INT, [_P, ctypes.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fm_expand_fetch": (_INT, [_P, _P, _I64, _P, _P, _P]),
    "fm_expand_info": (_INT, [_P, ctypes.POINTER(_I64), ctypes.POINTER(ctypes.c_int32)]),
    "fm_expand_trim": (_INT, [_P, _P, ctypes.c_int32]),
    "fm_expand_set_log": (_INT, [_P, _P, ctypes.c_int32]),
    "fm_expand_log_counts": (_INT, [_P, _P, ctypes.c_int32, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "fm_expand_fetch_log": (_INT, [_P, _P, ctypes.c_int32, _I64, _I64, _P, _P, _P, _P]),
    "fm_mem_info": (_INT, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "fm_comm_unique_id": (_INT, [_P]),
    "fm_comm_init": (_INT, [_P, _INT, _INT, _P]),
    "fm_comm_destroy": (_INT, [_P]),
    "fm_gather_matches": (_INT, [_P, _P, _P, _I64, _P, _P, _INT]),
    "fm_gather_matches_counted": (_INT, [_P, _P, _P, _I64, _P, _P, ctypes.POINTER(_I64)]),
    "fm_collection_create": (_INT, [_P, ctypes.POINTER(_P)]),
    "fm_collection_destroy": (_INT, [_P, _P]),
    "fm_collection_clear": (_INT, [_P, _P]),
    "fm_collection_add_u8": (_INT, [_P, _P, _P, _I64, _INT, ctypes.POINTER(_I32)]),
    "fm_collection_add_f32": (_INT, [_P, _P, _P, _I64, _INT, ctypes.POINTER(_I32)]),
    "fm_collection_add_bin": (_INT, [_P, _P, _P, _I64, _INT, ctypes.POINTER(_I32)]),
    "fm_collection_train": (_INT, [_P, _P]),
    "fm_collection_info": (_INT, [_P, ctypes.POINTER(_I32), ctypes.POINTER(_I64), ctypes.POINTER(_INT), ctypes.POINTER(_INT)]),
    "fm_collection_image_rows": (_INT, [_P, _P]),
    "fm_collection_locate": (_INT, [_P, _I32, _P, _I64, _P, _P]),
    "fm_collection_knn": (_INT, [_P, _P, _P, _I32, _P, _P, _P]),
    "fm_collection_knn2_ratio": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_collection_knn2_each": (_INT, [_P, _P, _P, _P, _P]),
    "fm_collection_votes": (_INT, [_P, _P, _P, ctypes.c_double, _I32, _P]),
    "fm_collection_match_accepted_each": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, _P]),
    "fm_collection_match_accepted_each_dev": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P]),
    "fm_collection_xcheck1_each": (_INT, [_P, _P, _P, ctypes.c_float, _P, _P, _P]),
    "fm_collection_xcheck1_each_dev": (_INT, [_P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, _P]),
    "fm_collection_mutual_ratio_each": (_INT, [_P, _P, _P, ctypes.c_double, ctypes.c_int32, _I64, _P, _P, _P, _P, _P]),
    "fm_collection_mutual_ratio_each_dev": (_INT, [_P, _P, _P, ctypes.c_double, ctypes.c_int32, _I64, _P, _P, _P, _P]),
    "fm_collection_pairs_mutual_ratio": (_INT, [_P, _P, _P, _I64, ctypes.c_double, ctypes.c_int32, _I64, _P, _P, _P, _P, _P,
                                                ctypes.POINTER(_I64)]),
    "fm_collection_pairs_mutual_ratio_dev": (_INT, [_P, _P, _P, _I64, ctypes.c_double, ctypes.c_int32, _I64, _P, _P,
                                                    ctypes.POINTER(_I64), _P]),
    "fm_collection_add_dev": (_INT, [_P, _P, _P, _INT, _I64, _INT, _I64, _P, ctypes.POINTER(_I32)]),
    # wide collections (K14): images of 129 .. 256 float values per row, served by fm_collection_pairs_mutual_ratio(_dev)
    "fm_collection_add_wide": (_INT, [_P, _P, _P, _I64, _INT, ctypes.POINTER(_I32)]),
    "fm_collection_add_wide_dev": (_INT, [_P, _P, _P, _INT, _I64, _INT, _I64, _P, ctypes.POINTER(_I32)]),
    # a wide query bank against every image of a wide collection
    "fm_collection_wide_knn2_each": (_INT, [_P, _P, _P, _P, _P]),
    "fm_collection_wide_mutual_ratio_each": (_INT, [_P, _P, _P, ctypes.c_double, ctypes.c_int32, _I64, _P, _P, _P, _P, _P,
                                                    ctypes.POINTER(_I64)]),
    "fm_collection_wide_mutual_ratio_each_dev": (_INT, [_P, _P, _P, ctypes.c_double, ctypes.c_int32, _I64, _P, _P,
                                                        ctypes.POINTER(_I64), _P]),
    "fm_collection_knn_dev": (_INT, [_P, _P, _P, _I32, _P, _P, _P, _P]),
    "fm_collection_knn2_ratio_dev": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, ctypes.POINTER(_I64), _P]),
    "fm_collection_radius_match": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_radius_match_dev": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, ctypes.POINTER(_I64), _P]),
    "fm_collection_radius_match_dev": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64), _P]),
    "fm_hamming_radius_match": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_hamming_radius_match_dev": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, ctypes.POINTER(_I64), _P]),
    "fm_collection_hamming_radius_match": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_collection_hamming_radius_match_dev": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64), _P]),
    "fm_wide_radius_match": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_wide_radius_match_dev": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, ctypes.POINTER(_I64), _P]),
    "fm_collection_wide_radius_match": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_collection_wide_radius_match_dev": (_INT, [_P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64), _P]),
    # Wide stacked knnMatch (csrc/wide_stack.hip): the argument lists of fm_collection_knn(_dev) / _knn2_ratio(_dev) / _votes
    "fm_collection_wide_knn": (_INT, [_P, _P, _P, _I32, _P, _P, _P]),
    "fm_collection_wide_knn_dev": (_INT, [_P, _P, _P, _I32, _P, _P, _P, _P]),
    "fm_collection_wide_knn2_ratio": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_collection_wide_knn2_ratio_dev": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, ctypes.POINTER(_I64), _P]),
    "fm_collection_wide_votes": (_INT, [_P, _P, _P, ctypes.c_double, _I32, _P]),
    # Hamming Fast-Match: the self-distance test on binary banks (csrc/hamming.hip, ham_self_kernel)
    "fm_hamming_self_dist": (_INT, [_P, _P, _P]),
    "fm_hamming_self_dist_batch": (_INT, [_P, ctypes.c_int32, _P, _P]),
    "fm_hamming_set_selfdist": (_INT, [_P, _P, _P]),
    "fm_hamming_match_ratio": (_INT, [_P, _P, _P, ctypes.c_double, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_hamming_match_accepted": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_hamming_match_accepted_dev": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, ctypes.POINTER(_I64)]),
    "fm_collection_hamming_match_accepted_each": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, _P]),
    "fm_collection_hamming_match_accepted_each_dev": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P]),
    "fm_wide_self_dist": (_INT, [_P, _P, _P]),
    "fm_wide_self_dist_batch": (_INT, [_P, ctypes.c_int32, _P, _P]),
    "fm_wide_set_selfdist": (_INT, [_P, _P, _P]),
    "fm_wide_match_ratio": (_INT, [_P, _P, _P, ctypes.c_double, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_wide_match_accepted": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_wide_match_accepted_dev": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, ctypes.POINTER(_I64)]),
    "fm_collection_wide_match_accepted_each": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P, _P]),
    "fm_collection_wide_match_accepted_each_dev": (_INT, [_P, _P, _P, ctypes.c_double, _I64, _P, _P, _P, _P]),
    # K13: knnMatch under a mask (csrc/masked.hip)
    "fm_mask_create": (_INT, [_P, _I64, _I64, ctypes.POINTER(_P)]),
    "fm_mask_create_coll": (_INT, [_P, _I64, _P, ctypes.POINTER(_P)]),
    "fm_mask_set_u8": (_INT, [_P, _P, _I32, _P, _I64]),
    "fm_mask_set_dev": (_INT, [_P, _P, _I32, _P, _I64, _P]),
    "fm_mask_set_all": (_INT, [_P, _P, _I32, _I32]),
    "fm_mask_destroy": (_INT, [_P, _P]),
    "fm_mask_info": (_INT, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I32), ctypes.POINTER(_I64)]),
    "fm_knn_masked": (_INT, [_P, _P, _P, _P, _I32, _P, _P]),
    "fm_knn_masked_dev": (_INT, [_P, _P, _P, _P, _I32, _P, _P, _P]),
    "fm_wide_knn_masked": (_INT, [_P, _P, _P, _P, _I32, _P, _P]),            # wide float banks (csrc/wide_masked.hip)
    "fm_wide_knn_masked_dev": (_INT, [_P, _P, _P, _P, _I32, _P, _P, _P]),
    "fm_collection_knn_masked": (_INT, [_P, _P, _P, _P, _I32, _P, _P, _P]),
    "fm_collection_knn_masked_dev": (_INT, [_P, _P, _P, _P, _I32, _P, _P, _P, _P]),
    # masked radiusMatch on all four bank kinds (csrc/radius.hip, the masked sweeps): the unmasked lists with `mask` behind the train operand
    "fm_radius_match_masked": (_INT, [_P, _P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_radius_match_masked_dev": (_INT, [_P, _P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, ctypes.POINTER(_I64), _P]),
    "fm_collection_radius_match_masked": (_INT, [_P, _P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    "fm_collection_radius_match_masked_dev": (_INT, [_P, _P, _P, _P, _P, ctypes.c_float, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64), _P]),
}

_lib = None
_lib_lock = threading.Lock()


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so.7 (and
    HSA runtime) under torch/lib; if this library pulled in /opt/rocm's copy first, a later
    ``import torch`` would mix the two sets and find no GPU.  So when torch is installed but
    not imported yet, its bundled runtime is loaded first and both share it (the order
    ``import torch`` -> this library already behaves that way).  FM_SYSTEM_HIP_RUNTIME=1 skips it."""
    if "torch" in sys.modules or os.environ.get("FM_SYSTEM_HIP_RUNTIME") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except Exception:
        pass


def load_library():
    """dlopen libfastmatch_hip.so and declare every prototype.  Raises if missing."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        _preload_torch_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise FastMatchHipError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            raise FastMatchHipError("cannot load %s: %s" % (LIB_PATH, e))
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)     # AttributeError here = ABI drift, fail loudly
            fn.restype = res
            fn.argtypes = args
        if lib.fm_abi_version() != FM_ABI_VERSION:
            raise FastMatchHipError("%s has ABI revision %d, this binding was written for %d: rebuild the library"
                                    % (LIB_PATH, lib.fm_abi_version(), FM_ABI_VERSION))
        _lib = lib
        return lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def pairs_array(pairs, n_images=None):
    """A pair list of the match-graph calls as a C-contiguous int32 [n_pairs, 2] array: a sequence of (a, b) image indices or
    an integer array of that shape.  ``ValueError`` for anything else and, with ``n_images``, for an index outside
    [0, n_images).  (An empty list still owns storage, so that its address is not NULL: NULL means "every a < b".)"""
    if isinstance(pairs, np.ndarray) and pairs.dtype == np.int32 and pairs.ndim == 2 and pairs.shape[1] == 2 \
            and pairs.flags.c_contiguous and pairs.shape[0] > 0:
        arr = pairs
    else:
        try:
            src = np.asarray(pairs if isinstance(pairs, np.ndarray) else list(pairs))
        except TypeError:
            raise ValueError("pairs must be a sequence of (a, b) image indices")
        if src.size == 0:
            src = np.zeros((0, 2), np.int32)
        if src.ndim != 2 or src.shape[1] != 2 or src.dtype.kind not in "iu":
            raise ValueError("pairs must be a sequence of (a, b) integer image indices, shape [n_pairs, 2]")
        if src.size and (src.min() < -2 ** 31 or src.max() >= 2 ** 31):
            raise ValueError("pairs: an image index does not fit int32")
        arr = np.zeros((max(src.shape[0], 1), 2), np.int32)[:src.shape[0]]
        arr[...] = src
    if n_images is not None and arr.size and (arr.min() < 0 or arr.max() >= n_images):
        raise ValueError("pairs: an image index is outside [0, %d)" % n_images)
    return arr


def self_dist_plan(n_pad, stages=0):
    """fm_self_dist_plan (host code of the library): the workgroups of the triangular self-distance sweep of a bank
    padded to ``n_pad`` rows -> (table int32[n, 4] = (chunk, first stage, end stage, 0), n_diag, stages_used)."""
    lib = load_library()
    nwg, nd, su = _I32(), _I32(), _I32()
    rc = lib.fm_self_dist_plan(int(n_pad), int(stages), None, 0, ctypes.byref(nwg), ctypes.byref(nd), ctypes.byref(su))
    if rc == 0:
        table = np.empty((nwg.value, 4), dtype=np.int32)
        rc = lib.fm_self_dist_plan(int(n_pad), int(stages), _ptr(table), nwg.value, ctypes.byref(nwg), ctypes.byref(nd), ctypes.byref(su))
    if rc != 0:
        msg = lib.fm_last_error(None)
        e = FastMatchHipError("fm_self_dist_plan: %s" % (msg.decode() if msg else rc))
        e.code = rc
        raise e
    return table, nd.value, su.value


def grid_pack_cells(positions, width, height, cell_w, cell_h, rows, cols, margin):
    """fm_grid_pack_cells (host code of the library): (src_row int32[nt], target_pos f64[nt, 2], cell_off int64[rows * cols + 1])
    for a Grid_Cache over pre-extracted keypoints -- every cell's keypoints, cell after cell (cell id = col * rows + row)."""
    lib = load_library()
    pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 2)
    n = pos.shape[0]
    cell_off = np.zeros(int(rows) * int(cols) + 1, dtype=np.int64)
    cap = 5 * n + 16
    while True:
        src_row, t_pos, nt = np.empty(cap, dtype=np.int32), np.empty((cap, 2), dtype=np.float64), _I64()
        rc = lib.fm_grid_pack_cells(_ptr(pos), n, int(width), int(height), int(cell_w), int(cell_h), int(rows), int(cols), int(margin),
                                    cap, _ptr(cell_off), ctypes.byref(nt), _ptr(src_row), _ptr(t_pos))
        if rc != 0:
            msg = lib.fm_last_error(None)
            e = FastMatchHipError("fm_grid_pack_cells: %s" % (msg.decode() if msg else rc))
            e.code = rc
            raise e
        if nt.value <= cap:
            return src_row[:nt.value], t_pos[:nt.value], cell_off
        cap = nt.value


def _stream_arg(stream):
    """consumer_stream of the C-ABI: None -> FM_NO_STREAM, an integer handle (0 = the null stream) as is."""
    return _P(-1 & 0xFFFFFFFFFFFFFFFF) if stream is None else _P(int(stream))


class _LockedLib(object):
    """The library with every call serialised on one lock.  An fm_ctx is not re-entrant (it
    owns shared workspaces, the staging list and the timing events) and ctypes releases the
    GIL during a call, so two Python threads sharing a Context must not overlap inside it."""

    def __init__(self, lib):
        self._lib = lib
        self._lock = threading.RLock()
        self._wrapped = {}

    def __getattr__(self, name):
        fn = self._wrapped.get(name)
        if fn is None:
            raw, lock = getattr(self._lib, name), self._lock

            def fn(*args):
                with lock:
                    return raw(*args)
            self._wrapped[name] = fn
        return fn


class Bank(object):
    """Device-resident descriptor bank (fm_bank)."""

    def __init__(self, ctx, handle, n, dim, kind):
        self.ctx, self.handle, self.n, self.dim, self.kind = ctx, handle, n, dim, kind
        self.has_selfdist = False
        ctx._children.add(self)           # (a context that is closed first destroys what was made through it)

    def set_selfdist(self, selfdist, _name="fm_bank_set_selfdist"):
        sd = np.ascontiguousarray(selfdist, dtype=np.float64)
        if sd.shape != (self.n,):
            raise ValueError("selfdist must have shape (%d,)" % self.n)
        self.ctx._check(getattr(self.ctx.lib, _name)(self.ctx.handle, self.handle, _ptr(sd)))
        self.has_selfdist = True

    def set_hamming_selfdist(self, selfdist):
        """``fm_hamming_set_selfdist``: attach Hamming self distances (float64 [n]) to a binary bank."""
        self.set_selfdist(selfdist, _name="fm_hamming_set_selfdist")

    def set_wide_selfdist(self, selfdist):
        """``fm_wide_set_selfdist``: attach self distances (float64 [n]) to a wide float bank (FM_BANK_F32W)."""
        self.set_selfdist(selfdist, _name="fm_wide_set_selfdist")

    def refill_async(self, rows):
        """A new image's uint8 descriptors into this bank without allocation or host synchronisation
        (``fm_bank_refill_u8_async``): ``rows`` = [n, dim] uint8 from ``Context.pinned_empty`` with n within the
        bank's first size.  Nothing enqueued earlier may still read the bank; call ``Context.upload_fence()``
        before the first use, and recompute the self distances (``Context.self_dist_batch``)."""
        a = np.asarray(rows)
        if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != self.dim or not a.flags.c_contiguous:
            raise ValueError("rows must be a contiguous [n, %d] uint8 array" % self.dim)
        self.ctx._check(self.ctx.lib.fm_bank_refill_u8_async(self.ctx.handle, self.handle, _ptr(a), a.shape[0]))
        self.n = a.shape[0]
        self.has_selfdist = False
        self._refill_src = a          # (the copy is asynchronous: keep the source alive)

    def append(self, rows):
        """More uint8 rows into a bank made with room for them (``Context.bank_with_capacity``), placed at the next
        multiple of 32 rows; returns the index of the first one."""
        if self.kind == FM_BANK_F32:            # a growing float32-route bank (Context.bank_f32_with_capacity)
            a = np.ascontiguousarray(rows, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != self.dim:
                raise ValueError("rows must be [n, %d]" % self.dim)
            first = _I64(0)
            self.ctx._check(self.ctx.lib.fm_bank_append_f32(self.ctx.handle, self.handle, _ptr(a), a.shape[0], ctypes.byref(first)))
            if a.shape[0]:
                self.n = int(first.value) + a.shape[0]
            return int(first.value)
        a = np.ascontiguousarray(rows)
        if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != self.dim:
            raise ValueError("rows must be [n, %d] uint8" % self.dim)
        first = _I64(0)
        self.ctx._check(self.ctx.lib.fm_bank_append_u8(self.ctx.handle, self.handle, _ptr(a), a.shape[0], ctypes.byref(first)))
        if a.shape[0]:
            self.n = int(first.value) + a.shape[0]
        return int(first.value)

    def close(self):
        if self.handle is not None and self.ctx.handle is not None:
            self.ctx.lib.fm_bank_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def collection_locate(first_row, g):
    """``fm_collection_locate`` (host code, no context): (image int32[m], row int64[m]) of the logical global rows ``g`` of a
    collection whose image i starts at ``first_row[i]`` (``first_row[-1]`` = all rows); -1 / -1 for -1 or a row outside."""
    fr = np.ascontiguousarray(first_row, dtype=np.int64).reshape(-1)
    gg = np.ascontiguousarray(g, dtype=np.int64).reshape(-1)
    if fr.shape[0] < 1:
        raise ValueError("first_row needs n_images + 1 entries")
    img = np.empty(gg.shape[0], np.int32)
    loc = np.empty(gg.shape[0], np.int64)
    lib = load_library()
    rc = lib.fm_collection_locate(_ptr(fr), fr.shape[0] - 1, _ptr(gg), gg.shape[0], _ptr(img), _ptr(loc))
    if rc != 0:
        msg = lib.fm_last_error(None)
        raise FastMatchHipError("fm_collection_locate failed (%d): %s" % (rc, msg.decode() if msg else "?"))
    return img, loc


class Mask(object):
    """A match mask (fm_mask): a device-resident bit matrix over (query row, train row) -- cv2's ``mask`` argument of
    ``knnMatch`` for a bank pair (``Context.mask(nq, nt)``), or one matrix per image of a train collection
    (``Collection.mask(nq)``: cv2's ``masks``).  New masks forbid everything.  A context manager; closes with its context."""

    def __init__(self, ctx, handle, coll=None):
        self.ctx, self.handle, self.coll = ctx, handle, coll
        self.nq, self.nt, self.n_images, self.nbytes = self.info()
        ctx._children.add(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def info(self):
        """(nq, real train rows, images -- 0 for a pair mask --, bytes of the bit matrix)"""
        nq, nt, ni, nb = _I64(), _I64(), _I32(), _I64()
        self.ctx._check(self.ctx.lib.fm_mask_info(self.handle, ctypes.byref(nq), ctypes.byref(nt), ctypes.byref(ni), ctypes.byref(nb)))
        return int(nq.value), int(nt.value), int(ni.value), int(nb.value)

    def set(self, rows, img=0):
        """``fm_mask_set_u8``: ``rows`` = [nq, rows of image ``img``] uint8 / bool, nonzero = the pair may be matched."""
        a = np.asarray(rows)
        if a.dtype == np.bool_:
            a = a.view(np.uint8)
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError("a mask is a 2-D [nq, nt] uint8 or bool array, got %s %s" % (a.dtype, a.shape))
        if a.shape[0] != self.nq:
            raise ValueError("the mask has %d rows, the Mask was made for %d query rows" % (a.shape[0], self.nq))
        if a.shape[1] and a.strides[1] != 1 or (a.shape[0] > 1 and a.strides[0] < a.shape[1]):
            a = np.ascontiguousarray(a)
        pitch = a.strides[0] if a.shape[0] > 1 and a.shape[1] else 0
        self.ctx._check(self.ctx.lib.fm_mask_set_u8(self.ctx.handle, self.handle, int(img), _ptr(a) if a.size else None, int(pitch)))
        return self

    def set_dev(self, ptr, img=0, pitch=0, stream=None):
        """``fm_mask_set_dev``: the same from device memory (``ptr`` = device address of [nq, rows of the image] bytes, ``pitch``
        bytes between rows, 0 = dense; a ``torch.bool`` tensor is one byte per element); ``stream`` as in
        ``Context.bank_from_device``.  On return the source may be overwritten."""
        self.ctx._check(self.ctx.lib.fm_mask_set_dev(self.ctx.handle, self.handle, int(img), _P(int(ptr)) if ptr else None, int(pitch),
                                                     _stream_arg(stream)))
        return self

    def set_all(self, value=True, img=0):
        """``fm_mask_set_all``: every row of image ``img`` permitted (or forbidden) for every query row."""
        self.ctx._check(self.ctx.lib.fm_mask_set_all(self.ctx.handle, self.handle, int(img), 1 if value else 0))
        return self

    def close(self):
        if self.handle is not None and self.ctx.handle is not None:
            self.ctx.lib.fm_mask_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Collection(object):
    """Train collection (fm_collection): an ordered list of images resident on the device in one set of arrays --
    ``cv2.BFMatcher.add`` / ``train`` / ``clear``.  A context manager; closes with its context."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.handle = None
        h = _P()
        ctx._check(ctx.lib.fm_collection_create(ctx.handle, ctypes.byref(h)))
        self.handle = h
        ctx._children.add(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def add(self, rows):
        """Append one image ([n, dim] uint8, or float32 with integer values in 0 .. 255; n may be 0); returns its index."""
        a = np.asarray(rows)
        if a.ndim != 2:
            raise ValueError("an image's descriptors must be 2-D [n, dim]")
        i = _I32(-1)
        if a.dtype == np.uint8:
            a = np.ascontiguousarray(a)
            fn = self.ctx.lib.fm_collection_add_u8
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
            fn = self.ctx.lib.fm_collection_add_f32
        self.ctx._check(fn(self.ctx.handle, self.handle, _ptr(a) if a.shape[0] else None, a.shape[0], a.shape[1], ctypes.byref(i)))
        return int(i.value)

    def add_binary(self, rows):
        a = np.ascontiguousarray(rows, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("an image's descriptors must be 2-D [n, bytes]")
        i = _I32(-1)
        self.ctx._check(self.ctx.lib.fm_collection_add_bin(self.ctx.handle, self.handle, _ptr(a) if a.shape[0] else None,
                                                           a.shape[0], a.shape[1], ctypes.byref(i)))
        return int(i.value)

    def add_from_device(self, ptr, dtype, n, dim, pitch=0, stream=None):
        """Append one image whose ``n`` rows of ``dim`` elements are already in device memory (``fm_collection_add_dev``);
        ``ptr`` / ``dtype`` / ``pitch`` / ``stream`` as in ``Context.bank_from_device`` (``FM_DT_BIN``: dim = bytes per row).
        The collection is the one ``add`` / ``add_binary`` builds from the same values on the host; on return the source may
        be overwritten.  Returns the image's index."""
        i = _I32(-1)
        self.ctx._check(self.ctx.lib.fm_collection_add_dev(self.ctx.handle, self.handle, _P(int(ptr)) if ptr else None, int(dtype),
                                                           int(n), int(dim), int(pitch), _stream_arg(stream), ctypes.byref(i)))
        return int(i.value)

    def add_wide(self, rows):
        """Append one WIDE image ([n, dim] float32, 129 <= dim <= 256, any values; n may be 0) -- ``fm_collection_add_wide``.
        The first one makes the collection a wide one (kind ``FM_BANK_F32W``): it takes no other images and serves ``info``,
        ``image_rows``, ``train``, ``clear``, the ``pairs_mutual_ratio*`` calls and, for a wide query bank, ``wide_knn2_each``
        and the ``wide_mutual_ratio_each*`` calls.  Returns the image's index."""
        a = np.ascontiguousarray(rows, dtype=np.float32)
        if a.ndim != 2:
            raise ValueError("an image's descriptors must be 2-D [n, dim]")
        i = _I32(-1)
        self.ctx._check(self.ctx.lib.fm_collection_add_wide(self.ctx.handle, self.handle, _ptr(a) if a.shape[0] else None, a.shape[0],
                                                            a.shape[1], ctypes.byref(i)))
        return int(i.value)

    def add_wide_from_device(self, ptr, dtype, n, dim, pitch=0, stream=None):
        """``add_wide`` from rows in device memory (``fm_collection_add_wide_dev``): ``FM_DT_F32`` / ``FM_DT_F16`` /
        ``FM_DT_BF16`` elements, otherwise as ``add_from_device``.  The collection is the one ``add_wide`` builds from the same
        (widened) values."""
        i = _I32(-1)
        self.ctx._check(self.ctx.lib.fm_collection_add_wide_dev(self.ctx.handle, self.handle, _P(int(ptr)) if ptr else None, int(dtype),
                                                                int(n), int(dim), int(pitch), _stream_arg(stream), ctypes.byref(i)))
        return int(i.value)

    def knn_dev(self, q, k, img_ptr, idx_ptr, dist_ptr, consumer_stream=None, _name="fm_collection_knn_dev"):
        """``knn`` with the lists left on the device (``fm_collection_knn_dev``): device addresses of int32 / int32 / float32
        [nq, k] buffers; enqueued, ``consumer_stream`` as in ``Context.knn_dev``."""
        self.ctx._check(getattr(self.ctx.lib, _name)(
            self.ctx.handle, self.handle, q.handle, int(k), _P(int(img_ptr)) if img_ptr else None,
            _P(int(idx_ptr)) if idx_ptr else None, _P(int(dist_ptr)) if dist_ptr else None, _stream_arg(consumer_stream)))

    def knn2_ratio_dev(self, q, tau, rows_ptr, count_ptr, cap, want_count=False, consumer_stream=None,
                       _name="fm_collection_knn2_ratio_dev"):
        """``knn2_ratio`` with the accepted matches left on the device (``fm_collection_knn2_ratio_dev``): ``rows_ptr`` = device
        address of an int32 [cap, 4] buffer (query, image, row inside the image, float32 distance bits), ``count_ptr`` of an
        int64 word that receives min(accepted, cap).  ``want_count``: also return the full number accepted (one host
        synchronisation); else None."""
        n = _I64(0)
        self.ctx._check(getattr(self.ctx.lib, _name)(
            self.ctx.handle, self.handle, q.handle, float(tau), int(cap), _P(int(rows_ptr)) if rows_ptr else None,
            _P(int(count_ptr)) if count_ptr else None, ctypes.byref(n) if want_count else None, _stream_arg(consumer_stream)))
        return int(n.value) if want_count else None

    def wide_knn_dev(self, q, k, img_ptr, idx_ptr, dist_ptr, consumer_stream=None):
        """``wide_knn`` with the lists left on the device (``fm_collection_wide_knn_dev``); arguments as ``knn_dev``."""
        self.knn_dev(q, k, img_ptr, idx_ptr, dist_ptr, consumer_stream, _name="fm_collection_wide_knn_dev")

    def wide_knn2_ratio_dev(self, q, tau, rows_ptr, count_ptr, cap, want_count=False, consumer_stream=None):
        """``wide_knn2_ratio`` with the accepted matches left on the device (``fm_collection_wide_knn2_ratio_dev``); arguments
        and return value as ``knn2_ratio_dev``."""
        return self.knn2_ratio_dev(q, tau, rows_ptr, count_ptr, cap, want_count, consumer_stream,
                                   _name="fm_collection_wide_knn2_ratio_dev")

    def radius_match(self, q, r, _name="fm_collection_radius_match"):
        """``fm_collection_radius_match``: every row of the stacked images with distance < r per query row.  ``r`` is a scalar
        or a float32 [nq] array.  Returns (offsets int64[nq + 1], img int32[n], idx int32[n], dist float32[n]): row i's list is
        img / idx / dist[offsets[i]:offsets[i + 1]], ascending (distance, image, row inside the image).  A counts call sizes
        the arrays, a second call fills them."""
        nq = q.n
        if np.ndim(r) == 0:
            rad, r_all = None, float(np.float32(r))
        else:
            rad = np.ascontiguousarray(r, dtype=np.float32).reshape(-1)
            if rad.shape[0] != nq:
                raise ValueError("radius_match: %d radii for %d query rows" % (rad.shape[0], nq))
            r_all = 0.0
        rp = _ptr(rad) if rad is not None and nq > 0 else None
        offsets = np.zeros(nq + 1, dtype=np.int64)
        total = _I64(0)
        fn = getattr(self.ctx.lib, _name)
        self.ctx._check(fn(self.ctx.handle, self.handle, q.handle, rp, r_all, 0, _ptr(offsets), None, None, None, ctypes.byref(total)))
        n = int(total.value)
        img = np.empty(n, dtype=np.int32)
        idx = np.empty(n, dtype=np.int32)
        dist = np.empty(n, dtype=np.float32)
        if n > 0:
            self.ctx._check(fn(self.ctx.handle, self.handle, q.handle, rp, r_all, n, _ptr(offsets), _ptr(img), _ptr(idx), _ptr(dist),
                               ctypes.byref(total)))
            if int(total.value) != n:
                raise FastMatchHipError("%s: %d entries on the second call, %d on the first" % (_name, total.value, n))
        return offsets, img, idx, dist

    def radius_match_masked(self, q, mask, r):
        """``fm_collection_radius_match_masked``: ``radius_match`` (an integer, float32 or binary collection: for a binary one
        ``hamming_radius_match``) with every entry whose pair ``mask`` (``Collection.mask``) forbids removed; nothing else
        changes.  Arguments after ``mask`` and the return value as ``radius_match``."""
        nq = q.n
        if np.ndim(r) == 0:
            rad, r_all = None, float(np.float32(r))
        else:
            rad = np.ascontiguousarray(r, dtype=np.float32).reshape(-1)
            if rad.shape[0] != nq:
                raise ValueError("radius_match_masked: %d radii for %d query rows" % (rad.shape[0], nq))
            r_all = 0.0
        rp = _ptr(rad) if rad is not None and nq > 0 else None
        mh = mask.handle if mask is not None else None
        offsets = np.zeros(nq + 1, dtype=np.int64)
        total = _I64(0)
        fn = self.ctx.lib.fm_collection_radius_match_masked
        self.ctx._check(fn(self.ctx.handle, self.handle, q.handle, mh, rp, r_all, 0, _ptr(offsets), None, None, None, ctypes.byref(total)))
        n = int(total.value)
        img = np.empty(n, dtype=np.int32)
        idx = np.empty(n, dtype=np.int32)
        dist = np.empty(n, dtype=np.float32)
        if n > 0:
            self.ctx._check(fn(self.ctx.handle, self.handle, q.handle, mh, rp, r_all, n, _ptr(offsets), _ptr(img), _ptr(idx), _ptr(dist),
                               ctypes.byref(total)))
            if int(total.value) != n:
                raise FastMatchHipError("fm_collection_radius_match_masked: %d entries on the second call, %d on the first" % (total.value, n))
        return offsets, img, idx, dist

    def radius_match_masked_dev(self, q, mask, radius_ptr, radius_all, cap, offsets_ptr, img_ptr, idx_ptr, dist_ptr, want_total=True,
                                consumer_stream=None):
        """``radius_match_masked`` with the radii read from and the lists left in device memory
        (``fm_collection_radius_match_masked_dev``); arguments after ``mask`` as ``radius_match_dev``."""
        n = _I64(0)
        self.ctx._check(self.ctx.lib.fm_collection_radius_match_masked_dev(
            self.ctx.handle, self.handle, q.handle, mask.handle if mask is not None else None,
            _P(int(radius_ptr)) if radius_ptr else None, float(np.float32(radius_all)), int(cap),
            _P(int(offsets_ptr)) if offsets_ptr else None, _P(int(img_ptr)) if img_ptr else None, _P(int(idx_ptr)) if idx_ptr else None,
            _P(int(dist_ptr)) if dist_ptr else None, ctypes.byref(n) if want_total else None, _stream_arg(consumer_stream)))
        return int(n.value) if want_total else None

    def hamming_radius_match(self, q, r):
        """``fm_collection_hamming_radius_match``: ``radius_match`` of a binary query against a binary collection -- every
        row of the stacked images with ``popcount(q XOR t) < r`` (strict, float32; ``h <= H`` is ``r = H + 0.5``), lists
        ascending (h, image, row inside the image).  Arguments and return value as ``radius_match``."""
        return self.radius_match(q, r, _name="fm_collection_hamming_radius_match")

    def hamming_radius_match_dev(self, q, radius_ptr, radius_all, cap, offsets_ptr, img_ptr, idx_ptr, dist_ptr, want_total=True,
                                 consumer_stream=None):
        """``hamming_radius_match`` with the radii read from and the lists left in device memory
        (``fm_collection_hamming_radius_match_dev``); arguments as ``radius_match_dev``."""
        return self.radius_match_dev(q, radius_ptr, radius_all, cap, offsets_ptr, img_ptr, idx_ptr, dist_ptr, want_total,
                                     consumer_stream, _name="fm_collection_hamming_radius_match_dev")

    def wide_radius_match(self, q, r):
        """``fm_collection_wide_radius_match``: ``radius_match`` of a wide float query bank (129 .. 256 values per row) against
        a wide collection (``add_wide``) -- every row of the stacked images with K14's distance < r, lists ascending
        (distance, image, row inside the image).  Arguments and return value as ``radius_match``."""
        return self.radius_match(q, r, _name="fm_collection_wide_radius_match")

    def wide_radius_match_dev(self, q, radius_ptr, radius_all, cap, offsets_ptr, img_ptr, idx_ptr, dist_ptr, want_total=True,
                              consumer_stream=None):
        """``wide_radius_match`` with the radii read from and the lists left in device memory
        (``fm_collection_wide_radius_match_dev``); arguments as ``radius_match_dev``."""
        return self.radius_match_dev(q, radius_ptr, radius_all, cap, offsets_ptr, img_ptr, idx_ptr, dist_ptr, want_total,
                                     consumer_stream, _name="fm_collection_wide_radius_match_dev")

    def radius_match_dev(self, q, radius_ptr, radius_all, cap, offsets_ptr, img_ptr, idx_ptr, dist_ptr, want_total=True,
                         consumer_stream=None, _name="fm_collection_radius_match_dev"):
        """``radius_match`` with the radii read from and the lists left in device memory (``fm_collection_radius_match_dev``):
        ``radius_ptr`` = device address of float32 [nq] radii, or 0 for the scalar ``radius_all``; ``offsets_ptr`` of an int64
        [nq + 1] buffer; ``img_ptr`` / ``idx_ptr`` / ``dist_ptr`` of int32 / int32 / float32 [cap] buffers (0 with cap = 0).
        Returns the number of entries (``want_total``) or None.  The call synchronises (the counts plan the chunks);
        ``consumer_stream`` as in ``Context.knn_dev``."""
        n = _I64(0)
        self.ctx._check(getattr(self.ctx.lib, _name)(
            self.ctx.handle, self.handle, q.handle, _P(int(radius_ptr)) if radius_ptr else None, float(np.float32(radius_all)), int(cap),
            _P(int(offsets_ptr)) if offsets_ptr else None, _P(int(img_ptr)) if img_ptr else None, _P(int(idx_ptr)) if idx_ptr else None,
            _P(int(dist_ptr)) if dist_ptr else None, ctypes.byref(n) if want_total else None, _stream_arg(consumer_stream)))
        return int(n.value) if want_total else None

    def train(self):
        self.ctx._check(self.ctx.lib.fm_collection_train(self.ctx.handle, self.handle))

    def clear(self):
        self.ctx._check(self.ctx.lib.fm_collection_clear(self.ctx.handle, self.handle))

    def info(self):
        """(n_images, n_rows_total, dim, kind)"""
        ni, nr, dim, kind = _I32(), _I64(), _INT(), _INT()
        self.ctx._check(self.ctx.lib.fm_collection_info(self.handle, ctypes.byref(ni), ctypes.byref(nr), ctypes.byref(dim), ctypes.byref(kind)))
        return int(ni.value), int(nr.value), int(dim.value), int(kind.value)

    def image_rows(self):
        rows = np.zeros(self.info()[0], np.int64)
        self.ctx._check(self.ctx.lib.fm_collection_image_rows(self.handle, _ptr(rows) if rows.shape[0] else None))
        return rows

    def knn(self, q, k, _name="fm_collection_knn"):
        """``fm_collection_knn``: (img, idx, dist) [nq, k] against the stacked rows of all images."""
        k = int(k)
        img = np.empty((q.n, max(k, 0)), np.int32)
        idx = np.empty((q.n, max(k, 0)), np.int32)
        dist = np.empty((q.n, max(k, 0)), np.float32)
        self.ctx._check(getattr(self.ctx.lib, _name)(self.ctx.handle, self.handle, q.handle, k, _ptr(img), _ptr(idx), _ptr(dist)))
        return img, idx, dist

    def wide_knn(self, q, k):
        """``fm_collection_wide_knn``: ``knn`` of a wide float query bank (129 .. 256 values per row) against the stacked rows
        of a wide collection (``add_wide``), k = 1, 2: (img, idx, dist) [nq, k], the lists ``Context.knn`` gives for one bank of
        the images' rows concatenated, every entry as (image, row inside the image)."""
        return self.knn(q, k, _name="fm_collection_wide_knn")

    def mask(self, nq):
        """An all-forbidding ``Mask`` for ``nq`` query rows laid out on this collection's images as they are now
        (``fm_mask_create_coll``); a later ``add`` / ``clear`` makes it stale."""
        h = _P()
        self.ctx._check(self.ctx.lib.fm_mask_create_coll(self.ctx.handle, int(nq), self.handle, ctypes.byref(h)))
        return Mask(self.ctx, h, self)

    def knn_masked(self, q, mask, k):
        """``fm_collection_knn_masked``: ``knn`` over the train rows ``mask`` (``Collection.mask``) permits per query row."""
        k = int(k)
        img = np.empty((q.n, max(k, 0)), np.int32)
        idx = np.empty((q.n, max(k, 0)), np.int32)
        dist = np.empty((q.n, max(k, 0)), np.float32)
        self.ctx._check(self.ctx.lib.fm_collection_knn_masked(self.ctx.handle, self.handle, q.handle, mask.handle if mask is not None else None,
                                                              k, _ptr(img), _ptr(idx), _ptr(dist)))
        return img, idx, dist

    def knn_masked_dev(self, q, mask, k, img_ptr, idx_ptr, dist_ptr, consumer_stream=None):
        """``knn_masked`` with the lists left on the device (``fm_collection_knn_masked_dev``); pointers and ``consumer_stream``
        as in ``knn_dev``."""
        self.ctx._check(self.ctx.lib.fm_collection_knn_masked_dev(
            self.ctx.handle, self.handle, q.handle, mask.handle if mask is not None else None, int(k),
            _P(int(img_ptr)) if img_ptr else None, _P(int(idx_ptr)) if idx_ptr else None, _P(int(dist_ptr)) if dist_ptr else None,
            _stream_arg(consumer_stream)))

    def knn2_ratio(self, q, tau, _name="fm_collection_knn2_ratio"):
        """``fm_collection_knn2_ratio``: (qidx, img, tidx, dist, ratio) of the accepted matches, ascending query index."""
        cap = q.n
        qidx, img, tidx = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int32)
        dist, ratio = np.empty(cap, np.float32), np.empty(cap, np.float64)
        n = _I64(0)
        self.ctx._check(getattr(self.ctx.lib, _name)(self.ctx.handle, self.handle, q.handle, float(tau), cap, _ptr(qidx),
                                                     _ptr(img), _ptr(tidx), _ptr(dist), _ptr(ratio), ctypes.byref(n)))
        m = min(int(n.value), cap)
        return qidx[:m], img[:m], tidx[:m], dist[:m], ratio[:m]

    def wide_knn2_ratio(self, q, tau):
        """``fm_collection_wide_knn2_ratio``: ``knn2_ratio`` of a wide query bank against a wide collection -- Lowe's ratio
        test on the 2-NN lists over ALL images' rows."""
        return self.knn2_ratio(q, tau, _name="fm_collection_wide_knn2_ratio")

    def knn2_each(self, q):
        """``fm_collection_knn2_each``: (idx, dist) [n_images, nq, 2], slot by slot ``Context.knn2(q, image_i)``."""
        ni = self.info()[0]
        idx = np.empty((ni, q.n, 2), np.int32)
        dist = np.empty((ni, q.n, 2), np.float32)
        self.ctx._check(self.ctx.lib.fm_collection_knn2_each(self.ctx.handle, self.handle, q.handle, _ptr(idx), _ptr(dist)))
        return idx, dist

    def votes(self, q, tau, mode=0, _name="fm_collection_votes"):
        """``fm_collection_votes``: int64[n_images] query rows passing the ratio test per image (mode 0: stacked lists, 1: per image)."""
        v = np.zeros(self.info()[0], np.int64)
        self.ctx._check(getattr(self.ctx.lib, _name)(self.ctx.handle, self.handle, q.handle, float(tau), int(mode),
                                                     _ptr(v) if v.shape[0] else None))
        return v

    def wide_votes(self, q, tau, mode=0):
        """``fm_collection_wide_votes``: ``votes`` of a wide query bank against a wide collection."""
        return self.votes(q, tau, mode, _name="fm_collection_wide_votes")

    def hamming_match_accepted_each(self, q, tau, cap=None):
        """``fm_collection_hamming_match_accepted_each``: ``match_accepted_each`` on a binary collection -- slot i equal to
        ``Context.hamming_match_accepted(q, bank(image_i), tau)``; ``q`` is a binary bank with Hamming self distances."""
        return self.match_accepted_each(q, tau, cap, _name="fm_collection_hamming_match_accepted_each")

    def hamming_match_accepted_each_dev(self, q, tau, rows_ptr, counts_ptr, cap, h_counts=None, consumer_stream=None):
        """``match_accepted_each_dev`` on a binary collection (``fm_collection_hamming_match_accepted_each_dev``)."""
        return self.match_accepted_each_dev(q, tau, rows_ptr, counts_ptr, cap, h_counts, consumer_stream,
                                            _name="fm_collection_hamming_match_accepted_each_dev")

    def wide_match_accepted_each(self, q, tau, cap=None):
        """``fm_collection_wide_match_accepted_each``: ``match_accepted_each`` on a wide collection -- slot i equal to
        ``Context.wide_match_accepted(q, bank(image_i), tau)``; ``q`` is a wide float bank with wide self distances."""
        return self.match_accepted_each(q, tau, cap, _name="fm_collection_wide_match_accepted_each")

    def wide_match_accepted_each_dev(self, q, tau, rows_ptr, counts_ptr, cap, h_counts=None, consumer_stream=None):
        """``match_accepted_each_dev`` on a wide collection (``fm_collection_wide_match_accepted_each_dev``)."""
        return self.match_accepted_each_dev(q, tau, rows_ptr, counts_ptr, cap, h_counts, consumer_stream,
                                            _name="fm_collection_wide_match_accepted_each_dev")

    def match_accepted_each(self, q, tau, cap=None, _name="fm_collection_match_accepted_each"):
        """``fm_collection_match_accepted_each``: Fast-Match's accepted-match test of ``q`` (a bank with self distances) inside
        every image separately -- a list of (qidx, tidx, dist, ratio) per image, slot i equal to
        ``Context.match_accepted(q, bank(image_i), tau)``; ``tidx`` is the row inside the image.  ``cap`` (default ``q.n``)
        bounds the rows returned per image."""
        ni = self.info()[0]
        cap = q.n if cap is None else int(cap)
        kept = max(cap, 0)
        qidx, tidx = np.empty((ni, kept), np.int32), np.empty((ni, kept), np.int32)
        dist, ratio = np.empty((ni, kept), np.float32), np.empty((ni, kept), np.float64)
        n = np.zeros(ni, np.int64)
        self.ctx._check(getattr(self.ctx.lib, _name)(
            self.ctx.handle, self.handle, q.handle, float(tau), cap, _ptr(qidx) if qidx.size else None,
            _ptr(tidx) if tidx.size else None, _ptr(dist) if dist.size else None, _ptr(ratio) if ratio.size else None,
            _ptr(n) if ni else None))
        out = []
        for i in range(ni):
            m = min(int(n[i]), kept)
            out.append((qidx[i, :m], tidx[i, :m], dist[i, :m], ratio[i, :m]))
        return out

    def accepted_votes(self, q, tau):
        """int64[n_images]: the number of matches ``match_accepted_each`` accepts per image (its counts-only call, cap = 0:
        only n_images words come back)."""
        n = np.zeros(self.info()[0], np.int64)
        self.ctx._check(self.ctx.lib.fm_collection_match_accepted_each(self.ctx.handle, self.handle, q.handle, float(tau), 0,
                                                                       None, None, None, None, _ptr(n) if n.shape[0] else None))
        return n

    def match_accepted_each_dev(self, q, tau, rows_ptr, counts_ptr, cap, h_counts=None, consumer_stream=None,
                                _name="fm_collection_match_accepted_each_dev"):
        """``match_accepted_each`` with device outputs (``fm_collection_match_accepted_each_dev``), as
        ``Context.match_accepted_dev_batch``: ``rows_ptr`` = device address of an int32 [n_images, cap, 3] block (query, row
        inside the image, float32 distance bits), ``counts_ptr`` of an int64 [n_images] array that receives min(count, cap);
        ``h_counts`` = an int64 [n_images] host array for the full counts (the call then synchronises once) or None
        (enqueued only); ``consumer_stream`` as in ``Context.match_accepted_dev_async``."""
        ni = self.info()[0]
        if h_counts is not None and (not isinstance(h_counts, np.ndarray) or h_counts.dtype != np.int64 or h_counts.size < ni
                                     or not h_counts.flags.c_contiguous):
            raise ValueError("h_counts must be a contiguous int64 array of n_images words")
        self.ctx._check(getattr(self.ctx.lib, _name)(
            self.ctx.handle, self.handle, q.handle, float(tau), int(cap), _P(int(rows_ptr)) if rows_ptr else None,
            _P(int(counts_ptr)) if counts_ptr else None, _ptr(h_counts) if h_counts is not None else None,
            _stream_arg(consumer_stream)))

    def xcheck1_each(self, q, max_dist=float("inf")):
        """``fm_collection_xcheck1_each``: the cross-checked 1-NN of ``q`` inside every image separately --
        ``(tidx int32 [n_images, nq], dist float32 [n_images, nq])``, slot i equal to ``Context.xcheck1(q, bank(image_i))``
        (-1 / inf: unmatched); a match is kept while ``dist < max_dist`` (strict; inf: every match, <= 0 or NaN: none)."""
        ni = self.info()[0]
        tidx, dist = np.full((ni, q.n), -1, np.int32), np.full((ni, q.n), np.inf, np.float32)
        if tidx.size:
            self.ctx._check(self.ctx.lib.fm_collection_xcheck1_each(self.ctx.handle, self.handle, q.handle, float(max_dist),
                                                                    _ptr(tidx), _ptr(dist), None))
        else:       # (nothing to fill: the call still checks the pair)
            n = np.zeros(ni, np.int64)
            self.ctx._check(self.ctx.lib.fm_collection_xcheck1_each(self.ctx.handle, self.handle, q.handle, float(max_dist),
                                                                    None, None, _ptr(n) if ni else None))
        return tidx, dist

    def mutual_votes(self, q, max_dist=float("inf")):
        """int64[n_images]: the number of query rows ``xcheck1_each`` matches per image (its counts-only call: only n_images
        words come back)."""
        n = np.zeros(self.info()[0], np.int64)
        self.ctx._check(self.ctx.lib.fm_collection_xcheck1_each(self.ctx.handle, self.handle, q.handle, float(max_dist), None, None,
                                                                _ptr(n) if n.shape[0] else None))
        return n

    def xcheck1_each_dev(self, q, max_dist, rows_ptr, counts_ptr, cap, h_counts=None, consumer_stream=None):
        """``xcheck1_each`` with device outputs (``fm_collection_xcheck1_each_dev``); the arguments are those of
        ``match_accepted_each_dev`` with ``max_dist`` in the place of ``tau``: ``rows_ptr`` = device address of an int32
        [n_images, cap, 3] block (query, row inside the image, float32 distance bits), ``counts_ptr`` of an int64 [n_images]
        array that receives min(count, cap); ``h_counts`` = an int64 [n_images] host array for the full counts (the call then
        synchronises once) or None (enqueued only)."""
        ni = self.info()[0]
        if h_counts is not None and (not isinstance(h_counts, np.ndarray) or h_counts.dtype != np.int64 or h_counts.size < ni
                                     or not h_counts.flags.c_contiguous):
            raise ValueError("h_counts must be a contiguous int64 array of n_images words")
        self.ctx._check(self.ctx.lib.fm_collection_xcheck1_each_dev(
            self.ctx.handle, self.handle, q.handle, float(max_dist), int(cap), _P(int(rows_ptr)) if rows_ptr else None,
            _P(int(counts_ptr)) if counts_ptr else None, _ptr(h_counts) if h_counts is not None else None,
            _stream_arg(consumer_stream)))

    def mutual_ratio_each(self, q, tau, symmetric=False, cap=None):
        """``fm_collection_mutual_ratio_each``: mutual nearest neighbours + ratio test of ``q`` inside every image separately
        -- a list of (qidx, tidx, dist, ratio) per image, slot i equal to ``Context.mutual_ratio(q, bank(image_i), tau,
        symmetric)``; ``tidx`` is the row inside the image.  ``cap`` (default ``q.n``) bounds the rows returned per image."""
        ni = self.info()[0]
        cap = q.n if cap is None else int(cap)
        kept = max(cap, 0)
        qidx, tidx = np.empty((ni, kept), np.int32), np.empty((ni, kept), np.int32)
        dist, ratio = np.empty((ni, kept), np.float32), np.empty((ni, kept), np.float64)
        n = np.zeros(ni, np.int64)
        self.ctx._check(self.ctx.lib.fm_collection_mutual_ratio_each(
            self.ctx.handle, self.handle, q.handle, float(tau), int(bool(symmetric)), cap, _ptr(qidx) if qidx.size else None,
            _ptr(tidx) if tidx.size else None, _ptr(dist) if dist.size else None, _ptr(ratio) if ratio.size else None,
            _ptr(n) if ni else None))
        out = []
        for i in range(ni):
            m = min(int(n[i]), kept)
            out.append((qidx[i, :m], tidx[i, :m], dist[i, :m], ratio[i, :m]))
        return out

    def mutual_ratio_votes(self, q, tau, symmetric=False):
        """int64[n_images]: the number of matches ``mutual_ratio_each`` accepts per image (its counts-only call, cap = 0: only
        n_images words come back)."""
        n = np.zeros(self.info()[0], np.int64)
        self.ctx._check(self.ctx.lib.fm_collection_mutual_ratio_each(self.ctx.handle, self.handle, q.handle, float(tau),
                                                                     int(bool(symmetric)), 0, None, None, None, None,
                                                                     _ptr(n) if n.shape[0] else None))
        return n

    def mutual_ratio_each_dev(self, q, tau, symmetric, rows_ptr, counts_ptr, cap, h_counts=None, consumer_stream=None):
        """``mutual_ratio_each`` with device outputs (``fm_collection_mutual_ratio_each_dev``); rows, counts, ``h_counts`` and
        ``consumer_stream`` are those of ``xcheck1_each_dev``: ``rows_ptr`` = device address of an int32 [n_images, cap, 3]
        block (query, row inside the image, float32 distance bits), ``counts_ptr`` of an int64 [n_images] array that receives
        min(count, cap); ``h_counts`` = an int64 [n_images] host array for the full counts, or None."""
        ni = self.info()[0]
        if h_counts is not None and (not isinstance(h_counts, np.ndarray) or h_counts.dtype != np.int64 or h_counts.size < ni
                                     or not h_counts.flags.c_contiguous):
            raise ValueError("h_counts must be a contiguous int64 array of n_images words")
        self.ctx._check(self.ctx.lib.fm_collection_mutual_ratio_each_dev(
            self.ctx.handle, self.handle, q.handle, float(tau), int(bool(symmetric)), int(cap), _P(int(rows_ptr)) if rows_ptr else None,
            _P(int(counts_ptr)) if counts_ptr else None, _ptr(h_counts) if h_counts is not None else None,
            _stream_arg(consumer_stream)))

    def _pairs(self, pairs):
        ni = self.info()[0]
        if pairs is None:
            return None, ni * (ni - 1) // 2
        arr = pairs_array(pairs)
        return arr, arr.shape[0]

    def pairs_mutual_ratio_counts(self, pairs=None, tau=0.8, symmetric=False):
        """int64[n_pairs + 1]: the offsets of ``pairs_mutual_ratio`` alone (its counts-only call, cap = 0) -- the number of
        matches of pair p is ``offsets[p + 1] - offsets[p]``, the edge weights of the match graph."""
        arr, n = self._pairs(pairs)
        offsets = np.zeros(n + 1, np.int64)
        self.ctx._check(self.ctx.lib.fm_collection_pairs_mutual_ratio(
            self.ctx.handle, self.handle, _ptr(arr), n, float(tau), int(bool(symmetric)), 0,
            _ptr(offsets), None, None, None, None, None))
        return offsets

    def pairs_mutual_ratio(self, pairs=None, tau=0.8, symmetric=False, cap=None):
        """``fm_collection_pairs_mutual_ratio``: the images of the collection matched against each other.  ``pairs``: a
        sequence of ordered (a, b) image indices, or None for every a < b in lexicographic order.  A list of (qidx, tidx,
        dist, ratio) per pair, entry p equal to ``Context.mutual_ratio(bank(image_a), bank(image_b), tau, symmetric)``:
        ``qidx`` is the row inside image a, ``tidx`` the row inside image b.  ``cap`` None: the counts first, then one fill
        call of exactly that size; else the rows of the longest prefix of whole pairs that fits are returned and the later
        pairs come back empty."""
        arr, n = self._pairs(pairs)
        if cap is None:
            cap = int(self.pairs_mutual_ratio_counts(arr if pairs is not None else None, tau, symmetric)[-1])
        cap = int(cap)
        kept = max(cap, 0)
        qidx, tidx = np.empty(kept, np.int32), np.empty(kept, np.int32)
        dist, ratio = np.empty(kept, np.float32), np.empty(kept, np.float64)
        offsets = np.zeros(n + 1, np.int64)
        self.ctx._check(self.ctx.lib.fm_collection_pairs_mutual_ratio(
            self.ctx.handle, self.handle, _ptr(arr), n, float(tau), int(bool(symmetric)), cap,
            _ptr(offsets), _ptr(qidx) if kept else None, _ptr(tidx) if kept else None, _ptr(dist) if kept else None,
            _ptr(ratio) if kept else None, None))
        out = []
        for p in range(n):
            lo, hi = int(offsets[p]), int(offsets[p + 1])
            if hi > kept:
                lo = hi = 0
            out.append((qidx[lo:hi], tidx[lo:hi], dist[lo:hi], ratio[lo:hi]))
        return out

    def pairs_mutual_ratio_dev(self, pairs, tau, symmetric, offsets_ptr, rows_ptr, cap, want_total=False, consumer_stream=None):
        """``pairs_mutual_ratio`` with device outputs (``fm_collection_pairs_mutual_ratio_dev``): ``offsets_ptr`` = device
        address of an int64 [n_pairs + 1] array, ``rows_ptr`` of an int32 [cap, 3] block (row in a, row in b, float32
        distance bits).  Enqueued only; ``want_total``: also return the total number of matches (the call's one host wait)."""
        arr, n = self._pairs(pairs)
        total = _I64(0)
        self.ctx._check(self.ctx.lib.fm_collection_pairs_mutual_ratio_dev(
            self.ctx.handle, self.handle, _ptr(arr), n, float(tau), int(bool(symmetric)), int(cap),
            _P(int(offsets_ptr)) if offsets_ptr else None, _P(int(rows_ptr)) if rows_ptr else None,
            ctypes.byref(total) if want_total else None, _stream_arg(consumer_stream)))
        return int(total.value) if want_total else None

    def wide_knn2_each(self, q):
        """``fm_collection_wide_knn2_each``: a wide query bank against every image of a wide collection -- (idx, dist)
        [n_images, nq, 2], slot i equal to ``Context.knn2(q, bank(image_i))``."""
        ni = self.info()[0]
        idx = np.empty((ni, q.n, 2), np.int32)
        dist = np.empty((ni, q.n, 2), np.float32)
        self.ctx._check(self.ctx.lib.fm_collection_wide_knn2_each(self.ctx.handle, self.handle, q.handle,
                                                                  _ptr(idx) if idx.size else None, _ptr(dist) if dist.size else None))
        return idx, dist

    def wide_mutual_ratio_each_counts(self, q, tau, symmetric=False):
        """int64[n_images + 1]: the offsets of ``wide_mutual_ratio_each`` alone (its counts-only call, cap = 0) -- the number
        of matches of image i is ``offsets[i + 1] - offsets[i]``, the per-image votes."""
        offsets = np.zeros(self.info()[0] + 1, np.int64)
        self.ctx._check(self.ctx.lib.fm_collection_wide_mutual_ratio_each(
            self.ctx.handle, self.handle, q.handle, float(tau), int(bool(symmetric)), 0, _ptr(offsets), None, None, None, None, None))
        return offsets

    def wide_mutual_ratio_each(self, q, tau, symmetric=False, cap=None):
        """``fm_collection_wide_mutual_ratio_each``: a wide query bank matched against every image of a wide collection,
        image by image.  A list of (qidx, tidx, dist, ratio) per image, entry i equal to
        ``Context.mutual_ratio(q, bank(image_i), tau, symmetric)``: ``qidx`` is the query row, ``tidx`` the row inside image
        i.  ``cap`` None: the counts first, then one fill call of exactly that size; else the rows of the longest prefix of
        whole images that fits are returned and the later images come back empty."""
        n = self.info()[0]
        if cap is None:
            cap = int(self.wide_mutual_ratio_each_counts(q, tau, symmetric)[-1])
        cap = int(cap)
        kept = max(cap, 0)
        qidx, tidx = np.empty(kept, np.int32), np.empty(kept, np.int32)
        dist, ratio = np.empty(kept, np.float32), np.empty(kept, np.float64)
        offsets = np.zeros(n + 1, np.int64)
        self.ctx._check(self.ctx.lib.fm_collection_wide_mutual_ratio_each(
            self.ctx.handle, self.handle, q.handle, float(tau), int(bool(symmetric)), cap,
            _ptr(offsets), _ptr(qidx) if kept else None, _ptr(tidx) if kept else None, _ptr(dist) if kept else None,
            _ptr(ratio) if kept else None, None))
        out = []
        for p in range(n):
            lo, hi = int(offsets[p]), int(offsets[p + 1])
            if hi > kept:
                lo = hi = 0
            out.append((qidx[lo:hi], tidx[lo:hi], dist[lo:hi], ratio[lo:hi]))
        return out

    def wide_mutual_ratio_each_dev(self, q, tau, symmetric, offsets_ptr, rows_ptr, cap, want_total=False, consumer_stream=None):
        """``wide_mutual_ratio_each`` with device outputs (``fm_collection_wide_mutual_ratio_each_dev``): ``offsets_ptr`` =
        device address of an int64 [n_images + 1] array, ``rows_ptr`` of an int32 [cap, 3] block (query row, row inside the
        image, float32 distance bits).  Enqueued only; ``want_total``: also return the total number of matches (the call's
        one host wait)."""
        total = _I64(0)
        self.ctx._check(self.ctx.lib.fm_collection_wide_mutual_ratio_each_dev(
            self.ctx.handle, self.handle, q.handle, float(tau), int(bool(symmetric)), int(cap),
            _P(int(offsets_ptr)) if offsets_ptr else None, _P(int(rows_ptr)) if rows_ptr else None,
            ctypes.byref(total) if want_total else None, _stream_arg(consumer_stream)))
        return int(total.value) if want_total else None

    def close(self):
        if self.handle is not None and self.ctx.handle is not None:
            self.ctx.lib.fm_collection_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Expander(object):
    """Device-resident expansion state of one image pair (fm_expand)."""

    def __init__(self, ctx, q_bank, q_pos, index, t_bank, cell_off, t_pos, grid, radius,
                 match_cap=0, stack_cap=0, lazy=False):
        """``lazy``: the target's cells are added one by one (``set_cell``) as the loop asks for them (``run_lazy``);
        ``t_bank`` is then a bank from ``Context.bank_with_capacity`` and ``cell_off`` / ``t_pos`` are None."""
        self.ctx = ctx
        self.handle = None
        self.lazy = bool(lazy)
        # keep every host array alive until fm_expand_create has copied it
        q_pos = np.ascontiguousarray(q_pos, dtype=np.float64).reshape(-1, 2)
        order = np.ascontiguousarray(index.order, dtype=np.int32)
        start = np.ascontiguousarray(index.start, dtype=np.int32)
        cell_off = None if lazy else np.ascontiguousarray(cell_off, dtype=np.int64)
        t_pos = None if lazy else np.ascontiguousarray(t_pos, dtype=np.float64).reshape(-1, 2)
        d = fm_expand_desc()
        d.query, d.query_pos = q_bank.handle, _ptr(q_pos)
        d.index_bucket, d.index_x0, d.index_y0 = index.bucket, index.x0, index.y0
        d.index_nbx, d.index_nby = index.nbx, index.nby
        d.index_order, d.index_start = _ptr(order), _ptr(start)
        d.target, d.cell_off, d.target_pos = t_bank.handle, _ptr(cell_off), _ptr(t_pos)
        d.width, d.height = grid["width"], grid["height"]
        d.cell_w, d.cell_h = grid["cell_w"], grid["cell_h"]
        d.rows, d.cols, d.margin, d.radius = grid["rows"], grid["cols"], grid["margin"], int(radius)
        d.match_cap, d.stack_cap = int(match_cap), int(stack_cap)
        d.metric = int(getattr(index, "metric", 0))         # Position_Index.metric = FM_METRIC_*
        d.lazy = 1 if lazy else 0
        h = _P()
        ctx._check(ctx.lib.fm_expand_create(ctx.handle, ctypes.byref(d), ctypes.byref(h)))
        self.handle = h
        ctx._children.add(self)
        self._banks = (q_bank, t_bank)            # the banks must outlive the expander
        # host copies of the positions the log's records are rebuilt from (fetch_log)
        self.q_pos = q_pos
        self.t_pos = t_pos
        self._lazy_pos = {}                       # lazy targets: first row -> positions of the cell added there
        self.logging = False

    def set_log(self, enable=True, first_capacity=0):
        """Runs of this pair record the reference's per-round log on the device (fm_expand_set_log);
        ``first_capacity`` > 1: the log arrays start that small (they grow fourfold when a run fills them)."""
        if bool(enable) != self.logging or first_capacity > 1:
            self.ctx._check(self.ctx.lib.fm_expand_set_log(self.ctx.handle, self.handle,
                                                           int(first_capacity) if enable and first_capacity > 1 else (1 if enable else 0)))
            self.logging = bool(enable)

    def fetch_log(self, slot=0):
        """The log of the last run in ``slot``: (query_pos f64[n, 2], target_pos f64[n, 2], cell i64[n], n_accepted i64[n]
        (-1: the cell had no features, -2: no cross-checked pair), query_row i32[m], target_row i32[m], ratio f64[m]) -- rounds in order, the accepted
        matches of all rounds back to back."""
        nr, ne = _I64(0), _I64(0)
        self.ctx._check(self.ctx.lib.fm_expand_log_counts(self.ctx.handle, self.handle, int(slot), ctypes.byref(nr), ctypes.byref(ne)))
        rounds = np.empty((nr.value, 6), dtype=np.int64)
        q, t, ratio = np.empty(ne.value, dtype=np.int32), np.empty(ne.value, dtype=np.int32), np.empty(ne.value, dtype=np.float64)
        self.ctx._check(self.ctx.lib.fm_expand_fetch_log(self.ctx.handle, self.handle, int(slot), nr.value, ne.value,
                                                         _ptr(rounds), _ptr(q), _ptr(t), _ptr(ratio)))
        pos = np.ascontiguousarray(rounds[:, :4]).view(np.float64)
        return pos[:, 0:2], pos[:, 2:4], rounds[:, 4].copy(), rounds[:, 5].copy(), q, t, ratio

    def target_positions(self):
        """Full-image positions of the target bank's rows (lazy targets: of the cells added so far)."""
        if not self.lazy:
            return self.t_pos
        n = max([r + len(p) for r, p in self._lazy_pos.items()] + [0])
        out = np.zeros((n, 2), dtype=np.float64)
        for r, p in self._lazy_pos.items():
            out[r:r + len(p)] = p
        return out

    def set_cell(self, cell, first_row, positions):
        """Register a computed cell of a lazy target: rows [first_row, first_row + len(positions)) of the target bank."""
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 2)
        self.ctx._check(self.ctx.lib.fm_expand_set_cell(self.ctx.handle, self.handle, int(cell), int(first_row), pos.shape[0],
                                                        _ptr(pos) if pos.shape[0] else None))
        if pos.shape[0]:
            self._lazy_pos[int(first_row)] = pos

    def run_lazy(self, seeds, tau, resume):
        """One launch of a lazy pair: (n_matches, n_rounds, n_pairs, status, need_cell); status 7 = compute ``need_cell``
        (col * rows + row), ``set_cell`` it and call again with ``resume=True``."""
        seeds = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 2, 2)
        nm, nr, npairs = _I64(0), _I64(0), _I64(0)
        st, need = ctypes.c_int32(0), ctypes.c_int32(-1)
        self.ctx._check(self.ctx.lib.fm_expand_run_lazy(self.ctx.handle, self.handle, _ptr(seeds) if seeds.shape[0] else None,
                                                        seeds.shape[0], float(tau), 1 if resume else 0, ctypes.byref(nm),
                                                        ctypes.byref(nr), ctypes.byref(npairs), ctypes.byref(st), ctypes.byref(need)))
        return int(nm.value), int(nr.value), int(npairs.value), int(st.value), int(need.value)

    def info(self):
        """(bytes of one run state, run states that exist): see fm_expand_info."""
        b, k = _I64(0), ctypes.c_int32(0)
        self.ctx._check(self.ctx.lib.fm_expand_info(self.handle, ctypes.byref(b), ctypes.byref(k)))
        return int(b.value), int(k.value)

    def trim(self, keep=1):
        """Free the run states from slot ``keep`` on (they are re-created on demand)."""
        self.ctx._check(self.ctx.lib.fm_expand_trim(self.ctx.handle, self.handle, int(keep)))

    def fetch(self, n):
        index = np.empty(n, dtype=np.int32)
        pos = np.empty((n, 2, 2), dtype=np.float64)
        ratio = np.empty(n, dtype=np.float64)
        self.ctx._check(self.ctx.lib.fm_expand_fetch(self.ctx.handle, self.handle, n, _ptr(index), _ptr(pos), _ptr(ratio)))
        return index, pos, ratio

    def close(self):
        if self.handle is not None and self.ctx.handle is not None:
            self.ctx.lib.fm_expand_destroy(self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(object):
    """One fm_ctx (= one device + one HIP stream)."""

    def __init__(self, device=0):
        self.lib = _LockedLib(load_library())
        self.handle = None
        h = _P()
        rc = self.lib.fm_ctx_create(int(device), ctypes.byref(h))
        if rc != 0:
            msg = self.lib.fm_last_error(None)
            raise FastMatchHipError("fm_ctx_create(%d) failed (%d): %s"
                                    % (device, rc, msg.decode() if msg else "?"))
        self.handle = h
        self.device = int(device)
        # banks and expanders made through this context (weak references): fm_bank_destroy / fm_expand_destroy need a live
        # context, so close() destroys the ones still open first -- r06's memory soak found 9.5 MB of device memory per
        # context left behind by `c.close()` with banks open (their own close() could no longer reach the library)
        self._children = weakref.WeakSet()

    def _check(self, rc):
        if rc != 0:
            msg = self.lib.fm_last_error(self.handle) if self.handle is not None else None
            e = FastMatchHipError("libfastmatch_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
            e.code = rc
            raise e

    def close(self):
        if self.handle is not None:
            kids = list(getattr(self, "_children", ()))
            for k in kids:                        # expanders first: they borrow their banks
                if isinstance(k, Expander):
                    k.close()
            for k in kids:
                if not isinstance(k, Expander):
                    k.close()
            for p in getattr(self, "_pinned", []):
                self.lib.fm_host_free(self.handle, p)
            self._pinned = []
            self.lib.fm_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        """Per-context tuning / batch shape (fm_ctx_set_option): "batch_group", "batch_tail", "nsplit", "nb",
        "nw", "nbuf", "prio", "glds", "coop", "f32_filter", "f32_nw", "f32_nsplit", "f32_fused", "f32_lpc", "f32_bound_every",
        "async_time_every", "k1_order", "bound_every", "self_tri", "tri_stages", "refill_grid", "expand_big", "expand_huge", "expand_delegate", "expand_grow", "expand_prof",
        "radius_ws_bytes", "coll_ws_bytes", "fp6_filter", "fp6_cap", "fp6_nsplit", "masked_mfma", "mask_pack_words".  Results never depend on them."""
        self._check(self.lib.fm_ctx_set_option(self.handle, name.encode(), int(value)))

    def get_option(self, name):
        v = _I64(0)
        self._check(self.lib.fm_ctx_get_option(self.handle, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def pinned_empty(self, shape, dtype):
        """ndarray in page-locked host memory (lives as long as the context): pass it as an
        ``out=`` buffer so results arrive by direct DMA."""
        dt = np.dtype(dtype)
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        nbytes = int(np.prod(shape)) * dt.itemsize
        p = _P()
        self._check(self.lib.fm_host_alloc(self.handle, nbytes, ctypes.byref(p)))
        if not hasattr(self, "_pinned"):
            self._pinned = []
        self._pinned.append(p)
        buf = (ctypes.c_char * max(nbytes, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    # -- banks -------------------------------------------------------------------------
    def bank(self, rows, float_route=False):
        """Upload an [n, dim] uint8 or float32 matrix.  Other dtypes are converted to
        float32 first (cv2 would reject them).  Float rows of 129 .. 256 values make a wide float bank (``FM_BANK_F32W``:
        knn with k <= 2, xcheck1, knn2_ratio, mutual_ratio and their device forms), whatever the values.  ``float_route``: keep the float32 route even
        if the values are integers (to pair with a bank that is not integer valued)."""
        a = np.asarray(rows)
        if a.ndim != 2:
            raise ValueError("descriptor bank must be 2-D [n, dim]")
        h = _P()
        if float_route:
            a = np.ascontiguousarray(a, dtype=np.float32)
            self._check(self.lib.fm_bank_create_f32_route(self.handle, _ptr(a), a.shape[0], a.shape[1], ctypes.byref(h)))
        elif a.dtype == np.uint8:
            a = np.ascontiguousarray(a)
            self._check(self.lib.fm_bank_create_u8(self.handle, _ptr(a), a.shape[0], a.shape[1], ctypes.byref(h)))
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
            self._check(self.lib.fm_bank_create_f32(self.handle, _ptr(a), a.shape[0], a.shape[1], ctypes.byref(h)))
        n, dim, kind = _I64(), _INT(), _INT()
        self._check(self.lib.fm_bank_info(h, ctypes.byref(n), ctypes.byref(dim), ctypes.byref(kind)))
        return Bank(self, h, n.value, dim.value, kind.value)

    def bank_binary(self, rows):
        """Upload binary descriptors (ORB, BRIEF, BRISK, FREAK, AKAZE): uint8 [n, bytes], 1 <= bytes <= 64, for NORM_HAMMING
        (``fm_bank_create_bin``; kind ``FM_BANK_BIN``).  knn2 / knn / xcheck1 / knn2_ratio take a pair of such banks."""
        a = np.asarray(rows)
        if a.ndim != 2:
            raise ValueError("descriptor bank must be 2-D [n, bytes]")
        if a.dtype != np.uint8:
            raise ValueError("binary descriptors must be uint8 (cv2 asserts CV_8U for NORM_HAMMING), got %s" % a.dtype)
        a = np.ascontiguousarray(a)
        h = _P()
        self._check(self.lib.fm_bank_create_bin(self.handle, _ptr(a) if a.shape[0] else None, a.shape[0], a.shape[1], ctypes.byref(h)))
        n, dim, kind = _I64(), _INT(), _INT()
        self._check(self.lib.fm_bank_info(h, ctypes.byref(n), ctypes.byref(dim), ctypes.byref(kind)))
        return Bank(self, h, n.value, dim.value, kind.value)

    def bank_binary2(self, rows):
        """Upload binary descriptors whose elements are 2-bit values (ORB with ``WTA_K`` = 3 or 4): uint8 [n, bytes],
        1 <= bytes <= 64, for NORM_HAMMING2 (``fm_bank_create_bin2``; kind ``FM_BANK_BIN2``).  knn2 / knn / xcheck1 / knn2_ratio /
        mutual_ratio, their ``_dev`` forms and hamming_radius_match take a pair of such banks; every other call refuses one."""
        a = np.asarray(rows)
        if a.ndim != 2:
            raise ValueError("descriptor bank must be 2-D [n, bytes]")
        if a.dtype != np.uint8:
            raise ValueError("binary descriptors must be uint8 (cv2 asserts CV_8U for NORM_HAMMING2), got %s" % a.dtype)
        a = np.ascontiguousarray(a)
        h = _P()
        self._check(self.lib.fm_bank_create_bin2(self.handle, _ptr(a) if a.shape[0] else None, a.shape[0], a.shape[1], ctypes.byref(h)))
        n, dim, kind = _I64(), _INT(), _INT()
        self._check(self.lib.fm_bank_info(h, ctypes.byref(n), ctypes.byref(dim), ctypes.byref(kind)))
        return Bank(self, h, n.value, dim.value, kind.value)

    def bank_from_device(self, ptr, dtype, n, dim, pitch=0, float_route=False, stream=None):
        """A bank from ``n`` rows of ``dim`` elements that are already in device memory (``fm_bank_create_dev``): ``ptr`` =
        their device address (``tensor.data_ptr()``), ``dtype`` = ``FM_DT_U8`` / ``_F32`` / ``_F16`` / ``_BF16`` / ``_BIN``
        (binary: dim = bytes per row), ``pitch`` = bytes between rows (0 = dense).  The preparation kernels read the memory in
        place behind the work ``stream`` (a raw handle, 0 = the null stream; None = the rows are complete) has been given so
        far; on return the source may be overwritten.  The bank equals the one ``bank`` / ``bank_binary`` builds from the same
        values on the host."""
        h = _P()
        self._check(self.lib.fm_bank_create_dev(self.handle, _P(int(ptr)) if ptr else None, int(dtype), int(n), int(dim), int(pitch),
                                                1 if float_route else 0, _stream_arg(stream), ctypes.byref(h)))
        bn, bdim, kind = _I64(), _INT(), _INT()
        self._check(self.lib.fm_bank_info(h, ctypes.byref(bn), ctypes.byref(bdim), ctypes.byref(kind)))
        return Bank(self, h, bn.value, bdim.value, kind.value)

    def knn_dev(self, q, t, k, idx_ptr, dist_ptr, consumer_stream=None):
        """``knn`` with the lists left on the device (``fm_knn_dev``): ``idx_ptr`` / ``dist_ptr`` = device addresses of
        int32 / float32 [nq, k] buffers; enqueued, no host synchronisation on the integer and binary routes.
        ``consumer_stream`` as in ``match_accepted_dev_async``."""
        self._check(self.lib.fm_knn_dev(self.handle, q.handle, t.handle, int(k), _P(int(idx_ptr)) if idx_ptr else None,
                                        _P(int(dist_ptr)) if dist_ptr else None, _stream_arg(consumer_stream)))

    def xcheck1_dev(self, q, t, tidx_ptr, dist_ptr, consumer_stream=None):
        """``xcheck1`` with the results left on the device (``fm_xcheck1_dev``): int32 / float32 [nq] buffers."""
        self._check(self.lib.fm_xcheck1_dev(self.handle, q.handle, t.handle, _P(int(tidx_ptr)) if tidx_ptr else None,
                                            _P(int(dist_ptr)) if dist_ptr else None, _stream_arg(consumer_stream)))

    def knn2_ratio_dev(self, q, t, tau, rows_ptr, count_ptr, cap, want_count=False, consumer_stream=None):
        """``knn2_ratio`` with the accepted matches left on the device (``fm_knn2_ratio_dev``): ``rows_ptr`` = device address
        of an int32 [cap, 3] buffer (query, train, float32 distance bits), ``count_ptr`` of an int64 word that receives
        min(accepted, cap).  ``want_count``: also return the full number accepted (one host synchronisation); else None."""
        n = _I64(0)
        self._check(self.lib.fm_knn2_ratio_dev(self.handle, q.handle, t.handle, float(tau), int(cap),
                                               _P(int(rows_ptr)) if rows_ptr else None, _P(int(count_ptr)) if count_ptr else None,
                                               ctypes.byref(n) if want_count else None, _stream_arg(consumer_stream)))
        return int(n.value) if want_count else None

    def radius_match_dev(self, q, t, radius_ptr, radius_all, cap, offsets_ptr, idx_ptr, dist_ptr, want_total=True, consumer_stream=None,
                         _name="fm_radius_match_dev"):
        """``radius_match`` with the radii read from and the lists left in device memory (``fm_radius_match_dev``):
        ``radius_ptr`` = device address of float32 [nq] radii, or 0 for the scalar ``radius_all``; ``offsets_ptr`` of an int64
        [nq + 1] buffer; ``idx_ptr`` / ``dist_ptr`` of int32 / float32 [cap] buffers (0 with cap = 0: a counts call).  Returns
        the number of entries (``want_total``) or None.  The call synchronises (the counts plan the chunks); what it spares
        is the radii going up and the lists coming down.  ``consumer_stream`` as in ``knn_dev``."""
        n = _I64(0)
        self._check(getattr(self.lib, _name)(
            self.handle, q.handle, t.handle, _P(int(radius_ptr)) if radius_ptr else None, float(np.float32(radius_all)), int(cap),
            _P(int(offsets_ptr)) if offsets_ptr else None, _P(int(idx_ptr)) if idx_ptr else None,
            _P(int(dist_ptr)) if dist_ptr else None, ctypes.byref(n) if want_total else None, _stream_arg(consumer_stream)))
        return int(n.value) if want_total else None

    def hamming_radius_match_dev(self, q, t, radius_ptr, radius_all, cap, offsets_ptr, idx_ptr, dist_ptr, want_total=True,
                                 consumer_stream=None):
        """``hamming_radius_match`` with the radii read from and the lists left in device memory
        (``fm_hamming_radius_match_dev``); arguments as ``radius_match_dev``."""
        return self.radius_match_dev(q, t, radius_ptr, radius_all, cap, offsets_ptr, idx_ptr, dist_ptr, want_total, consumer_stream,
                                     _name="fm_hamming_radius_match_dev")

    def wide_radius_match_dev(self, q, t, radius_ptr, radius_all, cap, offsets_ptr, idx_ptr, dist_ptr, want_total=True,
                              consumer_stream=None):
        """``wide_radius_match`` with the radii read from and the lists left in device memory
        (``fm_wide_radius_match_dev``); arguments as ``radius_match_dev``."""
        return self.radius_match_dev(q, t, radius_ptr, radius_all, cap, offsets_ptr, idx_ptr, dist_ptr, want_total, consumer_stream,
                                     _name="fm_wide_radius_match_dev")

    def bank_gather(self, rows, src_row, float_route=False):
        """The bank ``rows[src_row]`` without building that matrix on the host: the n_src rows are uploaded once and
        gathered by the upload kernel (fm_bank_create_*_gather).  dtype handling as ``bank``."""
        a = np.asarray(rows)
        if a.ndim != 2:
            raise ValueError("descriptor bank must be 2-D [n, dim]")
        m = np.ascontiguousarray(src_row, dtype=np.int32).reshape(-1)
        h = _P()
        if float_route or a.dtype != np.uint8:
            a = np.ascontiguousarray(a, dtype=np.float32)
            self._check(self.lib.fm_bank_create_f32_gather(self.handle, _ptr(a), a.shape[0], a.shape[1], 1 if float_route else 0,
                                                           _ptr(m), m.shape[0], ctypes.byref(h)))
        else:
            a = np.ascontiguousarray(a)
            self._check(self.lib.fm_bank_create_u8_gather(self.handle, _ptr(a), a.shape[0], a.shape[1], _ptr(m), m.shape[0],
                                                          ctypes.byref(h)))
        n, dim, kind = _I64(), _INT(), _INT()
        self._check(self.lib.fm_bank_info(h, ctypes.byref(n), ctypes.byref(dim), ctypes.byref(kind)))
        return Bank(self, h, n.value, dim.value, kind.value)

    def bank_with_capacity(self, rows, capacity):
        """A uint8 bank with room for ``capacity`` rows (``Bank.append``): the growing target bank of a lazy pair."""
        a = np.ascontiguousarray(rows, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("descriptor bank must be 2-D [n, dim]")
        h = _P()
        self._check(self.lib.fm_bank_create_u8_cap(self.handle, _ptr(a) if a.shape[0] else None, a.shape[0], a.shape[1],
                                                   int(max(capacity, a.shape[0])), ctypes.byref(h)))
        n, dim, kind = _I64(), _INT(), _INT()
        self._check(self.lib.fm_bank_info(h, ctypes.byref(n), ctypes.byref(dim), ctypes.byref(kind)))
        return Bank(self, h, n.value, dim.value, kind.value)

    def bank_f32_with_capacity(self, dim, capacity, scale_like):
        """An empty float32-route bank with room for ``capacity`` rows whose fp16 planes use ``scale_like``'s scale
        (``Bank.append`` takes float32 rows): the growing target bank of a lazy pair with non-integer descriptors."""
        h = _P()
        self._check(self.lib.fm_bank_create_f32_cap(self.handle, int(dim), int(capacity), scale_like.handle, ctypes.byref(h)))
        return Bank(self, h, 0, int(dim), FM_BANK_F32)

    def collection(self):
        """An empty train collection (``Collection``: add / train / clear, knn / knn2_each / votes / match_accepted_each against all images)."""
        return Collection(self)

    # -- operators -----------------------------------------------------------------------
    def knn2(self, q, t):
        idx = np.empty((q.n, 2), dtype=np.int32)
        dist = np.empty((q.n, 2), dtype=np.float32)
        self._check(self.lib.fm_knn2(self.handle, q.handle, t.handle, _ptr(idx), _ptr(dist)))
        return idx, dist

    def knn(self, q, t, k):
        """``fm_knn``: k-NN lists for 1 <= k <= 8 (idx int32[nq, k], dist float32[nq, k]; -1 / inf where t has fewer rows)."""
        idx = np.empty((q.n, int(k)), dtype=np.int32)
        dist = np.empty((q.n, int(k)), dtype=np.float32)
        self._check(self.lib.fm_knn(self.handle, q.handle, t.handle, int(k), _ptr(idx), _ptr(dist)))
        return idx, dist

    def mask(self, nq, nt):
        """An all-forbidding ``Mask`` for a bank pair of ``nq`` query and ``nt`` train rows (``fm_mask_create``)."""
        h = _P()
        self._check(self.lib.fm_mask_create(self.handle, int(nq), int(nt), ctypes.byref(h)))
        return Mask(self, h)

    def knn_masked(self, q, t, mask, k):
        """``fm_knn_masked``: ``knn`` over the train rows ``mask`` (``Context.mask``) permits per query row -- cv2's
        ``knnMatch(q, t, k, mask)``; -1 / inf where fewer than k rows are permitted."""
        idx = np.empty((q.n, max(int(k), 0)), dtype=np.int32)
        dist = np.empty((q.n, max(int(k), 0)), dtype=np.float32)
        self._check(self.lib.fm_knn_masked(self.handle, q.handle, t.handle, mask.handle if mask is not None else None, int(k),
                                           _ptr(idx), _ptr(dist)))
        return idx, dist

    def knn_masked_dev(self, q, t, mask, k, idx_ptr, dist_ptr, consumer_stream=None):
        """``knn_masked`` with the lists left on the device (``fm_knn_masked_dev``); pointers and ``consumer_stream`` as in
        ``knn_dev``."""
        self._check(self.lib.fm_knn_masked_dev(self.handle, q.handle, t.handle, mask.handle if mask is not None else None, int(k),
                                               _P(int(idx_ptr)) if idx_ptr else None, _P(int(dist_ptr)) if dist_ptr else None,
                                               _stream_arg(consumer_stream)))

    def wide_knn_masked(self, q, t, mask, k):
        """``fm_wide_knn_masked``: ``knn_masked`` on two wide float banks (129 .. 256 values per row), k = 1 or 2, on the matrix
        cores -- ``knn``'s lists for the wide pair over the train rows ``mask`` (``Context.mask``) permits per query row, the same
        distance bits; -1 / inf where fewer than k rows are permitted.  (``knn_masked`` keeps refusing wide banks.)"""
        idx = np.empty((q.n, max(int(k), 0)), dtype=np.int32)
        dist = np.empty((q.n, max(int(k), 0)), dtype=np.float32)
        self._check(self.lib.fm_wide_knn_masked(self.handle, q.handle, t.handle, mask.handle if mask is not None else None, int(k),
                                                _ptr(idx), _ptr(dist)))
        return idx, dist

    def wide_knn_masked_dev(self, q, t, mask, k, idx_ptr, dist_ptr, consumer_stream=None):
        """``wide_knn_masked`` with the lists left on the device (``fm_wide_knn_masked_dev``); pointers and ``consumer_stream``
        as in ``knn_dev``."""
        self._check(self.lib.fm_wide_knn_masked_dev(self.handle, q.handle, t.handle, mask.handle if mask is not None else None, int(k),
                                                    _P(int(idx_ptr)) if idx_ptr else None, _P(int(dist_ptr)) if dist_ptr else None,
                                                    _stream_arg(consumer_stream)))

    def hamming_radius_match(self, q, t, r):
        """``fm_hamming_radius_match``: ``radius_match`` on two binary banks (``bank_binary``) -- every train row with
        ``popcount(q XOR t) < r`` per query row (strict, float32: ``h <= H`` is ``r = H + 0.5``), lists ascending (h, index).
        Arguments and return value as ``radius_match``."""
        return self.radius_match(q, t, r, _name="fm_hamming_radius_match")

    def wide_radius_match(self, q, t, r):
        """``fm_wide_radius_match``: ``radius_match`` on two wide float banks (129 .. 256 values per row) -- every train row
        whose distance (K14's float32 chain over the real dim) is < r per query row, lists ascending (distance bits, index).
        Arguments and return value as ``radius_match``."""
        return self.radius_match(q, t, r, _name="fm_wide_radius_match")

    def radius_match(self, q, t, r, _name="fm_radius_match"):
        """``fm_radius_match``: every train row with distance < r per query row -- cv2's radiusMatch with compactResult
        False.  ``r`` is a scalar or a float32 [nq] array (one radius per query row).  Returns (offsets int64[nq + 1],
        idx int32[n], dist float32[n]): row i's list is idx / dist[offsets[i]:offsets[i + 1]], ascending (distance, index).
        A counts call sizes the arrays, a second call fills them."""
        nq = q.n
        if np.ndim(r) == 0:
            rad, r_all = None, float(np.float32(r))
        else:
            rad = np.ascontiguousarray(r, dtype=np.float32).reshape(-1)
            if rad.shape[0] != nq:
                raise ValueError("radius_match: %d radii for %d query rows" % (rad.shape[0], nq))
            r_all = 0.0
        rp = _ptr(rad) if rad is not None and nq > 0 else None
        offsets = np.zeros(nq + 1, dtype=np.int64)
        total = _I64(0)
        fn = getattr(self.lib, _name)
        self._check(fn(self.handle, q.handle, t.handle, rp, r_all, 0, _ptr(offsets), None, None, ctypes.byref(total)))
        n = int(total.value)
        idx = np.empty(n, dtype=np.int32)
        dist = np.empty(n, dtype=np.float32)
        if n > 0:
            self._check(fn(self.handle, q.handle, t.handle, rp, r_all, n, _ptr(offsets), _ptr(idx), _ptr(dist), ctypes.byref(total)))
            if int(total.value) != n:
                raise FastMatchHipError("%s: %d entries on the second call, %d on the first" % (_name, total.value, n))
        return offsets, idx, dist

    def radius_match_masked(self, q, t, mask, r):
        """``fm_radius_match_masked``: ``radius_match`` -- for two binary banks ``hamming_radius_match``, for two wide float banks
        ``wide_radius_match`` -- with every entry whose pair ``mask`` (``Context.mask``) forbids removed: cv2's
        radiusMatch(q, t, maxDistance, mask).  Distances, order, radii and the return value are the unmasked call's."""
        nq = q.n
        if np.ndim(r) == 0:
            rad, r_all = None, float(np.float32(r))
        else:
            rad = np.ascontiguousarray(r, dtype=np.float32).reshape(-1)
            if rad.shape[0] != nq:
                raise ValueError("radius_match_masked: %d radii for %d query rows" % (rad.shape[0], nq))
            r_all = 0.0
        rp = _ptr(rad) if rad is not None and nq > 0 else None
        mh = mask.handle if mask is not None else None
        offsets = np.zeros(nq + 1, dtype=np.int64)
        total = _I64(0)
        fn = self.lib.fm_radius_match_masked
        self._check(fn(self.handle, q.handle, t.handle, mh, rp, r_all, 0, _ptr(offsets), None, None, ctypes.byref(total)))
        n = int(total.value)
        idx = np.empty(n, dtype=np.int32)
        dist = np.empty(n, dtype=np.float32)
        if n > 0:
            self._check(fn(self.handle, q.handle, t.handle, mh, rp, r_all, n, _ptr(offsets), _ptr(idx), _ptr(dist), ctypes.byref(total)))
            if int(total.value) != n:
                raise FastMatchHipError("fm_radius_match_masked: %d entries on the second call, %d on the first" % (total.value, n))
        return offsets, idx, dist

    def radius_match_masked_dev(self, q, t, mask, radius_ptr, radius_all, cap, offsets_ptr, idx_ptr, dist_ptr, want_total=True,
                                consumer_stream=None):
        """``radius_match_masked`` with the radii read from and the lists left in device memory (``fm_radius_match_masked_dev``);
        arguments after ``mask`` as ``radius_match_dev``."""
        n = _I64(0)
        self._check(self.lib.fm_radius_match_masked_dev(
            self.handle, q.handle, t.handle, mask.handle if mask is not None else None,
            _P(int(radius_ptr)) if radius_ptr else None, float(np.float32(radius_all)), int(cap),
            _P(int(offsets_ptr)) if offsets_ptr else None, _P(int(idx_ptr)) if idx_ptr else None,
            _P(int(dist_ptr)) if dist_ptr else None, ctypes.byref(n) if want_total else None, _stream_arg(consumer_stream)))
        return int(n.value) if want_total else None

    def self_dist(self, bank, _name="fm_self_dist"):
        out = np.empty(bank.n, dtype=np.float64)
        self._check(getattr(self.lib, _name)(self.handle, bank.handle, _ptr(out)))
        return out

    def hamming_self_dist(self, bank):
        """``fm_hamming_self_dist``: float64 [n], row i's Hamming distance to its nearest OTHER row of a binary bank
        (+inf for a bank of one row, 0 for a row with a duplicate)."""
        return self.self_dist(bank, _name="fm_hamming_self_dist")

    def hamming_self_dist_batch(self, banks, want_host=True):
        """``fm_hamming_self_dist_batch``: ``self_dist_batch`` for binary banks -- the Hamming self distances of every bank,
        attached to it on the device; banks of one K-step count (16 bytes of row width each) share a launch."""
        return self.self_dist_batch(banks, want_host, _name="fm_hamming_self_dist_batch")

    def wide_self_dist(self, bank):
        """``fm_wide_self_dist``: float64 [n], row i's distance (K14's exact float32 chain) to its nearest OTHER row of a wide
        float bank; +inf for a bank of one row or a row that holds a NaN, 0 for a row with an exact duplicate."""
        return self.self_dist(bank, _name="fm_wide_self_dist")

    def wide_self_dist_batch(self, banks, want_host=True):
        """``fm_wide_self_dist_batch``: ``self_dist_batch`` for wide float banks -- the self distances of every bank, attached
        to it on the device; ``want_host=False`` only enqueues."""
        return self.self_dist_batch(banks, want_host, _name="fm_wide_self_dist_batch")

    def self_dist_batch(self, banks, want_host=True, _name="fm_self_dist_batch"):
        """Metric_Cache builds of several images in one call (``fm_self_dist_batch``): the self distances of
        every bank, attached to it on the device; runs of integer banks (of any sizes, r05) share the
        triangular sweep's launches, up to ``batch_group`` banks each.
        ``want_host``: also return them (list of float64 arrays; synchronous); False = enqueue only."""
        n = len(banks)
        if n == 0:
            return []
        hs = (_P * n)(*[b.handle for b in banks])
        outs = [np.empty(b.n, dtype=np.float64) for b in banks] if want_host else None
        op = (_P * n)(*[_P(o.ctypes.data) if o.shape[0] else None for o in outs]) if want_host else None
        self._check(getattr(self.lib, _name)(self.handle, n, hs, op))
        for b in banks:
            b.has_selfdist = True
        return outs

    def upload_fence(self):
        """Later calls on this context wait (on the device) for the refills enqueued so far."""
        self._check(self.lib.fm_upload_fence(self.handle))

    def xcheck1(self, q, t):
        tidx = np.empty(q.n, dtype=np.int32)
        dist = np.empty(q.n, dtype=np.float32)
        self._check(self.lib.fm_xcheck1(self.handle, q.handle, t.handle, _ptr(tidx), _ptr(dist)))
        return tidx, dist

    def xcheck1_keys(self, q, t, t_offset=0):
        """X1 election keys of a train-set shard (see sharding.xcheck1_sharded): uint64[nq]."""
        keys = np.empty(q.n, dtype=np.uint64)
        self._check(self.lib.fm_xcheck1_keys(self.handle, q.handle, t.handle, int(t_offset), _ptr(keys)))
        return keys

    def xcheck1_keys_dev(self, q, t, t_offset, keys_ptr):
        """``xcheck1_keys`` into device memory: ``keys_ptr`` = device address of a uint64/int64 [nq]
        buffer (``tensor.data_ptr()``)."""
        self._check(self.lib.fm_xcheck1_keys_dev(self.handle, q.handle, t.handle, int(t_offset), _P(int(keys_ptr))))

    def hamming_match_ratio(self, q, t, tau, out=None):
        """``match_ratio`` on two binary banks (``fm_hamming_match_ratio``): dist = popcount(q XOR t), the query bank
        carries Hamming self distances."""
        return self.match_ratio(q, t, tau, out, _name="fm_hamming_match_ratio")

    def hamming_match_accepted(self, q, t, tau, out=None):
        """``match_accepted`` on two binary banks (``fm_hamming_match_accepted``)."""
        return self.match_accepted(q, t, tau, out, _name="fm_hamming_match_accepted")

    def hamming_match_accepted_dev(self, q, t, tau, rows_ptr, count_ptr, cap):
        """``match_accepted_dev`` on two binary banks (``fm_hamming_match_accepted_dev``)."""
        return self.match_accepted_dev(q, t, tau, rows_ptr, count_ptr, cap, _name="fm_hamming_match_accepted_dev")

    def wide_match_ratio(self, q, t, tau, out=None):
        """``match_ratio`` on two wide float banks (``fm_wide_match_ratio``): the query bank carries wide self distances."""
        return self.match_ratio(q, t, tau, out, _name="fm_wide_match_ratio")

    def wide_match_accepted(self, q, t, tau, out=None):
        """``match_accepted`` on two wide float banks (``fm_wide_match_accepted``)."""
        return self.match_accepted(q, t, tau, out, _name="fm_wide_match_accepted")

    def wide_match_accepted_dev(self, q, t, tau, rows_ptr, count_ptr, cap):
        """``match_accepted_dev`` on two wide float banks (``fm_wide_match_accepted_dev``)."""
        return self.match_accepted_dev(q, t, tau, rows_ptr, count_ptr, cap, _name="fm_wide_match_accepted_dev")

    def match_ratio(self, q, t, tau, out=None, _name="fm_match_ratio"):
        """X1 + R1 fused.  ``out`` = optional (tidx i32[nq], dist f32[nq], ratio f64[nq],
        passed u8[nq]) buffers to fill (e.g. from ``pinned_empty``); then ``passed`` is
        returned as that uint8 array instead of a bool copy."""
        if out is not None:
            tidx, dist, ratio, passed = out
            for a, dt in ((tidx, np.int32), (dist, np.float32), (ratio, np.float64), (passed, np.uint8)):
                if a.dtype != dt or a.shape != (q.n,) or not a.flags.c_contiguous:
                    raise ValueError("out buffers must be contiguous [nq] int32/float32/float64/uint8")
            npass = _I64(0)
            self._check(getattr(self.lib, _name)(self.handle, q.handle, t.handle, float(tau), _ptr(tidx),
                                                 _ptr(dist), _ptr(ratio), _ptr(passed), ctypes.byref(npass)))
            return tidx, dist, ratio, passed, npass.value
        tidx = np.empty(q.n, dtype=np.int32)
        dist = np.empty(q.n, dtype=np.float32)
        ratio = np.empty(q.n, dtype=np.float64)
        passed = np.empty(q.n, dtype=np.uint8)
        npass = _I64(0)
        self._check(getattr(self.lib, _name)(self.handle, q.handle, t.handle, float(tau), _ptr(tidx),
                                             _ptr(dist), _ptr(ratio), _ptr(passed), ctypes.byref(npass)))
        return tidx, dist, ratio, passed.astype(bool), npass.value

    def match_accepted(self, q, t, tau, out=None, _name="fm_match_accepted"):
        """X1 + R1, returning only the accepted matches in ascending query index:
        (qidx i32[m], tidx i32[m], dist f32[m], ratio f64[m]).  ``out`` = optional buffers
        (qidx, tidx, dist, ratio) of equal capacity (e.g. pinned); views of them are returned."""
        if out is None:
            cap = q.n
            out = (np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.float32), np.empty(cap, np.float64))
        qidx, tidx, dist, ratio = out
        cap = self._check_accepted_out(out)
        n = _I64(0)
        self._check(getattr(self.lib, _name)(self.handle, q.handle, t.handle, float(tau), cap, _ptr(qidx),
                                             _ptr(tidx), _ptr(dist), _ptr(ratio), ctypes.byref(n)))
        m = min(n.value, cap)
        return qidx[:m], tidx[:m], dist[:m], ratio[:m]

    @staticmethod
    def _check_accepted_out(out):
        """Capacity of an (qidx, tidx, dist, ratio) output tuple; the library (or, for pinned
        buffers, the device) writes up to that many rows into each array."""
        qidx, tidx, dist, ratio = out
        cap = qidx.shape[0] if getattr(qidx, "ndim", 0) == 1 else -1
        for a, dt in ((qidx, np.int32), (tidx, np.int32), (dist, np.float32), (ratio, np.float64)):
            if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != (cap,) or not a.flags.c_contiguous \
                    or not a.flags.writeable:
                raise ValueError("out buffers must be writable contiguous 1-D int32/int32/float32/float64 of one length")
        return cap

    def match_accepted_async(self, q, t, tau, out, count):
        """Enqueue X1 + R1 + compaction and return at once.  ``out`` = (qidx, tidx, dist, ratio)
        and ``count`` (int64[1]) must come from ``pinned_empty``; they are valid after ``sync()``:
        ``m = int(count[0])`` accepted matches in ``out[i][:m]``."""
        cap = self._check_accepted_out(out)
        if not isinstance(count, np.ndarray) or count.dtype != np.int64 or count.size < 1:
            raise ValueError("count must be an int64 array (pinned_empty(1, np.int64))")
        qidx, tidx, dist, ratio = out
        self._check(self.lib.fm_match_accepted_async(self.handle, q.handle, t.handle, float(tau), cap, _ptr(qidx),
                                                     _ptr(tidx), _ptr(dist), _ptr(ratio), _ptr(count)))

    def prepare_batch(self, pairs, outs, counts):
        """Argument block of ``match_accepted_batch`` for a fixed list of (query bank, train bank) pairs
        and their output buffers, built once (the per-call cost of a batch sits in front of its first
        launch): ``outs[i]`` = (qidx, tidx, dist, ratio), ``counts[i]`` = int64[1], all ``pinned_empty``."""
        n = len(pairs)
        if len(outs) != n or len(counts) != n:
            raise ValueError("pairs, outs and counts must have the same length")
        cap = None
        for out, cnt in zip(outs, counts):
            c = self._check_accepted_out(out)
            cap = c if cap is None else min(cap, c)
            if not isinstance(cnt, np.ndarray) or cnt.dtype != np.int64 or cnt.size < 1:
                raise ValueError("count must be an int64 array (pinned_empty(1, np.int64))")
        arr = lambda vals: (_P * n)(*[_P(int(v)) if v is not None else None for v in vals])
        args = (n, arr([q.handle.value for q, _ in pairs]), arr([t.handle.value for _, t in pairs]), int(cap or 0),
                arr([_ptr(o[0]) for o in outs]), arr([_ptr(o[1]) for o in outs]), arr([_ptr(o[2]) for o in outs]),
                arr([_ptr(o[3]) for o in outs]), arr([_ptr(c) for c in counts]))
        return {"args": args, "keep": (list(pairs), list(outs), list(counts))}     # (keeps banks and buffers alive)

    def match_accepted_batch(self, pairs, tau, outs=None, counts=None):
        """``match_accepted_async`` for a list of (query bank, train bank) pairs in ONE call: consecutive
        pairs share distance-kernel launches (up to eight per launch; r05: of any sizes).  Either the lists
        (``outs[i]`` = (qidx, tidx, dist, ratio), ``counts[i]`` = int64[1], all from ``pinned_empty``) or
        the block ``prepare_batch`` built from them; results are valid after ``sync()``."""
        batch = pairs if isinstance(pairs, dict) else self.prepare_batch(pairs, outs, counts)
        n, qh, th, cap, a0, a1, a2, a3, ac = batch["args"]
        self._check(self.lib.fm_match_accepted_batch(self.handle, n, qh, th, float(tau), cap, a0, a1, a2, a3, ac))

    def match_accepted_dev_batch(self, pairs, tau, rows_ptr, counts_ptr, cap, h_counts=None, consumer_stream=None):
        """``match_accepted_batch`` with device outputs: ``rows_ptr`` = device address of an int32
        [n, cap, 3] block, ``counts_ptr`` of an int64 [n] array; ``h_counts`` = ``pinned_empty(n, np.int64)``
        or None; ``consumer_stream`` as in ``match_accepted_dev_async``.  ``pairs`` may be the list of
        (query bank, train bank) or a ``prepare_pairs`` block."""
        n, qh, th = pairs["args"] if isinstance(pairs, dict) else self.prepare_pairs(pairs)["args"]
        if h_counts is not None and (not isinstance(h_counts, np.ndarray) or h_counts.dtype != np.int64 or h_counts.size < n):
            raise ValueError("h_counts must be an int64 array of n words (pinned_empty(n, np.int64))")
        self._check(self.lib.fm_match_accepted_dev_batch(self.handle, n, qh, th, float(tau), int(cap), _P(int(rows_ptr)),
                                                         _P(int(counts_ptr)), _ptr(h_counts) if h_counts is not None else None,
                                                         _stream_arg(consumer_stream)))

    def prepare_pairs(self, pairs):
        """The bank-handle arrays of a fixed list of pairs, built once (``match_accepted_dev_batch``)."""
        n = len(pairs)
        arr = lambda vals: (_P * n)(*[_P(int(v)) for v in vals])
        return {"args": (n, arr([q.handle.value for q, _ in pairs]), arr([t.handle.value for _, t in pairs])), "keep": list(pairs)}

    def match_accepted_dev(self, q, t, tau, rows_ptr, count_ptr, cap, _name="fm_match_accepted_dev"):
        """X1 + R1 with the accepted matches left on the device: ``rows_ptr`` = device address of
        an int32 [cap, 3] buffer (query index, train index, float32 distance bits), ``count_ptr``
        = device address of an int64 word (e.g. ``tensor.data_ptr()`` of torch tensors on this
        context's device).  Returns the number accepted."""
        n = _I64(0)
        self._check(getattr(self.lib, _name)(self.handle, q.handle, t.handle, float(tau), int(cap),
                                             _P(int(rows_ptr)), _P(int(count_ptr)), ctypes.byref(n)))
        return n.value

    def match_accepted_dev_async(self, q, t, tau, rows_ptr, count_ptr, cap, h_count=None, consumer_stream=None):
        """``match_accepted_dev`` enqueued without a synchronisation (``sync()`` later).  ``h_count``:
        a ``pinned_empty(1, np.int64)`` array that also receives the count, or None;
        ``consumer_stream``: the raw handle of the stream that will read the buffers
        (``torch.cuda.current_stream().cuda_stream`` -- 0 is a stream, PyTorch's default one), ordered
        against the fill in both directions; None = no such stream."""
        if h_count is not None and (not isinstance(h_count, np.ndarray) or h_count.dtype != np.int64 or h_count.size < 1):
            raise ValueError("h_count must be an int64 array (pinned_empty(1, np.int64))")
        self._check(self.lib.fm_match_accepted_dev_async(self.handle, q.handle, t.handle, float(tau), int(cap),
                                                         _P(int(rows_ptr)), _P(int(count_ptr)),
                                                         _ptr(h_count) if h_count is not None else None,
                                                         _stream_arg(consumer_stream)))

    def knn2_ratio(self, q, t, tau, out=None):
        """Classic Ratio-Match: 2-NN + d1/d2 < tau, accepted matches in ascending query index:
        (qidx i32[m], tidx i32[m], dist f32[m] (= d1), ratio f64[m])."""
        if out is None:
            cap = q.n
            out = (np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.float32), np.empty(cap, np.float64))
        qidx, tidx, dist, ratio = out
        cap = self._check_accepted_out(out)
        n = _I64(0)
        self._check(self.lib.fm_knn2_ratio(self.handle, q.handle, t.handle, float(tau), cap, _ptr(qidx), _ptr(tidx),
                                           _ptr(dist), _ptr(ratio), ctypes.byref(n)))
        m = min(n.value, cap)
        return qidx[:m], tidx[:m], dist[:m], ratio[:m]

    def mutual_ratio(self, q, t, tau, symmetric=False, cap=None):
        """Mutual nearest neighbours + ratio test (``fm_mutual_ratio``): query row i is kept iff d0 / d1 < tau on its 2-NN list
        and i is the nearest query row of its first neighbour; ``symmetric``: the reverse 2-NN list passes the ratio test
        too.  (qidx i32[m], tidx i32[m], dist f32[m] (= d0), ratio f64[m]) ascending in query index; ``ratio`` is the larger of
        the two ratios in symmetric mode.  ``cap`` (default ``q.n``) bounds the rows returned."""
        cap = q.n if cap is None else int(cap)
        kept = max(cap, 0)
        qidx, tidx, dist, ratio = np.empty(kept, np.int32), np.empty(kept, np.int32), np.empty(kept, np.float32), np.empty(kept, np.float64)
        n = _I64(0)
        self._check(self.lib.fm_mutual_ratio(self.handle, q.handle, t.handle, float(tau), int(bool(symmetric)), cap,
                                             _ptr(qidx) if kept else None, _ptr(tidx) if kept else None, _ptr(dist) if kept else None,
                                             _ptr(ratio) if kept else None, ctypes.byref(n)))
        m = min(n.value, kept)
        return qidx[:m], tidx[:m], dist[:m], ratio[:m]

    def mutual_ratio_count(self, q, t, tau, symmetric=False):
        """The number of matches ``mutual_ratio`` accepts (its counts-only call, cap = 0)."""
        n = _I64(0)
        self._check(self.lib.fm_mutual_ratio(self.handle, q.handle, t.handle, float(tau), int(bool(symmetric)), 0, None, None, None,
                                             None, ctypes.byref(n)))
        return int(n.value)

    def mutual_ratio_dev(self, q, t, tau, symmetric, rows_ptr, count_ptr, cap, want_count=False, consumer_stream=None):
        """``mutual_ratio`` with the accepted matches left on the device (``fm_mutual_ratio_dev``): rows and count as
        ``knn2_ratio_dev`` leaves them -- ``rows_ptr`` = device address of an int32 [cap, 3] buffer (query, train, float32
        distance bits), ``count_ptr`` of an int64 word that receives min(accepted, cap).  The call waits once for the
        candidate count; ``want_count``: also return the full number accepted (else None)."""
        n = _I64(0)
        self._check(self.lib.fm_mutual_ratio_dev(self.handle, q.handle, t.handle, float(tau), int(bool(symmetric)), int(cap),
                                                 _P(int(rows_ptr)) if rows_ptr else None, _P(int(count_ptr)) if count_ptr else None,
                                                 ctypes.byref(n) if want_count else None, _stream_arg(consumer_stream)))
        return int(n.value) if want_count else None

    def ratio_filter(self, dist, selfdist, tau, qrows=None):
        dist = np.ascontiguousarray(dist, dtype=np.float32)
        selfdist = np.ascontiguousarray(selfdist, dtype=np.float64)
        n = dist.shape[0]
        if qrows is not None:
            qrows = np.ascontiguousarray(qrows, dtype=np.int32)
            if qrows.shape[0] != n:
                raise ValueError("qrows and dist must have the same length")
            if n and int(qrows.max()) >= selfdist.shape[0]:
                raise ValueError("qrows index beyond selfdist")
        elif selfdist.shape[0] < n:
            raise ValueError("selfdist shorter than dist")
        ratio = np.empty(n, dtype=np.float64)
        passed = np.empty(n, dtype=np.uint8)
        npass = _I64(0)
        self._check(self.lib.fm_ratio_filter(self.handle, _ptr(dist), _ptr(selfdist), _ptr(qrows), n,
                                             float(tau), _ptr(ratio), _ptr(passed), ctypes.byref(npass)))
        return ratio, passed.astype(bool), npass.value

    def xcheck1_batched(self, q, q_rows, q_off, t, t_off):
        q_rows = np.ascontiguousarray(q_rows, dtype=np.int32)
        q_off = np.ascontiguousarray(q_off, dtype=np.int64)
        t_off = np.ascontiguousarray(t_off, dtype=np.int64)
        if q_off.shape != t_off.shape or q_off.ndim != 1 or q_off.shape[0] < 1:
            raise ValueError("q_off and t_off must both be [B+1]")
        nb = q_off.shape[0] - 1
        tot = int(q_off[-1])
        if q_rows.shape[0] != tot:
            raise ValueError("q_rows length must equal q_off[-1]")
        tidx = np.empty(tot, dtype=np.int32)
        dist = np.empty(tot, dtype=np.float32)
        ratio = np.empty(tot, dtype=np.float64)
        self._check(self.lib.fm_xcheck1_batched(self.handle, q.handle, _ptr(q_rows), _ptr(q_off), t.handle,
                                                _ptr(t_off), nb, _ptr(tidx), _ptr(dist), _ptr(ratio)))
        return tidx, dist, ratio

    @staticmethod
    def expand_slots(expanders):
        """Run slot of every entry of a launch: the k-th entry that names an Expander uses its slot k
        (fm_expand_run's rule; several thresholds of one pair run side by side, each in a state of its own)."""
        seen, slots = {}, []
        for e in expanders:
            k = seen.get(id(e), 0)
            slots.append(k)
            seen[id(e)] = k + 1
        return slots

    def expand_run(self, expanders, seeds, taus):
        """Run the device-resident expansion loop for several runs in one launch (one workgroup each); an
        Expander may appear several times (e.g. once per threshold).  Returns per run
        (n_matches, n_rounds, n_pairs, status)."""
        n = len(expanders)
        seeds = [np.ascontiguousarray(s, dtype=np.float64).reshape(-1, 2, 2) for s in seeds]
        hs = (_P * n)(*[e.handle for e in expanders])
        sp = (_P * n)(*[s.ctypes.data if s.shape[0] else None for s in seeds])
        ns = np.array([s.shape[0] for s in seeds], dtype=np.int64)
        tau = np.ascontiguousarray(taus, dtype=np.float64)
        nm = np.zeros(n, dtype=np.int64)
        nr = np.zeros(n, dtype=np.int64)
        npairs = np.zeros(n, dtype=np.int64)
        st = np.zeros(n, dtype=np.int32)
        self._check(self.lib.fm_expand_run(self.handle, n, hs, sp, _ptr(ns), _ptr(tau), _ptr(nm), _ptr(nr),
                                           _ptr(npairs), _ptr(st)))
        return [(int(nm[i]), int(nr[i]), int(npairs[i]), int(st[i])) for i in range(n)]

    # -- result gather over RCCL (fm_comm_*, fm_gather_matches) ----------------------------
    def comm_unique_id(self):
        """128 opaque bytes drawn by ONE rank; hand them to every rank's ``comm_init``."""
        buf = ctypes.create_string_buffer(128)
        rc = self.lib.fm_comm_unique_id(buf)
        if rc != 0:
            msg = self.lib.fm_last_error(None)
            raise FastMatchHipError("fm_comm_unique_id failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        return buf.raw

    def comm_init(self, nranks, rank, unique_id):
        uid = ctypes.create_string_buffer(bytes(unique_id), 128)
        self._check(self.lib.fm_comm_init(self.handle, int(nranks), int(rank), uid))

    def comm_destroy(self):
        self._check(self.lib.fm_comm_destroy(self.handle))

    def gather_matches(self, rows_ptr, count_ptr, cap, all_rows_ptr, all_counts_ptr, wait=True):
        """All-gather the device rows / count left by ``match_accepted_dev`` into device buffers
        [nranks, cap, 3] int32 and [nranks] int64 (addresses, e.g. ``tensor.data_ptr()``)."""
        self._check(self.lib.fm_gather_matches(self.handle, _P(int(rows_ptr)), _P(int(count_ptr)), int(cap),
                                               _P(int(all_rows_ptr)), _P(int(all_counts_ptr)), 1 if wait else 0))

    def gather_matches_counted(self, rows_ptr, count_ptr, cap, all_rows_ptr, all_counts_ptr):
        """Two-phase form of ``gather_matches``: counts first, then only ``m`` = the fullest rank's rows per
        rank; the rows arrive as [nranks, m, 3] at ``all_rows_ptr``.  Returns m.  Synchronous."""
        m = _I64(0)
        self._check(self.lib.fm_gather_matches_counted(self.handle, _P(int(rows_ptr)), _P(int(count_ptr)), int(cap),
                                                       _P(int(all_rows_ptr)), _P(int(all_counts_ptr)), ctypes.byref(m)))
        return int(m.value)

    # -- bookkeeping ---------------------------------------------------------------------
    def stats(self):
        s = fm_stats_ex()
        self._check(self.lib.fm_get_stats_ex(self.handle, ctypes.byref(s), ctypes.sizeof(s)))
        return {"kernel_ms": s.kernel_ms, "total_ms": s.total_ms, "kernel_launches": s.kernel_launches,
                "pairs": s.pairs, "calls": s.calls, "bytes_moved": s.bytes_moved}

    def reset_stats(self):
        self._check(self.lib.fm_reset_stats(self.handle))

    def sync(self):
        self._check(self.lib.fm_sync(self.handle))

    def expand_fetch_many(self, expanders, counts, slots=None):
        """(index, positions, ratio) arrays of several runs after one ``expand_run``: every copy
        enqueued, one synchronisation (``Expander.fetch`` costs one per pair).  ``slots[i]`` = run slot of
        ``expanders[i]`` (``expand_slots`` of the launch's list); None = slots by appearance in THIS list."""
        n = len(expanders)
        out = [(np.empty(c, dtype=np.int32), np.empty((c, 2, 2), dtype=np.float64), np.empty(c, dtype=np.float64)) for c in counts]
        if n:
            arr = lambda vals: (_P * n)(*[_P(int(v)) if v is not None else None for v in vals])
            slots = self.expand_slots(expanders) if slots is None else slots
            sl = np.ascontiguousarray(slots, dtype=np.int32)
            self._check(self.lib.fm_expand_fetch_many(self.handle, n, arr([e.handle.value for e in expanders]), _ptr(sl),
                                                      (_I64 * n)(*[int(c) for c in counts]), arr([_ptr(o[0]) for o in out]),
                                                      arr([_ptr(o[1]) for o in out]), arr([_ptr(o[2]) for o in out])))
        return out

    def mark(self):
        """Ticket for "everything enqueued so far" (``wait(ticket)`` blocks until it is done, later work keeps running)."""
        t = _I64(0)
        self._check(self.lib.fm_mark(self.handle, ctypes.byref(t)))
        return t.value

    def wait(self, ticket):
        self._check(self.lib.fm_wait(self.handle, int(ticket)))

    def f32_filter_stats(self):
        """(row-reduces routed through the bf16x3 filter, of which redone by the all-pairs kernel)."""
        a, b = _I64(0), _I64(0)
        self._check(self.lib.fm_f32_filter_stats(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def mem_info(self):
        """(free, total) bytes of the context's device."""
        f, t = _I64(0), _I64(0)
        self._check(self.lib.fm_mem_info(self.handle, ctypes.byref(f), ctypes.byref(t)))
        return int(f.value), int(t.value)

    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        self._check(self.lib.fm_device_name(self.handle, buf, 256))
        return buf.value.decode()


_default_ctx = {}
_default_lock = threading.Lock()


def default_context(device=None):
    """Process-wide context per device.  ``device=None`` uses LOCAL_RANK (one process per
    GPU under torch.distributed.run) or 0."""
    if device is None:
        device = int(os.environ.get("FM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    with _default_lock:
        ctx = _default_ctx.get(device)
        if ctx is None or ctx.handle is None:
            ctx = Context(device)
            _default_ctx[device] = ctx
        return ctx
