"""ctypes binding of libclover_hip.so (include/clover_hip.h) for tests and bench.py.

No fallback: if the library is missing or a call fails this raises -- the HIP path is the only path.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from .build import hip_library_path

DOT_EXACT = 0
DOT_FAST = 1
THRESHOLD_FAST = 0          # radix select, lowest-index ties
THRESHOLD_REFERENCE = 1     # the reference's survivor set (its min-heap walk, CloverVector4.h:1927-1972)

_vp = C.c_void_p
_u64 = C.c_uint64

# name -> (restype, argtypes); everything include/clover_hip.h declares
SIGNATURES = {
    "clv_version": (C.c_char_p, []),
    "clv_last_error": (C.c_char_p, []),
    "clv_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "clv_set_device": (C.c_int, [C.c_int]),
    "clv_get_device": (C.c_int, [C.POINTER(C.c_int)]),
    "clv_device_info": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(_u64)]),
    "clv_malloc": (C.c_int, [C.POINTER(_vp), _u64]),
    "clv_free": (C.c_int, [_vp]),
    "clv_memset": (C.c_int, [_vp, C.c_int, _u64, _vp]),
    "clv_memcpy_h2d": (C.c_int, [_vp, _vp, _u64, _vp]),
    "clv_memcpy_d2h": (C.c_int, [_vp, _vp, _u64, _vp]),
    "clv_memcpy_d2d": (C.c_int, [_vp, _vp, _u64, _vp]),
    "clv_host_alloc": (C.c_int, [C.POINTER(_vp), _u64]),
    "clv_host_free": (C.c_int, [_vp]),
    "clv_stream_create": (C.c_int, [C.POINTER(_vp)]),
    "clv_stream_destroy": (C.c_int, [_vp]),
    "clv_stream_sync": (C.c_int, [_vp]),
    "clv_device_sync": (C.c_int, []),
    "clv_event_create": (C.c_int, [C.POINTER(_vp)]),
    "clv_event_destroy": (C.c_int, [_vp]),
    "clv_event_record": (C.c_int, [_vp, _vp]),
    "clv_event_sync": (C.c_int, [_vp]),
    "clv_event_elapsed_ms": (C.c_int, [_vp, _vp, C.POINTER(C.c_float)]),
    "clv_rng_seed": (C.c_int, [_vp, _u64, _u64, _vp]),
    "clv_rng_set": (C.c_int, [_vp, C.POINTER(_u64), C.POINTER(_u64), _vp]),
    "clv_rng_get": (C.c_int, [_vp, C.POINTER(_u64), C.POINTER(_u64), _vp]),
    "clv_rng_graph_mode": (C.c_int, [_vp, C.c_int, _vp]),
    "clv_rng_set_segments": (C.c_int, [C.c_int]),
    "clv4_quantize": (C.c_int, [_vp, _u64, _vp, _vp, _vp, _vp]),
    "clv4_restore": (C.c_int, [_vp, _vp, _u64, _vp, _vp]),
    "clv4_dot_workspace_bytes": (_u64, [_u64]),
    "clv4_dot": (C.c_int, [_vp, _vp, _vp, _vp, _u64, C.c_int, _vp, _vp, _vp]),
    "clv8_dot_workspace_bytes": (_u64, [_u64]),
    "clv8_dot": (C.c_int, [_vp, _vp, _vp, _vp, _u64, C.c_int, _vp, _vp, _vp]),
    "clv4_word_isums": (C.c_int, [_vp, _vp, _u64, _vp, _vp]),
    "clm4_quantize": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "clm4_restore": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp]),
    "clm4_mvm": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_rowdots": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "clm4_gemm": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp]),
    "clm4_gemm_prepare": (C.c_int, [_vp, _u64, _u64, C.POINTER(_vp), _vp]),
    "clm4_gemm_release": (C.c_int, [_vp]),
    "clm4_gemm_prepared": (C.c_int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp, _vp]),
    "clm4_gemm_i32": (C.c_int, [_vp, _u64, _u64, _vp, _u64, _u64, _u64, _vp, _vp]),
    "clm4_gemm_i32_prepared": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _u64, _u64, _u64, _vp, _vp]),
    "clv4_scale_and_add": (C.c_int, [_vp, _vp, _vp, _vp, C.c_float, _u64, _vp, _vp, _vp, _vp]),
    "clm4_mvm_scale_and_add": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clv8_quantize": (C.c_int, [_vp, _u64, _vp, _vp, _vp, _vp]),
    "clv8_restore": (C.c_int, [_vp, _vp, _u64, _vp, _vp]),
    "clv8_scale_and_add": (C.c_int, [_vp, _vp, _vp, _vp, C.c_float, _u64, _vp, _vp, _vp, _vp]),
    "clv8_threshold_workspace_bytes": (_u64, [_u64]),
    "clv8_threshold": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp]),
    "clv8_threshold_mode": (C.c_int, [_vp, _vp, _u64, _u64, _u64, C.c_int, _vp, _vp]),
    "clm4_mvm_v8": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_mvm_v8_scale_and_add": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clv_iht_persistent_launches": (_u64, []),
    "clm4_iht_v8": (C.c_int, [_vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float,
                              C.c_int, _vp, _vp]),
    "clm4_rowdots_v8": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "clv4_threshold_workspace_bytes": (_u64, [_u64]),
    "clv4_threshold": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp]),
    "clv_threshold_reference_workspace_bytes": (_u64, [_u64]),
    "clv_threshold_reference_workspace_bytes_k": (_u64, [_u64, _u64]),
    "clv4_threshold_mode": (C.c_int, [_vp, _vp, _u64, _u64, _u64, C.c_int, _vp, _vp]),
    "clv4_threshold_heap": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp]),
    "clv8_threshold_heap": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp]),
    "clm4_transpose": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "clm4_mvm_f32": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "clm4_mvm_transposed": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_mvm_transposed_scale_and_add": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_iht_one_matrix": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float,
                                     C.c_int, _vp, _vp]),
    "clm4_mvm_v8_transposed": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_mvm_v8_transposed_scale_and_add": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_iht_v8_one_matrix": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float,
                                        C.c_int, _vp, _vp]),
    "clm8_quantize": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "clm8_restore": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp]),
    "clm8_mvm": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm8_mvm_scale_and_add": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm8_iht": (C.c_int, [_vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float,
                           C.c_int, _vp, _vp]),
    "clm8_mvm_f32": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "clm8_transpose": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "clm8_mvm_transposed": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm8_mvm_transposed_scale_and_add": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm8_iht_one_matrix": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float,
                                     C.c_int, _vp, _vp]),
    "clm8_gemm": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp]),
    "clm8_gemm_i32": (C.c_int, [_vp, _u64, _u64, _vp, _u64, _u64, _u64, _vp, _vp]),
    "clm4_gemm_m8": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp]),
    "clv_f16_quantize": (C.c_int, [_vp, _u64, _vp, _vp]),
    "clv_f16_restore": (C.c_int, [_vp, _u64, _vp, _vp]),
    "clv_f16_scale_and_add": (C.c_int, [_vp, _vp, C.c_float, _u64, _vp, _vp]),
    "clv_f16_dot_workspace_bytes": (_u64, [_u64]),
    "clv_f16_dot": (C.c_int, [_vp, _vp, _u64, C.c_int, _vp, _vp, _vp]),
    "clv_f16_threshold_workspace_bytes": (_u64, [_u64]),
    "clv_f16_threshold_mode": (C.c_int, [_vp, _u64, _u64, _u64, C.c_int, _vp, _vp]),
    "clv_f16_threshold_heap": (C.c_int, [_vp, _u64, _u64, _u64, _vp, _vp, _vp]),
    "clm_f16_quantize": (C.c_int, [_vp, _u64, _u64, _vp, _vp]),
    "clm_f16_mvm": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _vp]),
    "clm_f16_mvm_f32": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _vp]),
    "clm_f16_mvm_scale_and_add": (C.c_int, [_vp, _u64, _u64, _vp, _vp, C.c_float, _vp, _vp, _vp]),
    "clm_f16_iht": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float, C.c_int, _vp]),
    "clm_f16_transpose": (C.c_int, [_vp, _u64, _u64, _vp, _vp]),
    "clm4_iht": (C.c_int, [_vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64,
                          C.c_float, C.c_int, _vp, _vp]),
    # the batch calls: pointer arrays are HOST arrays (ctypes arrays of c_void_p) of device pointers
    "clm4_mvm_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_mvm_batch_at": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp]),
    "clv_mvm_batch_launches": (_u64, []),
    "clm4_mvm_scale_and_add_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clv4_threshold_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _u64, C.c_int, _vp]),
    "clm4_iht_batch": (C.c_int, [_vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64,
                                C.c_float, C.c_int, _vp, _vp]),
    # the same with CloverVector8 vectors (mvm_batch8.hip)
    "clm4_mvm_v8_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_mvm_v8_batch_at": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp]),
    "clm4_mvm_v8_scale_and_add_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clv8_threshold_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _u64, C.c_int, _vp]),
    "clm4_iht_v8_batch": (C.c_int, [_vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64,
                                   C.c_float, C.c_int, _vp, _vp]),
    # the pure 8-bit path (matrix8_batch.hip)
    "clm8_mvm_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm8_mvm_batch_at": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp]),
    "clm8_mvm_scale_and_add_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm8_iht_batch": (C.c_int, [_vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64,
                                C.c_float, C.c_int, _vp, _vp]),
    "clm4_shard_partition": (C.c_int, [_u64, C.c_int, C.c_int, C.POINTER(_u64), C.POINTER(_u64)]),
    "clm4_sharded_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.POINTER(C.c_int), _u64, _u64]),
    "clm4_sharded_destroy": (C.c_int, [_vp]),
    "clm4_sharded_info": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_vp), C.POINTER(_vp)]),
    "clm4_sharded_timing": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "clm4_sharded_comm_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "clm4_sharded_upload": (C.c_int, [_vp, _vp, _vp]),
    "clm4_sharded_fill_random": (C.c_int, [_vp, _u64]),
    "clm4_sharded_mvm": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp]),
    "clm4_sharded_result": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(_vp)]),
    "clm4_sharded_set_x": (C.c_int, [_vp, _vp, _vp, C.c_int]),
    "clm4_sharded_loop_begin": (C.c_int, [_vp, C.c_int]),
    "clm4_sharded_mvm_enqueue": (C.c_int, [_vp, C.c_int, C.c_int]),
    "clm4_sharded_sync": (C.c_int, [_vp]),
    "clm4_sharded_step_timing": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "clm4_sharded_result_buf": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_vp)]),
    "clm4_sharded_gemm": (C.c_int, [_vp, _vp, _vp, _u64, C.c_int, _vp]),
    "clm4_sharded_gemm_result": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "clm4_sharded_gemm_begin": (C.c_int, [_vp, _vp, _vp, _u64, C.c_int, C.c_int]),
    "clm4_sharded_gemm_begin_mode": (C.c_int, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, C.c_int]),
    "clm4_sharded_gemm_enqueue": (C.c_int, [_vp, C.c_int, C.c_int]),
    "clm4_sharded_gemm_full": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "clv_fill_random_nibbles": (C.c_int, [_vp, _u64, _u64, _u64, _vp]),
    "clv_fill_random_scales": (C.c_int, [_vp, _u64, _u64, _u64, _vp]),
    "clv_fill_random_ints_f32": (C.c_int, [_vp, _u64, C.c_int, _u64, _u64, _vp]),
}

# name -> (restype, argtypes); everything include/clover_hip_fp32.h declares (CloverVector32 / CloverMatrix32 on the device)
SIGNATURES_FP32 = {
    "clv_f32_scale_and_add": (C.c_int, [_vp, _vp, C.c_float, _u64, _vp, _vp]),
    "clv_f32_dot_workspace_bytes": (_u64, [_u64]),
    "clv_f32_dot": (C.c_int, [_vp, _vp, _u64, C.c_int, _vp, _vp, _vp]),
    "clv_f32_threshold_workspace_bytes": (_u64, [_u64]),
    "clv_f32_threshold_mode": (C.c_int, [_vp, _u64, _u64, _u64, C.c_int, _vp, _vp]),
    "clm_f32_mvm": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _vp]),
    "clm_f32_mvm_scale_and_add": (C.c_int, [_vp, _u64, _u64, _vp, _vp, C.c_float, _vp, _vp, _vp]),
    "clm_f32_transpose": (C.c_int, [_vp, _u64, _u64, _vp, _vp]),
    "clm_f32_iht": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float, C.c_int, _vp]),
}

# name -> (restype, argtypes); everything include/clover_hip_batch_t.h declares (the batched transposed 4-bit mvm, the one-matrix batched
# IHT / GD loop): the signatures of the clm4_*_batch family, clm4_iht_batch_one_matrix without the PhiT / sPhiT pair
SIGNATURES_BATCH_T = {
    "clm4_mvm_transposed_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_mvm_transposed_batch_at": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp]),
    "clm4_mvm_transposed_scale_and_add_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_iht_batch_one_matrix": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64,
                                           C.c_float, C.c_int, _vp, _vp]),
}

# name -> (restype, argtypes); everything include/clover_hip_batch_t8.h declares (the batched transposed 8-bit mvm, the one-matrix batched
# 8-bit IHT / GD loop): the signatures of the clm8_*_batch family, clm8_iht_batch_one_matrix without the PhiT / sPhiT pair
SIGNATURES_BATCH_T8 = {
    "clm8_mvm_transposed_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm8_mvm_transposed_batch_at": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp]),
    "clm8_mvm_transposed_scale_and_add_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm8_iht_batch_one_matrix": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64,
                                           C.c_float, C.c_int, _vp, _vp]),
}

# name -> (restype, argtypes); everything include/clover_hip_batch_t_v8.h declares (the batched transposed mixed mvm, CloverMatrix4 x
# CloverVector8, and the one-matrix batched mixed IHT / GD loop): the signatures of the clm4_*_v8_batch family, clm4_iht_v8_batch_one_matrix
# without the PhiT / sPhiT pair
SIGNATURES_BATCH_T_V8 = {
    "clm4_mvm_v8_transposed_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_mvm_v8_transposed_batch_at": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _vp]),
    "clm4_mvm_v8_transposed_scale_and_add_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "clm4_iht_v8_batch_one_matrix": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64,
                                              C.c_float, C.c_int, _vp, _vp]),
}


# name -> (restype, argtypes); everything include/clover_hip_batch_f16.h declares (the batched half-precision mvm, CloverMatrix16 x
# CloverVector16: plain, fused, the threshold of several vectors and the IHT / GD loop for several signals): no scales, no generator
SIGNATURES_BATCH_F16 = {
    "clm_f16_mvm_batch": (C.c_int, [_vp, _u64, _u64, _u64, _vp, _vp, _vp]),
    "clm_f16_mvm_scale_and_add_batch": (C.c_int, [_vp, _u64, _u64, _u64, _vp, _vp, C.c_float, _vp, _vp, _vp]),
    "clv_f16_threshold_batch": (C.c_int, [_vp, _u64, _u64, _u64, _u64, C.c_int, _vp]),
    "clm_f16_iht_batch": (C.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float, C.c_int, _vp]),
}


# name -> (restype, argtypes); everything include/clover_hip_f16_t.h declares (the transposed half-precision mvm, A' x straight from a
# CloverMatrix16's own bytes: f16 and fp32 vectors, the fused form, the IHT / GD loop that holds one matrix)
SIGNATURES_F16_T = {
    "clm_f16_mvm_transposed": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _vp]),
    "clm_f16_mvm_f32_transposed": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _vp]),
    "clm_f16_mvm_transposed_scale_and_add": (C.c_int, [_vp, _u64, _u64, _vp, _vp, C.c_float, _vp, _vp, _vp]),
    "clm_f16_iht_one_matrix": (C.c_int, [_vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float, C.c_int, _vp]),
}


# name -> (restype, argtypes); everything include/clover_hip_batch_f16_t.h declares (the batched transposed half-precision mvm, A' x[j]
# for several CloverVector16 in one pass over a CloverMatrix16's own bytes: plain, fused, the IHT / GD loop for several signals that holds
# one matrix)
SIGNATURES_BATCH_F16_T = {
    "clm_f16_mvm_transposed_batch": (C.c_int, [_vp, _u64, _u64, _u64, _vp, _vp, _vp]),
    "clm_f16_mvm_transposed_scale_and_add_batch": (C.c_int, [_vp, _u64, _u64, _u64, _vp, _vp, C.c_float, _vp, _vp, _vp]),
    "clm_f16_iht_batch_one_matrix": (C.c_int, [_vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float, C.c_int, _vp]),
}

# name -> (restype, argtypes); everything include/clover_hip_m4_f32.h declares (CloverMatrix4 on fp32 vectors: the fused mvm + scaleAndAdd,
# A' x straight from A's own bytes with its fused form, the IHT / GD loop of <CloverMatrix4, CloverVector32> with two matrices or one)
SIGNATURES_M4_F32 = {
    "clm4_mvm_f32_scale_and_add": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, C.c_float, _vp, _vp, _vp]),
    "clm4_mvm_f32_transposed": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "clm4_mvm_f32_transposed_scale_and_add": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, C.c_float, _vp, _vp, _vp]),
    "clm4_iht_f32": (C.c_int, [_vp, _vp, _vp, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float, C.c_int, _vp]),
    "clm4_iht_f32_one_matrix": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, C.c_float, C.c_int, _vp]),
}

# name -> (restype, argtypes); everything include/clover_hip_m8_f32.h declares: the same column for CloverMatrix8
SIGNATURES_M8_F32 = {"clm8" + name[4:]: sig for name, sig in SIGNATURES_M4_F32.items()}


class CloverHipError(RuntimeError):
    pass


def load_library(path: str | Path | None = None, allow_probe: bool = False) -> C.CDLL:
    """dlopen the HIP library and attach prototypes; raises if it is not built.  The bench-only probe build (tools/_build/, GEMM loop variants
    that are wrong by construction) announces itself through clv_version() and is refused unless allow_probe is set."""
    p = Path(path) if path else hip_library_path()
    if not p.exists():
        raise CloverHipError(
            f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP extension is mandatory, there is no CPU fallback)")
    lib = C.CDLL(str(p))
    for name, (res, args) in (*SIGNATURES.items(), *SIGNATURES_FP32.items(), *SIGNATURES_BATCH_T.items(), *SIGNATURES_BATCH_T8.items(), *SIGNATURES_BATCH_T_V8.items(),
                              *SIGNATURES_BATCH_F16.items(), *SIGNATURES_F16_T.items(), *SIGNATURES_BATCH_F16_T.items(), *SIGNATURES_M4_F32.items(),
                              *SIGNATURES_M8_F32.items()):
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.clv_version().decode().startswith("clover_hip_probe") and not allow_probe:
        raise CloverHipError(f"{p} is the bench-only probe build ({lib.clv_version().decode()}): not a product library")
    return lib


class DevBuf:
    """A device allocation owned by Python (freed on GC)."""

    def __init__(self, hip: "CloverHip", nbytes: int):
        self.hip = hip
        self.nbytes = int(nbytes)
        p = _vp()
        hip.check(hip.lib.clv_malloc(C.byref(p), self.nbytes))
        self.ptr = p.value or 0

    def __del__(self):
        try:
            if self.ptr:
                self.hip.lib.clv_free(self.ptr)
                self.ptr = 0
        except Exception:
            pass

    def upload(self, arr: np.ndarray, stream=None) -> "DevBuf":
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        self.hip.check(self.hip.lib.clv_memcpy_h2d(self.ptr, a.ctypes.data, a.nbytes, stream))
        self.hip.check(self.hip.lib.clv_stream_sync(stream))
        return self

    def download(self, dtype, count: int | None = None, stream=None) -> np.ndarray:
        dt = np.dtype(dtype)
        n = self.nbytes // dt.itemsize if count is None else int(count)
        out = np.empty(n, dtype=dt)
        self.hip.check(self.hip.lib.clv_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, stream))
        return out

    def offset(self, nbytes: int) -> int:
        return self.ptr + int(nbytes)


class CloverHip:
    """Thin object wrapper: error checking + numpy convenience around the C ABI."""

    def __init__(self, path: str | Path | None = None, device: int | None = None, allow_probe: bool = False):
        self.lib = load_library(path, allow_probe=allow_probe)
        n = C.c_int(0)
        self.check(self.lib.clv_device_count(C.byref(n)))
        self.device_count = n.value
        if self.device_count < 1:
            raise CloverHipError("no HIP device visible (libclover_hip.so needs an MI355X / gfx950 GPU)")
        if device is not None:
            self.check(self.lib.clv_set_device(device))

    # -- plumbing ------------------------------------------------------------------------------
    def check(self, rc: int) -> None:
        if rc != 0:
            raise CloverHipError(f"clover_hip error {rc}: {self.lib.clv_last_error().decode()}")

    def alloc(self, nbytes: int) -> DevBuf:
        return DevBuf(self, nbytes)

    def to_device(self, arr: np.ndarray) -> DevBuf:
        a = np.ascontiguousarray(arr)
        return DevBuf(self, max(a.nbytes, 1)).upload(a)

    def sync(self) -> None:
        self.check(self.lib.clv_device_sync())

    def device_info(self) -> dict:
        name = C.create_string_buffer(256)
        cu = C.c_int(0)
        mem = _u64(0)
        self.check(self.lib.clv_device_info(name, 256, C.byref(cu), C.byref(mem)))
        return {"name": name.value.decode(), "compute_units": cu.value, "hbm_bytes": mem.value}

    def new_rng(self, key1: int, key2: int) -> DevBuf:
        st = self.alloc(256)      # CLV_RNG_STATE_BYTES
        self.check(self.lib.clv_rng_seed(st.ptr, key1, key2, None))
        return st

    def rng_get(self, st: DevBuf) -> tuple[np.ndarray, np.ndarray]:
        k1 = (_u64 * 4)()
        k2 = (_u64 * 4)()
        self.check(self.lib.clv_rng_get(st.ptr, k1, k2, None))
        return np.array(k1[:], dtype=np.uint64), np.array(k2[:], dtype=np.uint64)

    # -- CloverVector4 ---------------------------------------------------------------------------
    def v4_quantize(self, x: np.ndarray, rng: DevBuf | None = None):
        """numpy fp32 (padded) -> (bytes uint8[n/2], scales fp32[n/64]) through the device."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.size
        dx = self.to_device(x)
        dq, ds = self.alloc(max(n // 2, 1)), self.alloc(max(n // 16, 4))
        self.check(self.lib.clv4_quantize(dx.ptr, n, dq.ptr, ds.ptr, rng.ptr if rng else None, None))
        return dq.download(np.uint8, n // 2), ds.download(np.float32, n // 64)

    def v4_restore(self, q: np.ndarray, s: np.ndarray) -> np.ndarray:
        n = q.size * 2
        dq, ds = self.to_device(q), self.to_device(s)
        dx = self.alloc(max(4 * n, 4))
        self.check(self.lib.clv4_restore(dq.ptr, ds.ptr, n, dx.ptr, None))
        return dx.download(np.float32, n)

    def v4_dot(self, qu, su, qv, sv, mode: int = DOT_EXACT) -> np.float32:
        n = qu.size * 2
        bufs = [self.to_device(a) for a in (qu, su, qv, sv)]
        out = self.alloc(4)
        self.check(self.lib.clv4_dot(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, mode, out.ptr, None, None))
        return out.download(np.float32, 1)[0]

    def v4_word_isums(self, qu, qv) -> np.ndarray:
        n = qu.size * 2
        du, dv = self.to_device(qu), self.to_device(qv)
        out = self.alloc(max(n // 2, 4))
        self.check(self.lib.clv4_word_isums(du.ptr, dv.ptr, n, out.ptr, None))
        return out.download(np.int32, n // 8)

    # -- CloverMatrix4 ---------------------------------------------------------------------------
    def m4_quantize(self, A: np.ndarray, rng: DevBuf | None = None):
        A = np.ascontiguousarray(A, dtype=np.float32)
        rows, cols = A.shape
        dA = self.to_device(A)
        dq, ds = self.alloc(max(rows * cols // 2, 1)), self.alloc(max((rows // 64) * (cols // 64) * 4, 4))
        self.check(self.lib.clm4_quantize(dA.ptr, rows, cols, dq.ptr, ds.ptr, rng.ptr if rng else None, None))
        return dq.download(np.uint8, rows * cols // 2), ds.download(np.float32, (rows // 64) * (cols // 64))

    def m4_restore(self, q, s, rows, cols) -> np.ndarray:
        dq, ds, dA = self.to_device(q), self.to_device(s), self.alloc(max(4 * rows * cols, 4))
        self.check(self.lib.clm4_restore(dq.ptr, ds.ptr, rows, cols, dA.ptr, None))
        return dA.download(np.float32, rows * cols).reshape(rows, cols)

    def m4_mvm(self, qA, sA, rows, cols, qx, sx, rng: DevBuf | None = None):
        b = [self.to_device(a) for a in (qA, sA, qx, sx)]
        dr, dsr = self.alloc(max(rows // 2, 1)), self.alloc(max(rows // 16, 4))
        self.check(self.lib.clm4_mvm(b[0].ptr, b[1].ptr, rows, cols, b[2].ptr, b[3].ptr, dr.ptr, dsr.ptr,
                                     rng.ptr if rng else None, None))
        return dr.download(np.uint8, rows // 2), dsr.download(np.float32, rows // 64)

    def m4_rowdots(self, qA, sA, rows, cols, qx, sx) -> np.ndarray:
        b = [self.to_device(a) for a in (qA, sA, qx, sx)]
        d = self.alloc(max(rows * 4, 4))
        self.check(self.lib.clm4_rowdots(b[0].ptr, b[1].ptr, rows, cols, b[2].ptr, b[3].ptr, d.ptr, None))
        return d.download(np.float32, rows)

    def v4_scale_and_add(self, qu, su, qv, sv, a: float, rng: DevBuf | None = None, in_place: bool = False):
        n = qu.size * 2
        b = [self.to_device(x) for x in (qu, su, qv, sv)]
        dr, dsr = (b[0], b[1]) if in_place else (self.alloc(max(n // 2, 1)), self.alloc(max(n // 16, 4)))
        self.check(self.lib.clv4_scale_and_add(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, a, n, dr.ptr, dsr.ptr,
                                               rng.ptr if rng else None, None))
        return dr.download(np.uint8, n // 2), dsr.download(np.float32, n // 64)

    def m4_mvm_scale_and_add(self, qA, sA, rows, cols, qx, sx, qu, su, a: float, rng: DevBuf | None = None, in_place: bool = False,
                             want_t: bool = True):
        """(t, st, r, sr) of clm4_mvm_scale_and_add; t/st are None when want_t is False"""
        b = [self.to_device(v) for v in (qA, sA, qx, sx, qu, su)]
        dt, dst = (self.alloc(rows // 2), self.alloc(rows // 16)) if want_t else (None, None)
        dr, dsr = (b[4], b[5]) if in_place else (self.alloc(rows // 2), self.alloc(rows // 16))
        self.check(self.lib.clm4_mvm_scale_and_add(b[0].ptr, b[1].ptr, rows, cols, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, a,
                                                   dt.ptr if dt else None, dst.ptr if dst else None, dr.ptr, dsr.ptr,
                                                   rng.ptr if rng else None, None))
        t = (dt.download(np.uint8, rows // 2), dst.download(np.float32, rows // 64)) if want_t else (None, None)
        return t[0], t[1], dr.download(np.uint8, rows // 2), dsr.download(np.float32, rows // 64)

    # -- several vectors with one CloverMatrix4 (host arrays of device pointers; lists in, lists out) ------------------------------
    @staticmethod
    def ptr_array(ptrs):
        """a host array of device pointers for the batch calls, from DevBufs / addresses; None stays NULL"""
        if ptrs is None:
            return None
        return (_vp * len(ptrs))(*[p.ptr if isinstance(p, DevBuf) else p for p in ptrs])

    def m4_mvm_batch(self, qA, sA, rows, cols, xs, rng: DevBuf | None = None):
        """xs: list of (qx, sx); returns the list of (r, sr) of clm4_mvm_batch.  qA may be a DevBuf (a matrix uploaded once)"""
        dA, dsA = (qA, sA) if isinstance(qA, DevBuf) else (self.to_device(qA), self.to_device(sA))
        dx = [(self.to_device(q), self.to_device(s)) for q, s in xs]
        dr = [(self.alloc(max(rows // 2, 1)), self.alloc(max(rows // 16, 4))) for _ in xs]
        pa = self.ptr_array
        self.check(self.lib.clm4_mvm_batch(dA.ptr, dsA.ptr, rows, cols, len(xs), pa([d[0] for d in dx]), pa([d[1] for d in dx]),
                                           pa([d[0] for d in dr]), pa([d[1] for d in dr]), rng.ptr if rng else None, None))
        return [(r.download(np.uint8, rows // 2), sr.download(np.float32, rows // 64)) for r, sr in dr]

    def m4_mvm_scale_and_add_batch(self, qA, sA, rows, cols, xs, us, a: float, rng: DevBuf | None = None, in_place: bool = False,
                                   want_t: bool = True):
        """xs, us: lists of (q, s); returns the list of (t, st, r, sr) of clm4_mvm_scale_and_add_batch; t/st are None when want_t is False"""
        dA, dsA = (qA, sA) if isinstance(qA, DevBuf) else (self.to_device(qA), self.to_device(sA))
        dx = [(self.to_device(q), self.to_device(s)) for q, s in xs]
        du = [(self.to_device(q), self.to_device(s)) for q, s in us]
        dt = [(self.alloc(rows // 2), self.alloc(rows // 16)) for _ in xs] if want_t else None
        dr = du if in_place else [(self.alloc(rows // 2), self.alloc(rows // 16)) for _ in xs]
        pa = self.ptr_array
        self.check(self.lib.clm4_mvm_scale_and_add_batch(
            dA.ptr, dsA.ptr, rows, cols, len(xs), pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([d[0] for d in du]), pa([d[1] for d in du]), a,
            pa([d[0] for d in dt]) if dt else None, pa([d[1] for d in dt]) if dt else None, pa([d[0] for d in dr]), pa([d[1] for d in dr]),
            rng.ptr if rng else None, None))
        out = []
        for j in range(len(xs)):
            t = (dt[j][0].download(np.uint8, rows // 2), dt[j][1].download(np.float32, rows // 64)) if want_t else (None, None)
            out.append((t[0], t[1], dr[j][0].download(np.uint8, rows // 2), dr[j][1].download(np.float32, rows // 64)))
        return out

    def v4_threshold_batch(self, vs, n: int, k: int, mode: int = THRESHOLD_FAST):
        """vs: list of (q, s) of one padded size; returns the list of thresholded q"""
        dv = [(self.to_device(q), self.to_device(s)) for q, s in vs]
        pa = self.ptr_array
        self.check(self.lib.clv4_threshold_batch(pa([d[0] for d in dv]), pa([d[1] for d in dv]), len(vs), n, vs[0][0].size * 2 if vs else 0, k,
                                                 mode, None))
        return [d[0].download(np.uint8, q.size) for d, (q, _) in zip(dv, vs)]

    def m4_iht_batch(self, qPhi, sPhi, qPhiT, sPhiT, m, n, ys, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
                     rng: DevBuf | None = None, prefill: int = 0x55):
        """clm4_iht_batch on buffers prefilled with `prefill` bytes -- or, with qPhiT None, clm4_iht_batch_one_matrix; ys: list of (qy, sy);
        returns per vector {"x": (q, s), "t1": ..., "t2": ..., "t3": ...}"""
        b = [self.to_device(v) for v in ((qPhi, sPhi) if qPhiT is None else (qPhi, sPhi, qPhiT, sPhiT))]
        dy = [(self.to_device(q), self.to_device(s)) for q, s in ys]
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {name: [(self.alloc(ln // 2), self.alloc(ln // 16)) for _ in ys] for name, ln in lens.items()}
        for bufs in v.values():
            for pair in bufs:
                for d in pair:
                    self.check(self.lib.clv_memset(d.ptr, prefill, d.nbytes, None))
        pa = self.ptr_array
        arr = {name: (pa([d[0] for d in bufs]), pa([d[1] for d in bufs])) for name, bufs in v.items()}
        tail = (m, n, len(ys), arr["x"][0], arr["x"][1], n if x_len is None else x_len, pa([d[0] for d in dy]), pa([d[1] for d in dy]),
                arr["t1"][0], arr["t1"][1], arr["t2"][0], arr["t2"][1], arr["t3"][0], arr["t3"][1], iterations, K, mu, threshold,
                rng.ptr if rng else None, None)
        if qPhiT is None:
            self.check(self.lib.clm4_iht_batch_one_matrix(b[0].ptr, b[1].ptr, *tail))
        else:
            self.check(self.lib.clm4_iht_batch(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, *tail))
        return [{name: (v[name][j][0].download(np.uint8, ln // 2), v[name][j][1].download(np.float32, ln // 64)) for name, ln in lens.items()}
                for j in range(len(ys))]

    # -- mixed precision (CloverVector8) ----------------------------------------------------------
    def v8_quantize(self, x: np.ndarray, rng: DevBuf | None = None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.size
        dx, dq, ds = self.to_device(x), self.alloc(max(n, 1)), self.alloc(max(n // 16, 4))
        self.check(self.lib.clv8_quantize(dx.ptr, n, dq.ptr, ds.ptr, rng.ptr if rng else None, None))
        return dq.download(np.int8, n), ds.download(np.float32, n // 64)

    def v8_restore(self, q, s) -> np.ndarray:
        n = q.size
        dq, ds, dx = self.to_device(q), self.to_device(s), self.alloc(max(4 * n, 4))
        self.check(self.lib.clv8_restore(dq.ptr, ds.ptr, n, dx.ptr, None))
        return dx.download(np.float32, n)

    def v8_scale_and_add(self, qu, su, qv, sv, a: float, rng: DevBuf | None = None, in_place: bool = False):
        n = qu.size
        b = [self.to_device(x) for x in (qu, su, qv, sv)]
        dr, dsr = (b[0], b[1]) if in_place else (self.alloc(max(n, 1)), self.alloc(max(n // 16, 4)))
        self.check(self.lib.clv8_scale_and_add(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, a, n, dr.ptr, dsr.ptr, rng.ptr if rng else None, None))
        return dr.download(np.int8, n), dsr.download(np.float32, n // 64)

    def v8_dot(self, qu, su, qv, sv, mode: int = DOT_EXACT) -> np.float32:
        n = qu.size
        bufs = [self.to_device(a) for a in (qu, su, qv, sv)]
        out = self.alloc(4)
        self.check(self.lib.clv8_dot(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, mode, out.ptr, None, None))
        return out.download(np.float32, 1)[0]

    def v8_threshold(self, q, s, n: int, k: int, mode: int = THRESHOLD_FAST) -> np.ndarray:
        dq, ds = self.to_device(q), self.to_device(s)
        self.check(self.lib.clv8_threshold_mode(dq.ptr, ds.ptr, n, q.size, k, mode, None, None))
        return dq.download(np.int8, q.size)

    def m4_mvm_v8(self, qA, sA, rows, cols, qx, sx, rng: DevBuf | None = None):
        b = [self.to_device(a) for a in (qA, sA, qx, sx)]
        dr, dsr = self.alloc(max(rows, 1)), self.alloc(max(rows // 16, 4))
        self.check(self.lib.clm4_mvm_v8(b[0].ptr, b[1].ptr, rows, cols, b[2].ptr, b[3].ptr, dr.ptr, dsr.ptr, rng.ptr if rng else None, None))
        return dr.download(np.int8, rows), dsr.download(np.float32, rows // 64)

    def m4_rowdots_v8(self, qA, sA, rows, cols, qx, sx) -> np.ndarray:
        b = [self.to_device(a) for a in (qA, sA, qx, sx)]
        d = self.alloc(max(rows * 4, 4))
        self.check(self.lib.clm4_rowdots_v8(b[0].ptr, b[1].ptr, rows, cols, b[2].ptr, b[3].ptr, d.ptr, None))
        return d.download(np.float32, rows)

    def v4_threshold(self, q, s, n: int, k: int, mode: int = THRESHOLD_FAST) -> np.ndarray:
        dq, ds = self.to_device(q), self.to_device(s)
        self.check(self.lib.clv4_threshold_mode(dq.ptr, ds.ptr, n, q.size * 2, k, mode, None, None))
        return dq.download(np.uint8, q.size)

    def m4_transpose(self, q, s, rows, cols):
        dq, ds = self.to_device(q), self.to_device(s)
        dt, dst = self.alloc(max(rows * cols // 2, 1)), self.alloc(max((rows // 64) * (cols // 64) * 4, 4))
        self.check(self.lib.clm4_transpose(dq.ptr, ds.ptr, rows, cols, dt.ptr, dst.ptr, None))
        return dt.download(np.uint8, rows * cols // 2), dst.download(np.float32, (rows // 64) * (cols // 64))

    def m4_mvm_transposed(self, qA, sA, rows, cols, qx, sx, rng: DevBuf | None = None):
        """(r, sr) of clm4_mvm_transposed: A is rows x cols, x has rows elements, r has cols.  qA may be a DevBuf (a matrix uploaded once)"""
        dA, dsA = (qA, sA) if isinstance(qA, DevBuf) else (self.to_device(qA), self.to_device(sA))
        dx, dsx = self.to_device(qx), self.to_device(sx)
        dr, dsr = self.alloc(max(cols // 2, 1)), self.alloc(max(cols // 16, 4))
        self.check(self.lib.clm4_mvm_transposed(dA.ptr, dsA.ptr, rows, cols, dx.ptr, dsx.ptr, dr.ptr, dsr.ptr, rng.ptr if rng else None, None))
        return dr.download(np.uint8, cols // 2), dsr.download(np.float32, cols // 64)

    def m4_mvm_transposed_scale_and_add(self, qA, sA, rows, cols, qx, sx, qu, su, a: float, rng: DevBuf | None = None, in_place: bool = False,
                                        want_t: bool = True):
        """(t, st, r, sr) of clm4_mvm_transposed_scale_and_add (u, t, r: cols elements); t/st are None when want_t is False"""
        dA, dsA = (qA, sA) if isinstance(qA, DevBuf) else (self.to_device(qA), self.to_device(sA))
        b = [self.to_device(v) for v in (qx, sx, qu, su)]
        dt, dst = (self.alloc(cols // 2), self.alloc(cols // 16)) if want_t else (None, None)
        dr, dsr = (b[2], b[3]) if in_place else (self.alloc(cols // 2), self.alloc(cols // 16))
        self.check(self.lib.clm4_mvm_transposed_scale_and_add(dA.ptr, dsA.ptr, rows, cols, b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, a,
                                                              dt.ptr if dt else None, dst.ptr if dst else None, dr.ptr, dsr.ptr,
                                                              rng.ptr if rng else None, None))
        t = (dt.download(np.uint8, cols // 2), dst.download(np.float32, cols // 64)) if want_t else (None, None)
        return t[0], t[1], dr.download(np.uint8, cols // 2), dsr.download(np.float32, cols // 64)

    def m4_mvm_transposed_batch(self, qA, sA, rows, cols, xs, rng: DevBuf | None = None, at=None):
        """xs: list of (qx, sx) of `rows` elements; returns the list of (r, sr), `cols` elements each, of clm4_mvm_transposed_batch -- or,
        with at = (draw_base, draw_stride, commit_draws), of clm4_mvm_transposed_batch_at.  qA may be a DevBuf (a matrix uploaded once);
        an x that is the same object twice is uploaded once (a repeated input pointer)"""
        dA, dsA = (qA, sA) if isinstance(qA, DevBuf) else (self.to_device(qA), self.to_device(sA))
        dx = self._upload_pairs(xs)
        dr = [(self.alloc(max(cols // 2, 1)), self.alloc(max(cols // 16, 4))) for _ in xs]
        pa = self.ptr_array
        args = (dA.ptr, dsA.ptr, rows, cols, len(xs), pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([d[0] for d in dr]), pa([d[1] for d in dr]),
                rng.ptr if rng else None)
        if at is None:
            self.check(self.lib.clm4_mvm_transposed_batch(*args, None))
        else:
            self.check(self.lib.clm4_mvm_transposed_batch_at(*args, *at, None))
        return [(r.download(np.uint8, cols // 2), sr.download(np.float32, cols // 64)) for r, sr in dr]

    def m4_mvm_transposed_scale_and_add_batch(self, qA, sA, rows, cols, xs, us, a: float, rng: DevBuf | None = None, in_place: bool = False,
                                              want_t: bool = True):
        """xs: list of (q, s) of `rows` elements, us: of `cols`; returns the list of (t, st, r, sr) of
        clm4_mvm_transposed_scale_and_add_batch; t/st are None when want_t is False"""
        dA, dsA = (qA, sA) if isinstance(qA, DevBuf) else (self.to_device(qA), self.to_device(sA))
        dx = self._upload_pairs(xs)
        du = [(self.to_device(q), self.to_device(s)) for q, s in us]
        dt = [(self.alloc(cols // 2), self.alloc(cols // 16)) for _ in xs] if want_t else None
        dr = du if in_place else [(self.alloc(cols // 2), self.alloc(cols // 16)) for _ in xs]
        pa = self.ptr_array
        self.check(self.lib.clm4_mvm_transposed_scale_and_add_batch(
            dA.ptr, dsA.ptr, rows, cols, len(xs), pa([d[0] for d in dx]), pa([d[1] for d in dx]), pa([d[0] for d in du]), pa([d[1] for d in du]), a,
            pa([d[0] for d in dt]) if dt else None, pa([d[1] for d in dt]) if dt else None, pa([d[0] for d in dr]), pa([d[1] for d in dr]),
            rng.ptr if rng else None, None))
        out = []
        for j in range(len(xs)):
            t = (dt[j][0].download(np.uint8, cols // 2), dt[j][1].download(np.float32, cols // 64)) if want_t else (None, None)
            out.append((t[0], t[1], dr[j][0].download(np.uint8, cols // 2), dr[j][1].download(np.float32, cols // 64)))
        return out

    def _upload_pairs(self, pairs):
        """device copies of a list of (q, s); a pair whose q is the same object as an earlier one shares that pair's buffers"""
        seen, out = {}, []
        for q, s in pairs:
            if id(q) not in seen:
                seen[id(q)] = (self.to_device(q), self.to_device(s))
            out.append(seen[id(q)])
        return out

    def m4_iht(self, qPhi, sPhi, qPhiT, sPhiT, m, n, qy, sy, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
               rng: DevBuf | None = None, prefill: int = 0x55):
        """clm4_iht on buffers prefilled with `prefill` bytes -- or, with qPhiT None, clm4_iht_one_matrix:
        {"x": (q, s), "t1": ..., "t2": ..., "t3": ...}"""
        b = [self.to_device(v) for v in ((qPhi, sPhi, qy, sy) if qPhiT is None else (qPhi, sPhi, qy, sy, qPhiT, sPhiT))]
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {}
        for name, ln in lens.items():
            v[name] = (self.alloc(ln // 2), self.alloc(ln // 16))
            for d in v[name]:
                self.check(self.lib.clv_memset(d.ptr, prefill, d.nbytes, None))
        tail = (v["x"][0].ptr, v["x"][1].ptr, n if x_len is None else x_len, b[2].ptr, b[3].ptr, v["t1"][0].ptr, v["t1"][1].ptr, v["t2"][0].ptr,
                v["t2"][1].ptr, v["t3"][0].ptr, v["t3"][1].ptr, iterations, K, mu, threshold, rng.ptr if rng else None, None)
        if qPhiT is None:
            self.check(self.lib.clm4_iht_one_matrix(b[0].ptr, b[1].ptr, m, n, *tail))
        else:
            self.check(self.lib.clm4_iht(b[0].ptr, b[1].ptr, b[4].ptr, b[5].ptr, m, n, *tail))
        return {name: (v[name][0].download(np.uint8, ln // 2), v[name][1].download(np.float32, ln // 64)) for name, ln in lens.items()}

    def m4_mvm_v8_transposed(self, qA, sA, rows, cols, qx, sx, rng: DevBuf | None = None):
        """(r, sr) of clm4_mvm_v8_transposed: A is rows x cols, x has rows int8, r has cols.  qA may be a DevBuf (a matrix uploaded once)"""
        dA, dsA = (qA, sA) if isinstance(qA, DevBuf) else (self.to_device(qA), self.to_device(sA))
        dx, dsx = self.to_device(qx), self.to_device(sx)
        dr, dsr = self.alloc(max(cols, 1)), self.alloc(max(cols // 16, 4))
        self.check(self.lib.clm4_mvm_v8_transposed(dA.ptr, dsA.ptr, rows, cols, dx.ptr, dsx.ptr, dr.ptr, dsr.ptr, rng.ptr if rng else None, None))
        return dr.download(np.int8, cols), dsr.download(np.float32, cols // 64)

    def m4_mvm_v8_transposed_scale_and_add(self, qA, sA, rows, cols, qx, sx, qu, su, a: float, rng: DevBuf | None = None, in_place: bool = False,
                                           want_t: bool = True):
        """(t, st, r, sr) of clm4_mvm_v8_transposed_scale_and_add (u, t, r: cols int8); t/st are None when want_t is False"""
        dA, dsA = (qA, sA) if isinstance(qA, DevBuf) else (self.to_device(qA), self.to_device(sA))
        b = [self.to_device(v) for v in (qx, sx, qu, su)]
        dt, dst = (self.alloc(cols), self.alloc(cols // 16)) if want_t else (None, None)
        dr, dsr = (b[2], b[3]) if in_place else (self.alloc(cols), self.alloc(cols // 16))
        self.check(self.lib.clm4_mvm_v8_transposed_scale_and_add(dA.ptr, dsA.ptr, rows, cols, b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, a,
                                                                 dt.ptr if dt else None, dst.ptr if dst else None, dr.ptr, dsr.ptr,
                                                                 rng.ptr if rng else None, None))
        t = (dt.download(np.int8, cols), dst.download(np.float32, cols // 64)) if want_t else (None, None)
        return t[0], t[1], dr.download(np.int8, cols), dsr.download(np.float32, cols // 64)

    def m4_iht_v8(self, qPhi, sPhi, qPhiT, sPhiT, m, n, qy, sy, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
                  rng: DevBuf | None = None, prefill: int = 0x55):
        """clm4_iht_v8 on buffers prefilled with `prefill` bytes -- or, with qPhiT None, clm4_iht_v8_one_matrix:
        {"x": (q, s), "t1": ..., "t2": ..., "t3": ...}"""
        b = [self.to_device(v) for v in ((qPhi, sPhi, qy, sy) if qPhiT is None else (qPhi, sPhi, qy, sy, qPhiT, sPhiT))]
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {}
        for name, ln in lens.items():
            v[name] = (self.alloc(ln), self.alloc(ln // 16))
            for d in v[name]:
                self.check(self.lib.clv_memset(d.ptr, prefill, d.nbytes, None))
        tail = (v["x"][0].ptr, v["x"][1].ptr, n if x_len is None else x_len, b[2].ptr, b[3].ptr, v["t1"][0].ptr, v["t1"][1].ptr, v["t2"][0].ptr,
                v["t2"][1].ptr, v["t3"][0].ptr, v["t3"][1].ptr, iterations, K, mu, threshold, rng.ptr if rng else None, None)
        if qPhiT is None:
            self.check(self.lib.clm4_iht_v8_one_matrix(b[0].ptr, b[1].ptr, m, n, *tail))
        else:
            self.check(self.lib.clm4_iht_v8(b[0].ptr, b[1].ptr, b[4].ptr, b[5].ptr, m, n, *tail))
        return {name: (v[name][0].download(np.int8, ln), v[name][1].download(np.float32, ln // 64)) for name, ln in lens.items()}

    def m4_iht_v8_batch(self, qPhi, sPhi, qPhiT, sPhiT, m, n, ys, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
                        rng: DevBuf | None = None, prefill: int = 0x55):
        """clm4_iht_v8_batch on buffers prefilled with `prefill` bytes -- or, with qPhiT None, clm4_iht_v8_batch_one_matrix; ys: list of
        (qy, sy); returns per vector {"x": (q, s), "t1": ..., "t2": ..., "t3": ...}"""
        b = [self.to_device(v) for v in ((qPhi, sPhi) if qPhiT is None else (qPhi, sPhi, qPhiT, sPhiT))]
        dy = [(self.to_device(q), self.to_device(s)) for q, s in ys]
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {name: [(self.alloc(ln), self.alloc(ln // 16)) for _ in ys] for name, ln in lens.items()}
        for bufs in v.values():
            for pair in bufs:
                for d in pair:
                    self.check(self.lib.clv_memset(d.ptr, prefill, d.nbytes, None))
        pa = self.ptr_array
        arr = {name: (pa([d[0] for d in bufs]), pa([d[1] for d in bufs])) for name, bufs in v.items()}
        tail = (m, n, len(ys), arr["x"][0], arr["x"][1], n if x_len is None else x_len, pa([d[0] for d in dy]), pa([d[1] for d in dy]),
                arr["t1"][0], arr["t1"][1], arr["t2"][0], arr["t2"][1], arr["t3"][0], arr["t3"][1], iterations, K, mu, threshold,
                rng.ptr if rng else None, None)
        if qPhiT is None:
            self.check(self.lib.clm4_iht_v8_batch_one_matrix(b[0].ptr, b[1].ptr, *tail))
        else:
            self.check(self.lib.clm4_iht_v8_batch(b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, *tail))
        return [{name: (v[name][j][0].download(np.int8, ln), v[name][j][1].download(np.float32, ln // 64)) for name, ln in lens.items()}
                for j in range(len(ys))]

    def m4_mvm_f32(self, qA, sA, rows, cols, x) -> np.ndarray:
        b = [self.to_device(a) for a in (qA, sA, np.ascontiguousarray(x, dtype=np.float32))]
        d = self.alloc(max(rows * 4, 4))
        self.check(self.lib.clm4_mvm_f32(b[0].ptr, b[1].ptr, rows, cols, b[2].ptr, d.ptr, None))
        return d.download(np.float32, rows)

    # CloverMatrix4 on fp32 vectors (include/clover_hip_m4_f32.h); the matrix pair and every vector a numpy array or a DevBuf
    def _m4_dev(self, q, s):
        return (q if isinstance(q, DevBuf) else self.to_device(q)), (s if isinstance(s, DevBuf) else self.to_device(s))

    def _m4_f32_fused(self, fn, qA, sA, rows, cols, nout, x, u, a, in_place, want_t):
        (dq, ds), dx, du = self._m4_dev(qA, sA), self._f32_dev(x), self._f32_dev(u)
        dt = self.alloc(max(4 * nout, 4)) if want_t else None
        dr = du if in_place else self.alloc(max(4 * nout, 4))
        self.check(fn(dq.ptr, ds.ptr, rows, cols, dx.ptr, du.ptr, a, dt.ptr if dt else None, dr.ptr, None))
        return (dt.download(np.float32, nout) if want_t else None), dr.download(np.float32, nout)

    def m4_mvm_f32_scale_and_add(self, qA, sA, rows, cols, x, u, a: float, in_place: bool = False, want_t: bool = True):
        """(t, r2) of clm4_mvm_f32_scale_and_add, `rows` values each; t is None when want_t is False"""
        return self._m4_f32_fused(self.lib.clm4_mvm_f32_scale_and_add, qA, sA, rows, cols, rows, x, u, a, in_place, want_t)

    def m4_mvm_f32_transposed(self, qA, sA, rows, cols, x) -> np.ndarray:
        (dq, ds), dx, dr = self._m4_dev(qA, sA), self._f32_dev(x), self.alloc(max(4 * cols, 4))
        self.check(self.lib.clm4_mvm_f32_transposed(dq.ptr, ds.ptr, rows, cols, dx.ptr, dr.ptr, None))
        return dr.download(np.float32, cols)

    def m4_mvm_f32_transposed_scale_and_add(self, qA, sA, rows, cols, x, u, a: float, in_place: bool = False, want_t: bool = True):
        """(t, r2) of clm4_mvm_f32_transposed_scale_and_add, `cols` values each; t is None when want_t is False"""
        return self._m4_f32_fused(self.lib.clm4_mvm_f32_transposed_scale_and_add, qA, sA, rows, cols, cols, x, u, a, in_place, want_t)

    def m4_iht_f32(self, qPhi, sPhi, qPhiT, sPhiT, m, n, y, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
                   prefill: int = 0x55):
        """clm4_iht_f32 (qPhiT None: clm4_iht_f32_one_matrix) on buffers prefilled with `prefill` bytes:
        {"x": fp32[n], "t1": fp32[m], "t2": fp32[m], "t3": fp32[n]}"""
        return self._q_iht_f32(self.lib.clm4_iht_f32, self.lib.clm4_iht_f32_one_matrix, qPhi, sPhi, qPhiT, sPhiT, m, n, y, iterations, K, mu,
                               threshold, x_len, prefill)

    def _q_iht_f32(self, two, one, qPhi, sPhi, qPhiT, sPhiT, m, n, y, iterations, K, mu, threshold, x_len, prefill):
        """the fp32-vector loop of a quantized matrix width: `two` with (qPhiT, sPhiT), `one` when qPhiT is None"""
        b = [*self._m4_dev(qPhi, sPhi), *(self._m4_dev(qPhiT, sPhiT) if qPhiT is not None else ())]
        dy = self._f32_dev(y)
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {}
        for name, ln in lens.items():
            v[name] = self.alloc(4 * ln)
            self.check(self.lib.clv_memset(v[name].ptr, prefill, v[name].nbytes, None))
        tail = (m, n, v["x"].ptr, n if x_len is None else x_len, dy.ptr, v["t1"].ptr, v["t2"].ptr, v["t3"].ptr, iterations, K, mu, threshold, None)
        fn = one if qPhiT is None else two
        self.check(fn(*[d.ptr for d in b], *tail))
        return {name: v[name].download(np.float32, ln) for name, ln in lens.items()}

    def m4_iht_f32_one_matrix(self, qPhi, sPhi, m, n, y, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
                              prefill: int = 0x55):
        return self.m4_iht_f32(qPhi, sPhi, None, None, m, n, y, iterations, K, mu, threshold, x_len=x_len, prefill=prefill)

    # -- CloverMatrix8 ---------------------------------------------------------------------------
    def m8_quantize(self, A: np.ndarray, rng: DevBuf | None = None):
        A = np.ascontiguousarray(A, dtype=np.float32)
        rows, cols = A.shape
        dA = self.to_device(A)
        dq, ds = self.alloc(max(rows * cols, 1)), self.alloc(max((rows // 64) * (cols // 64) * 4, 4))
        self.check(self.lib.clm8_quantize(dA.ptr, rows, cols, dq.ptr, ds.ptr, rng.ptr if rng else None, None))
        return dq.download(np.int8, rows * cols), ds.download(np.float32, (rows // 64) * (cols // 64))

    def m8_restore(self, q, s, rows, cols) -> np.ndarray:
        dq, ds, dA = self.to_device(q), self.to_device(s), self.alloc(max(4 * rows * cols, 4))
        self.check(self.lib.clm8_restore(dq.ptr, ds.ptr, rows, cols, dA.ptr, None))
        return dA.download(np.float32, rows * cols).reshape(rows, cols)

    def m8_mvm(self, qA, sA, rows, cols, qx, sx, rng: DevBuf | None = None):
        b = [self.to_device(a) for a in (qA, sA, qx, sx)]
        dr, dsr = self.alloc(max(rows, 1)), self.alloc(max(rows // 16, 4))
        self.check(self.lib.clm8_mvm(b[0].ptr, b[1].ptr, rows, cols, b[2].ptr, b[3].ptr, dr.ptr, dsr.ptr, rng.ptr if rng else None, None))
        return dr.download(np.int8, rows), dsr.download(np.float32, rows // 64)

    def m8_mvm_scale_and_add(self, qA, sA, rows, cols, qx, sx, qu, su, a: float, rng: DevBuf | None = None, in_place: bool = False,
                             want_t: bool = True):
        """(t, st, r, sr) of clm8_mvm_scale_and_add; t/st are None when want_t is False"""
        b = [self.to_device(v) for v in (qA, sA, qx, sx, qu, su)]
        dt, dst = (self.alloc(rows), self.alloc(rows // 16)) if want_t else (None, None)
        dr, dsr = (b[4], b[5]) if in_place else (self.alloc(rows), self.alloc(rows // 16))
        self.check(self.lib.clm8_mvm_scale_and_add(b[0].ptr, b[1].ptr, rows, cols, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, a,
                                                   dt.ptr if dt else None, dst.ptr if dst else None, dr.ptr, dsr.ptr,
                                                   rng.ptr if rng else None, None))
        t = (dt.download(np.int8, rows), dst.download(np.float32, rows // 64)) if want_t else (None, None)
        return t[0], t[1], dr.download(np.int8, rows), dsr.download(np.float32, rows // 64)

    def m8_iht(self, qPhi, sPhi, qPhiT, sPhiT, m, n, qy, sy, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
               rng: DevBuf | None = None, prefill: int = 0x55):
        """clm8_iht on buffers prefilled with `prefill` bytes -- or, with qPhiT None, clm8_iht_one_matrix:
        {"x": (q, s), "t1": ..., "t2": ..., "t3": ...}"""
        b = [self.to_device(v) for v in ((qPhi, sPhi, qy, sy) if qPhiT is None else (qPhi, sPhi, qy, sy, qPhiT, sPhiT))]
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {}
        for name, ln in lens.items():
            v[name] = (self.alloc(ln), self.alloc(ln // 16))
            for d in v[name]:
                self.check(self.lib.clv_memset(d.ptr, prefill, d.nbytes, None))
        tail = (v["x"][0].ptr, v["x"][1].ptr, n if x_len is None else x_len, b[2].ptr, b[3].ptr, v["t1"][0].ptr, v["t1"][1].ptr, v["t2"][0].ptr,
                v["t2"][1].ptr, v["t3"][0].ptr, v["t3"][1].ptr, iterations, K, mu, threshold, rng.ptr if rng else None, None)
        if qPhiT is None:
            self.check(self.lib.clm8_iht_one_matrix(b[0].ptr, b[1].ptr, m, n, *tail))
        else:
            self.check(self.lib.clm8_iht(b[0].ptr, b[1].ptr, b[4].ptr, b[5].ptr, m, n, *tail))
        return {name: (v[name][0].download(np.int8, ln), v[name][1].download(np.float32, ln // 64)) for name, ln in lens.items()}

    def m8_mvm_transposed(self, qA, sA, rows, cols, qx, sx, rng: DevBuf | None = None):
        """(r, sr) of clm8_mvm_transposed: A is rows x cols, x has rows int8, r has cols.  qA may be a DevBuf (a matrix uploaded once)"""
        dA, dsA = (qA, sA) if isinstance(qA, DevBuf) else (self.to_device(qA), self.to_device(sA))
        dx, dsx = self.to_device(qx), self.to_device(sx)
        dr, dsr = self.alloc(max(cols, 1)), self.alloc(max(cols // 16, 4))
        self.check(self.lib.clm8_mvm_transposed(dA.ptr, dsA.ptr, rows, cols, dx.ptr, dsx.ptr, dr.ptr, dsr.ptr, rng.ptr if rng else None, None))
        return dr.download(np.int8, cols), dsr.download(np.float32, cols // 64)

    def m8_mvm_transposed_scale_and_add(self, qA, sA, rows, cols, qx, sx, qu, su, a: float, rng: DevBuf | None = None, in_place: bool = False,
                                        want_t: bool = True):
        """(t, st, r, sr) of clm8_mvm_transposed_scale_and_add (u, t, r: cols int8); t/st are None when want_t is False"""
        dA, dsA = (qA, sA) if isinstance(qA, DevBuf) else (self.to_device(qA), self.to_device(sA))
        b = [self.to_device(v) for v in (qx, sx, qu, su)]
        dt, dst = (self.alloc(cols), self.alloc(cols // 16)) if want_t else (None, None)
        dr, dsr = (b[2], b[3]) if in_place else (self.alloc(cols), self.alloc(cols // 16))
        self.check(self.lib.clm8_mvm_transposed_scale_and_add(dA.ptr, dsA.ptr, rows, cols, b[0].ptr, b[1].ptr, b[2].ptr, b[3].ptr, a,
                                                              dt.ptr if dt else None, dst.ptr if dst else None, dr.ptr, dsr.ptr,
                                                              rng.ptr if rng else None, None))
        t = (dt.download(np.int8, cols), dst.download(np.float32, cols // 64)) if want_t else (None, None)
        return t[0], t[1], dr.download(np.int8, cols), dsr.download(np.float32, cols // 64)

    def m8_mvm_f32(self, qA, sA, rows, cols, x) -> np.ndarray:
        b = [self.to_device(a) for a in (qA, sA, np.ascontiguousarray(x, dtype=np.float32))]
        d = self.alloc(max(rows * 4, 4))
        self.check(self.lib.clm8_mvm_f32(b[0].ptr, b[1].ptr, rows, cols, b[2].ptr, d.ptr, None))
        return d.download(np.float32, rows)

    # CloverMatrix8 on fp32 vectors (include/clover_hip_m8_f32.h), shaped like their m4_ neighbours: the matrix pair and every vector a numpy
    # array or a DevBuf
    def m8_mvm_f32_scale_and_add(self, qA, sA, rows, cols, x, u, a: float, in_place: bool = False, want_t: bool = True):
        """(t, r2) of clm8_mvm_f32_scale_and_add, `rows` values each; t is None when want_t is False"""
        return self._m4_f32_fused(self.lib.clm8_mvm_f32_scale_and_add, qA, sA, rows, cols, rows, x, u, a, in_place, want_t)

    def m8_mvm_f32_transposed(self, qA, sA, rows, cols, x) -> np.ndarray:
        (dq, ds), dx, dr = self._m4_dev(qA, sA), self._f32_dev(x), self.alloc(max(4 * cols, 4))
        self.check(self.lib.clm8_mvm_f32_transposed(dq.ptr, ds.ptr, rows, cols, dx.ptr, dr.ptr, None))
        return dr.download(np.float32, cols)

    def m8_mvm_f32_transposed_scale_and_add(self, qA, sA, rows, cols, x, u, a: float, in_place: bool = False, want_t: bool = True):
        """(t, r2) of clm8_mvm_f32_transposed_scale_and_add, `cols` values each; t is None when want_t is False"""
        return self._m4_f32_fused(self.lib.clm8_mvm_f32_transposed_scale_and_add, qA, sA, rows, cols, cols, x, u, a, in_place, want_t)

    def m8_iht_f32(self, qPhi, sPhi, qPhiT, sPhiT, m, n, y, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
                   prefill: int = 0x55):
        """clm8_iht_f32 (qPhiT None: clm8_iht_f32_one_matrix) on buffers prefilled with `prefill` bytes:
        {"x": fp32[n], "t1": fp32[m], "t2": fp32[m], "t3": fp32[n]}"""
        return self._q_iht_f32(self.lib.clm8_iht_f32, self.lib.clm8_iht_f32_one_matrix, qPhi, sPhi, qPhiT, sPhiT, m, n, y, iterations, K, mu,
                               threshold, x_len, prefill)

    def m8_iht_f32_one_matrix(self, qPhi, sPhi, m, n, y, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
                              prefill: int = 0x55):
        return self.m8_iht_f32(qPhi, sPhi, None, None, m, n, y, iterations, K, mu, threshold, x_len=x_len, prefill=prefill)

    def m8_transpose(self, q, s, rows, cols):
        dq, ds = self.to_device(q), self.to_device(s)
        dt, dst = self.alloc(max(rows * cols, 1)), self.alloc(max((rows // 64) * (cols // 64) * 4, 4))
        self.check(self.lib.clm8_transpose(dq.ptr, ds.ptr, rows, cols, dt.ptr, dst.ptr, None))
        return dt.download(np.int8, rows * cols), dst.download(np.float32, (rows // 64) * (cols // 64))

    # -- CloverVector16 / CloverMatrix16 (raw binary16 bit patterns as uint16) ---------------------
    def f16_quantize(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        dx, dh = self.to_device(x), self.alloc(max(2 * x.size, 2))
        self.check(self.lib.clv_f16_quantize(dx.ptr, x.size, dh.ptr, None))
        return dh.download(np.uint16, x.size)

    def f16_restore(self, h: np.ndarray) -> np.ndarray:
        dh, dx = self.to_device(h), self.alloc(max(4 * h.size, 4))
        self.check(self.lib.clv_f16_restore(dh.ptr, h.size, dx.ptr, None))
        return dx.download(np.float32, h.size)

    def f16_scale_and_add(self, u, v, a: float, in_place: bool = False) -> np.ndarray:
        du, dv = self.to_device(u), self.to_device(v)
        dr = du if in_place else self.alloc(max(2 * u.size, 2))
        self.check(self.lib.clv_f16_scale_and_add(du.ptr, dv.ptr, a, u.size, dr.ptr, None))
        return dr.download(np.uint16, u.size)

    def f16_dot(self, u, v, mode: int = DOT_EXACT) -> np.float32:
        du, dv, out = self.to_device(u), self.to_device(v), self.alloc(4)
        self.check(self.lib.clv_f16_dot(du.ptr, dv.ptr, u.size, mode, out.ptr, None, None))
        return out.download(np.float32, 1)[0]

    def f16_threshold(self, h, n: int, k: int, mode: int = THRESHOLD_FAST) -> np.ndarray:
        dh = self.to_device(h)
        self.check(self.lib.clv_f16_threshold_mode(dh.ptr, n, h.size, k, mode, None, None))
        return dh.download(np.uint16, h.size)

    def f16_threshold_heap(self, h, n: int, k: int):
        """(thresholded vector, heap values fp32[k], heap indices uint32[k]) of clv_f16_threshold_heap"""
        dh, dheap = self.to_device(h), self.alloc(8 * k)
        self.check(self.lib.clv_f16_threshold_heap(dh.ptr, n, h.size, k, dheap.ptr, None, None))
        heap = dheap.download(np.uint32, 2 * k).reshape(k, 2)
        return dh.download(np.uint16, h.size), heap[:, 0].copy().view(np.float32), heap[:, 1].copy()

    def mf16_quantize(self, A: np.ndarray) -> np.ndarray:
        A = np.ascontiguousarray(A, dtype=np.float32)
        rows, cols = A.shape
        dA, dh = self.to_device(A), self.alloc(max(2 * rows * cols, 2))
        self.check(self.lib.clm_f16_quantize(dA.ptr, rows, cols, dh.ptr, None))
        return dh.download(np.uint16, rows * cols)

    def mf16_mvm(self, hA, rows, cols, hx) -> np.ndarray:
        dA, dx, dr = self.to_device(hA), self.to_device(hx), self.alloc(max(2 * rows, 2))
        self.check(self.lib.clm_f16_mvm(dA.ptr, rows, cols, dx.ptr, dr.ptr, None))
        return dr.download(np.uint16, rows)

    def mf16_mvm_f32(self, hA, rows, cols, x) -> np.ndarray:
        dA, dx, dr = self.to_device(hA), self.to_device(np.ascontiguousarray(x, dtype=np.float32)), self.alloc(max(4 * rows, 4))
        self.check(self.lib.clm_f16_mvm_f32(dA.ptr, rows, cols, dx.ptr, dr.ptr, None))
        return dr.download(np.float32, rows)

    def mf16_mvm_scale_and_add(self, hA, rows, cols, hx, hu, a: float, in_place: bool = False, want_t: bool = True):
        """(t, r) of clm_f16_mvm_scale_and_add; t is None when want_t is False.  hA may be a DevBuf (a matrix uploaded once)"""
        dA = hA if isinstance(hA, DevBuf) else self.to_device(hA)
        dx, du = self.to_device(hx), self.to_device(hu)
        dt = self.alloc(max(2 * rows, 2)) if want_t else None
        dr = du if in_place else self.alloc(max(2 * rows, 2))
        self.check(self.lib.clm_f16_mvm_scale_and_add(dA.ptr, rows, cols, dx.ptr, du.ptr, a, dt.ptr if dt else None, dr.ptr, None))
        return (dt.download(np.uint16, rows) if want_t else None), dr.download(np.uint16, rows)

    def mf16_iht(self, hPhi, hPhiT, m, n, hy, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None, prefill: int = 0x55):
        """clm_f16_iht on buffers prefilled with `prefill` bytes: {"x": bits, "t1": ..., "t2": ..., "t3": ...}"""
        b = [self.to_device(v) for v in (hPhi, hPhiT, hy)]
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {}
        for name, ln in lens.items():
            v[name] = self.alloc(2 * ln)
            self.check(self.lib.clv_memset(v[name].ptr, prefill, v[name].nbytes, None))
        self.check(self.lib.clm_f16_iht(b[0].ptr, b[1].ptr, m, n, v["x"].ptr, n if x_len is None else x_len, b[2].ptr, v["t1"].ptr, v["t2"].ptr,
                                        v["t3"].ptr, iterations, K, mu, threshold, None))
        return {name: v[name].download(np.uint16, ln) for name, ln in lens.items()}

    # A' x straight from A (clover_hip_f16_t.h): x has `rows` elements, the results `cols`.  hA may be a DevBuf (a matrix uploaded once)
    def mf16_mvm_transposed(self, hA, rows, cols, hx) -> np.ndarray:
        dA = hA if isinstance(hA, DevBuf) else self.to_device(hA)
        dx, dr = self.to_device(hx), self.alloc(max(2 * cols, 2))
        self.check(self.lib.clm_f16_mvm_transposed(dA.ptr, rows, cols, dx.ptr, dr.ptr, None))
        return dr.download(np.uint16, cols)

    def mf16_mvm_f32_transposed(self, hA, rows, cols, x) -> np.ndarray:
        dA = hA if isinstance(hA, DevBuf) else self.to_device(hA)
        dx, dr = self.to_device(np.ascontiguousarray(x, dtype=np.float32)), self.alloc(max(4 * cols, 4))
        self.check(self.lib.clm_f16_mvm_f32_transposed(dA.ptr, rows, cols, dx.ptr, dr.ptr, None))
        return dr.download(np.float32, cols)

    def mf16_mvm_transposed_scale_and_add(self, hA, rows, cols, hx, hu, a: float, in_place: bool = False, want_t: bool = True):
        """(t, r) of clm_f16_mvm_transposed_scale_and_add; t is None when want_t is False"""
        dA = hA if isinstance(hA, DevBuf) else self.to_device(hA)
        dx, du = self.to_device(hx), self.to_device(hu)
        dt = self.alloc(max(2 * cols, 2)) if want_t else None
        dr = du if in_place else self.alloc(max(2 * cols, 2))
        self.check(self.lib.clm_f16_mvm_transposed_scale_and_add(dA.ptr, rows, cols, dx.ptr, du.ptr, a, dt.ptr if dt else None, dr.ptr, None))
        return (dt.download(np.uint16, cols) if want_t else None), dr.download(np.uint16, cols)

    def mf16_iht_one_matrix(self, hPhi, m, n, hy, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None, prefill: int = 0x55):
        """clm_f16_iht_one_matrix on buffers prefilled with `prefill` bytes: {"x": bits, "t1": ..., "t2": ..., "t3": ...}"""
        dPhi = hPhi if isinstance(hPhi, DevBuf) else self.to_device(hPhi)
        dy = self.to_device(hy)
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {}
        for name, ln in lens.items():
            v[name] = self.alloc(2 * ln)
            self.check(self.lib.clv_memset(v[name].ptr, prefill, v[name].nbytes, None))
        self.check(self.lib.clm_f16_iht_one_matrix(dPhi.ptr, m, n, v["x"].ptr, n if x_len is None else x_len, dy.ptr, v["t1"].ptr, v["t2"].ptr,
                                                   v["t3"].ptr, iterations, K, mu, threshold, None))
        return {name: v[name].download(np.uint16, ln) for name, ln in lens.items()}

    # several CloverVector16 with one CloverMatrix16 (clover_hip_batch_f16.h; host arrays of device pointers; lists in, lists out)
    def mf16_mvm_batch(self, hA, rows, cols, hxs):
        """hxs: list of x bit patterns; returns the list of r of clm_f16_mvm_batch.  hA may be a DevBuf (a matrix uploaded once)"""
        dA = hA if isinstance(hA, DevBuf) else self.to_device(hA)
        dx = [self.to_device(h) for h in hxs]
        dr = [self.alloc(max(2 * rows, 2)) for _ in hxs]
        pa = self.ptr_array
        self.check(self.lib.clm_f16_mvm_batch(dA.ptr, rows, cols, len(hxs), pa(dx), pa(dr), None))
        return [r.download(np.uint16, rows) for r in dr]

    def mf16_mvm_scale_and_add_batch(self, hA, rows, cols, hxs, hus, a: float, in_place: bool = False, want_t: bool = True):
        """hxs, hus: lists of bit patterns; returns the list of (t, r) of clm_f16_mvm_scale_and_add_batch; t is None when want_t is False"""
        dA = hA if isinstance(hA, DevBuf) else self.to_device(hA)
        dx, du = [self.to_device(h) for h in hxs], [self.to_device(h) for h in hus]
        dt = [self.alloc(max(2 * rows, 2)) for _ in hxs] if want_t else None
        dr = du if in_place else [self.alloc(max(2 * rows, 2)) for _ in hxs]
        pa = self.ptr_array
        self.check(self.lib.clm_f16_mvm_scale_and_add_batch(dA.ptr, rows, cols, len(hxs), pa(dx), pa(du), a, pa(dt), pa(dr), None))
        return [((dt[j].download(np.uint16, rows) if want_t else None), dr[j].download(np.uint16, rows)) for j in range(len(hxs))]

    def f16_threshold_batch(self, hs, n: int, k: int, mode: int = THRESHOLD_FAST):
        """hs: list of vectors of one padded size; returns the list of thresholded vectors of clv_f16_threshold_batch"""
        dh = [self.to_device(h) for h in hs]
        self.check(self.lib.clv_f16_threshold_batch(self.ptr_array(dh), len(hs), n, hs[0].size if hs else 0, k, mode, None))
        return [d.download(np.uint16, h.size) for d, h in zip(dh, hs)]

    def mf16_iht_batch(self, hPhi, hPhiT, m, n, hys, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
                       prefill: int = 0x55):
        """clm_f16_iht_batch on buffers prefilled with `prefill` bytes; hys: list of y bit patterns; returns per signal
        {"x": bits, "t1": ..., "t2": ..., "t3": ...}.  hPhi / hPhiT may be DevBufs"""
        dPhi, dPhiT = [h if isinstance(h, DevBuf) else self.to_device(h) for h in (hPhi, hPhiT)]
        dy = [self.to_device(h) for h in hys]
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {name: [self.alloc(max(2 * ln, 2)) for _ in hys] for name, ln in lens.items()}
        for bufs in v.values():
            for d in bufs:
                self.check(self.lib.clv_memset(d.ptr, prefill, d.nbytes, None))
        pa = self.ptr_array
        self.check(self.lib.clm_f16_iht_batch(dPhi.ptr, dPhiT.ptr, m, n, len(hys), pa(v["x"]), n if x_len is None else x_len, pa(dy), pa(v["t1"]),
                                              pa(v["t2"]), pa(v["t3"]), iterations, K, mu, threshold, None))
        return [{name: v[name][j].download(np.uint16, ln) for name, ln in lens.items()} for j in range(len(hys))]

    # A' x[j] for several CloverVector16 straight from A (clover_hip_batch_f16_t.h): every x has `rows` elements, the results `cols`
    def mf16_mvm_transposed_batch(self, hA, rows, cols, hxs, prefill: int = 0xEE):
        """hxs: list of x bit patterns; returns the list of r of clm_f16_mvm_transposed_batch.  hA may be a DevBuf (a matrix uploaded once)"""
        dA = hA if isinstance(hA, DevBuf) else self.to_device(hA)
        dx = [self.to_device(h) for h in hxs]
        dr = [self.alloc(max(2 * cols, 2)) for _ in hxs]
        for d in dr:
            self.check(self.lib.clv_memset(d.ptr, prefill, d.nbytes, None))
        pa = self.ptr_array
        self.check(self.lib.clm_f16_mvm_transposed_batch(dA.ptr, rows, cols, len(hxs), pa(dx), pa(dr), None))
        return [r.download(np.uint16, cols) for r in dr]

    def mf16_mvm_transposed_scale_and_add_batch(self, hA, rows, cols, hxs, hus, a: float, in_place: bool = False, want_t: bool = True,
                                                prefill: int = 0xEE):
        """hxs, hus: lists of bit patterns; returns the list of (t, r) of clm_f16_mvm_transposed_scale_and_add_batch.  t is always
        allocated and prefilled; with want_t False the call is given no t array and the (untouched) buffer is returned all the same"""
        dA = hA if isinstance(hA, DevBuf) else self.to_device(hA)
        dx, du = [self.to_device(h) for h in hxs], [self.to_device(h) for h in hus]
        dt = [self.alloc(max(2 * cols, 2)) for _ in hxs]
        dr = du if in_place else [self.alloc(max(2 * cols, 2)) for _ in hxs]
        for d in dt + ([] if in_place else dr):
            self.check(self.lib.clv_memset(d.ptr, prefill, d.nbytes, None))
        pa = self.ptr_array
        self.check(self.lib.clm_f16_mvm_transposed_scale_and_add_batch(dA.ptr, rows, cols, len(hxs), pa(dx), pa(du), a, pa(dt) if want_t else None,
                                                                       pa(dr), None))
        return [(dt[j].download(np.uint16, cols), dr[j].download(np.uint16, cols)) for j in range(len(hxs))]

    def mf16_iht_batch_one_matrix(self, hPhi, m, n, hys, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None,
                                  prefill: int = 0x55):
        """clm_f16_iht_batch_one_matrix on buffers prefilled with `prefill` bytes; hys: list of y bit patterns; returns per signal
        {"x": bits, "t1": ..., "t2": ..., "t3": ...}.  hPhi may be a DevBuf"""
        dPhi = hPhi if isinstance(hPhi, DevBuf) else self.to_device(hPhi)
        dy = [self.to_device(h) for h in hys]
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {name: [self.alloc(max(2 * ln, 2)) for _ in hys] for name, ln in lens.items()}
        for bufs in v.values():
            for d in bufs:
                self.check(self.lib.clv_memset(d.ptr, prefill, d.nbytes, None))
        pa = self.ptr_array
        self.check(self.lib.clm_f16_iht_batch_one_matrix(dPhi.ptr, m, n, len(hys), pa(v["x"]), n if x_len is None else x_len, pa(dy), pa(v["t1"]),
                                                         pa(v["t2"]), pa(v["t3"]), iterations, K, mu, threshold, None))
        return [{name: v[name][j].download(np.uint16, ln) for name, ln in lens.items()} for j in range(len(hys))]

    def mf16_transpose(self, h, rows, cols) -> np.ndarray:
        dh, dt = self.to_device(h), self.alloc(max(2 * rows * cols, 2))
        self.check(self.lib.clm_f16_transpose(dh.ptr, rows, cols, dt.ptr, None))
        return dt.download(np.uint16, rows * cols)

    # -- CloverVector32 / CloverMatrix32 (plain fp32; every operand a numpy array or a DevBuf, so that a matrix is uploaded once) ----
    def _f32_dev(self, a) -> DevBuf:
        return a if isinstance(a, DevBuf) else self.to_device(np.ascontiguousarray(a, dtype=np.float32))

    def f32_scale_and_add(self, u, v, a: float, n_pad: int | None = None, in_place: bool = False) -> np.ndarray:
        du, dv = self._f32_dev(u), self._f32_dev(v)
        n = du.nbytes // 4 if n_pad is None else n_pad
        dr = du if in_place else self.alloc(max(4 * n, 4))
        self.check(self.lib.clv_f32_scale_and_add(du.ptr, dv.ptr, a, n, dr.ptr, None))
        return dr.download(np.float32, n)

    def f32_dot(self, u, v, mode: int = DOT_EXACT, n_pad: int | None = None) -> np.float32:
        du, dv, out = self._f32_dev(u), self._f32_dev(v), self.alloc(4)
        self.check(self.lib.clv_f32_dot(du.ptr, dv.ptr, du.nbytes // 4 if n_pad is None else n_pad, mode, out.ptr, None, None))
        return out.download(np.float32, 1)[0]

    def f32_threshold(self, x, n: int, k: int, mode: int = THRESHOLD_FAST, n_pad: int | None = None) -> np.ndarray:
        """thresholds in place: a DevBuf given as x holds the result afterwards"""
        dx = self._f32_dev(x)
        n_pad = dx.nbytes // 4 if n_pad is None else n_pad
        self.check(self.lib.clv_f32_threshold_mode(dx.ptr, n, n_pad, k, mode, None, None))
        return dx.download(np.float32, n_pad)

    def f32_mvm(self, A, rows, cols, x) -> np.ndarray:
        dA, dx, dr = self._f32_dev(A), self._f32_dev(x), self.alloc(max(4 * rows, 4))
        self.check(self.lib.clm_f32_mvm(dA.ptr, rows, cols, dx.ptr, dr.ptr, None))
        return dr.download(np.float32, rows)

    def f32_mvm_scale_and_add(self, A, rows, cols, x, u, a: float, in_place: bool = False, want_t: bool = True):
        """(t, r2) of clm_f32_mvm_scale_and_add; t is None when want_t is False"""
        dA, dx, du = self._f32_dev(A), self._f32_dev(x), self._f32_dev(u)
        dt = self.alloc(max(4 * rows, 4)) if want_t else None
        dr = du if in_place else self.alloc(max(4 * rows, 4))
        self.check(self.lib.clm_f32_mvm_scale_and_add(dA.ptr, rows, cols, dx.ptr, du.ptr, a, dt.ptr if dt else None, dr.ptr, None))
        return (dt.download(np.float32, rows) if want_t else None), dr.download(np.float32, rows)

    def f32_transpose(self, A, rows, cols) -> np.ndarray:
        dA, dt = self._f32_dev(A), self.alloc(max(4 * rows * cols, 4))
        self.check(self.lib.clm_f32_transpose(dA.ptr, rows, cols, dt.ptr, None))
        return dt.download(np.float32, rows * cols)

    def f32_iht(self, Phi, PhiT, m, n, y, iterations: int, K: int, mu: float, threshold: int, x_len: int | None = None, prefill: int = 0x55):
        """clm_f32_iht on buffers prefilled with `prefill` bytes: {"x": fp32[n], "t1": fp32[m], "t2": fp32[m], "t3": fp32[n]}"""
        b = [self._f32_dev(v) for v in (Phi, PhiT, y)]
        lens = {"x": n, "t1": m, "t2": m, "t3": n}
        v = {}
        for name, ln in lens.items():
            v[name] = self.alloc(4 * ln)
            self.check(self.lib.clv_memset(v[name].ptr, prefill, v[name].nbytes, None))
        self.check(self.lib.clm_f32_iht(b[0].ptr, b[1].ptr, m, n, v["x"].ptr, n if x_len is None else x_len, b[2].ptr, v["t1"].ptr, v["t2"].ptr,
                                        v["t3"].ptr, iterations, K, mu, threshold, None))
        return {name: v[name].download(np.float32, ln) for name, ln in lens.items()}

    def m4_gemm_i32(self, qA, M, K, qB, N, kb_begin=0, kb_count=None) -> np.ndarray:
        b = [self.to_device(a) for a in (qA, qB)]
        c = self.alloc(max(M * N * 4, 4))
        self.check(self.lib.clm4_gemm_i32(b[0].ptr, M, K, b[1].ptr, N, kb_begin, K // 64 - kb_begin if kb_count is None else kb_count, c.ptr, None))
        return c.download(np.int32, M * N).reshape(M, N)

    def m4_gemm_i32_prepared(self, qA, M, K, qB, N, kb_begin=0, kb_count=None, prepare=("A", "B")) -> np.ndarray:
        b = [self.to_device(a) for a in (qA, qB)]
        c = self.alloc(max(M * N * 4, 4))
        ops = {"A": C.c_void_p(), "B": C.c_void_p()}
        if "A" in prepare:
            self.check(self.lib.clm4_gemm_prepare(b[0].ptr, M, K, C.byref(ops["A"]), None))
        if "B" in prepare:
            self.check(self.lib.clm4_gemm_prepare(b[1].ptr, N, K, C.byref(ops["B"]), None))
        try:
            self.check(self.lib.clm4_gemm_i32_prepared(ops["A"], None if "A" in prepare else b[0].ptr, M, K, ops["B"], None if "B" in prepare else b[1].ptr, N,
                                                       kb_begin, K // 64 - kb_begin if kb_count is None else kb_count, c.ptr, None))
            return c.download(np.int32, M * N).reshape(M, N)
        finally:
            for o in ops.values():
                self.check(self.lib.clm4_gemm_release(o))

    def m4_gemm_prepared(self, qA, sA, M, K, qB, sB, N, prepare=("A", "B")) -> np.ndarray:
        b = [self.to_device(a) for a in (qA, sA, qB, sB)]
        c = self.alloc(max(M * N * 4, 4))
        ops = {"A": C.c_void_p(), "B": C.c_void_p()}
        if "A" in prepare:
            self.check(self.lib.clm4_gemm_prepare(b[0].ptr, M, K, C.byref(ops["A"]), None))
        if "B" in prepare:
            self.check(self.lib.clm4_gemm_prepare(b[2].ptr, N, K, C.byref(ops["B"]), None))
        try:
            for _ in range(2):          # the second call re-uses the images
                self.check(self.lib.clv_memset(c.ptr, 0xFF, c.nbytes, None))
                self.check(self.lib.clm4_gemm_prepared(ops["A"], None if "A" in prepare else b[0].ptr, b[1].ptr, M, K,
                                                       ops["B"], None if "B" in prepare else b[2].ptr, b[3].ptr, N, c.ptr, None))
            return c.download(np.float32, M * N).reshape(M, N)
        finally:
            for o in ops.values():
                self.check(self.lib.clm4_gemm_release(o))

    def m4_gemm(self, qA, sA, M, K, qB, sB, N) -> np.ndarray:
        b = [self.to_device(a) for a in (qA, sA, qB, sB)]
        c = self.alloc(max(M * N * 4, 4))
        self.check(self.lib.clm4_gemm(b[0].ptr, b[1].ptr, M, K, b[2].ptr, b[3].ptr, N, c.ptr, None))
        return c.download(np.float32, M * N).reshape(M, N)

    # -- GEMM with 8-bit operands (int8 matrix cores) ------------------------------------------------
    def m8_gemm(self, qA, sA, M, K, qB, sB, N) -> np.ndarray:
        b = [self.to_device(a) for a in (qA, sA, qB, sB)]
        c = self.alloc(max(M * N * 4, 4))
        self.check(self.lib.clm8_gemm(b[0].ptr, b[1].ptr, M, K, b[2].ptr, b[3].ptr, N, c.ptr, None))
        return c.download(np.float32, M * N).reshape(M, N)

    def m8_gemm_i32(self, qA, M, K, qB, N, kb_begin=0, kb_count=None) -> np.ndarray:
        b = [self.to_device(a) for a in (qA, qB)]
        c = self.alloc(max(M * N * 4, 4))
        self.check(self.lib.clm8_gemm_i32(b[0].ptr, M, K, b[1].ptr, N, kb_begin, K // 64 - kb_begin if kb_count is None else kb_count, c.ptr, None))
        return c.download(np.int32, M * N).reshape(M, N)

    def m4_gemm_m8(self, qA4, sA, M, K, qB8, sB, N) -> np.ndarray:
        """A: CloverMatrix4 image (packed nibbles), B: CloverMatrix8 image"""
        b = [self.to_device(a) for a in (qA4, sA, qB8, sB)]
        c = self.alloc(max(M * N * 4, 4))
        self.check(self.lib.clm4_gemm_m8(b[0].ptr, b[1].ptr, M, K, b[2].ptr, b[3].ptr, N, c.ptr, None))
        return c.download(np.float32, M * N).reshape(M, N)
