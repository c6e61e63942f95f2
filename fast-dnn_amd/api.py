"""Python mirror of ``suskun.nn.QuantizedDnn`` over the C-ABI of libfast-dnn.so.

Same names, argument meaning and error behaviour as the Java facade
(src/java/suskun/nn/QuantizedDnn.java), so tests read like the reference's own
FuncTest / MultiThreadedStressTest.  This module is a binding only: every
computation happens in the HIP library; there is no fallback, and importing
works without a GPU only so that host-side helpers and symbol checks can run.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FDNN_LIB") or os.path.join(_HERE, "lib", "libfast-dnn.so")  # FDNN_LIB: experiment builds
CSRC = os.path.join(_HERE, "csrc")

FDNN_OK, FDNN_E_ARG, FDNN_E_IO, FDNN_E_FORMAT, FDNN_E_DEVICE, FDNN_E_NOMEM, FDNN_E_STATE = 0, -1, -2, -3, -4, -5, -6


class FdnnError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"fdnn error {code}: {msg}")
        self.code = code


def build(verbose: bool = False) -> str:
    """Compile libfast-dnn.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    jobs = str(max(1, min(8, os.cpu_count() or 1)))  # the three kernel files take a minute each: compile them side by side
    subprocess.check_call(["make", "-C", CSRC, "-j", jobs, "all"] + ([] if verbose else ["-s"]))
    return LIB_PATH


_lib = None

_c_f32p = C.POINTER(C.c_float)
_c_i8p = C.POINTER(C.c_int8)
_c_u8p = C.POINTER(C.c_uint8)
_c_i32p = C.POINTER(C.c_int32)

# name -> (restype, argtypes); also the list of exported C-ABI symbols that
# include/fdnn.h declares (tests check both directions)
SIGNATURES = {
    "fdnn_last_error": (C.c_char_p, []),
    "fdnn_version": (C.c_char_p, []),
    "fdnn_device_count": (C.c_int, []),
    "fdnn_model_load": (C.c_int, [C.c_char_p, C.c_float, C.POINTER(C.c_void_p)]),
    "fdnn_model_load_on": (C.c_int, [C.c_char_p, C.c_float, C.c_int, C.POINTER(C.c_void_p)]),
    "fdnn_model_free": (None, [C.c_void_p]),
    "fdnn_model_input_dim": (C.c_int, [C.c_void_p]),
    "fdnn_model_output_dim": (C.c_int, [C.c_void_p]),
    "fdnn_model_hidden_dim": (C.c_int, [C.c_void_p]),
    "fdnn_model_layer_count": (C.c_int, [C.c_void_p]),
    "fdnn_model_layer_dim": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_model_device": (C.c_int, [C.c_void_p]),
    "fdnn_model_set_l0_fma": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_debug_set_l0_kernel": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_debug_set_chain": (C.c_int, [C.c_int, C.c_int]),
    "fdnn_model_chain_faults": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "fdnn_debug_set_pp": (C.c_int, [C.c_int, C.c_int]),
    "fdnn_debug_set_ppo": (C.c_int, [C.c_int]),
    "fdnn_debug_launch_name_count": (C.c_int, []),
    "fdnn_debug_launch_name": (C.c_char_p, [C.c_int, C.POINTER(C.c_int)]),
    "fdnn_debug_launch_record": (C.c_int, [C.c_int]),
    "fdnn_debug_launch_reset": (C.c_int, []),
    "fdnn_debug_launch_counts": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_raise_fuse_fault": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_device_shared": (C.c_int, [C.c_int]),
    "fdnn_debug_set_fuse": (C.c_int, [C.c_int]),
    "fdnn_debug_set_l0_list_cap": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_debug_chain_clocks": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong), C.c_int]),
    "fdnn_calculate": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_int, _c_f32p]),
    "fdnn_calculate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_lazy": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_i8p, _c_f32p]),
    "fdnn_calculate_lazy_bits": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.POINTER(C.c_uint64), _c_f32p]),
    "fdnn_calculate_lazy_bits_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_ctx_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "fdnn_ctx_free": (None, [C.c_void_p]),
    "fdnn_ctx_frame_count": (C.c_int, [C.c_void_p]),
    "fdnn_ctx_output_dim": (C.c_int, [C.c_void_p]),
    "fdnn_ctx_forward_hidden": (C.c_int, [C.c_void_p, _c_f32p]),
    "fdnn_ctx_forward_hidden_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_ctx_lazy_output": (C.c_int, [C.c_void_p, C.c_int, _c_i8p, _c_f32p]),
    "fdnn_ctx_lazy_output_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _c_i8p, _c_f32p]),
    "fdnn_ctx_lazy_output_batch_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_ctx_output": (C.c_int, [C.c_void_p, _c_f32p]),
    "fdnn_ctx_output_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_ctx_read_hidden": (C.c_int, [C.c_void_p, _c_u8p]),
    "fdnn_server_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "fdnn_server_free": (None, [C.c_void_p]),
    "fdnn_server_set_linger_us": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_server_submit_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "fdnn_server_submit": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, _c_i8p, _c_f32p, C.POINTER(C.c_uint64)]),
    "fdnn_server_submit_lazy_bits": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_void_p, _c_f32p, C.POINTER(C.c_uint64)]),
    "fdnn_debug_lazy_expand": (C.c_int, [_c_f32p, _c_f32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "fdnn_server_wait": (C.c_int, [C.c_void_p, C.c_uint64]),
    "fdnn_server_drain": (C.c_int, [C.c_void_p]),
    "fdnn_server_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fdnn_model_enable_batcher": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "fdnn_group_load": (C.c_int, [C.c_char_p, C.c_float, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "fdnn_group_free": (None, [C.c_void_p]),
    "fdnn_group_size": (C.c_int, [C.c_void_p]),
    "fdnn_group_model": (C.c_void_p, [C.c_void_p, C.c_int]),
    "fdnn_group_weight_transport": (C.c_char_p, [C.c_void_p]),
    "fdnn_group_worker_cpus": (C.c_char_p, [C.c_void_p, C.c_int]),
    "fdnn_group_calculate": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_int, _c_f32p]),
    "fdnn_group_shard": (None, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fdnn_group_attach": (C.c_int, [C.c_void_p]),
    "fdnn_model_blob_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "fdnn_model_export_blob": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fdnn_model_import_blob": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]),
    "fdnn_debug_frame_chunks": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_int]),
    "fdnn_debug_frame_chunks_for": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]),
    "fdnn_debug_production_acc_out": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_i8p, _c_i32p, _c_f32p]),
    "fdnn_debug_forward_taps": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, _c_i8p, _c_f32p, _c_u8p, _c_i32p, _c_i32p, _c_f32p, _c_f32p]),
    "fdnn_debug_layer0": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, _c_u8p, C.POINTER(C.c_ulonglong)]),
    "fdnn_debug_layer0_screen": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, _c_u8p, _c_f32p, _c_f32p, C.POINTER(C.c_ulonglong)]),
    "fdnn_ctx_lazy_output_batch_bits": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fdnn_ctx_lazy_output_batch_bits_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_ctx_lazy_output_lists": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _c_i32p, _c_i32p, _c_f32p, _c_f32p]),
    "fdnn_ctx_lazy_output_lists_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_lazy_lists": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_i32p, _c_i32p, _c_f32p, _c_f32p]),
    "fdnn_debug_lists_check": (C.c_int, [_c_i32p, _c_i32p, C.c_int, C.c_int]),
    "fdnn_debug_ctx_lists_acc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _c_i32p, _c_i32p, _c_i32p]),
    "fdnn_debug_lists_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_model_set_lists_union": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_debug_lists_union_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_ctx_lists_union": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_i32p]),
    "fdnn_debug_lists_union_ref": (C.c_int, [_c_i32p, _c_i32p, C.c_int, C.c_int, C.c_int, _c_i32p, _c_i32p, _c_i32p]),
    "fdnn_ctx_lazy_output_set": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _c_i32p, C.c_int, _c_f32p, _c_f32p]),
    "fdnn_ctx_lazy_output_set_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_lazy_set": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_i32p, C.c_int, _c_f32p, _c_f32p]),
    "fdnn_debug_set_check": (C.c_int, [_c_i32p, C.c_int, C.c_int]),
    "fdnn_debug_ctx_set_acc": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _c_i32p, C.c_int, _c_i32p]),
    "fdnn_debug_set_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_set_kernel": (C.c_int, [C.c_int]),
    "fdnn_ctx_lazy_output_sets": (C.c_int, [C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_f32p, _c_f32p]),
    "fdnn_ctx_lazy_output_sets_device": (C.c_int, [C.c_void_p, _c_i32p, _c_i32p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_lazy_sets": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_f32p, _c_f32p]),
    "fdnn_debug_sets_check": (C.c_int, [_c_i32p, _c_i32p, _c_i32p, C.c_int, C.c_int, C.c_int]),
    "fdnn_debug_ctx_sets_acc": (C.c_int, [C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p]),
    "fdnn_debug_sets_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_server_submit_lazy_set": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, _c_i32p, C.c_int, _c_f32p, _c_f32p, C.POINTER(C.c_uint64)]),
    "fdnn_server_submit_raw_set": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, _c_i32p, C.c_int, _c_f32p, _c_f32p, C.POINTER(C.c_uint64)]),
    "fdnn_topk_rows_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_ctx_output_topk": (C.c_int, [C.c_void_p, C.c_int, _c_i32p, _c_f32p]),
    "fdnn_ctx_output_topk_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_topk": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_int, _c_i32p, _c_f32p]),
    "fdnn_calculate_topk_raw": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_int, _c_i32p, _c_f32p]),
    "fdnn_calculate_topk_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_server_submit_topk": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_i32p, _c_f32p, C.POINTER(C.c_uint64)]),
    "fdnn_server_submit_raw_topk": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_i32p, _c_f32p, C.POINTER(C.c_uint64)]),
    "fdnn_debug_topk_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_set_topk_kernel": (C.c_int, [C.c_int]),
    "fdnn_debug_topk_ref": (C.c_int, [_c_f32p, C.c_int, C.c_int, C.c_int, _c_i32p, _c_f32p]),
    "fdnn_debug_topk_limits": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fdnn_pool_create": (C.c_void_p, [_c_i32p, C.c_int, C.c_int]),
    "fdnn_pool_free": (None, [C.c_void_p]),
    "fdnn_pool_width": (C.c_int, [C.c_void_p]),
    "fdnn_pool_classes": (C.c_int, [C.c_void_p]),
    "fdnn_pool_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fdnn_ctx_output_pool": (C.c_int, [C.c_void_p, C.c_void_p, _c_f32p]),
    "fdnn_ctx_output_pool_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_pool": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, _c_f32p]),
    "fdnn_calculate_pool_raw": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, _c_f32p]),
    "fdnn_calculate_pool_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_server_submit_pool": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_void_p, _c_f32p, C.POINTER(C.c_uint64)]),
    "fdnn_server_submit_raw_pool": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_void_p, _c_f32p, C.POINTER(C.c_uint64)]),
    "fdnn_debug_pool_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_set_pool_kernel": (C.c_int, [C.c_int]),
    "fdnn_debug_pool_ref": (C.c_int, [_c_f32p, C.c_int, _c_i32p, C.c_int, C.c_int, _c_f32p]),
    "fdnn_debug_pool_limits": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fdnn_loglik_create": (C.c_void_p, [_c_f32p, C.c_int, C.c_float, C.c_int]),
    "fdnn_loglik_free": (None, [C.c_void_p]),
    "fdnn_loglik_width": (C.c_int, [C.c_void_p]),
    "fdnn_loglik_type": (C.c_int, [C.c_void_p]),
    "fdnn_loglik_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fdnn_loglik_entries_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "fdnn_ctx_output_loglik": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_ctx_output_loglik_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_loglik": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_loglik_raw": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_loglik_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_server_submit_loglik": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "fdnn_server_submit_raw_loglik": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "fdnn_server_live_push_loglik": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                             C.POINTER(C.c_uint64)]),
    "fdnn_debug_loglik_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_set_loglik_kernel": (C.c_int, [C.c_int]),
    "fdnn_debug_loglik_ref": (C.c_int, [_c_f32p, C.c_int, _c_f32p, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "fdnn_debug_loglik_entries_ref": (C.c_int, [_c_i32p, _c_f32p, C.c_longlong, _c_f32p, C.c_int, C.c_float, C.c_int, C.c_void_p]),
    "fdnn_align_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, _c_i32p, C.POINTER(C.c_longlong), _c_i32p, _c_i32p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_align_scratch_words": (C.c_int, [_c_i32p, _c_i32p, C.c_int, C.POINTER(C.c_longlong)]),
    "fdnn_ctx_align": (C.c_int, [C.c_void_p, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_f32p, _c_f32p, _c_i32p, _c_f32p]),
    "fdnn_ctx_align_device": (C.c_int, [C.c_void_p, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_f32p, _c_f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_align": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_f32p, _c_f32p, _c_i32p,
                                       _c_f32p]),
    "fdnn_calculate_align_raw": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_f32p, _c_f32p,
                                           _c_i32p, _c_f32p]),
    "fdnn_debug_align_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_set_align_kernel": (C.c_int, [C.c_int]),
    "fdnn_debug_align_limits": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "fdnn_debug_align_ref": (C.c_int, [_c_f32p, _c_i32p, C.POINTER(C.c_longlong), _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_f32p, C.c_int, C.c_float,
                                       C.c_int, _c_f32p, _c_f32p, _c_i32p, _c_f32p]),
    "fdnn_debug_align_sets": (C.c_int, [_c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_i32p]),
    "fdnn_align_graph_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, _c_i32p, C.POINTER(C.c_longlong), _c_i32p, _c_i32p, _c_i32p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_align_graph_scratch_words": (C.c_int, [_c_i32p, _c_i32p, C.c_int, C.POINTER(C.c_longlong)]),
    "fdnn_ctx_align_graph": (C.c_int, [C.c_void_p, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_i32p, _c_f32p, _c_f32p, _c_f32p, _c_i32p,
                                       _c_f32p]),
    "fdnn_ctx_align_graph_device": (C.c_int, [C.c_void_p, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_i32p, _c_f32p, _c_f32p, _c_f32p,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_align_graph": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_i32p,
                                             _c_f32p, _c_f32p, _c_f32p, _c_i32p, _c_f32p]),
    "fdnn_calculate_align_graph_raw": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_i32p,
                                                 _c_f32p, _c_f32p, _c_f32p, _c_i32p, _c_f32p]),
    "fdnn_debug_align_graph_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_set_align_graph_kernel": (C.c_int, [C.c_int]),
    "fdnn_debug_align_graph_limits": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "fdnn_debug_align_graph_ref": (C.c_int, [_c_f32p, _c_i32p, C.POINTER(C.c_longlong), _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_f32p, C.c_int,
                                             C.c_float, C.c_int, _c_i32p, _c_i32p, _c_f32p, _c_f32p, _c_f32p, _c_i32p, _c_f32p]),
    "fdnn_fb_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, _c_i32p, C.POINTER(C.c_longlong), _c_i32p, _c_i32p, _c_i32p, _c_i32p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fdnn_fb_scratch_words": (C.c_int, [_c_i32p, _c_i32p, C.c_int, C.c_int, C.POINTER(C.c_longlong)]),
    "fdnn_fb_transpose": (C.c_int, [_c_i32p, C.c_int, _c_i32p, _c_i32p, _c_f32p, _c_i32p, _c_i32p, _c_f32p]),
    "fdnn_ctx_fb": (C.c_int, [C.c_void_p, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_i32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p]),
    "fdnn_ctx_fb_device": (C.c_int, [C.c_void_p, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_i32p, _c_f32p, _c_f32p, _c_f32p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "fdnn_calculate_fb": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_i32p, _c_f32p,
                                    _c_f32p, _c_f32p, _c_f32p, _c_f32p]),
    "fdnn_calculate_fb_raw": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_i32p, _c_f32p,
                                        _c_f32p, _c_f32p, _c_f32p, _c_f32p]),
    "fdnn_debug_fb_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_set_fb_kernel": (C.c_int, [C.c_int]),
    "fdnn_debug_fb_limits": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "fdnn_debug_fb_ref": (C.c_int, [_c_f32p, _c_i32p, C.POINTER(C.c_longlong), _c_i32p, _c_i32p, C.c_int, _c_i32p, _c_i32p, _c_f32p, C.c_int, C.c_float,
                                    C.c_int, _c_i32p, _c_i32p, _c_f32p, _c_f32p, _c_f32p, _c_i32p, _c_i32p, _c_f32p, _c_f32p, _c_f32p]),
    "fdnn_debug_fb_math_ref": (C.c_int, [C.c_int, _c_f32p, _c_f32p, _c_f32p, C.c_longlong]),
    "fdnn_debug_fb_math_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]),
    "fdnn_debug_ln_ref": (C.c_int, [_c_f32p, C.c_longlong, _c_f32p]),
    "fdnn_model_fuse_giveups": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "fdnn_debug_device_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_scratch_count": (C.c_int, []),
    "fdnn_debug_scratch_name": (C.c_char_p, [C.c_int]),
    "fdnn_debug_ctx_scratch": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_ctx_scratch_words": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_debug_ctx_scratch_poke": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_uint]),
    "fdnn_debug_scratch_audit": (C.c_int, [C.c_int]),
    "fdnn_debug_scratch_dirty": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_profile_begin": (C.c_int, [C.c_void_p]),
    "fdnn_profile_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "fdnn_model_set_splice": (C.c_int, [C.c_void_p, _c_i32p, C.c_int, C.c_int]),
    "fdnn_model_get_splice": (C.c_int, [C.c_void_p, _c_i32p, C.c_int, _c_i32p]),
    "fdnn_calculate_raw": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_f32p]),
    "fdnn_calculate_raw_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _c_i32p, C.c_int, C.c_void_p, C.c_void_p]),
    "fdnn_calculate_lazy_bits_raw": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, _c_f32p]),
    "fdnn_ctx_forward_hidden_raw": (C.c_int, [C.c_void_p, _c_f32p]),
    "fdnn_stream_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "fdnn_stream_free": (None, [C.c_void_p]),
    "fdnn_stream_reset": (C.c_int, [C.c_void_p]),
    "fdnn_stream_position": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "fdnn_stream_push": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_f32p, _c_i32p]),
    "fdnn_stream_ctx": (C.c_void_p, [C.c_void_p]),
    "fdnn_server_submit_raw": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_void_p, _c_f32p, C.POINTER(C.c_uint64)]),
    "fdnn_server_live_open": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "fdnn_server_live_close": (None, [C.c_void_p]),
    "fdnn_server_live_reset": (C.c_int, [C.c_void_p]),
    "fdnn_server_live_position": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "fdnn_server_live_push": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_f32p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "fdnn_server_live_push_topk": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_int, _c_i32p, _c_f32p, C.POINTER(C.c_int),
                                             C.POINTER(C.c_uint64)]),
    "fdnn_server_live_push_pool": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, C.c_void_p, _c_f32p, C.POINTER(C.c_int),
                                             C.POINTER(C.c_uint64)]),
    "fdnn_server_live_push_set": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_i32p, C.c_int, _c_f32p, _c_f32p, C.POINTER(C.c_int),
                                            C.POINTER(C.c_uint64)]),
    "fdnn_debug_splice_table": (C.c_int, [_c_i32p, C.c_int, C.c_int, C.c_int, _c_f32p, C.c_int, _c_i32p, C.c_int, C.c_int, C.c_int, _c_f32p,
                                          C.c_int]),
    "fdnn_debug_live_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "fdnn_debug_server_hold": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_host_model_load": (C.c_int, [C.c_char_p, C.c_float, C.POINTER(C.c_void_p)]),
    "fdnn_host_model_free": (None, [C.c_void_p]),
    "fdnn_host_model_layers": (C.c_int, [C.c_void_p]),
    "fdnn_host_model_layer_in": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_host_model_layer_out": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_host_model_multiplier": (C.c_float, [C.c_void_p, C.c_int]),
    "fdnn_host_model_weights_q": (C.c_int, [C.c_void_p, C.c_int, _c_i8p]),
    "fdnn_host_model_bias": (C.c_int, [C.c_void_p, C.c_int, _c_f32p]),
    "fdnn_host_model_wsum128": (C.c_int, [C.c_void_p, C.c_int, _c_i32p]),
    "fdnn_host_model_risky_pairs": (C.c_longlong, [C.c_void_p, C.c_int]),
    "fdnn_host_model_blob_size": (C.c_size_t, [C.c_void_p]),
    "fdnn_host_model_blob": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fdnn_host_blob_check": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                       C.POINTER(C.c_int)]),
    "fdnn_host_sigmoid_lut": (C.c_int, [_c_u8p]),
    "fdnn_host_quantize": (C.c_int, [_c_f32p, C.c_int, C.c_int, C.c_float, _c_i8p, _c_f32p]),
    "fdnn_float_model_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "fdnn_float_model_load_on": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "fdnn_float_model_free": (None, [C.c_void_p]),
    "fdnn_float_model_input_dim": (C.c_int, [C.c_void_p]),
    "fdnn_float_model_output_dim": (C.c_int, [C.c_void_p]),
    "fdnn_float_model_layer_count": (C.c_int, [C.c_void_p]),
    "fdnn_float_model_layer_dim": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_float_model_device": (C.c_int, [C.c_void_p]),
    "fdnn_float_calculate": (C.c_int, [C.c_void_p, _c_f32p, C.c_int, C.c_int, _c_f32p]),
    "fdnn_float_calculate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fdnn_debug_float_layer": (C.c_int, [C.c_void_p, C.c_int, _c_f32p, C.c_int, _c_f32p, _c_f32p]),
    "fdnn_debug_float_layer_us": (C.c_int, [C.c_void_p, C.c_int, _c_f32p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "fdnn_debug_float_layer_ref": (C.c_int, [_c_f32p, _c_f32p, C.c_int, C.c_int, _c_f32p, C.c_int, _c_f32p]),
    "fdnn_debug_float_input_ref": (C.c_int, [_c_f32p, _c_f32p, C.c_int, _c_f32p, C.c_int, _c_f32p, _c_f32p]),
    "fdnn_debug_float_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "fdnn_debug_float_launches": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
    "fdnn_report_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "fdnn_report_free": (None, [C.c_void_p]),
    "fdnn_report_reset": (C.c_int, [C.c_void_p]),
    "fdnn_report_add_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "fdnn_report_add": (C.c_int, [C.c_void_p, _c_f32p, _c_f32p, C.c_int]),
    "fdnn_report_read": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.POINTER(C.c_double)]),
}

JNI_SYMBOLS = [
    "Java_suskun_nn_QuantizedDnn_" + n
    for n in ("initialize", "inputDimension", "outputDimension", "calculate", "getContext", "calculateUntilOutput",
              "calculateLazy", "deleteLazyContext", "delete", "layerDimension", "layerCount",
              "calculateLazyBatch")  # (the last one: an extension)
]


def _one_hip_runtime() -> None:
    """A process must hold ONE HIP runtime.  PyTorch wheels bundle their own ``libamdhip64.so``
    (same SONAME as ROCm's); if libfast-dnn.so pulls in /opt/rocm's copy first and torch is
    imported afterwards, torch loads a second runtime, which finds no device.  So when torch is
    installed but not imported yet, its copy is loaded first and both sides share it (the order
    bench.py uses anyway: torch first)."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(p):
        try:
            C.CDLL(p, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib() -> C.CDLL:
    """Load libfast-dnn.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the scorer)")
        _one_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc: int) -> None:
    if rc != FDNN_OK:
        raise FdnnError(rc, lib().fdnn_last_error().decode(errors="replace"))


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def device_count() -> int:
    return int(lib().fdnn_device_count())


def device_shared(device: int = 0) -> bool:
    """True when another process held the GPU's marker first: this process runs the unfused soft-max (fdnn_device_shared)."""
    r = int(lib().fdnn_device_shared(int(device)))
    if r < 0:
        _check(r)
    return r == 1


def set_fuse(mode: int) -> None:
    """Soft-max scale of large batches (process-wide, tests): 0 = separate pass, 1 = inside the output kernel, -1 = default."""
    _check(lib().fdnn_debug_set_fuse(int(mode)))


def set_chain(mode: int, min_frames: int = 0) -> None:
    """How the int8 hidden layers run (process-wide; results are bit-identical): 1 = one persistent launch for batches of
    at least min_frames frames, 0 = one launch per layer, -1 = the default."""
    _check(lib().fdnn_debug_set_chain(int(mode), int(min_frames)))


def set_pp(mode: int, min_frames: int = 0) -> None:
    """How a large batch's int8 hidden layers run when launched layer by layer (process-wide; results are bit-identical):
    1 = the role-split kernel (fdnn_pp.hip) for batches of at least min_frames frames, 0 = the in-phase tiles, -1 = default."""
    _check(lib().fdnn_debug_set_pp(int(mode), int(min_frames)))


def set_ppo(mode: int) -> None:
    """How a large dense batch's output layer runs when its soft-max is fused (process-wide; results are bit-identical):
    1 = the role-split kernel (fdnn_ppo.hip) whenever the shape allows, 0 = the in-phase fused tiles, -1 = default."""
    _check(lib().fdnn_debug_set_ppo(int(mode)))


LAUNCH_ABLATION, LAUNCH_LOAD_TIME = 1, 2  # flags of launch_names()


def launch_names() -> dict:
    """The launch recorder's table: name of every host launch branch -> flags (LAUNCH_ABLATION: the branch exists only in
    measurement builds, LAUNCH_LOAD_TIME: the kernel runs at model load).  Needs no device."""
    L = lib()
    out = {}
    for i in range(L.fdnn_debug_launch_name_count()):
        flags = C.c_int(0)
        name = L.fdnn_debug_launch_name(i, C.byref(flags)).decode()
        out[name] = flags.value
    return out


def launch_record(on: bool = True) -> None:
    """Count launches per name from here on (process-wide, every thread); off by default."""
    _check(lib().fdnn_debug_launch_record(1 if on else 0))


def launch_reset() -> None:
    _check(lib().fdnn_debug_launch_reset())


def launch_counts(nonzero: bool = True) -> dict:
    """name -> launches counted since the last launch_reset() (only the names that ran unless nonzero=False)."""
    L = lib()
    n = L.fdnn_debug_launch_name_count()
    buf = (C.c_ulonglong * n)()
    if L.fdnn_debug_launch_counts(buf, n) != n:
        raise RuntimeError("launch table changed size")
    names = list(launch_names())
    return {names[i]: int(buf[i]) for i in range(n) if buf[i] or not nonzero}


def scratch_names() -> tuple:
    """The self-rewinding scratch buffers of a context, in the library's table order (fdnn_ctx_layout.hpp): counters every
    launch assumes zero and only the kernels put back to zero.  Needs no device."""
    L = lib()
    return tuple(L.fdnn_debug_scratch_name(i).decode() for i in range(L.fdnn_debug_scratch_count()))


def scratch_audit(on: bool = True) -> None:
    """Process-wide, off by default: while on, every context is audited (LazyContext.scratchState's count) when it goes back
    to its model's pool and when it is destroyed, and the counts add up for scratch_dirty()."""
    _check(lib().fdnn_debug_scratch_audit(1 if on else 0))


def scratch_dirty() -> dict:
    """Reads and resets the audit's totals -> {buffer name: non-zero words found, ..., "contexts": contexts audited,
    "unreadable": contexts whose buffers could not be copied, "seconds": what the audits themselves took}."""
    names = scratch_names()
    buf = (C.c_ulonglong * (len(names) + 3))()
    _check(lib().fdnn_debug_scratch_dirty(buf, len(names) + 3))
    out = {k: int(buf[i]) for i, k in enumerate(names)}
    out["contexts"] = int(buf[len(names)])
    out["unreadable"] = int(buf[len(names) + 1])
    out["seconds"] = int(buf[len(names) + 2]) * 1e-9
    return out


def _lists(rowPtr, nodes):
    """(row_ptr, nodes) as C-contiguous int32 arrays; the shapes every list entry point needs."""
    rp = np.ascontiguousarray(rowPtr, dtype=np.int32)
    nd = np.ascontiguousarray(nodes, dtype=np.int32)
    if rp.ndim != 1 or rp.size < 1 or nd.ndim != 1:
        raise ValueError("rowPtr must be [count + 1] and nodes [nnz]")
    if int(rp[-1]) > nd.size:  # (the C side reads rowPtr[count] nodes)
        raise ValueError(f"rowPtr ends at {int(rp[-1])} but there are {nd.size} nodes")
    return rp, nd


def lists_check(rowPtr, nodes, outputDimension: int) -> int:
    """The validator of the list entry points (``fdnn_debug_lists_check``; host code, no device): 0, or -(row + 1) of the
    first row whose list is not well formed -- rowPtr starts at 0 and never decreases, a row's nodes ascend strictly
    inside [0, outputDimension)."""
    rp = np.ascontiguousarray(rowPtr, dtype=np.int32)
    nd = np.ascontiguousarray(nodes, dtype=np.int32)
    if rp.ndim != 1 or rp.size < 1 or nd.ndim != 1:
        raise ValueError("rowPtr must be [count + 1] and nodes [nnz]")
    if rp.size > 1 and int(rp.max()) > nd.size:  # never let the C side read past the node array
        return -(int(np.argmax(rp[1:] > nd.size)) + 1)
    return int(lib().fdnn_debug_lists_check(rp.ctypes.data_as(_c_i32p), nd.ctypes.data_as(_c_i32p), rp.size - 1, int(outputDimension)))


def lists_launches():
    """Process-wide launch counts of the list kernels since load: (score without the pair walk, score with it, finish)."""
    buf = (C.c_ulonglong * 3)()
    if lib().fdnn_debug_lists_launches(buf, 3) != 3:
        raise RuntimeError("fdnn_debug_lists_launches")
    return tuple(int(v) for v in buf)


def lists_union_launches():
    """Process-wide counts of the union path of the list calls since load (``fdnn_debug_lists_union_launches``): (union-build
    launches, score launches without the pair walk, with it, calls with the switch on that the dot-product kernels served)."""
    buf = (C.c_ulonglong * 4)()
    if lib().fdnn_debug_lists_union_launches(buf, 4) != 4:
        raise RuntimeError("fdnn_debug_lists_union_launches")
    return tuple(int(v) for v in buf)


def _union_buffers(rp, group_tiles):
    rows = SET_FRAME_TILE * int(group_tiles)
    groups = -(-(rp.size - 1) // rows) if group_tiles >= 1 else 0
    nnz = int(rp[-1])
    return np.full(max(groups, 0), -1, np.int32), np.full(nnz, -1, np.int32), np.full(nnz, -1, np.int32)


def lists_union_ref(rowPtr, nodes, outputDimension: int, group_tiles: int):
    """The unions of every ``32 * group_tiles`` rows' lists from the host restatement (``fdnn_debug_lists_union_ref``, no
    device) -> (u_len [groups], u_nodes [nnz]: group q's union ascending from index rowPtr[q * 32 * group_tiles] on, -1
    where no union reaches, pos [nnz]: every entry's rank in its group's union)."""
    rp, nd = _lists(rowPtr, nodes)
    u_len, u_nodes, pos = _union_buffers(rp, group_tiles)
    _check(lib().fdnn_debug_lists_union_ref(rp.ctypes.data_as(_c_i32p), nd.ctypes.data_as(_c_i32p), rp.size - 1, int(outputDimension), int(group_tiles),
                                            u_len.ctypes.data_as(_c_i32p), u_nodes.ctypes.data_as(_c_i32p), pos.ctypes.data_as(_c_i32p)))
    return u_len, u_nodes, pos


# The set kernel's tiles (fdnn_set.hpp: kNodeTile, kFrameTile; tests/test_lazy_set_host.py holds the two files together)
SET_NODE_TILE = 64
SET_FRAME_TILE = 32


def _set(nodes):
    """The node set as a C-contiguous int32 vector."""
    nd = np.ascontiguousarray(nodes, dtype=np.int32)
    if nd.ndim != 1:
        raise ValueError("nodes must be [len]")
    return nd


def set_check(nodes, outputDimension: int) -> int:
    """The validator of the set entry points (``fdnn_debug_set_check``; host code, no device): 0, or -1 for a set that does
    not ascend strictly inside [0, outputDimension)."""
    nd = _set(nodes)
    return int(lib().fdnn_debug_set_check(nd.ctypes.data_as(_c_i32p), nd.size, int(outputDimension)))


def set_launches():
    """Process-wide counts since load: (MFMA set kernel without the pair walk, with it, calls served by the list kernels)."""
    buf = (C.c_ulonglong * 3)()
    if lib().fdnn_debug_set_launches(buf, 3) != 3:
        raise RuntimeError("fdnn_debug_set_launches")
    return tuple(int(v) for v in buf)


def set_kernel(mode: int) -> None:
    """Process-wide (``fdnn_debug_set_kernel``): 0 the default rule, 1 the MFMA kernel where its shape applies, 2 the fallback."""
    _check(lib().fdnn_debug_set_kernel(int(mode)))


# The top-k selection's limits (fdnn_topk.hpp: kTopkMaxK, kTopkResidentWidth; tests/test_topk_host.py holds the two files
# together and compares both with fdnn_debug_topk_limits)
TOPK_MAX_K = 256
TOPK_RESIDENT_WIDTH = 16384


def topk_rows_device(d_rows: int, n: int, width: int, k: int, d_nodes: int, d_vals: int, stream: int = 0) -> None:
    """The selection alone (``fdnn_topk_rows_device``) on device-resident fp32 rows [n][width] of the current device: the k
    first-ranked nodes of every row and their values into d_nodes int32 [n][k] / d_vals float32 [n][k]; raw device pointers,
    enqueued on ``stream``, not synchronised."""
    _check(lib().fdnn_topk_rows_device(C.c_void_p(d_rows), int(n), int(width), int(k), C.c_void_p(d_nodes), C.c_void_p(d_vals), C.c_void_p(stream)))


def topk_ref(rows, k: int):
    """The same selection from the host restatement (``fdnn_debug_topk_ref``; host code, no device) on rows [n][width]
    float32 (any bit patterns) -> (nodes int32 [n][k], vals float32 [n][k])."""
    r = np.ascontiguousarray(rows, dtype=np.float32)
    if r.ndim != 2:
        raise ValueError("rows must be [n][width]")
    nodes = np.empty((r.shape[0], int(k)), dtype=np.int32)
    vals = np.empty((r.shape[0], int(k)), dtype=np.float32)
    _check(lib().fdnn_debug_topk_ref(r.ctypes.data_as(_c_f32p), r.shape[0], r.shape[1], int(k), nodes.ctypes.data_as(_c_i32p), vals.ctypes.data_as(_c_f32p)))
    return nodes, vals


def topk_launches():
    """Process-wide counts since load: (launches of the resident form of the selection, of the streaming form)."""
    buf = (C.c_ulonglong * 2)()
    if lib().fdnn_debug_topk_launches(buf, 2) != 2:
        raise RuntimeError("fdnn_debug_topk_launches")
    return tuple(int(v) for v in buf)


def set_topk_kernel(mode: int) -> None:
    """Process-wide (``fdnn_debug_set_topk_kernel``): 0 the plan's rule, 1 resident where the width allows, 2 always streaming."""
    _check(lib().fdnn_debug_set_topk_kernel(int(mode)))


def topk_limits():
    """(largest k, widest resident row) as the library was built (``fdnn_debug_topk_limits``)."""
    a, b = C.c_int(), C.c_int()
    _check(lib().fdnn_debug_topk_limits(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


# The class pooling's limits (fdnn_pool.hpp: kPoolLanes, kPoolResidentWidth; tests/test_pool_host.py holds the two files
# together and compares both with fdnn_debug_pool_limits)
POOL_LANES = 16
POOL_RESIDENT_WIDTH = 16384


class ClassPool:
    """A node -> class map registered once (``fdnn_pool_create``): ``class_of`` int32 [width], every entry -1 (in no class)
    or a class in [0, n_classes); validated on the host, its CSR uploaded to the device that is current.  Immutable; threads, contexts and scoring loops may share it; it must outlive every call and ticket that uses it."""

    def __init__(self, class_of, n_classes: int):
        co = np.ascontiguousarray(class_of, dtype=np.int32)
        if co.ndim != 1:
            raise ValueError("class_of must be a vector [width]")
        self.handle = lib().fdnn_pool_create(co.ctypes.data_as(_c_i32p), co.size, int(n_classes))
        if not self.handle:
            # (the C call returns no status: a map it takes is one pool_ref's validation takes -- then the device refused)
            bad_map = co.size < 1 or not 1 <= int(n_classes) <= co.size or bool(((co < -1) | (co >= int(n_classes))).any())
            raise FdnnError(FDNN_E_ARG if bad_map else FDNN_E_DEVICE, lib().fdnn_last_error().decode(errors="replace"))
        self.class_of = co.copy()

    def width(self) -> int:
        return int(lib().fdnn_pool_width(self.handle))

    def classes(self) -> int:
        return int(lib().fdnn_pool_classes(self.handle))

    def rows_device(self, d_rows: int, n: int, d_out: int, stream: int = 0) -> None:
        """The pooling alone (``fdnn_pool_rows_device``) on device-resident fp32 rows [n][width] -> d_out float32
        [n][classes]; raw device pointers, enqueued on ``stream``, not synchronised."""
        _check(lib().fdnn_pool_rows_device(self.handle, C.c_void_p(d_rows), int(n), C.c_void_p(d_out), C.c_void_p(stream)))

    def delete(self) -> None:
        if self.handle:
            lib().fdnn_pool_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.delete()
        except Exception:
            pass


def pool_ref(rows, class_of, n_classes: int):
    """The pooling from the host restatement (``fdnn_debug_pool_ref``; host code, no device) on rows [n][width] float32 (any
    bit patterns) under the map class_of [width] -> float32 [n][n_classes]."""
    r = np.ascontiguousarray(rows, dtype=np.float32)
    co = np.ascontiguousarray(class_of, dtype=np.int32)
    if r.ndim != 2 or co.ndim != 1 or co.size != r.shape[1]:
        raise ValueError("rows must be [n][width] and class_of [width]")
    out = np.empty((r.shape[0], max(int(n_classes), 0)), dtype=np.float32)
    _check(lib().fdnn_debug_pool_ref(r.ctypes.data_as(_c_f32p), r.shape[0], co.ctypes.data_as(_c_i32p), co.size, int(n_classes), out.ctypes.data_as(_c_f32p)))
    return out


def pool_launches():
    """Process-wide counts since load: (launches of the resident form of the pooling, of the streaming form)."""
    buf = (C.c_ulonglong * 2)()
    if lib().fdnn_debug_pool_launches(buf, 2) != 2:
        raise RuntimeError("fdnn_debug_pool_launches")
    return tuple(int(v) for v in buf)


def set_pool_kernel(mode: int) -> None:
    """Process-wide (``fdnn_debug_set_pool_kernel``): 0 the plan's rule, 1 resident where the width allows, 2 always streaming."""
    _check(lib().fdnn_debug_set_pool_kernel(int(mode)))


def pool_limits():
    """(partial sums of a class, widest resident row) as the library was built (``fdnn_debug_pool_limits``)."""
    a, b = C.c_int(), C.c_int()
    _check(lib().fdnn_debug_pool_limits(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def _pool_out(n: int, classes: int, out):
    """The [n][C] result array of a pool call, made or checked."""
    if out is None:
        return np.empty((n, classes), dtype=np.float32)
    if out.dtype != np.float32 or out.shape != (n, classes) or not out.flags.c_contiguous:
        raise ValueError(f"out must be a C-contiguous float32 array of shape {(n, classes)}")
    return out


# The output types of a score handle (include/fdnn.h: FDNN_LOGLIK_F32, FDNN_LOGLIK_F16)
LOGLIK_F32 = 0
LOGLIK_F16 = 1
_LOGLIK_DTYPE = {LOGLIK_F32: np.float32, LOGLIK_F16: np.float16}


def _loglik_args_bad(lp, floor, type) -> bool:
    """What fdnn_loglik_create refuses as an argument (fdnn_loglik.hpp: check_handle), for the error code of a NULL handle."""
    f = np.float32(floor)
    return bool(lp.size < 1 or lp.size > (1 << 19) or type not in _LOGLIK_DTYPE or not np.isfinite(lp).all() or np.isnan(f) or f == np.inf
                or (type == LOGLIK_F16 and np.isfinite(f) and f < np.float32(-65504.0)))


class Loglik:
    """A decoder-score handle registered once (``fdnn_loglik_create``): ``log_prior`` float32 [width], all finite; ``floor``
    (-inf: none) and the output ``type`` (``LOGLIK_F32`` or ``LOGLIK_F16``).  The score of a row p is ln(p_i) - log_prior[i],
    floored, by the ONE logarithm of include/fdnn.h (``ln_ref``); F16 results are ``numpy.float16``.  Note that the k best
    probabilities are not the k best scores.  Immutable; threads, contexts and scoring loops may share it; it must outlive
    every call and ticket that uses it."""

    def __init__(self, log_prior, floor: float = -np.inf, type: int = LOGLIK_F32):
        lp = np.ascontiguousarray(log_prior, dtype=np.float32)
        if lp.ndim != 1:
            raise ValueError("log_prior must be a vector [width]")
        self.handle = lib().fdnn_loglik_create(lp.ctypes.data_as(_c_f32p), lp.size, C.c_float(float(floor)), int(type))
        if not self.handle:
            raise FdnnError(FDNN_E_ARG if _loglik_args_bad(lp, floor, int(type)) else FDNN_E_DEVICE, lib().fdnn_last_error().decode(errors="replace"))
        self.log_prior, self.floor = lp.copy(), float(floor)
        self.dtype = _LOGLIK_DTYPE[int(type)]

    def width(self) -> int:
        return int(lib().fdnn_loglik_width(self.handle))

    def type(self) -> int:
        return int(lib().fdnn_loglik_type(self.handle))

    def rows_device(self, d_rows: int, n: int, d_out: int, stream: int = 0) -> None:
        """The scores alone (``fdnn_loglik_rows_device``) of device-resident fp32 rows [n][width] -> d_out [n][width] of the
        handle's type; raw device pointers, enqueued on ``stream``, not synchronised."""
        _check(lib().fdnn_loglik_rows_device(self.handle, C.c_void_p(d_rows), int(n), C.c_void_p(d_out), C.c_void_p(stream)))

    def entries_device(self, d_nodes: int, d_p: int, count: int, d_out: int, stream: int = 0) -> None:
        """The scores of a flat list of (node, probability) entries (``fdnn_loglik_entries_device``) -> d_out [count]; a node
        outside [0, width) gives a NaN."""
        _check(lib().fdnn_loglik_entries_device(self.handle, C.c_void_p(d_nodes), C.c_void_p(d_p), int(count), C.c_void_p(d_out), C.c_void_p(stream)))

    def delete(self) -> None:
        if self.handle:
            lib().fdnn_loglik_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.delete()
        except Exception:
            pass


def ln_ref(x):
    """The contract's logarithm (``fdnn_debug_ln_ref``, fdnn_loglik.hpp: ln) of float32 values of any shape, any bit patterns."""
    v = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(v)
    _check(lib().fdnn_debug_ln_ref(v.ctypes.data_as(_c_f32p), v.size, out.ctypes.data_as(_c_f32p)))
    return out


def loglik_ref(rows, log_prior, floor: float = -np.inf, type: int = LOGLIK_F32):
    """The scores from the host restatement (``fdnn_debug_loglik_ref``; host code, no device) of rows [n][width] float32 (any
    bit patterns) -> [n][width] float32 or float16."""
    r = np.ascontiguousarray(rows, dtype=np.float32)
    lp = np.ascontiguousarray(log_prior, dtype=np.float32)
    if r.ndim != 2 or lp.ndim != 1 or lp.size != r.shape[1]:
        raise ValueError("rows must be [n][width] and log_prior [width]")
    out = np.empty(r.shape, dtype=_LOGLIK_DTYPE.get(int(type), np.float32))
    _check(lib().fdnn_debug_loglik_ref(r.ctypes.data_as(_c_f32p), r.shape[0], lp.ctypes.data_as(_c_f32p), lp.size, C.c_float(float(floor)), int(type),
                                       C.c_void_p(out.ctypes.data)))
    return out


def loglik_entries_ref(nodes, p, log_prior, floor: float = -np.inf, type: int = LOGLIK_F32):
    """The same for a flat list of (node, probability) entries (``fdnn_debug_loglik_entries_ref``) -> [count]."""
    nd = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
    v = np.ascontiguousarray(p, dtype=np.float32).ravel()
    lp = np.ascontiguousarray(log_prior, dtype=np.float32)
    if nd.size != v.size or lp.ndim != 1:
        raise ValueError("nodes and p must have one length, log_prior must be [width]")
    out = np.empty(nd.size, dtype=_LOGLIK_DTYPE.get(int(type), np.float32))
    _check(lib().fdnn_debug_loglik_entries_ref(nd.ctypes.data_as(_c_i32p), v.ctypes.data_as(_c_f32p), nd.size, lp.ctypes.data_as(_c_f32p), lp.size,
                                               C.c_float(float(floor)), int(type), C.c_void_p(out.ctypes.data)))
    return out


def loglik_launches():
    """Process-wide counts since load: launches of (the rows kernel's vector form, its scalar-access form, the entries kernel)."""
    buf = (C.c_ulonglong * 3)()
    if lib().fdnn_debug_loglik_launches(buf, 3) != 3:
        raise RuntimeError("fdnn_debug_loglik_launches")
    return tuple(int(v) for v in buf)


def set_loglik_kernel(mode: int) -> None:
    """Process-wide (``fdnn_debug_set_loglik_kernel``): 0 the plan's rule, 1 vector where allowed, 2 always scalar access."""
    _check(lib().fdnn_debug_set_loglik_kernel(int(mode)))


ALIGN_SCORES = -1  # the ``type`` of an align call without a handle: the rows are scores already


def _fp(a):
    """A float32 array's pointer, or NULL for None."""
    return None if a is None else a.ctypes.data_as(_c_f32p)


def _align_tables(segRows, statePtr, states, selfLp, nextLp):
    """(seg_rows, state_ptr, states, self_lp, next_lp) as C-contiguous vectors of the shapes every align entry point needs ->
    them, the segment count and the rows."""
    sr = np.ascontiguousarray(segRows, dtype=np.int32)
    sp = np.ascontiguousarray(statePtr, dtype=np.int32)
    st = np.ascontiguousarray(states, dtype=np.int32)
    if sr.ndim != 1 or sp.ndim != 1 or st.ndim != 1 or sr.size != sp.size or sr.size < 1:
        raise ValueError("segRows and statePtr must be [segments + 1] and states [statePtr[-1]]")
    if int(sp.max()) > st.size:  # (the C side reads statePtr[segments] states)
        raise ValueError(f"statePtr reaches {int(sp.max())} but there are {st.size} states")
    lps = []
    for lp in (selfLp, nextLp):
        if lp is not None:
            lp = np.ascontiguousarray(lp, dtype=np.float32)
            if lp.shape != st.shape:
                raise ValueError("selfLp and nextLp are [states] like the transcript")
        lps.append(lp)
    return sr, sp, st, lps[0], lps[1], sr.size - 1, max(int(sr[-1]) - int(sr[0]), 0)


def _align_rows_tables(segT, rowOff, rowLd, statePtr):
    t = np.ascontiguousarray(segT, dtype=np.int32)
    off = np.ascontiguousarray(rowOff, dtype=np.int64)
    ld = np.ascontiguousarray(rowLd, dtype=np.int32)
    sp = np.ascontiguousarray(statePtr, dtype=np.int32)
    if t.ndim != 1 or off.shape != t.shape or ld.shape != t.shape or sp.shape != (t.size + 1,):
        raise ValueError("segT, rowOff and rowLd must be [segments] and statePtr [segments + 1]")
    return t, off, ld, sp


def align_sets(statePtr, states):
    """The transcripts' node sets as the align calls build them (``fdnn_debug_align_sets``; host code): (set_ptr [segments + 1],
    nodes, col [states]) -- each segment's distinct nodes, ascending, the form ``calculateLazySets`` takes, and the position of
    every state's node in its segment's set."""
    sp = np.ascontiguousarray(statePtr, dtype=np.int32)
    st = np.ascontiguousarray(states, dtype=np.int32)
    if sp.ndim != 1 or sp.size < 1 or st.ndim != 1 or int(sp.max()) > st.size:
        raise ValueError("statePtr must be [segments + 1] and states [statePtr[-1]]")
    set_ptr = np.zeros(sp.size, np.int32)
    nodes = np.empty(max(st.size, 1), np.int32)
    col = np.empty(max(st.size, 1), np.int32)
    _check(lib().fdnn_debug_align_sets(sp.ctypes.data_as(_c_i32p), st.ctypes.data_as(_c_i32p), sp.size - 1, set_ptr.ctypes.data_as(_c_i32p),
                                       nodes.ctypes.data_as(_c_i32p), col.ctypes.data_as(_c_i32p)))
    return set_ptr, nodes[:int(set_ptr[-1])].copy(), col[:int(sp[-1])].copy()


def align_ref(rows, segT, rowOff, rowLd, statePtr, col, stateNode=None, log_prior=None, floor: float = -np.inf, type: int = ALIGN_SCORES,
              selfLp=None, nextLp=None):
    """The recursion from the host restatement (``fdnn_debug_align_ref``; host code, no device): rows a flat float32 array (any
    bit patterns), segment s = segT[s] rows of stride rowLd[s] beginning at element rowOff[s]; col [states]; with ``type``
    LOGLIK_F32 / LOGLIK_F16 the rows are probabilities and stateNode [states], log_prior and floor make the scores, with
    ALIGN_SCORES they are scores -> (path int32 [sum segT], total float32 [segments])."""
    r = np.ascontiguousarray(rows, dtype=np.float32).ravel()
    t, off, ld, sp = _align_rows_tables(segT, rowOff, rowLd, statePtr)
    c = np.ascontiguousarray(col, dtype=np.int32)
    nd = None if stateNode is None else np.ascontiguousarray(stateNode, dtype=np.int32)
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float32)
    sl = None if selfLp is None else np.ascontiguousarray(selfLp, dtype=np.float32)
    nl = None if nextLp is None else np.ascontiguousarray(nextLp, dtype=np.float32)
    if t.size and ((off + (t.astype(np.int64) - 1) * ld + ld > r.size).any() or (off < 0).any() or c.size < int(sp[-1])):
        raise ValueError("a segment's rows run past the rows, or col is shorter than the transcripts")
    path = np.empty(int(t.astype(np.int64).sum()), np.int32)
    total = np.empty(t.size, np.float32)
    _check(lib().fdnn_debug_align_ref(r.ctypes.data_as(_c_f32p), t.ctypes.data_as(_c_i32p), off.ctypes.data_as(C.POINTER(C.c_longlong)),
                                      ld.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), t.size, c.ctypes.data_as(_c_i32p),
                                      None if nd is None else nd.ctypes.data_as(_c_i32p), _fp(lp), 0 if lp is None else lp.size, C.c_float(float(floor)),
                                      int(type), _fp(sl), _fp(nl), path.ctypes.data_as(_c_i32p), total.ctypes.data_as(_c_f32p)))
    return path, total


def align_scratch_words(segT, statePtr) -> int:
    """The 32-bit scratch words ``align_rows_device`` needs for these tables under the current kernel mode
    (``fdnn_align_scratch_words``): the back-pointer words of the segments that do not fit LDS."""
    t = np.ascontiguousarray(segT, dtype=np.int32)
    sp = np.ascontiguousarray(statePtr, dtype=np.int32)
    words = C.c_longlong(0)
    _check(lib().fdnn_align_scratch_words(t.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), t.size, C.byref(words)))
    return int(words.value)


def align_rows_device(ll, d_rows: int, segT, rowOff, rowLd, statePtr, d_col: int, d_state_node: int, d_self_lp: int, d_next_lp: int, d_scratch: int,
                      scratch_words: int, d_path: int, d_total: int, stream: int = 0) -> None:
    """The recursion alone on device-resident fp32 rows (``fdnn_align_rows_device``): host tables as ``align_ref``, device
    pointers for everything they index; ``ll`` a ``Loglik`` (the rows are probabilities) or None (they are scores).  Enqueued on
    ``stream``, not synchronised."""
    t, off, ld, sp = _align_rows_tables(segT, rowOff, rowLd, statePtr)
    _check(lib().fdnn_align_rows_device(None if ll is None else ll.handle, C.c_void_p(d_rows), t.ctypes.data_as(_c_i32p),
                                        off.ctypes.data_as(C.POINTER(C.c_longlong)), ld.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), t.size,
                                        C.c_void_p(d_col), C.c_void_p(d_state_node), C.c_void_p(d_self_lp), C.c_void_p(d_next_lp), C.c_void_p(d_scratch),
                                        int(scratch_words), C.c_void_p(d_path), C.c_void_p(d_total), C.c_void_p(stream)))


def align_launches():
    """Process-wide counts since load: (launches of the align kernel's wave form, of its workgroup form)."""
    buf = (C.c_ulonglong * 2)()
    if lib().fdnn_debug_align_launches(buf, 2) != 2:
        raise RuntimeError("fdnn_debug_align_launches")
    return tuple(int(v) for v in buf)


def set_align_kernel(mode: int) -> None:
    """Process-wide (``fdnn_debug_set_align_kernel``): 0 the plan's rule, 1 the wave form where allowed, 2 always the workgroup form."""
    _check(lib().fdnn_debug_set_align_kernel(int(mode)))


def align_limits() -> dict:
    """The align kernels' limits as built (``fdnn_debug_align_limits``)."""
    buf = (C.c_int * 6)()
    if lib().fdnn_debug_align_limits(buf, 6) != 6:
        raise RuntimeError("fdnn_debug_align_limits")
    return dict(zip(("max_states", "segs_per_launch", "wave_states", "frames_in_flight", "lds_bp_words", "scratch_cap_mib"), (int(v) for v in buf)))


# ---------------------------------------------------------------- alignment graphs (fdnn_align_graph.hip)
# A GRAPH is a dict of one segment's tables: states [S] (output nodes), arc_ptr [S + 1] from 0, arc_src / arc_lp [arcs] (the
# sources are state indices of the graph), start_lp / final_lp [S] or None (state 0 / state S - 1).  pack_graphs makes a call's
# tables of several: a dict with statePtr, states, arcPtr (global), arcSrc (local), arcLp, startLp, finalLp.
def _ip(a):
    """An int32 array's pointer, or NULL for None."""
    return None if a is None else a.ctypes.data_as(_c_i32p)


def chain_graph(states, self_lp=None, next_lp=None) -> dict:
    """The chain of ``calculateAlign`` as a graph: state j is entered from j (self_lp[j], listed first) and from j - 1
    (next_lp[j - 1]); state 0 has the self-loop alone; None scores are +0; start and final are the defaults (state 0, state
    S - 1).  On emissions that are neither a NaN nor +inf it gives ``calculateAlign``'s bytes."""
    st = np.ascontiguousarray(states, dtype=np.int32).ravel()
    S = st.size
    if S < 1:
        raise ValueError("a chain has at least one state")
    sl = np.zeros(S, np.float32) if self_lp is None else np.ascontiguousarray(self_lp, dtype=np.float32).ravel()
    nl = np.zeros(S, np.float32) if next_lp is None else np.ascontiguousarray(next_lp, dtype=np.float32).ravel()
    if sl.size != S or nl.size != S:
        raise ValueError("self_lp and next_lp are [states]")
    j = np.arange(S, dtype=np.int32)
    src = np.concatenate([[0], np.stack([j[1:], j[1:] - 1], axis=1).ravel()]).astype(np.int32)
    lp = np.concatenate([sl[:1], np.stack([sl[1:], nl[:-1]], axis=1).ravel()]).astype(np.float32)
    ptr = np.concatenate([[0], 1 + 2 * j]).astype(np.int32)
    return dict(states=st, arc_ptr=ptr, arc_src=src, arc_lp=lp, start_lp=None, final_lp=None)


def optional_silence_graph(words, sil_node: int, self_lp: float = 0.0, next_lp: float = 0.0, sil_self_lp: float = 0.0, enter_sil_lp: float = 0.0,
                           leave_sil_lp: float = 0.0, skip_sil_lp: float = 0.0) -> dict:
    """A transcript with OPTIONAL silence: ``words`` is a list of node lists, one chain each; there is one silence state (node
    ``sil_node``) before each word and one after the last.  State order: sil, word 0's states, sil, word 1's states, .., sil.
    Every state has a self-loop, listed first.  Inside a word state j is entered from j - 1.  A word's first state is
    entered from the previous word's last state (skip_sil_lp, listed before the silence) and from the silence before it
    (leave_sil_lp); a silence is entered from the last state of the word before it (enter_sil_lp); the leading silence has its
    self-loop alone.  The path starts in the leading silence or the first word's first state and ends in the last word's last
    state or the trailing silence (start and final values +0 there, -inf elsewhere)."""
    if not len(words) or any(not len(w) for w in words):
        raise ValueError("words is a non-empty list of non-empty node lists")
    states, ptr, src, lp = [], [0], [], []
    prev_last = -1  # the last state of the previous word
    for w in words:
        sil = len(states)
        states.append(int(sil_node))
        src.append(sil), lp.append(sil_self_lp)
        if prev_last >= 0:
            src.append(prev_last), lp.append(enter_sil_lp)
        ptr.append(len(src))
        for i, node in enumerate(w):
            j = len(states)
            states.append(int(node))
            src.append(j), lp.append(self_lp)
            if i:
                src.append(j - 1), lp.append(next_lp)
            else:
                if prev_last >= 0:
                    src.append(prev_last), lp.append(skip_sil_lp)
                src.append(sil), lp.append(leave_sil_lp)
            ptr.append(len(src))
        prev_last = len(states) - 1
    sil = len(states)
    states.append(int(sil_node))
    src.extend([sil, prev_last]), lp.extend([sil_self_lp, enter_sil_lp])
    ptr.append(len(src))
    S = len(states)
    start = np.full(S, -np.inf, np.float32)
    final = np.full(S, -np.inf, np.float32)
    start[[0, 1]] = 0.0
    final[[S - 2, S - 1]] = 0.0
    return dict(states=np.array(states, np.int32), arc_ptr=np.array(ptr, np.int32), arc_src=np.array(src, np.int32), arc_lp=np.array(lp, np.float32),
                start_lp=start, final_lp=final)


def pack_graphs(graphs) -> dict:
    """A call's tables from a list of graphs: statePtr [segments + 1], states, arcPtr [states + 1] GLOBAL (from 0, running
    over the segments), arcSrc LOCAL to each segment, arcLp, and startLp / finalLp [states] -- None when every graph has
    None, else the defaults (state 0 / the last state) written out where a graph has None."""
    sp, ap, st, src, lp, start, final = [0], [0], [], [], [], [], []
    any_start = any(g.get("start_lp") is not None for g in graphs)
    any_final = any(g.get("final_lp") is not None for g in graphs)
    for g in graphs:
        s = np.ascontiguousarray(g["states"], dtype=np.int32).ravel()
        p = np.ascontiguousarray(g["arc_ptr"], dtype=np.int64).ravel()
        if p.size != s.size + 1 or p[0] != 0:
            raise ValueError("a graph's arc_ptr is [states + 1] and begins at 0")
        st.append(s), sp.append(sp[-1] + s.size)
        ap.extend((ap[-1] + p[1:]).tolist())
        src.append(np.ascontiguousarray(g["arc_src"], dtype=np.int32).ravel())
        lp.append(np.ascontiguousarray(g["arc_lp"], dtype=np.float32).ravel())
        if src[-1].size != p[-1] or lp[-1].size != p[-1]:
            raise ValueError("a graph's arc_src and arc_lp are [arc_ptr[-1]]")
        for out, key, at in ((start, "start_lp", 0), (final, "final_lp", s.size - 1)):
            v = g.get(key)
            if v is None:
                v = np.full(s.size, -np.inf, np.float32)
                v[at] = 0.0
            v = np.ascontiguousarray(v, dtype=np.float32).ravel()
            if v.size != s.size:
                raise ValueError("a graph's start_lp and final_lp are [states]")
            out.append(v)
    cat = lambda parts, t: np.concatenate(parts).astype(t) if parts else np.zeros(0, t)
    return dict(statePtr=np.array(sp, np.int32), states=cat(st, np.int32), arcPtr=np.array(ap, np.int32), arcSrc=cat(src, np.int32),
                arcLp=cat(lp, np.float32), startLp=cat(start, np.float32) if any_start else None, finalLp=cat(final, np.float32) if any_final else None)


def _graph_tables(g):
    """A packed call's tables as C-contiguous vectors, shapes checked -> (sp, st, ap, src, lp, start, final)."""
    sp = np.ascontiguousarray(g["statePtr"], dtype=np.int32)
    st = np.ascontiguousarray(g["states"], dtype=np.int32)
    ap = np.ascontiguousarray(g["arcPtr"], dtype=np.int32)
    src = np.ascontiguousarray(g["arcSrc"], dtype=np.int32)
    lp = np.ascontiguousarray(g["arcLp"], dtype=np.float32)
    if sp.ndim != 1 or sp.size < 1 or st.ndim != 1 or int(sp.max()) > st.size or ap.shape != (st.size + 1,):
        raise ValueError("statePtr must be [segments + 1], states [statePtr[-1]] and arcPtr [states + 1]")
    if src.ndim != 1 or lp.shape != src.shape or (ap.size and int(ap.max()) > src.size):
        raise ValueError("arcSrc and arcLp are [arcPtr[-1]]")
    ends = []
    for key in ("startLp", "finalLp"):
        v = g.get(key)
        if v is not None:
            v = np.ascontiguousarray(v, dtype=np.float32)
            if v.shape != st.shape:
                raise ValueError("startLp and finalLp are [states]")
        ends.append(v)
    return sp, st, ap, src, lp, ends[0], ends[1]


def _graph_call_tables(segRows, g):
    sr = np.ascontiguousarray(segRows, dtype=np.int32)
    sp, st, ap, src, lp, start, final = _graph_tables(g)
    if sr.ndim != 1 or sr.size != sp.size:
        raise ValueError("segRows and statePtr must be [segments + 1]")
    return sr, sp, st, ap, src, lp, start, final, sr.size - 1, max(int(sr[-1]) - int(sr[0]), 0)


def align_graph_ref(rows, segT, rowOff, rowLd, graphs, col, stateNode=None, log_prior=None, floor: float = -np.inf, type: int = ALIGN_SCORES):
    """The graph recursion from the host restatement (``fdnn_debug_align_graph_ref``; host code, no device): rows, segT, rowOff,
    rowLd, col, stateNode, log_prior, floor and type as ``align_ref``; ``graphs`` a packed call (``pack_graphs``; its states
    are not read: col and stateNode say what a state reads) -> (path int32 [sum segT], total float32 [segments])."""
    r = np.ascontiguousarray(rows, dtype=np.float32).ravel()
    sp, _, ap, src, alp, start, final = _graph_tables(graphs)
    t, off, ld, sp = _align_rows_tables(segT, rowOff, rowLd, sp)
    c = np.ascontiguousarray(col, dtype=np.int32)
    nd = None if stateNode is None else np.ascontiguousarray(stateNode, dtype=np.int32)
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float32)
    if t.size and ((off + (t.astype(np.int64) - 1) * ld + ld > r.size).any() or (off < 0).any() or c.size < int(sp[-1])):
        raise ValueError("a segment's rows run past the rows, or col is shorter than the graphs")
    path = np.empty(int(t.astype(np.int64).sum()), np.int32)
    total = np.empty(t.size, np.float32)
    _check(lib().fdnn_debug_align_graph_ref(r.ctypes.data_as(_c_f32p), t.ctypes.data_as(_c_i32p), off.ctypes.data_as(C.POINTER(C.c_longlong)),
                                            ld.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), t.size, c.ctypes.data_as(_c_i32p), _ip(nd), _fp(lp),
                                            0 if lp is None else lp.size, C.c_float(float(floor)), int(type), _ip(ap), _ip(src), _fp(alp), _fp(start),
                                            _fp(final), path.ctypes.data_as(_c_i32p), total.ctypes.data_as(_c_f32p)))
    return path, total


def align_graph_scratch_words(segT, statePtr) -> int:
    """The 32-bit scratch words ``align_graph_rows_device`` needs for these tables under the current kernel mode
    (``fdnn_align_graph_scratch_words``): the back-pointers of the segments whose do not fit LDS."""
    t = np.ascontiguousarray(segT, dtype=np.int32)
    sp = np.ascontiguousarray(statePtr, dtype=np.int32)
    words = C.c_longlong(0)
    _check(lib().fdnn_align_graph_scratch_words(t.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), t.size, C.byref(words)))
    return int(words.value)


def align_graph_rows_device(ll, d_rows: int, segT, rowOff, rowLd, statePtr, arcPtr, d_col: int, d_state_node: int, d_arc_ptr: int, d_arc_src: int,
                            d_arc_lp: int, d_start_lp: int, d_final_lp: int, d_scratch: int, scratch_words: int, d_path: int, d_total: int,
                            stream: int = 0) -> None:
    """The graph recursion alone on device-resident fp32 rows (``fdnn_align_graph_rows_device``): host tables segT, rowOff,
    rowLd, statePtr and arcPtr, device pointers for everything they index (0 for NULL start / final values); ``ll`` a
    ``Loglik`` or None (the rows are scores).  Enqueued on ``stream``, not synchronised."""
    t, off, ld, sp = _align_rows_tables(segT, rowOff, rowLd, statePtr)
    ap = np.ascontiguousarray(arcPtr, dtype=np.int32)
    if ap.shape != (int(sp[-1]) + 1,):
        raise ValueError("arcPtr must be [states + 1]")
    _check(lib().fdnn_align_graph_rows_device(None if ll is None else ll.handle, C.c_void_p(d_rows), t.ctypes.data_as(_c_i32p),
                                              off.ctypes.data_as(C.POINTER(C.c_longlong)), ld.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p),
                                              ap.ctypes.data_as(_c_i32p), t.size, C.c_void_p(d_col), C.c_void_p(d_state_node), C.c_void_p(d_arc_ptr),
                                              C.c_void_p(d_arc_src), C.c_void_p(d_arc_lp), C.c_void_p(d_start_lp), C.c_void_p(d_final_lp),
                                              C.c_void_p(d_scratch), int(scratch_words), C.c_void_p(d_path), C.c_void_p(d_total), C.c_void_p(stream)))


def align_graph_launches():
    """Process-wide counts since load: (launches of the align-graph kernel's wave form, of its workgroup form)."""
    buf = (C.c_ulonglong * 2)()
    if lib().fdnn_debug_align_graph_launches(buf, 2) != 2:
        raise RuntimeError("fdnn_debug_align_graph_launches")
    return tuple(int(v) for v in buf)


def set_align_graph_kernel(mode: int) -> None:
    """Process-wide (``fdnn_debug_set_align_graph_kernel``): 0 the plan's rule (the wave form up to 64 states), 1 the wave form
    where allowed (up to 256), 2 always the workgroup form."""
    _check(lib().fdnn_debug_set_align_graph_kernel(int(mode)))


def align_graph_limits() -> dict:
    """The align-graph kernels' limits as built (``fdnn_debug_align_graph_limits``)."""
    buf = (C.c_int * 8)()
    if lib().fdnn_debug_align_graph_limits(buf, 8) != 8:
        raise RuntimeError("fdnn_debug_align_graph_limits")
    return dict(zip(("max_states", "segs_per_launch", "wave_states", "max_arcs", "lds_arcs", "lds_bp_words", "scratch_cap_mib", "wave_rule_states"),
                    (int(v) for v in buf)))


# ---------------------------------------------------------------- alignment graphs, summed (fdnn_fb.hip)
# The graphs are the alignment graphs' (chain_graph, optional_silence_graph, pack_graphs); the results are the total
# likelihood ln(sum over paths) per segment and the occupancies gamma, flat float32 [sum of T S]: segment s's block is
# row-major [T_s][S_s] (``fb_gamma_blocks`` cuts it).
FB_EXP_NEG, FB_LADD = 0, 1


def fb_transpose(graphs) -> dict:
    """The transposed tables of a packed call (``fdnn_fb_transpose``; host code): a stable counting sort of every segment's arcs
    by source -> dict(tPtr [states + 1] global, tSrc [arcs] the DESTINATION local to the segment, tLp [arcs])."""
    sp, _, ap, src, lp, _, _ = _graph_tables(graphs)
    tp = np.zeros(ap.size, np.int32)
    ts = np.zeros(src.size, np.int32)
    tl = np.zeros(src.size, np.float32)
    _check(lib().fdnn_fb_transpose(_ip(sp), sp.size - 1, _ip(ap), _ip(src), _fp(lp), _ip(tp), _ip(ts), _fp(tl)))
    return dict(tPtr=tp, tSrc=ts, tLp=tl)


def fb_gamma_blocks(gamma, segT, statePtr):
    """The flat occupancies cut into one [T][S] view per segment."""
    t = np.asarray(segT, dtype=np.int64)
    S = np.diff(np.asarray(statePtr, dtype=np.int64))
    off = np.concatenate([[0], np.cumsum(t * S)])
    return [gamma[off[s]:off[s + 1]].reshape(int(t[s]), int(S[s])) for s in range(t.size)]


def fb_ref(rows, segT, rowOff, rowLd, graphs, col, stateNode=None, log_prior=None, floor: float = -np.inf, type: int = ALIGN_SCORES,
           want_gamma: bool = True, transposed=None):
    """Forward-backward from the host restatement (``fdnn_debug_fb_ref``; host code, no device): the arguments of
    ``align_graph_ref``; ``transposed`` the dict of ``fb_transpose`` (made here when None) -> (total float32 [segments], gamma
    float32 [sum of T S], or None unless ``want_gamma``)."""
    r = np.ascontiguousarray(rows, dtype=np.float32).ravel()
    sp, _, ap, src, alp, start, final = _graph_tables(graphs)
    t, off, ld, sp = _align_rows_tables(segT, rowOff, rowLd, sp)
    c = np.ascontiguousarray(col, dtype=np.int32)
    nd = None if stateNode is None else np.ascontiguousarray(stateNode, dtype=np.int32)
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float32)
    if t.size and ((off + (t.astype(np.int64) - 1) * ld + ld > r.size).any() or (off < 0).any() or c.size < int(sp[-1])):
        raise ValueError("a segment's rows run past the rows, or col is shorter than the graphs")
    total = np.empty(t.size, np.float32)
    gamma = tp = ts = tl = None
    if want_gamma:
        tr = fb_transpose(graphs) if transposed is None else transposed
        tp = np.ascontiguousarray(tr["tPtr"], dtype=np.int32)
        ts = np.ascontiguousarray(tr["tSrc"], dtype=np.int32)
        tl = np.ascontiguousarray(tr["tLp"], dtype=np.float32)
        if tp.shape != ap.shape or ts.shape != src.shape or tl.shape != src.shape:
            raise ValueError("the transposed tables have the shapes of the arc tables")
        gamma = np.empty(int((t.astype(np.int64) * np.diff(sp.astype(np.int64))).sum()), np.float32)
    _check(lib().fdnn_debug_fb_ref(r.ctypes.data_as(_c_f32p), t.ctypes.data_as(_c_i32p), off.ctypes.data_as(C.POINTER(C.c_longlong)),
                                   ld.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), t.size, c.ctypes.data_as(_c_i32p), _ip(nd), _fp(lp),
                                   0 if lp is None else lp.size, C.c_float(float(floor)), int(type), _ip(ap), _ip(src), _fp(alp), _fp(start),
                                   _fp(final), _ip(tp), _ip(ts), _fp(tl), total.ctypes.data_as(_c_f32p), _fp(gamma)))
    return total, gamma


def fb_scratch_words(segT, statePtr, want_gamma: bool = True) -> int:
    """The fp32 scratch words ``fb_rows_device`` needs for these tables (``fdnn_fb_scratch_words``): the lattice, T S words a
    segment where gamma is wanted, else 0."""
    t = np.ascontiguousarray(segT, dtype=np.int32)
    sp = np.ascontiguousarray(statePtr, dtype=np.int32)
    words = C.c_longlong(0)
    _check(lib().fdnn_fb_scratch_words(t.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), t.size, int(bool(want_gamma)), C.byref(words)))
    return int(words.value)


def fb_rows_device(ll, d_rows: int, segT, rowOff, rowLd, statePtr, arcPtr, tPtr, d_col: int, d_state_node: int, d_arc_ptr: int, d_arc_src: int,
                   d_arc_lp: int, d_start_lp: int, d_final_lp: int, d_t_ptr: int, d_t_src: int, d_t_lp: int, d_scratch: int, scratch_words: int,
                   d_total: int, d_gamma: int, stream: int = 0) -> None:
    """The sweeps alone on device-resident fp32 rows (``fdnn_fb_rows_device``): host tables segT, rowOff, rowLd, statePtr,
    arcPtr and tPtr (None without gamma), device pointers for everything they index (0 for NULL); ``d_gamma`` 0 = forward
    only; ``ll`` a ``Loglik`` or None (the rows are scores).  Enqueued on ``stream``, not synchronised."""
    t, off, ld, sp = _align_rows_tables(segT, rowOff, rowLd, statePtr)
    ap = np.ascontiguousarray(arcPtr, dtype=np.int32)
    tp = None if tPtr is None else np.ascontiguousarray(tPtr, dtype=np.int32)
    if ap.shape != (int(sp[-1]) + 1,) or (tp is not None and tp.shape != ap.shape):
        raise ValueError("arcPtr and tPtr must be [states + 1]")
    _check(lib().fdnn_fb_rows_device(None if ll is None else ll.handle, C.c_void_p(d_rows), t.ctypes.data_as(_c_i32p),
                                     off.ctypes.data_as(C.POINTER(C.c_longlong)), ld.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p),
                                     ap.ctypes.data_as(_c_i32p), _ip(tp), t.size, C.c_void_p(d_col), C.c_void_p(d_state_node), C.c_void_p(d_arc_ptr),
                                     C.c_void_p(d_arc_src), C.c_void_p(d_arc_lp), C.c_void_p(d_start_lp), C.c_void_p(d_final_lp), C.c_void_p(d_t_ptr),
                                     C.c_void_p(d_t_src), C.c_void_p(d_t_lp), C.c_void_p(d_scratch), int(scratch_words), C.c_void_p(d_total),
                                     C.c_void_p(d_gamma), C.c_void_p(stream)))


def fb_launches():
    """Process-wide counts since load: launches (forward wave form, forward workgroup form, backward wave, backward workgroup)."""
    buf = (C.c_ulonglong * 4)()
    if lib().fdnn_debug_fb_launches(buf, 4) != 4:
        raise RuntimeError("fdnn_debug_fb_launches")
    return tuple(int(v) for v in buf)


def set_fb_kernel(mode: int) -> None:
    """Process-wide (``fdnn_debug_set_fb_kernel``): 0 the plan's rule, 1 the wave form where allowed (up to 256 states), 2
    always the workgroup form."""
    _check(lib().fdnn_debug_set_fb_kernel(int(mode)))


def fb_limits() -> dict:
    """The forward-backward kernels' limits as built (``fdnn_debug_fb_limits``)."""
    buf = (C.c_int * 8)()
    if lib().fdnn_debug_fb_limits(buf, 8) != 8:
        raise RuntimeError("fdnn_debug_fb_limits")
    return dict(zip(("max_states", "segs_per_launch", "wave_states", "max_arcs", "lds_arcs", "partials", "scratch_cap_mib", "wave_rule_states"),
                    (int(v) for v in buf)))


def fb_math_ref(op: int, a, b=None):
    """The stated functions on the host (``fdnn_debug_fb_math_ref``): op FB_EXP_NEG -> exp_neg(a), FB_LADD -> ladd(a, b)."""
    x = np.ascontiguousarray(a, dtype=np.float32).ravel()
    y = None if b is None else np.ascontiguousarray(b, dtype=np.float32).ravel()
    if y is not None and y.size != x.size:
        raise ValueError("a and b have one size")
    out = np.empty(x.size, np.float32)
    _check(lib().fdnn_debug_fb_math_ref(int(op), _fp(x), _fp(y), _fp(out), x.size))
    return out


def fb_math_device(op: int, d_a: int, d_b: int, d_out: int, n: int, stream: int = 0) -> None:
    """The same over device arrays in a trivial kernel (``fdnn_debug_fb_math_device``), enqueued on ``stream``."""
    _check(lib().fdnn_debug_fb_math_device(int(op), C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_out), int(n), C.c_void_p(stream)))


def _fb_out(n_segs: int, segRows, sp, want_gamma: bool):
    total = np.empty(n_segs, np.float32)
    words = int((np.diff(segRows.astype(np.int64)) * np.diff(sp.astype(np.int64))).sum()) if n_segs else 0
    return total, (np.empty(words, np.float32) if want_gamma else None)


def _loglik_out(n: int, ll: "Loglik", out):
    """The [n][width] result array of a loglik call, made or checked."""
    shape = (n, ll.width())
    if out is None:
        return np.empty(shape, dtype=ll.dtype)
    if out.dtype != ll.dtype or out.shape != shape or not out.flags.c_contiguous:
        raise ValueError(f"out must be a C-contiguous {np.dtype(ll.dtype).name} array of shape {shape}")
    return out


def _topk_out(n: int, k: int, nodes, probs):
    """The [n][k] result arrays of a top-k call, made or checked."""
    if nodes is None:
        nodes = np.empty((n, k), dtype=np.int32)
    elif nodes.dtype != np.int32 or nodes.shape != (n, k) or not nodes.flags.c_contiguous:
        raise ValueError(f"nodes must be a C-contiguous int32 array of shape {(n, k)}")
    if probs is None:
        probs = np.empty((n, k), dtype=np.float32)
    elif probs.dtype != np.float32 or probs.shape != (n, k) or not probs.flags.c_contiguous:
        raise ValueError(f"probs must be a C-contiguous float32 array of shape {(n, k)}")
    return nodes, probs


def _sets(segRows, setPtr, nodes):
    """(seg_rows, set_ptr, nodes) as C-contiguous int32 vectors of the shapes every sets entry point needs -> them, the
    segment count, the rows and the floats of probs."""
    sr = np.ascontiguousarray(segRows, dtype=np.int32)
    sp = np.ascontiguousarray(setPtr, dtype=np.int32)
    nd = np.ascontiguousarray(nodes, dtype=np.int32)
    if sr.ndim != 1 or sp.ndim != 1 or nd.ndim != 1 or sr.size != sp.size or sr.size < 1:
        raise ValueError("segRows and setPtr must be [segments + 1] and nodes [setPtr[-1]]")
    if sp.size and int(sp.max()) > nd.size:  # (the C side reads setPtr[segments] nodes)
        raise ValueError(f"setPtr reaches {int(sp.max())} but there are {nd.size} nodes")
    rows = max(int(sr[-1]) - int(sr[0]), 0)
    nnz = int((np.maximum(np.diff(sr.astype(np.int64)), 0) * np.maximum(np.diff(sp.astype(np.int64)), 0)).sum())
    return sr, sp, nd, sr.size - 1, rows, nnz


def sets_check(segRows, setPtr, nodes, outputDimension: int, contextRows: int) -> int:
    """The validator of the sets entry points (``fdnn_debug_sets_check``; host code, no device): 0, or -(s + 1) of the first
    malformed segment s (malformed tables as a whole answer as segment 0)."""
    sr = np.ascontiguousarray(segRows, dtype=np.int32)
    sp = np.ascontiguousarray(setPtr, dtype=np.int32)
    nd = np.ascontiguousarray(nodes, dtype=np.int32)
    if sr.ndim != 1 or sp.ndim != 1 or nd.ndim != 1 or sr.size != sp.size or sr.size < 1:
        raise ValueError("segRows and setPtr must be [segments + 1] and nodes [setPtr[-1]]")
    if sp.size > 1 and int(sp.max()) > nd.size:  # never let the C side read past the node array
        return -(int(np.argmax(sp[1:] > nd.size)) + 1)
    return int(lib().fdnn_debug_sets_check(sr.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), nd.ctypes.data_as(_c_i32p), sr.size - 1,
                                           int(outputDimension), int(contextRows)))


def sets_launches():
    """Process-wide counts since load: (launches of the segmented MFMA kernel without the pair walk, with it, calls served
    by the list kernels)."""
    buf = (C.c_ulonglong * 3)()
    if lib().fdnn_debug_sets_launches(buf, 3) != 3:
        raise RuntimeError("fdnn_debug_sets_launches")
    return tuple(int(v) for v in buf)


class LazyContext:
    """``QuantizedDnn.LazyContext`` (QuantizedDnn.java:72-98)."""

    def __init__(self, dnn: "QuantizedDnn", handle: int, input_vector_count: int, owned: bool = True):
        self.dnn = dnn
        self.handle = handle
        self.inputVectorCount = input_vector_count
        self.currentVectorIndex = 0
        self._owned = owned  # False: a view of a context that belongs to a SpliceStream

    def calculateUntilOutput(self, input) -> None:
        x = _f32(input)
        if x.shape != (self.inputVectorCount, self.dnn.inputDimension()):
            raise ValueError(f"expected {self.inputVectorCount}x{self.dnn.inputDimension()} frames, got {x.shape}")
        _check(lib().fdnn_ctx_forward_hidden(self.handle, x.ctypes.data_as(_c_f32p)))

    def calculateUntilOutputRaw(self, raw) -> None:
        """calculateUntilOutput on the context's inputVectorCount RAW frames of one utterance, spliced on the device
        (QuantizedDnn.setSplice): the same hidden activations as calculateUntilOutput on the host-spliced rows."""
        r = _f32(raw)
        spec = self.dnn.spliceSpec()
        if spec is not None and r.shape != (self.inputVectorCount, spec[1]):
            raise ValueError(f"expected {self.inputVectorCount}x{spec[1]} raw frames, got {r.shape}")
        _check(lib().fdnn_ctx_forward_hidden_raw(self.handle, r.ctypes.data_as(_c_f32p)))

    def calculateForOutputNodes(self, activeNodesMask) -> np.ndarray:
        mask = np.ascontiguousarray(activeNodesMask, dtype=np.int8)
        if mask.shape != (self.dnn.outputDimension(),):
            raise ValueError("mask length must equal the output dimension")
        out = np.empty(self.dnn.outputDimension(), dtype=np.float32)
        _check(lib().fdnn_ctx_lazy_output(self.handle, self.currentVectorIndex, mask.ctypes.data_as(_c_i8p),
                                          out.ctypes.data_as(_c_f32p)))
        self.currentVectorIndex += 1
        return out

    # batched form of the same contract
    def calculateForOutputNodesBatch(self, masks, first: int = 0) -> np.ndarray:
        masks = np.ascontiguousarray(masks, dtype=np.int8)
        if masks.ndim != 2 or masks.shape[1] != self.dnn.outputDimension():  # the C side reads count x output_dim bytes
            raise ValueError(f"masks must be count x {self.dnn.outputDimension()}, got {masks.shape}")
        count = masks.shape[0]
        if first < 0 or first + count > self.inputVectorCount:
            raise ValueError(f"frames [{first}, {first + count}) outside the context's {self.inputVectorCount} frames")
        out = np.empty((count, self.dnn.outputDimension()), dtype=np.float32)
        _check(lib().fdnn_ctx_lazy_output_batch(self.handle, first, count, masks.ctypes.data_as(_c_i8p),
                                                out.ctypes.data_as(_c_f32p)))
        return out

    def calculateForOutputNodesLists(self, rowPtr, nodes, first: int = 0):
        """Lazy output for the LISTED nodes only (``fdnn_ctx_lazy_output_lists``): rows first .. first + count - 1,
        rowPtr int32 [count + 1], nodes int32 [nnz] ascending inside a row -> (probs [nnz], inactive [count]): the listed
        nodes' probabilities and, per row, the value every unlisted node reads (``formats.lists_to_rows`` rebuilds rows)."""
        rp, nd = _lists(rowPtr, nodes)
        probs = np.empty(int(rp[-1]) if rp[-1] > 0 else 0, dtype=np.float32)
        inactive = np.empty(rp.size - 1, dtype=np.float32)
        _check(lib().fdnn_ctx_lazy_output_lists(self.handle, int(first), rp.size - 1, rp.ctypes.data_as(_c_i32p), nd.ctypes.data_as(_c_i32p),
                                                probs.ctypes.data_as(_c_f32p), inactive.ctypes.data_as(_c_f32p)))
        return probs, inactive

    def calculateForOutputNodesListsDevice(self, d_rowPtr: int, d_nodes: int, nnz: int, d_probs: int, d_inactive: int, first: int, count: int,
                                           stream: int = 0) -> None:
        """The same on device buffers, enqueued on ``stream``, not synchronised; the lists are not validated (fdnn.h)."""
        _check(lib().fdnn_ctx_lazy_output_lists_device(self.handle, int(first), int(count), C.c_void_p(d_rowPtr), C.c_void_p(d_nodes), int(nnz),
                                                       C.c_void_p(d_probs), C.c_void_p(d_inactive), C.c_void_p(stream)))

    def listsAccumulators(self, rowPtr, nodes, first: int = 0) -> np.ndarray:
        """Parity tests: the int32 accumulators of the listed entries as the score kernel holds them (``fdnn_debug_ctx_lists_acc``)."""
        rp, nd = _lists(rowPtr, nodes)
        acc = np.zeros(max(int(rp[-1]), 0), dtype=np.int32)
        _check(lib().fdnn_debug_ctx_lists_acc(self.handle, int(first), rp.size - 1, rp.ctypes.data_as(_c_i32p), nd.ctypes.data_as(_c_i32p),
                                              acc.ctypes.data_as(_c_i32p)))
        return acc

    def listsUnion(self, rowPtr, nodes, group_tiles: int, first: int = 0):
        """Tests: the union-build kernel of the union path alone (``fdnn_debug_ctx_lists_union``) -> (u_len, u_nodes, pos) as
        ``lists_union_ref`` lays them out."""
        rp, nd = _lists(rowPtr, nodes)
        u_len, u_nodes, pos = _union_buffers(rp, group_tiles)
        _check(lib().fdnn_debug_ctx_lists_union(self.handle, int(first), rp.size - 1, rp.ctypes.data_as(_c_i32p), nd.ctypes.data_as(_c_i32p), int(group_tiles),
                                                u_len.ctypes.data_as(_c_i32p), u_nodes.ctypes.data_as(_c_i32p), pos.ctypes.data_as(_c_i32p)))
        return u_len, u_nodes, pos

    def calculateForOutputNodeSet(self, nodes, first: int = 0, count=None):
        """Lazy output for ONE node set shared by rows first .. first + count - 1 (``fdnn_ctx_lazy_output_set``; count: up
        to the context's last row): nodes int32 [len] ascending -> (probs [count][len], inactive [count]), the bytes of
        ``calculateForOutputNodesLists`` with the set as every row's list."""
        nd = _set(nodes)
        count = self.inputVectorCount - int(first) if count is None else int(count)
        probs = np.empty((max(count, 0), nd.size), dtype=np.float32)
        inactive = np.empty(max(count, 0), dtype=np.float32)
        _check(lib().fdnn_ctx_lazy_output_set(self.handle, int(first), count, nd.ctypes.data_as(_c_i32p), nd.size, probs.ctypes.data_as(_c_f32p),
                                              inactive.ctypes.data_as(_c_f32p)))
        return probs, inactive

    def calculateForOutputNodeSetDevice(self, d_nodes: int, length: int, d_probs: int, d_inactive: int, first: int, count: int, stream: int = 0) -> None:
        """The same on device buffers, enqueued on ``stream``, not synchronised; the set is not validated (fdnn.h)."""
        _check(lib().fdnn_ctx_lazy_output_set_device(self.handle, int(first), int(count), C.c_void_p(d_nodes), int(length), C.c_void_p(d_probs),
                                                     C.c_void_p(d_inactive), C.c_void_p(stream)))

    def setAccumulators(self, nodes, first: int = 0, count=None) -> np.ndarray:
        """Parity tests: the int32 accumulators [count][len] as the set kernel holds them (``fdnn_debug_ctx_set_acc``)."""
        nd = _set(nodes)
        count = self.inputVectorCount - int(first) if count is None else int(count)
        acc = np.zeros((max(count, 0), nd.size), dtype=np.int32)
        _check(lib().fdnn_debug_ctx_set_acc(self.handle, int(first), count, nd.ctypes.data_as(_c_i32p), nd.size, acc.ctypes.data_as(_c_i32p)))
        return acc

    def calculateForOutputNodeSets(self, segRows, setPtr, nodes):
        """Lazy output with one node set per SEGMENT of a row range, all in one call (``fdnn_ctx_lazy_output_sets``):
        segment s is rows segRows[s] .. segRows[s + 1] - 1 with the set nodes[setPtr[s]:setPtr[s + 1]] -> (probs, flat: segment
        s's block [rows_s][len_s] after the blocks before it, inactive [rows]); ``formats.sets_to_lists`` gives the same
        layout as lists.  A row's bytes are those of ``calculateForOutputNodeSet`` on its segment alone."""
        sr, sp, nd, n_segs, rows, nnz = _sets(segRows, setPtr, nodes)
        probs = np.empty(nnz, dtype=np.float32)
        inactive = np.empty(rows, dtype=np.float32)
        _check(lib().fdnn_ctx_lazy_output_sets(self.handle, sr.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), n_segs, nd.ctypes.data_as(_c_i32p),
                                               probs.ctypes.data_as(_c_f32p), inactive.ctypes.data_as(_c_f32p)))
        return probs, inactive

    def calculateForOutputNodeSetsDevice(self, segRows, setPtr, d_nodes: int, d_probs: int, d_inactive: int, stream: int = 0) -> None:
        """The same on device buffers, enqueued on ``stream``, not synchronised; the tables are host arrays and are read before
        the call returns, the sets are not validated (fdnn.h)."""
        sr = np.ascontiguousarray(segRows, dtype=np.int32)
        sp = np.ascontiguousarray(setPtr, dtype=np.int32)
        if sr.ndim != 1 or sp.ndim != 1 or sr.size != sp.size or sr.size < 1:
            raise ValueError("segRows and setPtr must be [segments + 1]")
        _check(lib().fdnn_ctx_lazy_output_sets_device(self.handle, sr.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), sr.size - 1,
                                                      C.c_void_p(d_nodes), C.c_void_p(d_probs), C.c_void_p(d_inactive), C.c_void_p(stream)))

    def setsAccumulators(self, segRows, setPtr, nodes) -> np.ndarray:
        """Parity tests: the int32 accumulators, flat and ragged like probs, as the kernel holds them (``fdnn_debug_ctx_sets_acc``)."""
        sr, sp, nd, n_segs, rows, nnz = _sets(segRows, setPtr, nodes)
        acc = np.zeros(nnz, dtype=np.int32)
        _check(lib().fdnn_debug_ctx_sets_acc(self.handle, sr.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), n_segs, nd.ctypes.data_as(_c_i32p),
                                             acc.ctypes.data_as(_c_i32p)))
        return acc

    def calculateOutputTopK(self, k: int):
        """The dense output layer over the context's frames, of which only the k first-ranked nodes of every frame and their
        probabilities come back (``fdnn_ctx_output_topk``) -> (nodes int32 [frames][k], probs float32 [frames][k])."""
        nodes, probs = _topk_out(self.inputVectorCount, int(k), None, None)
        _check(lib().fdnn_ctx_output_topk(self.handle, int(k), nodes.ctypes.data_as(_c_i32p), probs.ctypes.data_as(_c_f32p)))
        return nodes, probs

    def calculateOutputTopKDevice(self, k: int, d_nodes: int, d_probs: int, stream: int = 0) -> None:
        """The same into device buffers [frames][k], enqueued on ``stream``, not synchronised (``fdnn_ctx_output_topk_device``)."""
        _check(lib().fdnn_ctx_output_topk_device(self.handle, int(k), C.c_void_p(d_nodes), C.c_void_p(d_probs), C.c_void_p(stream)))

    def calculateOutputPool(self, pool: "ClassPool") -> np.ndarray:
        """The dense output layer over the context's frames, of which only the class sums under ``pool`` come back
        (``fdnn_ctx_output_pool``) -> float32 [frames][classes]."""
        out = _pool_out(self.inputVectorCount, pool.classes(), None)
        _check(lib().fdnn_ctx_output_pool(self.handle, pool.handle, out.ctypes.data_as(_c_f32p)))
        return out

    def calculateOutputLoglik(self, ll: "Loglik") -> np.ndarray:
        """The dense output layer over the context's frames as decoder scores under ``ll`` (``fdnn_ctx_output_loglik``) ->
        float32 or float16 [frames][outputDimension]."""
        out = _loglik_out(self.inputVectorCount, ll, None)
        _check(lib().fdnn_ctx_output_loglik(self.handle, ll.handle, C.c_void_p(out.ctypes.data)))
        return out

    def align(self, ll: "Loglik", segRows, statePtr, states, selfLp=None, nextLp=None):
        """Forced alignment over rows of the context (``fdnn_ctx_align``): segment s = rows [segRows[s], segRows[s + 1]) with the
        transcript states[statePtr[s] .. statePtr[s + 1]) and optional transition scores -> (path int32 [rows], total float32
        [segments]); a segment without a finite total has -1 everywhere."""
        sr, sp, st, sl, nl, n_segs, rows = _align_tables(segRows, statePtr, states, selfLp, nextLp)
        path = np.empty(rows, np.int32)
        total = np.empty(n_segs, np.float32)
        _check(lib().fdnn_ctx_align(self.handle, ll.handle, sr.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), n_segs, st.ctypes.data_as(_c_i32p),
                                    _fp(sl), _fp(nl), path.ctypes.data_as(_c_i32p), total.ctypes.data_as(_c_f32p)))
        return path, total

    def alignDevice(self, ll: "Loglik", segRows, statePtr, states, d_path: int, d_total: int, selfLp=None, nextLp=None, stream: int = 0) -> None:
        """The same with device result buffers, enqueued on ``stream`` and not synchronised (``fdnn_ctx_align_device``)."""
        sr, sp, st, sl, nl, n_segs, _ = _align_tables(segRows, statePtr, states, selfLp, nextLp)
        _check(lib().fdnn_ctx_align_device(self.handle, ll.handle, sr.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), n_segs,
                                           st.ctypes.data_as(_c_i32p), _fp(sl), _fp(nl), C.c_void_p(d_path), C.c_void_p(d_total), C.c_void_p(stream)))

    def alignGraph(self, ll: "Loglik", segRows, graphs):
        """The best path over alignment graphs, over rows of the context (``fdnn_ctx_align_graph``): segment s = rows
        [segRows[s], segRows[s + 1]) with graph s of the packed call ``graphs`` (``pack_graphs``) -> (path int32 [rows], total
        float32 [segments]); a segment without a finite total has -1 everywhere."""
        sr, sp, st, ap, src, lp, start, final, n_segs, rows = _graph_call_tables(segRows, graphs)
        path = np.empty(rows, np.int32)
        total = np.empty(n_segs, np.float32)
        _check(lib().fdnn_ctx_align_graph(self.handle, ll.handle, _ip(sr), _ip(sp), n_segs, _ip(st), _ip(ap), _ip(src), _fp(lp), _fp(start), _fp(final),
                                          path.ctypes.data_as(_c_i32p), total.ctypes.data_as(_c_f32p)))
        return path, total

    def alignGraphDevice(self, ll: "Loglik", segRows, graphs, d_path: int, d_total: int, stream: int = 0) -> None:
        """The same with device result buffers, enqueued on ``stream`` and not synchronised (``fdnn_ctx_align_graph_device``)."""
        sr, sp, st, ap, src, lp, start, final, n_segs, _ = _graph_call_tables(segRows, graphs)
        _check(lib().fdnn_ctx_align_graph_device(self.handle, ll.handle, _ip(sr), _ip(sp), n_segs, _ip(st), _ip(ap), _ip(src), _fp(lp), _fp(start),
                                                 _fp(final), C.c_void_p(d_path), C.c_void_p(d_total), C.c_void_p(stream)))

    def forwardBackward(self, ll: "Loglik", segRows, graphs, want_gamma: bool = True):
        """The total likelihood ln(sum over paths) and the state occupancies of alignment graphs, over rows of the context
        (``fdnn_ctx_fb``): segment s = rows [segRows[s], segRows[s + 1]) with graph s of the packed call ``graphs`` -> (total
        float32 [segments], gamma float32 [sum of T S] -- ``fb_gamma_blocks`` cuts it -- or None unless ``want_gamma``:
        forward only)."""
        sr, sp, st, ap, src, lp, start, final, n_segs, _ = _graph_call_tables(segRows, graphs)
        total, gamma = _fb_out(n_segs, sr, sp, want_gamma)
        _check(lib().fdnn_ctx_fb(self.handle, ll.handle, _ip(sr), _ip(sp), n_segs, _ip(st), _ip(ap), _ip(src), _fp(lp), _fp(start), _fp(final),
                                 _fp(total), _fp(gamma)))
        return total, gamma

    def forwardBackwardDevice(self, ll: "Loglik", segRows, graphs, d_total: int, d_gamma: int = 0, stream: int = 0) -> None:
        """The same with device result buffers (``d_gamma`` 0: forward only), enqueued on ``stream`` and not synchronised
        (``fdnn_ctx_fb_device``)."""
        sr, sp, st, ap, src, lp, start, final, n_segs, _ = _graph_call_tables(segRows, graphs)
        _check(lib().fdnn_ctx_fb_device(self.handle, ll.handle, _ip(sr), _ip(sp), n_segs, _ip(st), _ip(ap), _ip(src), _fp(lp), _fp(start), _fp(final),
                                        C.c_void_p(d_total), C.c_void_p(d_gamma), C.c_void_p(stream)))

    def calculateOutputLoglikDevice(self, ll: "Loglik", d_out: int, stream: int = 0) -> None:
        """The same into a device buffer [frames][outputDimension] of the handle's type, enqueued on ``stream``, not
        synchronised (``fdnn_ctx_output_loglik_device``)."""
        _check(lib().fdnn_ctx_output_loglik_device(self.handle, ll.handle, C.c_void_p(d_out), C.c_void_p(stream)))

    def calculateOutputPoolDevice(self, pool: "ClassPool", d_out: int, stream: int = 0) -> None:
        """The same into a device buffer [frames][classes], enqueued on ``stream``, not synchronised (``fdnn_ctx_output_pool_device``)."""
        _check(lib().fdnn_ctx_output_pool_device(self.handle, pool.handle, C.c_void_p(d_out), C.c_void_p(stream)))

    # device-resident forms (raw device pointers, e.g. ``tensor.data_ptr()``; enqueued on ``stream``)
    def calculateForOutputNodesBatchBits(self, bits, first: int = 0, out=None) -> np.ndarray:
        """Batched lazy output with the masks as bits: uint64 [count][ceil(O / 64)] (formats.pack_mask_bits).
        ``out``: a resident float32 [count][O] array to fill (a JVM caller's float[] would be)."""
        b = np.ascontiguousarray(bits, dtype=np.uint64)
        O = self.dnn.outputDimension()
        if b.ndim != 2 or b.shape[1] != (O + 63) // 64:
            raise ValueError("bits must be [count][ceil(outputDimension / 64)] uint64")
        if out is None:
            out = np.empty((b.shape[0], O), dtype=np.float32)
        elif out.dtype != np.float32 or out.shape != (b.shape[0], O) or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous float32 [count][outputDimension] array")
        _check(lib().fdnn_ctx_lazy_output_batch_bits(self.handle, first, b.shape[0], b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def calculateForOutputNodesBatchBitsDevice(self, d_bits: int, d_out: int, first: int, count: int, stream: int = 0) -> None:
        _check(lib().fdnn_ctx_lazy_output_batch_bits_device(self.handle, first, count, C.c_void_p(d_bits), C.c_void_p(d_out), C.c_void_p(stream)))

    def calculateUntilOutputDevice(self, d_input: int, stream: int = 0) -> None:
        _check(lib().fdnn_ctx_forward_hidden_device(self.handle, C.c_void_p(d_input), C.c_void_p(stream)))

    def calculateForOutputNodesBatchDevice(self, d_masks: int, d_out: int, first: int, count: int, stream: int = 0) -> None:
        _check(lib().fdnn_ctx_lazy_output_batch_device(self.handle, first, count, C.c_void_p(d_masks), C.c_void_p(d_out),
                                                       C.c_void_p(stream)))

    def chainClocks(self, cap_tasks: int, fetch: bool = False):
        """Measurement builds (-DFDNN_CHAIN_CLK=1): arm (fetch=False) / read the chained kernel's per-task phase clocks."""
        if not fetch:
            _check(lib().fdnn_debug_chain_clocks(self.handle, None, int(cap_tasks)))
            return None
        buf = np.zeros(8 + 10 * int(cap_tasks), dtype=np.int64)
        _check(lib().fdnn_debug_chain_clocks(self.handle, buf.ctypes.data_as(C.POINTER(C.c_longlong)), int(cap_tasks)))
        k = int(buf[0] & 0xffffffff)
        return buf[8:8 + 10 * min(k, int(cap_tasks))].reshape(-1, 10)

    def calculateOutput(self) -> np.ndarray:
        """The dense output layer over the context's frames (``fdnn_ctx_output``) -> the soft-max rows [frames][outputDimension]."""
        out = np.empty((self.inputVectorCount, self.dnn.outputDimension()), dtype=np.float32)
        _check(lib().fdnn_ctx_output(self.handle, out.ctypes.data_as(_c_f32p)))
        return out

    def scratchState(self) -> dict:
        """The scratch audit of this context (``fdnn_debug_ctx_scratch``): waits for its last work -> {buffer name: non-zero
        words}, every value 0 between launches."""
        names = scratch_names()
        buf = (C.c_ulonglong * len(names))()
        _check(lib().fdnn_debug_ctx_scratch(self.handle, buf, len(names)))
        return {k: int(buf[i]) for i, k in enumerate(names)}

    def scratchWords(self) -> dict:
        """{buffer name: its length in 32-bit words}."""
        names = scratch_names()
        buf = (C.c_ulonglong * len(names))()
        _check(lib().fdnn_debug_ctx_scratch_words(self.handle, buf, len(names)))
        return {k: int(buf[i]) for i, k in enumerate(names)}

    def scratchPoke(self, name: str, index: int, value: int) -> None:
        """The audit's self-test only: writes one word of a scratch buffer.  Never launch on a context poked non-zero."""
        _check(lib().fdnn_debug_ctx_scratch_poke(self.handle, scratch_names().index(name), int(index), int(value)))

    def hiddenActivations(self) -> np.ndarray:
        out = np.empty((self.inputVectorCount, self.dnn.hiddenDimension()), dtype=np.uint8)
        _check(lib().fdnn_ctx_read_hidden(self.handle, out.ctypes.data_as(_c_u8p)))
        return out

    def delete(self) -> None:
        if self.handle and self._owned:
            lib().fdnn_ctx_free(self.handle)
        self.handle = None


class SpliceStream:
    """An utterance scored as its raw frames arrive (``fdnn_stream_*``): every push returns the rows it completes, in
    order; ``end=True`` flushes the rest, right-clamped to the last frame.  Made by ``QuantizedDnn.newStream``; it keeps
    the model's splice spec of that moment."""

    def __init__(self, dnn: "QuantizedDnn", maxChunk: int):
        spec = dnn.spliceSpec()
        h = C.c_void_p()
        _check(lib().fdnn_stream_create(dnn.nativeDnnHandle, int(maxChunk), C.byref(h)))
        self.handle = h.value
        self.dnn = dnn
        self.maxChunk = int(maxChunk)
        self.offsets, self.rawDim = spec
        self.right = max(0, max(self.offsets))

    def _push(self, raw, end: bool, out):
        r = np.ascontiguousarray(raw, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] != self.rawDim:
            raise ValueError(f"raw frames must be [n][{self.rawDim}], got {r.shape}")
        n = C.c_int(0)
        _check(lib().fdnn_stream_push(self.handle, r.ctypes.data_as(_c_f32p), r.shape[0], int(bool(end)),
                                      out.ctypes.data_as(_c_f32p) if out is not None else None, C.byref(n)))
        return int(n.value)

    def push(self, raw, end: bool = False) -> np.ndarray:
        """raw [n][rawDim] -> the soft-max rows of the frames this push completes ([k][outputDimension])."""
        out = np.empty((len(raw) + self.right, self.dnn.outputDimension()), dtype=np.float32)
        return out[:self._push(raw, end, out)]

    def pushHidden(self, raw, end: bool = False) -> LazyContext:
        """Hidden layers only: a LazyContext view whose frames are exactly the frames this push completes (valid until
        the next push; the stream owns it)."""
        k = self._push(raw, end, None)
        return LazyContext(self.dnn, lib().fdnn_stream_ctx(self.handle), k, owned=False)

    def reset(self) -> None:
        _check(lib().fdnn_stream_reset(self.handle))

    def position(self):
        """(raw frames pushed, rows emitted) since the utterance started."""
        p, e = C.c_int64(), C.c_int64()
        _check(lib().fdnn_stream_position(self.handle, C.byref(p), C.byref(e)))
        return int(p.value), int(e.value)

    def close(self) -> None:
        if self.handle:
            lib().fdnn_stream_free(self.handle)
            self.handle = None


def group_shard(n: int, world: int, rank: int):
    """[start, stop) of one device's contiguous frame shard (``fdnn_group_shard``)."""
    a, b = C.c_int(), C.c_int()
    lib().fdnn_group_shard(n, world, rank, C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


class DeviceGroup:
    """One process, several devices of one node (``fdnn_group_*``): weights quantized once and sent
    device-to-device at load, the frames of each ``calculate`` call sharded over the replicas."""

    def __init__(self, dnnFile: str, devices: Sequence[int], weightCutOffValue: float = 3.0):
        if weightCutOffValue <= 0:
            raise ValueError(f"Weight cut off value must be positive. But it is {weightCutOffValue}")
        h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        _check(lib().fdnn_group_load(os.path.abspath(dnnFile).encode(), weightCutOffValue, arr, len(devices), C.byref(h)))
        self.handle = h.value

    def size(self) -> int:
        return lib().fdnn_group_size(self.handle)

    def model(self, index: int) -> "QuantizedDnn":
        """A view of replica ``index`` (owned by the group: do not delete it)."""
        return QuantizedDnn(lib().fdnn_group_model(self.handle, index))

    def weightTransport(self) -> str:
        return lib().fdnn_group_weight_transport(self.handle).decode()

    def workerCpus(self, index: int) -> str:
        """CPU list replica `index`'s persistent host thread pinned itself to ("" before the first large call)."""
        return lib().fdnn_group_worker_cpus(self.handle, int(index)).decode()

    def calculate(self, input, batchSize: int = 10) -> np.ndarray:
        x = np.asarray(input, dtype=np.float32)
        if x.shape[0] == 0:
            return np.zeros((0, 0), dtype=np.float32)
        m = self.model(0)
        if x.ndim != 2 or x.shape[1] != m.inputDimension():
            raise ValueError(f"Input vector size {x.shape[-1]} must be equal with network input size {m.inputDimension()}")
        x = np.ascontiguousarray(x)
        out = np.empty((x.shape[0], m.outputDimension()), dtype=np.float32)
        _check(lib().fdnn_group_calculate(self.handle, x.ctypes.data_as(_c_f32p), x.shape[0], x.shape[1], batchSize,
                                          out.ctypes.data_as(_c_f32p)))
        return out

    def delete(self) -> None:
        if self.handle:
            lib().fdnn_group_free(self.handle)
            self.handle = None


class ScoringServer:
    """Multi-stream scoring loop over one model (``fdnn_server_*``): up to ``depth`` batches in
    flight, the soft-max scale of one batch under layer 0 of the next, host submissions from any
    number of threads coalesced into full batches.  Generalises ``QuantizedDnn.LazyContext`` /
    the caller-thread model of MultiThreadedStressTest.java to many utterances per GPU."""

    def __init__(self, dnn: "QuantizedDnn", max_frames: int, depth: int = 2, linger_us: int = 0):
        h = C.c_void_p()
        _check(lib().fdnn_server_create(dnn.nativeDnnHandle, max_frames, depth, C.byref(h)))
        self.handle = h.value
        self.dnn = dnn
        self._keep = {}  # ticket -> arrays that must outlive the submission
        if linger_us:
            _check(lib().fdnn_server_set_linger_us(self.handle, linger_us))

    def submit_device(self, d_x: int, n: int, d_out: int, d_masks: int = 0) -> int:
        t = C.c_uint64()
        _check(lib().fdnn_server_submit_device(self.handle, C.c_void_p(d_x), n, C.c_void_p(d_masks) if d_masks else None,
                                               C.c_void_p(d_out), C.byref(t)))
        return int(t.value)

    def submit(self, x, masks=None, out=None):
        """Host frames -> (ticket, out array).  ``out`` is valid after ``wait(ticket)``; pass a
        C-contiguous float32 [n][output_dim] array to have the result written there (reused buffers)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.dnn.inputDimension():
            raise ValueError(f"Input vector size {x.shape[-1]} must be equal with network input size {self.dnn.inputDimension()}")
        O = self.dnn.outputDimension()
        m = None
        if masks is not None:
            m = np.ascontiguousarray(masks, dtype=np.int8)
            if m.shape != (x.shape[0], O):
                raise ValueError(f"masks must be {x.shape[0]} x {O}, got {m.shape}")
        if out is None:
            out = np.empty((x.shape[0], O), dtype=np.float32)
        elif out.dtype != np.float32 or out.shape != (x.shape[0], O) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous float32 array of shape {(x.shape[0], O)}")
        t = C.c_uint64()
        _check(lib().fdnn_server_submit(self.handle, x.ctypes.data_as(_c_f32p), x.shape[0],
                                        m.ctypes.data_as(_c_i8p) if m is not None else None, out.ctypes.data_as(_c_f32p), C.byref(t)))
        self._keep[int(t.value)] = (x, m, out)
        return int(t.value), out

    def submitLazy(self, x, bits, out=None):
        """The lazy contract through the loop, masks as bits ([n][ceil(output_dim / 64)] uint64, ``formats.pack_mask_bits``):
        coalesced with the other callers' bit-mask submissions, rows back compacted and rebuilt inside ``out`` by the
        thread that waits for the ticket -> (ticket, out array)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.dnn.inputDimension():
            raise ValueError(f"Input vector size {x.shape[-1]} must be equal with network input size {self.dnn.inputDimension()}")
        O = self.dnn.outputDimension()
        b = np.ascontiguousarray(bits, dtype=np.uint64)
        if b.shape != (x.shape[0], (O + 63) // 64):
            raise ValueError(f"bits must be {x.shape[0]} x {(O + 63) // 64} uint64, got {b.shape}")
        if out is None:
            out = np.empty((x.shape[0], O), dtype=np.float32)
        elif out.dtype != np.float32 or out.shape != (x.shape[0], O) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous float32 array of shape {(x.shape[0], O)}")
        t = C.c_uint64()
        _check(lib().fdnn_server_submit_lazy_bits(self.handle, x.ctypes.data_as(_c_f32p), x.shape[0], C.c_void_p(b.ctypes.data),
                                                  out.ctypes.data_as(_c_f32p), C.byref(t)))
        self._keep[int(t.value)] = (x, b, out)
        return int(t.value), out

    def submitRaw(self, raw, bits=None, out=None):
        """Raw feature frames [n][rawDim] of one utterance (the model's splice spec, QuantizedDnn.setSplice): coalesced
        with the other callers' raw utterances, each keeping its own edges; ``bits`` selects the lazy contract (as
        ``submitLazy``) -> (ticket, out array)."""
        r = np.ascontiguousarray(raw, dtype=np.float32)
        spec = self.dnn.spliceSpec()
        if spec is not None and (r.ndim != 2 or r.shape[1] != spec[1]):
            raise ValueError(f"raw frames must be [n][{spec[1]}], got {r.shape}")
        n, O = r.shape[0], self.dnn.outputDimension()
        b = None
        if bits is not None:
            b = np.ascontiguousarray(bits, dtype=np.uint64)
            if b.shape != (n, (O + 63) // 64):
                raise ValueError(f"bits must be {n} x {(O + 63) // 64} uint64, got {b.shape}")
        if out is None:
            out = np.empty((n, O), dtype=np.float32)
        elif out.dtype != np.float32 or out.shape != (n, O) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous float32 array of shape {(n, O)}")
        t = C.c_uint64()
        _check(lib().fdnn_server_submit_raw(self.handle, r.ctypes.data_as(_c_f32p), n, C.c_void_p(b.ctypes.data) if b is not None else None,
                                            out.ctypes.data_as(_c_f32p), C.byref(t)))
        self._keep[int(t.value)] = (r, b, out)
        return int(t.value), out

    def submitLazySet(self, x, nodes, probs=None, inactive=None):
        """One utterance's frames with ITS node set through the loop (``fdnn_server_submit_lazy_set``): coalesced with the other
        callers' set submissions, the output layer is scored for the listed nodes only and only [n][len] + [n] floats come
        back -> (ticket, probs [n][len], inactive [n]), valid after ``wait(ticket)``; the bytes of ``calculateLazySet``."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.dnn.inputDimension():
            raise ValueError(f"Input vector size {x.shape[-1]} must be equal with network input size {self.dnn.inputDimension()}")
        return self._submit_set(lib().fdnn_server_submit_lazy_set, x, x.shape[0], nodes, probs, inactive)

    def submitRawSet(self, raw, nodes, probs=None, inactive=None):
        """The same for raw feature frames [n][rawDim] of one utterance, spliced on the device by the model's splice spec at
        submit time (``fdnn_server_submit_raw_set``)."""
        r = np.ascontiguousarray(raw, dtype=np.float32)
        spec = self.dnn.spliceSpec()
        if spec is not None and (r.ndim != 2 or r.shape[1] != spec[1]):
            raise ValueError(f"raw frames must be [n][{spec[1]}], got {r.shape}")
        return self._submit_set(lib().fdnn_server_submit_raw_set, r, r.shape[0], nodes, probs, inactive)

    def submitTopK(self, x, k: int, nodes=None, probs=None):
        """One utterance's k best nodes per frame through the loop (``fdnn_server_submit_topk``): coalesced with the other
        callers' top-k submissions, the dense rows stay on the device -> (ticket, nodes int32 [n][k], probs float32 [n][k]),
        valid after ``wait(ticket)``; the bytes of ``QuantizedDnn.calculateTopK``."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.dnn.inputDimension():
            raise ValueError(f"Input vector size {x.shape[-1]} must be equal with network input size {self.dnn.inputDimension()}")
        return self._submit_topk(lib().fdnn_server_submit_topk, x, int(k), nodes, probs)

    def submitRawTopK(self, raw, k: int, nodes=None, probs=None):
        """The same for raw feature frames [n][rawDim] of one utterance, spliced on the device by the model's splice spec at
        submit time (``fdnn_server_submit_raw_topk``); the bytes of ``QuantizedDnn.calculateTopKRaw``."""
        r = np.ascontiguousarray(raw, dtype=np.float32)
        spec = self.dnn.spliceSpec()
        if spec is not None and (r.ndim != 2 or r.shape[1] != spec[1]):
            raise ValueError(f"raw frames must be [n][{spec[1]}], got {r.shape}")
        return self._submit_topk(lib().fdnn_server_submit_raw_topk, r, int(k), nodes, probs)

    def submitPool(self, x, pool: "ClassPool", out=None):
        """One utterance's class posteriors through the loop (``fdnn_server_submit_pool``): coalesced with the other callers'
        submissions under the SAME pool, the dense rows stay on the device -> (ticket, out float32 [n][classes]), valid after
        ``wait(ticket)``; the bytes of ``QuantizedDnn.calculatePool``."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.dnn.inputDimension():
            raise ValueError(f"Input vector size {x.shape[-1]} must be equal with network input size {self.dnn.inputDimension()}")
        return self._submit_pool(lib().fdnn_server_submit_pool, x, pool, out)

    def submitRawPool(self, raw, pool: "ClassPool", out=None):
        """The same for raw feature frames [n][rawDim] of one utterance, spliced on the device by the model's splice spec at
        submit time (``fdnn_server_submit_raw_pool``); the bytes of ``QuantizedDnn.calculatePoolRaw``."""
        r = np.ascontiguousarray(raw, dtype=np.float32)
        spec = self.dnn.spliceSpec()
        if spec is not None and (r.ndim != 2 or r.shape[1] != spec[1]):
            raise ValueError(f"raw frames must be [n][{spec[1]}], got {r.shape}")
        return self._submit_pool(lib().fdnn_server_submit_raw_pool, r, pool, out)

    def _submit_pool(self, fn, frames, pool, out):
        n = frames.shape[0]
        out = _pool_out(n, pool.classes(), out)
        t = C.c_uint64()
        _check(fn(self.handle, frames.ctypes.data_as(_c_f32p), n, pool.handle, out.ctypes.data_as(_c_f32p), C.byref(t)))
        self._keep[int(t.value)] = (frames, pool, out)
        return int(t.value), out

    def submitLoglik(self, x, ll: "Loglik", out=None):
        """One utterance's decoder scores through the loop (``fdnn_server_submit_loglik``): coalesced with the other callers'
        submissions under the SAME handle, the dense rows stay on the device -> (ticket, out float32 or float16
        [n][outputDimension]), valid after ``wait(ticket)``; the bytes of ``QuantizedDnn.calculateLoglik``."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.dnn.inputDimension():
            raise ValueError(f"Input vector size {x.shape[-1]} must be equal with network input size {self.dnn.inputDimension()}")
        return self._submit_loglik(lib().fdnn_server_submit_loglik, x, ll, out)

    def submitRawLoglik(self, raw, ll: "Loglik", out=None):
        """The same for raw feature frames [n][rawDim] of one utterance, spliced on the device by the model's splice spec at
        submit time (``fdnn_server_submit_raw_loglik``); the bytes of ``QuantizedDnn.calculateLoglikRaw``."""
        r = np.ascontiguousarray(raw, dtype=np.float32)
        spec = self.dnn.spliceSpec()
        if spec is not None and (r.ndim != 2 or r.shape[1] != spec[1]):
            raise ValueError(f"raw frames must be [n][{spec[1]}], got {r.shape}")
        return self._submit_loglik(lib().fdnn_server_submit_raw_loglik, r, ll, out)

    def _submit_loglik(self, fn, frames, ll, out):
        n = frames.shape[0]
        out = _loglik_out(n, ll, out)
        t = C.c_uint64()
        _check(fn(self.handle, frames.ctypes.data_as(_c_f32p), n, ll.handle, C.c_void_p(out.ctypes.data), C.byref(t)))
        self._keep[int(t.value)] = (frames, ll, out)
        return int(t.value), out

    def _submit_topk(self, fn, frames, k, nodes, probs):
        n = frames.shape[0]
        nodes, probs = _topk_out(n, k, nodes, probs)
        t = C.c_uint64()
        _check(fn(self.handle, frames.ctypes.data_as(_c_f32p), n, k, nodes.ctypes.data_as(_c_i32p), probs.ctypes.data_as(_c_f32p), C.byref(t)))
        self._keep[int(t.value)] = (frames, nodes, probs)
        return int(t.value), nodes, probs

    def _submit_set(self, fn, frames, n, nodes, probs, inactive):
        nd = _set(nodes)
        if probs is None:
            probs = np.empty((n, nd.size), dtype=np.float32)
        elif probs.dtype != np.float32 or probs.shape != (n, nd.size) or not probs.flags.c_contiguous:
            raise ValueError(f"probs must be a C-contiguous float32 array of shape {(n, nd.size)}")
        if inactive is None:
            inactive = np.empty(n, dtype=np.float32)
        elif inactive.dtype != np.float32 or inactive.shape != (n,) or not inactive.flags.c_contiguous:
            raise ValueError(f"inactive must be a C-contiguous float32 array of shape {(n,)}")
        t = C.c_uint64()
        _check(fn(self.handle, frames.ctypes.data_as(_c_f32p), n, nd.ctypes.data_as(_c_i32p), nd.size, probs.ctypes.data_as(_c_f32p),
                  inactive.ctypes.data_as(_c_f32p), C.byref(t)))
        self._keep[int(t.value)] = (frames, probs, inactive)  # (the set itself is copied at submit)
        return int(t.value), probs, inactive

    def wait(self, ticket: int) -> None:
        try:
            _check(lib().fdnn_server_wait(self.handle, ticket))
        finally:
            self._keep.pop(ticket, None)

    def drain(self) -> None:
        _check(lib().fdnn_server_drain(self.handle))
        self._keep.clear()

    def stats(self) -> dict:
        v = [C.c_uint64() for _ in range(4)]
        _check(lib().fdnn_server_stats(self.handle, *[C.byref(a) for a in v]))
        return dict(zip(("batches", "frames", "requests", "coalesced_requests"), (int(a.value) for a in v)))

    def openLive(self, maxChunk: int) -> "LiveStream":
        """A live utterance of this loop (``fdnn_server_live_open``): its pushes share batches with the other handles'."""
        return LiveStream(self, maxChunk)

    def hold(self, on: bool = True) -> None:
        """Tests (``fdnn_debug_server_hold``): while on, the packer plans no batch and submissions queue up; switching it off
        wakes the packer -- what was queued goes out together."""
        _check(lib().fdnn_debug_server_hold(self.handle, 1 if on else 0))

    def close(self) -> None:
        if self.handle:
            lib().fdnn_server_free(self.handle)
            self.handle = None


class LiveStream:
    """One utterance at a time, pushed chunk by chunk through a scoring loop (``fdnn_server_live_*``).  A push returns at once
    with ``(ticket, arrays)``: the arrays hold the rows the push completes and are valid after ``server.wait(ticket)``; a
    push that completes no rows returns ``(None, empty arrays)`` and there is nothing to wait for.  The raw frames are copied
    by the push.  ``end=True`` flushes the rest, right-clamped to the last frame.  Made by ``ScoringServer.openLive``; it
    keeps the model's splice spec of that moment.  One thread at a time per handle."""

    def __init__(self, server: ScoringServer, maxChunk: int):
        h = C.c_void_p()
        spec = server.dnn.spliceSpec()
        _check(lib().fdnn_server_live_open(server.handle, int(maxChunk), C.byref(h)))
        self.handle = h.value
        self.server = server
        self.maxChunk = int(maxChunk)
        self.offsets, self.rawDim = spec
        self.right = max(0, max(self.offsets))

    def _raw(self, raw):
        r = np.ascontiguousarray(raw, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] != self.rawDim:
            raise ValueError(f"raw frames must be [n][{self.rawDim}], got {r.shape}")
        return r

    def _done(self, n, t, bufs):
        k, ticket = int(n.value), int(t.value) or None
        if ticket is not None:
            self.server._keep[ticket] = bufs
        return (ticket,) + tuple(b[:k] for b in bufs)

    def push(self, raw, end: bool = False):
        """raw [n][rawDim] -> (ticket or None, the soft-max rows of the frames this push completes [k][outputDimension])."""
        r = self._raw(raw)
        out = np.empty((r.shape[0] + self.right, self.server.dnn.outputDimension()), dtype=np.float32)
        n, t = C.c_int(0), C.c_uint64(0)
        _check(lib().fdnn_server_live_push(self.handle, r.ctypes.data_as(_c_f32p), r.shape[0], int(bool(end)), out.ctypes.data_as(_c_f32p),
                                           C.byref(n), C.byref(t)))
        return self._done(n, t, (out,))

    def pushTopK(self, raw, k: int, end: bool = False):
        """-> (ticket or None, nodes int32 [rows][k], probs float32 [rows][k]): the bytes of ``calculateTopKRaw``."""
        r = self._raw(raw)
        nodes, probs = _topk_out(r.shape[0] + self.right, max(int(k), 0), None, None)
        n, t = C.c_int(0), C.c_uint64(0)
        _check(lib().fdnn_server_live_push_topk(self.handle, r.ctypes.data_as(_c_f32p), r.shape[0], int(bool(end)), int(k),
                                                nodes.ctypes.data_as(_c_i32p), probs.ctypes.data_as(_c_f32p), C.byref(n), C.byref(t)))
        return self._done(n, t, (nodes, probs))

    def pushPool(self, raw, pool: "ClassPool", end: bool = False):
        """-> (ticket or None, class sums float32 [rows][classes]): the bytes of ``calculatePoolRaw``."""
        r = self._raw(raw)
        out = np.empty((r.shape[0] + self.right, pool.classes()), dtype=np.float32)
        n, t = C.c_int(0), C.c_uint64(0)
        _check(lib().fdnn_server_live_push_pool(self.handle, r.ctypes.data_as(_c_f32p), r.shape[0], int(bool(end)), pool.handle,
                                                out.ctypes.data_as(_c_f32p), C.byref(n), C.byref(t)))
        return self._done(n, t, (out,))

    def pushLoglik(self, raw, ll: "Loglik", end: bool = False):
        """-> (ticket or None, decoder scores float32 or float16 [rows][outputDimension]): the bytes of ``calculateLoglikRaw``."""
        r = self._raw(raw)
        out = np.empty((r.shape[0] + self.right, ll.width()), dtype=ll.dtype)
        n, t = C.c_int(0), C.c_uint64(0)
        _check(lib().fdnn_server_live_push_loglik(self.handle, r.ctypes.data_as(_c_f32p), r.shape[0], int(bool(end)), ll.handle,
                                                  C.c_void_p(out.ctypes.data), C.byref(n), C.byref(t)))
        return self._done(n, t, (out,))

    def pushSet(self, raw, nodes, end: bool = False):
        """-> (ticket or None, probs [rows][len], inactive [rows]): the bytes of ``calculateLazySet`` on the host-spliced rows."""
        r = self._raw(raw)
        nd = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
        probs = np.empty((r.shape[0] + self.right, nd.size), dtype=np.float32)
        inactive = np.empty(r.shape[0] + self.right, dtype=np.float32)
        n, t = C.c_int(0), C.c_uint64(0)
        _check(lib().fdnn_server_live_push_set(self.handle, r.ctypes.data_as(_c_f32p), r.shape[0], int(bool(end)), nd.ctypes.data_as(_c_i32p),
                                               nd.size, probs.ctypes.data_as(_c_f32p), inactive.ctypes.data_as(_c_f32p), C.byref(n), C.byref(t)))
        return self._done(n, t, (probs, inactive))

    def reset(self) -> None:
        _check(lib().fdnn_server_live_reset(self.handle))

    def position(self):
        """(raw frames pushed, rows emitted) since the utterance started."""
        p, e = C.c_int64(), C.c_int64()
        _check(lib().fdnn_server_live_position(self.handle, C.byref(p), C.byref(e)))
        return int(p.value), int(e.value)

    def close(self) -> None:
        if self.handle:
            lib().fdnn_server_live_close(self.handle)
            self.handle = None


def splice_table(offsets, rawDim: int, inputDim: int, raw, segs, rows: int, use_table: bool, device: int = 0) -> np.ndarray:
    """The splice alone (``fdnn_debug_splice_table``): raw [frames][rawDim], segs [n][4] = (row, center, lo, hi) -> rows
    [rows][inputDim]; ``use_table`` picks the kernel that reads the segment table from device memory."""
    off = np.ascontiguousarray(offsets, dtype=np.int32).ravel()
    r = np.ascontiguousarray(raw, dtype=np.float32)
    sg = np.ascontiguousarray(segs, dtype=np.int32)
    if r.ndim != 2 or r.shape[1] != rawDim or sg.ndim != 2 or sg.shape[1] != 4:
        raise ValueError("raw must be [frames][rawDim] and segs [n][4]")
    x = np.empty((int(rows), int(inputDim)), dtype=np.float32)
    _check(lib().fdnn_debug_splice_table(off.ctypes.data_as(_c_i32p), off.size, int(rawDim), int(inputDim), r.ctypes.data_as(_c_f32p), r.shape[0],
                                         sg.ctypes.data_as(_c_i32p), sg.shape[0], int(rows), 1 if use_table else 0, x.ctypes.data_as(_c_f32p),
                                         int(device)))
    return x


def live_launches() -> dict:
    """Process-wide since load (``fdnn_debug_live_launches``): launches of the table splice kernel, the longest table given."""
    a, b = C.c_ulonglong(0), C.c_ulonglong(0)
    _check(lib().fdnn_debug_live_launches(C.byref(a), C.byref(b)))
    return {"launches": int(a.value), "max_segs": int(b.value)}


class QuantizedDnn:
    """``suskun.nn.QuantizedDnn`` (QuantizedDnn.java) on one MI355X."""

    def __init__(self, handle: int):
        self.nativeDnnHandle = handle

    # -- construction ---------------------------------------------------
    @staticmethod
    def loadFromFile(dnnFile: str, weightCutOffValue: float = 3.0, device: Optional[int] = None) -> "QuantizedDnn":
        if weightCutOffValue <= 0:  # QuantizedDnn.java:55-57
            raise ValueError(f"Weight cut off value must be positive. But it is {weightCutOffValue}")
        h = C.c_void_p()
        path = os.path.abspath(dnnFile).encode()
        if device is None:
            _check(lib().fdnn_model_load(path, weightCutOffValue, C.byref(h)))
        else:
            _check(lib().fdnn_model_load_on(path, weightCutOffValue, device, C.byref(h)))
        return QuantizedDnn(h.value)

    @staticmethod
    def fromDeviceBlob(d_ptr: int, nbytes: int, device: int) -> "QuantizedDnn":
        h = C.c_void_p()
        _check(lib().fdnn_model_import_blob(C.c_void_p(d_ptr), nbytes, device, C.byref(h)))
        return QuantizedDnn(h.value)

    def delete(self) -> None:
        if self.nativeDnnHandle:
            lib().fdnn_model_free(self.nativeDnnHandle)
            self.nativeDnnHandle = None

    # -- queries ----------------------------------------------------------
    def inputDimension(self) -> int:
        return lib().fdnn_model_input_dim(self.nativeDnnHandle)

    def outputDimension(self) -> int:
        return lib().fdnn_model_output_dim(self.nativeDnnHandle)

    def hiddenDimension(self) -> int:
        return lib().fdnn_model_hidden_dim(self.nativeDnnHandle)

    def layerDimension(self, layerIndex: int) -> int:
        return lib().fdnn_model_layer_dim(self.nativeDnnHandle, layerIndex)

    def layerCount(self) -> int:
        return lib().fdnn_model_layer_count(self.nativeDnnHandle)

    def enableBatcher(self, max_frames: int, depth: int = 2, linger_us: int = 0) -> None:
        """Route ``calculate`` through an internal coalescing server (also: FDNN_BATCHER env at load)."""
        _check(lib().fdnn_model_enable_batcher(self.nativeDnnHandle, max_frames, depth, linger_us))

    def setInputLayerFma(self, on: bool) -> None:
        _check(lib().fdnn_model_set_l0_fma(self.nativeDnnHandle, int(on)))

    def setListsUnion(self, group_tiles: int) -> None:
        """How the list calls (``calculateLazyLists``, ``LazyContext.calculateForOutputNodesLists`` and its device form) score
        their entries (``fdnn_model_set_lists_union``): 0 (default) the dot-product kernels; 1 .. 8 the int8 MFMA over the
        union of every ``32 * group_tiles`` consecutive rows' lists; -1 the same with the library's default group.  The
        results are byte-identical either way; set it before the model is used from several threads."""
        _check(lib().fdnn_model_set_lists_union(self.nativeDnnHandle, int(group_tiles)))

    def setInputLayerListCap(self, cap: int) -> None:
        """Tests: cap the flagged-output list of the int8-screened input layer (contexts created afterwards)."""
        _check(lib().fdnn_debug_set_l0_list_cap(self.nativeDnnHandle, int(cap)))

    def setInputLayerKernel(self, kind: int) -> None:
        """0 = chosen by batch size, 1 = chain-pass kernel, 2 = 64 x 64-tile kernel, 3 = screened path where available (same bits)."""
        _check(lib().fdnn_debug_set_l0_kernel(self.nativeDnnHandle, int(kind)))

    # -- dense path ---------------------------------------------------------
    def calculate(self, input, batchSize: int = 10) -> np.ndarray:
        """float[][] calculate(float[][] input, int batchSize) -- QuantizedDnn.java:149-167."""
        x = np.asarray(input, dtype=np.float32)
        if x.shape[0] == 0:  # QuantizedDnn.java:154-156
            return np.zeros((0, 0), dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.inputDimension():
            raise ValueError(f"Input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        x = np.ascontiguousarray(x)
        out = np.empty((x.shape[0], self.outputDimension()), dtype=np.float32)
        _check(lib().fdnn_calculate(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), x.shape[0], x.shape[1], batchSize,
                                    out.ctypes.data_as(_c_f32p)))
        return out

    def calculate_device(self, d_x: int, n: int, d_out: int, stream: int = 0) -> None:
        """Device-resident form: raw device pointers (e.g. ``tensor.data_ptr()``), enqueued on ``stream``."""
        _check(lib().fdnn_calculate_device(self.nativeDnnHandle, C.c_void_p(d_x), n, C.c_void_p(d_out), C.c_void_p(stream)))

    def calculateLazy(self, input, masks=None, bits=None, out=None) -> np.ndarray:
        """One-call lazy scoring: hidden layers + masked output layer for every frame of ``input`` (LazyContext's
        calculateUntilOutput + calculateForOutputNodes per frame, QuantizedDnn.java:72-107, in one native call).
        ``masks`` [n][outputDimension] bytes (non-zero = active) or ``bits`` [n][ceil(O / 64)] uint64."""
        x = _f32(input)
        n, O = x.shape[0], self.outputDimension()
        if n and x.shape[1] != self.inputDimension():
            raise ValueError(f"input vector size {x.shape[1]} must be equal with network input size {self.inputDimension()}")
        if out is None:
            out = np.empty((n, O), dtype=np.float32)
        if bits is not None:
            b = np.ascontiguousarray(bits, dtype=np.uint64)
            if b.shape != (n, (O + 63) // 64):
                raise ValueError("bits must be [frames][ceil(outputDimension / 64)] uint64")
            _check(lib().fdnn_calculate_lazy_bits(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(),
                                                  b.ctypes.data_as(C.POINTER(C.c_uint64)), out.ctypes.data_as(_c_f32p)))
        else:
            m = np.ascontiguousarray(masks, dtype=np.int8)
            if m.shape != (n, O):
                raise ValueError("masks must be [frames][outputDimension]")
            _check(lib().fdnn_calculate_lazy(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(),
                                             m.ctypes.data_as(_c_i8p), out.ctypes.data_as(_c_f32p)))
        return out

    def calculateLazyLists(self, input, rowPtr, nodes):
        """One-call lazy scoring of the LISTED nodes only (``fdnn_calculate_lazy_lists``): hidden layers, then per frame the
        nodes rowPtr / nodes list -> (probs [nnz], inactive [frames]), as ``LazyContext.calculateForOutputNodesLists``."""
        x = _f32(input)
        n = x.shape[0]
        if n and (x.ndim != 2 or x.shape[1] != self.inputDimension()):
            raise ValueError(f"input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        rp, nd = _lists(rowPtr, nodes)
        if rp.size != n + 1:
            raise ValueError(f"rowPtr must have {n + 1} entries, got {rp.size}")
        probs = np.empty(max(int(rp[-1]), 0), dtype=np.float32)
        inactive = np.empty(n, dtype=np.float32)
        _check(lib().fdnn_calculate_lazy_lists(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(),
                                               rp.ctypes.data_as(_c_i32p), nd.ctypes.data_as(_c_i32p), probs.ctypes.data_as(_c_f32p),
                                               inactive.ctypes.data_as(_c_f32p)))
        return probs, inactive

    def calculateLazySet(self, input, nodes):
        """One-call lazy scoring of ONE node set for every frame (``fdnn_calculate_lazy_set``): hidden layers, then the set
        -> (probs [frames][len], inactive [frames]), as ``LazyContext.calculateForOutputNodeSet``."""
        x = _f32(input)
        n = x.shape[0]
        if n and (x.ndim != 2 or x.shape[1] != self.inputDimension()):
            raise ValueError(f"input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        nd = _set(nodes)
        probs = np.empty((n, nd.size), dtype=np.float32)
        inactive = np.empty(n, dtype=np.float32)
        _check(lib().fdnn_calculate_lazy_set(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(),
                                             nd.ctypes.data_as(_c_i32p), nd.size, probs.ctypes.data_as(_c_f32p), inactive.ctypes.data_as(_c_f32p)))
        return probs, inactive

    def calculateLazySets(self, input, segRows, setPtr, nodes):
        """One-call lazy scoring with one node set per segment of the frames (``fdnn_calculate_lazy_sets``; segRows must cover
        [0, frames)): hidden layers, then the sets -> (probs flat, inactive [frames]), as
        ``LazyContext.calculateForOutputNodeSets``."""
        x = _f32(input)
        n = x.shape[0]
        if n and (x.ndim != 2 or x.shape[1] != self.inputDimension()):
            raise ValueError(f"input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        sr, sp, nd, n_segs, rows, nnz = _sets(segRows, setPtr, nodes)
        probs = np.empty(nnz, dtype=np.float32)
        inactive = np.empty(n, dtype=np.float32)
        _check(lib().fdnn_calculate_lazy_sets(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(),
                                              sr.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), n_segs, nd.ctypes.data_as(_c_i32p),
                                              probs.ctypes.data_as(_c_f32p), inactive.ctypes.data_as(_c_f32p)))
        return probs, inactive

    def calculateTopK(self, input, k: int):
        """Dense scoring with a top-k return (``fdnn_calculate_topk``): the k first-ranked nodes of every frame's soft-max row
        -- larger probability first, the lower node first among equal ones -- and their probabilities, chosen on the
        device; only n x k x 8 bytes come back -> (nodes int32 [n][k], probs float32 [n][k]).  1 <= k <= min(O, 256)."""
        x = _f32(input)
        n = x.shape[0]
        if n and (x.ndim != 2 or x.shape[1] != self.inputDimension()):
            raise ValueError(f"input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        nodes, probs = _topk_out(n, int(k), None, None)
        _check(lib().fdnn_calculate_topk(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(), int(k),
                                         nodes.ctypes.data_as(_c_i32p), probs.ctypes.data_as(_c_f32p)))
        return nodes, probs

    def calculateTopKRaw(self, raw, k: int):
        """``calculateTopK`` on raw frames [n][rawDim] of one utterance, spliced on the device (``fdnn_calculate_topk_raw``)."""
        r = _f32(raw)
        if r.ndim != 2:
            raise ValueError(f"raw frames must be [n][rawDim], got {r.shape}")
        nodes, probs = _topk_out(r.shape[0], int(k), None, None)
        _check(lib().fdnn_calculate_topk_raw(self.nativeDnnHandle, r.ctypes.data_as(_c_f32p), r.shape[0], r.shape[1], int(k),
                                             nodes.ctypes.data_as(_c_i32p), probs.ctypes.data_as(_c_f32p)))
        return nodes, probs

    def calculate_topk_device(self, d_x: int, n: int, k: int, d_nodes: int, d_probs: int, stream: int = 0) -> None:
        """Device-resident form (``fdnn_calculate_topk_device``): d_x [n][inputDimension] -> d_nodes int32 [n][k], d_probs
        float32 [n][k]; raw device pointers, enqueued on ``stream``, not synchronised."""
        _check(lib().fdnn_calculate_topk_device(self.nativeDnnHandle, C.c_void_p(d_x), int(n), int(k), C.c_void_p(d_nodes), C.c_void_p(d_probs),
                                                C.c_void_p(stream)))

    def calculatePool(self, input, pool: "ClassPool") -> np.ndarray:
        """Dense scoring pooled over a node -> class map (``fdnn_calculate_pool``): of every frame's soft-max row the sum over
        each class of ``pool``, added on the device in the contract's order (include/fdnn.h); only n x classes x 4 bytes come
        back -> float32 [n][classes]."""
        x = _f32(input)
        n = x.shape[0]
        if n and (x.ndim != 2 or x.shape[1] != self.inputDimension()):
            raise ValueError(f"input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        out = _pool_out(n, pool.classes(), None)
        _check(lib().fdnn_calculate_pool(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(), pool.handle,
                                         out.ctypes.data_as(_c_f32p)))
        return out

    calculate_pool = calculatePool

    def calculatePoolRaw(self, raw, pool: "ClassPool") -> np.ndarray:
        """``calculatePool`` on raw frames [n][rawDim] of one utterance, spliced on the device (``fdnn_calculate_pool_raw``)."""
        r = _f32(raw)
        if r.ndim != 2:
            raise ValueError(f"raw frames must be [n][rawDim], got {r.shape}")
        out = _pool_out(r.shape[0], pool.classes(), None)
        _check(lib().fdnn_calculate_pool_raw(self.nativeDnnHandle, r.ctypes.data_as(_c_f32p), r.shape[0], r.shape[1], pool.handle, out.ctypes.data_as(_c_f32p)))
        return out

    def calculate_pool_device(self, d_x: int, n: int, pool: "ClassPool", d_out: int, stream: int = 0) -> None:
        """Device-resident form (``fdnn_calculate_pool_device``): d_x [n][inputDimension] -> d_out float32 [n][classes]; raw
        device pointers, enqueued on ``stream``, not synchronised."""
        _check(lib().fdnn_calculate_pool_device(self.nativeDnnHandle, C.c_void_p(d_x), int(n), pool.handle, C.c_void_p(d_out), C.c_void_p(stream)))

    def calculateLoglik(self, input, ll: "Loglik") -> np.ndarray:
        """Dense scoring returned as decoder scores (``fdnn_calculate_loglik``): of every frame's soft-max row
        ln(p_i) - log_prior[i], floored, computed on the device by the contract's logarithm (include/fdnn.h) -> float32 or
        float16 [n][outputDimension]; an F16 handle halves the bytes that come back."""
        x = _f32(input)
        n = x.shape[0]
        if n and (x.ndim != 2 or x.shape[1] != self.inputDimension()):
            raise ValueError(f"input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        out = _loglik_out(n, ll, None)
        _check(lib().fdnn_calculate_loglik(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(), ll.handle,
                                           C.c_void_p(out.ctypes.data)))
        return out

    calculate_loglik = calculateLoglik

    def calculateLoglikRaw(self, raw, ll: "Loglik") -> np.ndarray:
        """``calculateLoglik`` on raw frames [n][rawDim] of one utterance, spliced on the device (``fdnn_calculate_loglik_raw``)."""
        r = _f32(raw)
        if r.ndim != 2:
            raise ValueError(f"raw frames must be [n][rawDim], got {r.shape}")
        out = _loglik_out(r.shape[0], ll, None)
        _check(lib().fdnn_calculate_loglik_raw(self.nativeDnnHandle, r.ctypes.data_as(_c_f32p), r.shape[0], r.shape[1], ll.handle, C.c_void_p(out.ctypes.data)))
        return out

    def calculate_loglik_device(self, d_x: int, n: int, ll: "Loglik", d_out: int, stream: int = 0) -> None:
        """Device-resident form (``fdnn_calculate_loglik_device``): d_x [n][inputDimension] -> d_out [n][outputDimension] of the
        handle's type; raw device pointers, enqueued on ``stream``, not synchronised."""
        _check(lib().fdnn_calculate_loglik_device(self.nativeDnnHandle, C.c_void_p(d_x), int(n), ll.handle, C.c_void_p(d_out), C.c_void_p(stream)))

    def calculateAlign(self, input, ll: "Loglik", segRows, statePtr, states, selfLp=None, nextLp=None):
        """Forced alignment in one call (``fdnn_calculate_align``; segRows must cover [0, frames)): hidden layers, the
        transcripts' node sets, the recursion on the device -> (path int32 [frames], total float32 [segments]), as
        ``LazyContext.align``.  Many utterances per call is the batched form.  Host frames only: there is no device-frames
        form (no ``calculate_align_device``) -- the C-ABI has no entry for it."""
        x = _f32(input)
        n = x.shape[0]
        if n and (x.ndim != 2 or x.shape[1] != self.inputDimension()):
            raise ValueError(f"input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        sr, sp, st, sl, nl, n_segs, _ = _align_tables(segRows, statePtr, states, selfLp, nextLp)
        path = np.empty(n, np.int32)
        total = np.empty(n_segs, np.float32)
        _check(lib().fdnn_calculate_align(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(), ll.handle,
                                          sr.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), n_segs, st.ctypes.data_as(_c_i32p), _fp(sl), _fp(nl),
                                          path.ctypes.data_as(_c_i32p), total.ctypes.data_as(_c_f32p)))
        return path, total

    def calculateAlignRaw(self, raw, ll: "Loglik", segRows, statePtr, states, selfLp=None, nextLp=None):
        """``calculateAlign`` on raw frames [n][rawDim], spliced on the device, every segment an utterance of its own
        (``fdnn_calculate_align_raw``)."""
        r = _f32(raw)
        if r.ndim != 2:
            raise ValueError("raw must be [frames][rawDim]")
        sr, sp, st, sl, nl, n_segs, _ = _align_tables(segRows, statePtr, states, selfLp, nextLp)
        path = np.empty(r.shape[0], np.int32)
        total = np.empty(n_segs, np.float32)
        _check(lib().fdnn_calculate_align_raw(self.nativeDnnHandle, r.ctypes.data_as(_c_f32p), r.shape[0], r.shape[1], ll.handle,
                                              sr.ctypes.data_as(_c_i32p), sp.ctypes.data_as(_c_i32p), n_segs, st.ctypes.data_as(_c_i32p), _fp(sl), _fp(nl),
                                              path.ctypes.data_as(_c_i32p), total.ctypes.data_as(_c_f32p)))
        return path, total

    def calculateAlignGraph(self, input, ll: "Loglik", segRows, graphs):
        """The best path over alignment graphs in one call (``fdnn_calculate_align_graph``; segRows must cover [0, frames)):
        hidden layers, the graphs' node sets, the recursion on the device -> (path int32 [frames], total float32 [segments]),
        as ``LazyContext.alignGraph``.  ``graphs`` is a packed call (``pack_graphs`` over ``chain_graph`` /
        ``optional_silence_graph`` / hand-written graphs)."""
        x = _f32(input)
        n = x.shape[0]
        if n and (x.ndim != 2 or x.shape[1] != self.inputDimension()):
            raise ValueError(f"input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        sr, sp, st, ap, src, lp, start, final, n_segs, _ = _graph_call_tables(segRows, graphs)
        path = np.empty(n, np.int32)
        total = np.empty(n_segs, np.float32)
        _check(lib().fdnn_calculate_align_graph(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(), ll.handle,
                                                _ip(sr), _ip(sp), n_segs, _ip(st), _ip(ap), _ip(src), _fp(lp), _fp(start), _fp(final),
                                                path.ctypes.data_as(_c_i32p), total.ctypes.data_as(_c_f32p)))
        return path, total

    def calculateAlignGraphRaw(self, raw, ll: "Loglik", segRows, graphs):
        """``calculateAlignGraph`` on raw frames [n][rawDim], spliced on the device, every segment an utterance of its own
        (``fdnn_calculate_align_graph_raw``)."""
        r = _f32(raw)
        if r.ndim != 2:
            raise ValueError("raw must be [frames][rawDim]")
        sr, sp, st, ap, src, lp, start, final, n_segs, _ = _graph_call_tables(segRows, graphs)
        path = np.empty(r.shape[0], np.int32)
        total = np.empty(n_segs, np.float32)
        _check(lib().fdnn_calculate_align_graph_raw(self.nativeDnnHandle, r.ctypes.data_as(_c_f32p), r.shape[0], r.shape[1], ll.handle, _ip(sr), _ip(sp),
                                                    n_segs, _ip(st), _ip(ap), _ip(src), _fp(lp), _fp(start), _fp(final),
                                                    path.ctypes.data_as(_c_i32p), total.ctypes.data_as(_c_f32p)))
        return path, total

    def calculateForwardBackward(self, input, ll: "Loglik", segRows, graphs, want_gamma: bool = True):
        """The total likelihood and the state occupancies of alignment graphs in one call (``fdnn_calculate_fb``; segRows must
        cover [0, frames)): hidden layers, the graphs' node sets, the forward and backward sweeps on the device -> (total
        float32 [segments], gamma float32 [sum of T S] or None), as ``LazyContext.forwardBackward``."""
        x = _f32(input)
        n = x.shape[0]
        if n and (x.ndim != 2 or x.shape[1] != self.inputDimension()):
            raise ValueError(f"input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        sr, sp, st, ap, src, lp, start, final, n_segs, _ = _graph_call_tables(segRows, graphs)
        total, gamma = _fb_out(n_segs, sr, sp, want_gamma)
        _check(lib().fdnn_calculate_fb(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, x.shape[1] if n else self.inputDimension(), ll.handle,
                                       _ip(sr), _ip(sp), n_segs, _ip(st), _ip(ap), _ip(src), _fp(lp), _fp(start), _fp(final), _fp(total), _fp(gamma)))
        return total, gamma

    def calculateForwardBackwardRaw(self, raw, ll: "Loglik", segRows, graphs, want_gamma: bool = True):
        """``calculateForwardBackward`` on raw frames [n][rawDim], spliced on the device, every segment an utterance of its own
        (``fdnn_calculate_fb_raw``)."""
        r = _f32(raw)
        if r.ndim != 2:
            raise ValueError("raw must be [frames][rawDim]")
        sr, sp, st, ap, src, lp, start, final, n_segs, _ = _graph_call_tables(segRows, graphs)
        total, gamma = _fb_out(n_segs, sr, sp, want_gamma)
        _check(lib().fdnn_calculate_fb_raw(self.nativeDnnHandle, r.ctypes.data_as(_c_f32p), r.shape[0], r.shape[1], ll.handle, _ip(sr), _ip(sp), n_segs,
                                           _ip(st), _ip(ap), _ip(src), _fp(lp), _fp(start), _fp(final), _fp(total), _fp(gamma)))
        return total, gamma

    def calculate_lazy_bits_device(self, d_x: int, n: int, d_bits: int, d_out: int, stream: int = 0) -> None:
        _check(lib().fdnn_calculate_lazy_bits_device(self.nativeDnnHandle, C.c_void_p(d_x), n, C.c_void_p(d_bits), C.c_void_p(d_out), C.c_void_p(stream)))

    # -- raw feature frames (the <Splice> block on the device) ------------------
    def setSplice(self, offsets, rawDim: int = 0) -> None:
        """Frame offsets of the feature transform's <Splice> block (convert.load_splice_offsets) and the raw frame width;
        ``setSplice([], 0)`` clears the spec.  Set it before the model is used from several threads."""
        o = np.ascontiguousarray(list(offsets), dtype=np.int32)
        _check(lib().fdnn_model_set_splice(self.nativeDnnHandle, o.ctypes.data_as(_c_i32p) if o.size else None, int(o.size), int(rawDim)))

    def spliceSpec(self):
        """(offsets, rawDim), or None without a spec."""
        buf = np.zeros(64, dtype=np.int32)
        d = C.c_int32(0)
        k = lib().fdnn_model_get_splice(self.nativeDnnHandle, buf.ctypes.data_as(_c_i32p), 64, C.byref(d))
        if k < 0:
            _check(k)
        return ([int(v) for v in buf[:k]], int(d.value)) if k else None

    def calculateRaw(self, raw) -> np.ndarray:
        """``calculate`` on raw frames [n][rawDim] of one utterance, spliced on the device: one soft-max row per frame,
        bit-identical to ``calculate(convert.splice_frames(raw, offsets, inputDimension()))``."""
        r = _f32(raw)
        if r.ndim != 2:
            raise ValueError(f"raw frames must be [n][rawDim], got {r.shape}")
        out = np.empty((r.shape[0], self.outputDimension()), dtype=np.float32)
        _check(lib().fdnn_calculate_raw(self.nativeDnnHandle, r.ctypes.data_as(_c_f32p), r.shape[0], r.shape[1], out.ctypes.data_as(_c_f32p)))
        return out

    def calculateRawDevice(self, d_raw: int, n: int, d_out: int, segStarts=None, stream: int = 0) -> None:
        """Device-resident raw frames [n][rawDim] -> d_out [n][outputDimension], enqueued on ``stream``; ``segStarts``
        (first 0, ascending) cuts the frames into utterances with edges of their own."""
        seg = None
        if segStarts is not None:
            seg = np.ascontiguousarray(list(segStarts), dtype=np.int32)
        _check(lib().fdnn_calculate_raw_device(self.nativeDnnHandle, C.c_void_p(d_raw), int(n), seg.ctypes.data_as(_c_i32p) if seg is not None else None,
                                               int(seg.size) if seg is not None else 0, C.c_void_p(d_out), C.c_void_p(stream)))

    def calculateLazyRaw(self, raw, bits, out=None) -> np.ndarray:
        """``calculateLazy(bits=...)`` on raw frames (one call, rows back compacted)."""
        r = _f32(raw)
        if r.ndim != 2:
            raise ValueError(f"raw frames must be [n][rawDim], got {r.shape}")
        n, O = r.shape[0], self.outputDimension()
        b = np.ascontiguousarray(bits, dtype=np.uint64)
        if b.shape != (n, (O + 63) // 64):
            raise ValueError("bits must be [frames][ceil(outputDimension / 64)] uint64")
        if out is None:
            out = np.empty((n, O), dtype=np.float32)
        _check(lib().fdnn_calculate_lazy_bits_raw(self.nativeDnnHandle, r.ctypes.data_as(_c_f32p), n, r.shape[1], C.c_void_p(b.ctypes.data),
                                                  out.ctypes.data_as(_c_f32p)))
        return out

    def newStream(self, maxChunk: int) -> SpliceStream:
        """A stream of raw frames, pushed in chunks of at most ``maxChunk`` frames (``SpliceStream``)."""
        return SpliceStream(self, maxChunk)

    # -- lazy path ----------------------------------------------------------
    def getNewLazyContext(self, inputVectorCount: int, batchSize: int = 8) -> LazyContext:
        h = C.c_void_p()
        _check(lib().fdnn_ctx_create(self.nativeDnnHandle, inputVectorCount, batchSize, C.byref(h)))
        return LazyContext(self, h.value, inputVectorCount)

    # -- weight blob (multi-GPU) -------------------------------------------
    def blobSize(self) -> int:
        n = C.c_size_t()
        _check(lib().fdnn_model_blob_size(self.nativeDnnHandle, C.byref(n)))
        return int(n.value)

    def exportBlob(self, d_dst: int, capacity: int, stream: int = 0) -> None:
        _check(lib().fdnn_model_export_blob(self.nativeDnnHandle, C.c_void_p(d_dst), capacity, C.c_void_p(stream)))

    # -- per-kernel HIP-event timing ------------------------------------------
    PROF_KINDS = ("l0", "fix", "hidden_gemm", "output_gemm", "normalize")

    def raiseFuseFault(self, value: int = 1) -> None:
        """Tests: as if a fused soft-max launch of this model had just given up its bounded wait (1) / forget it (0)."""
        _check(lib().fdnn_debug_raise_fuse_fault(self.nativeDnnHandle, int(value)))

    def fuseGiveups(self) -> int:
        """Tiles of the fused soft-max that had to be finished by the clean-up kernel since load (fdnn_model_fuse_giveups)."""
        v = C.c_ulonglong(0)
        _check(lib().fdnn_model_fuse_giveups(self.nativeDnnHandle, C.byref(v)))
        return int(v.value)

    def chainFaults(self) -> int:
        """Waits of the chained hidden-layer kernel that ran into their bound since load (0 in a healthy setup)."""
        v = C.c_ulonglong()
        _check(lib().fdnn_model_chain_faults(self.nativeDnnHandle, C.byref(v)))
        return int(v.value)

    def deviceCounters(self, n: int = 32):
        a = (C.c_ulonglong * n)()
        _check(lib().fdnn_debug_device_counters(self.nativeDnnHandle, a, n))
        return list(a)

    def profileBegin(self) -> None:
        _check(lib().fdnn_profile_begin(self.nativeDnnHandle))

    def profileEnd(self) -> dict:
        ms = (C.c_double * 5)()
        cnt = (C.c_int * 5)()
        _check(lib().fdnn_profile_end(self.nativeDnnHandle, ms, cnt))
        return {k: {"ms": float(ms[i]), "launches": int(cnt[i])} for i, k in enumerate(self.PROF_KINDS)}

    def layer0(self, input):
        """Layer 0 alone through the production kernels: (u8 [n][hidden], outputs recomputed exactly)."""
        x = _f32(input)
        out = np.empty((x.shape[0], self.hiddenDimension()), dtype=np.uint8)
        rec = C.c_ulonglong()
        _check(lib().fdnn_debug_layer0(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), x.shape[0], out.ctypes.data_as(_c_u8p), C.byref(rec)))
        return out, int(rec.value)

    # -- parity taps ----------------------------------------------------------
    def layer0Screen(self, input):
        """(u8 [n][H], t~ [n][H], Dd [n][H], recomputed): the int8-screened input layer with what the screen saw per output."""
        x = _f32(input)
        H = self.hiddenDimension()
        out = np.empty((x.shape[0], H), dtype=np.uint8)
        t = np.empty((x.shape[0], H), dtype=np.float32)
        dd = np.empty((x.shape[0], H), dtype=np.float32)
        rec = C.c_ulonglong(0)
        _check(lib().fdnn_debug_layer0_screen(self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), x.shape[0], out.ctypes.data_as(_c_u8p),
                                              t.ctypes.data_as(_c_f32p), dd.ctypes.data_as(_c_f32p), C.byref(rec)))
        return out, t, dd, int(rec.value)

    def productionOutputAcc(self, input, stride: int, masks=None, probs: bool = False):
        """int32 accumulators of the output layer's PRODUCTION kernel instance for every stride-th frame
        ([ceil(n/stride)][O]); with probs=True also the call's probabilities."""
        x = _f32(input)
        n, O = x.shape[0], self.outputDimension()
        acc = np.empty(((n + stride - 1) // stride, O), dtype=np.int32)
        pr = np.empty((n, O), dtype=np.float32) if probs else None
        m = None
        if masks is not None:
            m = np.ascontiguousarray(masks, dtype=np.int8)
            assert m.shape == (n, O)
        _check(lib().fdnn_debug_production_acc_out(
            self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, stride, m.ctypes.data_as(_c_i8p) if m is not None else None,
            acc.ctypes.data_as(_c_i32p), pr.ctypes.data_as(_c_f32p) if pr is not None else None))
        return (acc, pr) if probs else acc

    def forwardTaps(self, input, masks=None) -> dict:
        x = _f32(input)
        n, H, O = x.shape[0], self.hiddenDimension(), self.outputDimension()
        nh = self.layerCount() - 1
        t = dict(
            l0_lin=np.empty((n, H), dtype=np.float32),
            u8_acts=np.empty((nh, n, H), dtype=np.uint8),
            acc_hid=np.empty((nh - 1, n, H), dtype=np.int32),
            acc_out=np.empty((n, O), dtype=np.int32),
            logits=np.empty((n, O), dtype=np.float32),
            probs=np.empty((n, O), dtype=np.float32),
        )
        m = None
        if masks is not None:
            m = np.ascontiguousarray(masks, dtype=np.int8)
            assert m.shape == (n, O)
        _check(lib().fdnn_debug_forward_taps(
            self.nativeDnnHandle, x.ctypes.data_as(_c_f32p), n, m.ctypes.data_as(_c_i8p) if m is not None else None,
            t["l0_lin"].ctypes.data_as(_c_f32p), t["u8_acts"].ctypes.data_as(_c_u8p), t["acc_hid"].ctypes.data_as(_c_i32p),
            t["acc_out"].ctypes.data_as(_c_i32p), t["logits"].ctypes.data_as(_c_f32p), t["probs"].ctypes.data_as(_c_f32p)))
        return t


class HostModel:
    """Load-time half only (no device): .bin parse + quantizer + packed sections."""

    def __init__(self, path: str, cutoff: float = 3.0):
        h = C.c_void_p()
        _check(lib().fdnn_host_model_load(os.path.abspath(path).encode(), cutoff, C.byref(h)))
        self.h = h.value
        L = lib()
        self.n_layers = L.fdnn_host_model_layers(self.h)

    def close(self):
        if self.h:
            lib().fdnn_host_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def layer_in(self, j):
        return lib().fdnn_host_model_layer_in(self.h, j)

    def layer_out(self, j):
        return lib().fdnn_host_model_layer_out(self.h, j)

    def multiplier(self, j) -> float:
        return float(lib().fdnn_host_model_multiplier(self.h, j))

    def weights_q(self, j) -> np.ndarray:
        out = np.empty((self.layer_out(j), self.layer_in(j)), dtype=np.int8)
        _check(lib().fdnn_host_model_weights_q(self.h, j, out.ctypes.data_as(_c_i8p)))
        return out

    def bias(self, j) -> np.ndarray:
        out = np.empty(self.layer_out(j), dtype=np.float32)
        _check(lib().fdnn_host_model_bias(self.h, j, out.ctypes.data_as(_c_f32p)))
        return out

    def wsum128(self, j) -> np.ndarray:
        out = np.empty(self.layer_out(j), dtype=np.int32)
        _check(lib().fdnn_host_model_wsum128(self.h, j, out.ctypes.data_as(_c_i32p)))
        return out

    def risky_pairs(self, j) -> int:
        return int(lib().fdnn_host_model_risky_pairs(self.h, j))

    def blob_size(self) -> int:
        return int(lib().fdnn_host_model_blob_size(self.h))

    def blob(self) -> np.ndarray:
        out = np.empty(self.blob_size(), dtype=np.uint8)
        _check(lib().fdnn_host_model_blob(self.h, out.ctypes.data_as(C.c_void_p), out.size))
        return out


def host_blob_check(blob: np.ndarray) -> dict:
    """Receiver-side validation of a broadcast weight blob (no device needed)."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    d = [C.c_int() for _ in range(4)]
    _check(lib().fdnn_host_blob_check(blob.ctypes.data_as(C.c_void_p), blob.size, *[C.byref(v) for v in d]))
    return dict(zip(("input_dim", "hidden_dim", "output_dim", "n_affine"), (int(v.value) for v in d)))


def frame_chunks(n: int, chained: bool = True):
    """(first frame, frame count) of every chunk a pass over ``n`` frames runs as (host logic, no device needed); ``chained``:
    whether the batch's hidden layers run as one chained launch (if not, a small tail past a whole round is split off)."""
    buf = (C.c_int * 4096)()
    k = lib().fdnn_debug_frame_chunks_for(int(n), 1 if chained else 0, buf, 2048)
    if k < 0:
        raise ValueError("fdnn_debug_frame_chunks")
    return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(k)]


def host_sigmoid_lut() -> np.ndarray:
    out = np.empty(1280, dtype=np.uint8)
    _check(lib().fdnn_host_sigmoid_lut(out.ctypes.data_as(_c_u8p)))
    return out


def host_quantize(w, cutoff: float = 3.0):
    w = _f32(w)
    out = np.empty(w.shape, dtype=np.int8)
    mult = C.c_float()
    _check(lib().fdnn_host_quantize(w.ctypes.data_as(_c_f32p), w.shape[0], w.shape[1], cutoff, out.ctypes.data_as(_c_i8p),
                                    C.byref(mult)))
    return out, float(mult.value)


# ------------------------------------------------------------------------------------------------ the unquantized net
FLOAT_LAUNCH_KINDS = ("fgemm.sigmoid", "fgemm.exp", "fgemm.sigmoid.tap", "fgemm.exp.tap", "input_step", "report.rows", "report.nodes",
                      "report.fold")


def float_launches() -> dict:
    """Process-wide launch counts of the float net's and the report's kernels since load (``fdnn_debug_float_launches``)."""
    buf = (C.c_ulonglong * len(FLOAT_LAUNCH_KINDS))()
    if lib().fdnn_debug_float_launches(buf, len(FLOAT_LAUNCH_KINDS)) != len(FLOAT_LAUNCH_KINDS):
        raise RuntimeError("fdnn_debug_float_launches")
    return dict(zip(FLOAT_LAUNCH_KINDS, (int(v) for v in buf)))


def float_layer_ref(weights, bias, input) -> np.ndarray:
    """The host restatement of one layer's sums (``fdnn_debug_float_layer_ref``, no device): per output, s = 0, for k
    ascending s = fmaf(x[k], w[k], s), then s + bias.  weights [rows][K], input [n][K] -> [n][rows]."""
    w, b, x = _f32(weights), _f32(bias), _f32(input)
    if w.ndim != 2 or x.ndim != 2 or x.shape[1] != w.shape[1] or b.shape != (w.shape[0],):
        raise ValueError("weights [rows][K], bias [rows], input [n][K]")
    out = np.empty((x.shape[0], w.shape[0]), dtype=np.float32)
    _check(lib().fdnn_debug_float_layer_ref(w.ctypes.data_as(_c_f32p), b.ctypes.data_as(_c_f32p), w.shape[0], w.shape[1],
                                            x.ctypes.data_as(_c_f32p), x.shape[0], out.ctypes.data_as(_c_f32p)))
    return out


def float_input_ref(shift, scale, input):
    """The host restatement of the input step (``fdnn_debug_float_input_ref``, no device) -> (x + shift, (x + shift) * scale)."""
    sh, sc, x = _f32(shift), _f32(scale), _f32(input)
    if x.ndim != 2 or sh.shape != (x.shape[1],) or sc.shape != sh.shape:
        raise ValueError("shift [dim], scale [dim], input [n][dim]")
    lin, act = np.empty_like(x), np.empty_like(x)
    _check(lib().fdnn_debug_float_input_ref(sh.ctypes.data_as(_c_f32p), sc.ctypes.data_as(_c_f32p), x.shape[1], x.ctypes.data_as(_c_f32p),
                                            x.shape[0], lin.ctypes.data_as(_c_f32p), act.ctypes.data_as(_c_f32p)))
    return lin, act


class FloatDnn:
    """The UNQUANTIZED net (``suskun.nn.FeedForwardNetwork``) on one MI355X: fp32 GEMMs on the f32-input MFMA.  The yardstick
    the quantized scorer is measured against, and a scorer in its own right."""

    def __init__(self, handle: int):
        self.nativeHandle = handle

    @staticmethod
    def loadFromFile(dnnFile: str, device: Optional[int] = None) -> "FloatDnn":
        h = C.c_void_p()
        path = os.path.abspath(dnnFile).encode()
        if device is None:
            _check(lib().fdnn_float_model_load(path, C.byref(h)))
        else:
            _check(lib().fdnn_float_model_load_on(path, int(device), C.byref(h)))
        return FloatDnn(h.value)

    def delete(self) -> None:
        if self.nativeHandle:
            lib().fdnn_float_model_free(self.nativeHandle)
            self.nativeHandle = None

    def inputDimension(self) -> int:
        return lib().fdnn_float_model_input_dim(self.nativeHandle)

    def outputDimension(self) -> int:
        return lib().fdnn_float_model_output_dim(self.nativeHandle)

    def layerCount(self) -> int:
        return lib().fdnn_float_model_layer_count(self.nativeHandle)

    def layerDimension(self, layerIndex: int) -> int:
        return lib().fdnn_float_model_layer_dim(self.nativeHandle, int(layerIndex))

    def device(self) -> int:
        return lib().fdnn_float_model_device(self.nativeHandle)

    def calculate(self, input) -> np.ndarray:
        """``FeedForwardNetwork.calculate`` (:133-148): [n][inputDimension] -> soft-max rows [n][outputDimension]."""
        x = _f32(input)
        if x.shape[0] == 0:
            return np.zeros((0, 0), dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.inputDimension():
            raise ValueError(f"Input vector size {x.shape[-1]} must be equal with network input size {self.inputDimension()}")
        out = np.empty((x.shape[0], self.outputDimension()), dtype=np.float32)
        _check(lib().fdnn_float_calculate(self.nativeHandle, x.ctypes.data_as(_c_f32p), x.shape[0], x.shape[1], out.ctypes.data_as(_c_f32p)))
        return out

    def calculateDevice(self, d_x: int, n: int, d_out: int, stream: int = 0) -> None:
        """Device-resident form: raw device pointers (e.g. ``tensor.data_ptr()``), enqueued on ``stream``, not synchronised."""
        _check(lib().fdnn_float_calculate_device(self.nativeHandle, C.c_void_p(d_x), int(n), C.c_void_p(d_out), C.c_void_p(stream)))

    def setChunk(self, rows: int) -> None:
        """Frames per internal chunk (``fdnn_debug_float_set_chunk``; 0 = default).  Results never depend on it."""
        _check(lib().fdnn_debug_float_set_chunk(self.nativeHandle, int(rows)))

    def layer(self, j: int, input):
        """ONE layer on the caller's rows (``fdnn_debug_float_layer``) -> (z, activation); j == -1 is the input step ->
        (x + shift, (x + shift) * scale)."""
        x = _f32(input)
        width = self.inputDimension() if j < 0 else self.layerDimension(j)
        if width < 0:
            raise ValueError(f"layer index {j} outside -1 .. {self.layerCount() - 1}")
        lin = np.empty((x.shape[0], width), dtype=np.float32)
        act = np.empty_like(lin)
        _check(lib().fdnn_debug_float_layer(self.nativeHandle, int(j), x.ctypes.data_as(_c_f32p), x.shape[0], lin.ctypes.data_as(_c_f32p),
                                            act.ctypes.data_as(_c_f32p)))
        return lin, act

    def layerMicros(self, j: int, input, reps: int = 10) -> float:
        """Device microseconds per run of layer j on the caller's rows: one upload, a warm-up run, ``reps`` runs back to back
        between two events (``fdnn_debug_float_layer_us``; measurement only)."""
        x = _f32(input)
        us = C.c_double()
        _check(lib().fdnn_debug_float_layer_us(self.nativeHandle, int(j), x.ctypes.data_as(_c_f32p), x.shape[0], int(reps), C.byref(us)))
        return float(us.value)


class _Accuracy(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("nan_rows", C.c_uint64), ("top1_agree", C.c_uint64), ("nodes_over", C.c_uint64),
                ("sum_abs", C.c_double), ("max_abs", C.c_double), ("max_node_sum", C.c_double)]


class AccuracyReport:
    """``FuncTest.diff`` on the device (``fdnn_report_*``): accumulates over any number of ``add`` calls."""

    def __init__(self, outputDimension: int, device: int = 0):
        h = C.c_void_p()
        _check(lib().fdnn_report_create(int(device), int(outputDimension), C.byref(h)))
        self.h = h.value
        self.O = int(outputDimension)

    def delete(self) -> None:
        if self.h:
            lib().fdnn_report_free(self.h)
            self.h = None

    def reset(self) -> None:
        _check(lib().fdnn_report_reset(self.h))

    def add(self, reference, quantized) -> None:
        r, q = _f32(reference), _f32(quantized)
        if r.ndim != 2 or r.shape != q.shape or r.shape[1] != self.O:
            raise ValueError(f"reference and quantized must both be [n][{self.O}]")
        _check(lib().fdnn_report_add(self.h, r.ctypes.data_as(_c_f32p), q.ctypes.data_as(_c_f32p), r.shape[0]))

    def addDevice(self, d_ref: int, d_q: int, n: int, stream: int = 0) -> None:
        _check(lib().fdnn_report_add_device(self.h, C.c_void_p(d_ref), C.c_void_p(d_q), int(n), C.c_void_p(stream)))

    def read(self, threshold: float = 0.1, nodeSums: bool = False) -> dict:
        """The keys of ``convert.quantization_report`` plus ``nan_rows`` (rows with a NaN in either matrix: counted there, left
        out of everything else); with ``nodeSums`` also ``node_sum`` [outputDimension] float64."""
        a = _Accuracy()
        ns = np.empty(self.O, dtype=np.float64) if nodeSums else None
        _check(lib().fdnn_report_read(self.h, float(threshold), C.byref(a), ns.ctypes.data_as(C.POINTER(C.c_double)) if nodeSums else None))
        used = int(a.frames) - int(a.nan_rows)
        out = {
            "frames": int(a.frames),
            "nodes": self.O,
            "nodes_over_0.1" if threshold == 0.1 else f"nodes_over_{threshold:g}": int(a.nodes_over),
            "max_node_sum_abs_diff": float(a.max_node_sum),
            "mean_abs_diff": float(a.sum_abs) / (used * self.O) if used else 0.0,
            "max_abs_diff": float(a.max_abs),
            "top1_agreement": int(a.top1_agree) / used if used else 0.0,
            "nan_rows": int(a.nan_rows),
            "sum_abs_diff": float(a.sum_abs),
            "top1_agree_rows": int(a.top1_agree),
        }
        if nodeSums:
            out["node_sum"] = ns
        return out
