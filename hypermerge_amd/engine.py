"""ctypes binding of the C-ABI in include/hypermerge_amd.h (libhmgpu.so).

This is the Python face of the boundary; the Node face is hypermerge_amd/js
(N-API).  There is no CPU fallback: if the HIP library or a GPU is missing,
``Engine()`` raises.
"""
from __future__ import annotations

import ctypes
import sys
import os
from typing import Optional, Sequence

import numpy as np

from .columnar import Batch, Results, CBatch, CResults

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.environ.get("HMGPU_LIB") or os.path.join(_HERE, "_lib", "libhmgpu.so")

# every symbol include/hypermerge_amd.h declares
EXPORTS = ("hm_abi_version", "hm_status_message", "hm_engine_create", "hm_engine_destroy",
           "hm_engine_last_error", "hm_merge_host", "hm_scratch_bytes", "hm_merge_device",
           "hm_last_kernel_ms", "hm_last_deferred", "hm_clock_cmp_device", "hm_clock_union_device",
           "hm_clock_intersection_device", "hm_store_create", "hm_store_destroy", "hm_doc_open",
           "hm_batch_submit", "hm_batch_wait", "hm_doc_info", "hm_doc_read", "hm_doc_log",
           "hm_doc_history_prefix", "hm_doc_set_min_clock", "hm_store_clock_update", "hm_sync_ranges_device",
           "hm_comm_unique_id", "hm_comm_create", "hm_comm_destroy", "hm_comm_group_start", "hm_comm_group_end",
           "hm_clock_records_scratch_bytes", "hm_clock_records_device", "hm_clock_count_allgather",
           "hm_clock_allgather", "hm_clock_min_allreduce", "hm_comm_create_local", "hm_clock_exchange_host",
           "hm_clock_min_host", "hm_decode_blocks", "hm_decoded_batch", "hm_decoded_status", "hm_decoded_n_strings",
           "hm_decoded_string", "hm_decoded_actor", "hm_decoded_obj", "hm_decoded_reg", "hm_decoded_free",
           "hm_store_set_incremental", "hm_store_last_routing", "hm_store_last_kernel_ms", "hm_store_inc_states", "hm_store_arena_info", "hm_debug_async_check", "hm_debug_inc_paths", "hm_debug_small_occupancy", "hm_doc_open_n", "hm_doc_reset", "hm_store_read_regs", "hm_store_read_history",
           "hm_cursors_create", "hm_cursors_destroy", "hm_cursors_reserve", "hm_cursors_update", "hm_cursors_get",
           "hm_cursors_entry", "hm_cursors_docs_with_actors", "hm_docset_create", "hm_docset_destroy",
           "hm_docset_engine", "hm_docset_open", "hm_docset_apply", "hm_text_data", "hm_text_results", "hm_text_free",
           "hm_docset_doc_info", "hm_docset_history_prefix", "hm_docset_clock_update", "hm_docset_view",
           "hm_docset_stats", "hm_docset_routing", "hm_docset_handles", "hm_sync_ranges_host", "hm_batch_submit_device", "hm_batch_wait_device",
           "hm_batch_undo", "hm_store_blocked", "hm_store_waiting", "hm_store_read_queue", "hm_missing_deps_device",
           "hm_missing_deps_host", "hm_docset_blocked", "hm_docset_waiting", "hm_store_missing_changes",
           "hm_missing_changes_device", "hm_missing_changes_host", "hm_docset_missing_changes",
           "hm_store_past_sizes", "hm_store_materialize", "hm_materialize_work_bytes", "hm_materialize_device",
           "hm_docset_materialize", "hm_store_op_diff_sizes", "hm_store_op_diffs", "hm_op_diffs_work_bytes",
           "hm_op_diffs_device", "hm_op_diffs_host", "hm_docset_materialize_patch",
           "hm_store_op_diff_sizes_ex", "hm_store_op_diffs_ex", "hm_op_diffs_work_bytes_ex", "hm_op_diffs_device_ex",
           "hm_op_diffs_host_ex", "hm_docset_materialize_patch_ex", "hm_docset_diff_stats",
           "hm_store_fields", "hm_fields_device", "hm_fields_host", "hm_docset_fields",
           "hm_store_op_diff_sizes_at", "hm_store_op_diffs_at", "hm_op_diffs_at_work_bytes", "hm_op_diffs_at_device",
           "hm_op_diffs_at_host", "hm_docset_materialize_patch_at", "hm_store_fork_submit", "hm_docset_fork",
           "hm_store_merge_from_submit", "hm_docset_merge_from", "hm_docset_merge_stats",
           "hm_store_state_sizes", "hm_store_state", "hm_state_work_bytes", "hm_state_device", "hm_state_host",
           "hm_docset_views", "hm_docset_get_patch")

_lib = None


class EngineError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise EngineError(f"{LIB} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        # PyTorch-ROCm bundles its own libamdhip64.so.7 (same soname as /opt/rocm's).  Whichever
        # loads first serves the whole process, so let torch's load first: then device pointers
        # and streams from torch tensors are valid in this library's calls.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB)
        L.hm_abi_version.restype = ctypes.c_uint32
        L.hm_status_message.argtypes = [ctypes.c_int]
        L.hm_status_message.restype = ctypes.c_char_p
        L.hm_engine_create.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        L.hm_engine_destroy.argtypes = [ctypes.c_void_p]
        L.hm_engine_last_error.argtypes = [ctypes.c_void_p]
        L.hm_engine_last_error.restype = ctypes.c_char_p
        L.hm_merge_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(CBatch), ctypes.POINTER(CResults)]
        L.hm_merge_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(CBatch), ctypes.POINTER(CResults),
                                      ctypes.c_void_p, ctypes.c_void_p]
        L.hm_scratch_bytes.argtypes = [ctypes.POINTER(CBatch)]
        L.hm_scratch_bytes.restype = ctypes.c_size_t
        L.hm_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
        L.hm_last_deferred.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        for f in ("hm_clock_cmp_device", "hm_clock_union_device", "hm_clock_intersection_device"):
            getattr(L, f).argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 3 + [ctypes.c_uint32] * 2 + [ctypes.c_void_p]
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        sig = {
            "hm_store_create": [vp, vp, vp], "hm_store_destroy": [vp], "hm_doc_open": [vp, vp],
            "hm_batch_submit": [vp, vp, vp, vp, vp], "hm_batch_wait": [vp, ctypes.c_uint64, vp, vp, vp, vp],
            "hm_batch_submit_device": [vp, vp, vp, vp, vp], "hm_batch_wait_device": [vp, ctypes.c_uint64, vp, vp],
            "hm_batch_undo": [vp, ctypes.c_uint64],
            "hm_doc_info": [vp, u32, vp], "hm_doc_read": [vp, u32] + [vp] * 7, "hm_doc_log": [vp, u32, vp, vp, vp],
            "hm_doc_history_prefix": [vp, u32, u32, vp], "hm_doc_set_min_clock": [vp, u32, vp],
            "hm_store_clock_update": [vp, u32, vp, vp, vp, vp],
            "hm_sync_ranges_device": [vp, vp, vp, vp, vp, vp, u32, vp],
            "hm_comm_unique_id": [vp], "hm_comm_create": [vp, ctypes.c_int, ctypes.c_int, vp, vp],
            "hm_comm_destroy": [vp], "hm_comm_group_start": [], "hm_comm_group_end": [],
            "hm_clock_records_scratch_bytes": [u32, u32],
            "hm_clock_records_device": [vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp],
            "hm_clock_count_allgather": [vp, ctypes.c_uint64, vp, vp],
            "hm_clock_allgather": [vp, vp, vp, vp, vp], "hm_clock_min_allreduce": [vp, vp, ctypes.c_uint64, vp],
            "hm_comm_create_local": [vp, ctypes.c_int, vp],
            "hm_clock_exchange_host": [vp, ctypes.c_int, vp, vp, vp, ctypes.c_uint64, vp],
            "hm_clock_min_host": [vp, ctypes.c_int, vp, ctypes.c_uint64],
            "hm_decode_blocks": [vp, vp, vp, u32, u32, ctypes.c_int, vp], "hm_decoded_batch": [vp, vp],
            "hm_decoded_status": [vp], "hm_decoded_n_strings": [vp], "hm_decoded_string": [vp, u32, vp],
            "hm_decoded_actor": [vp, u32, u32, vp], "hm_decoded_free": [vp],
            "hm_decoded_obj": [vp, u32, u32, vp], "hm_decoded_reg": [vp, u32, u32, vp, vp],
            "hm_store_set_incremental": [vp, ctypes.c_int], "hm_store_last_routing": [vp, vp], "hm_store_last_kernel_ms": [vp, vp], "hm_store_inc_states": [vp, vp], "hm_store_arena_info": [vp, vp, vp], "hm_debug_async_check": [vp, ctypes.c_int], "hm_debug_inc_paths": [vp, ctypes.c_int, ctypes.c_int], "hm_debug_small_occupancy": [vp, vp, vp],
            "hm_doc_open_n": [vp, u32, vp], "hm_doc_reset": [vp, vp, u32], "hm_store_read_regs": [vp, u32, vp, vp, vp, vp, u32, vp],
            "hm_store_read_history": [vp, u32, vp, vp, vp, vp, vp, vp],
            "hm_cursors_create": [vp, u32, vp], "hm_cursors_destroy": [vp], "hm_cursors_reserve": [vp, u32],
            "hm_cursors_update": [vp, u32, vp, vp, vp, vp, vp], "hm_cursors_get": [vp, u32, vp, vp, vp, vp],
            "hm_cursors_entry": [vp, u32, vp, vp, vp],
            "hm_cursors_docs_with_actors": [vp, u32, vp, vp, u32, vp, vp, vp, vp],
            "hm_docset_create": [vp, vp, vp], "hm_docset_destroy": [vp], "hm_docset_engine": [vp],
            "hm_docset_open": [vp, u32, vp], "hm_docset_apply": [vp, vp, vp, vp, vp, u32, vp],
            "hm_text_data": [vp, vp], "hm_text_results": [vp, vp], "hm_text_free": [vp],
            "hm_docset_doc_info": [vp, u32, vp], "hm_docset_history_prefix": [vp, u32, u32, vp],
            "hm_docset_clock_update": [vp, u32, vp, vp, vp, vp], "hm_docset_view": [vp, u32, vp],
            "hm_docset_stats": [vp, vp], "hm_docset_diff_stats": [vp, vp], "hm_docset_routing": [vp, vp], "hm_docset_handles": [vp, u32, vp, vp], "hm_sync_ranges_host": [vp, vp, vp, vp, vp, vp, u32, u32],
            "hm_store_blocked": [vp, vp, u32, vp], "hm_store_waiting": [vp, u32, vp, vp, vp, vp],
            "hm_store_read_queue": [vp, u32, vp, vp, vp],
            "hm_missing_deps_device": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), vp, vp],
            "hm_missing_deps_host": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), vp],
            "hm_docset_blocked": [vp, vp, u32, vp], "hm_docset_waiting": [vp, u32, vp, vp],
            "hm_store_missing_changes": [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, u32, vp],
            "hm_missing_changes_device": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), vp, vp, vp, u32, u32,
                                          vp, vp, vp, u32, vp, vp, vp],
            "hm_missing_changes_host": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), vp, vp, vp, u32,
                                        vp, vp, vp, u32, vp],
            "hm_docset_missing_changes": [vp, u32, vp, vp, vp, vp, vp, u32, vp],
            "hm_store_past_sizes": [vp, u32, vp, vp, vp, vp, vp],
            "hm_store_materialize": [vp, u32, vp, vp, vp, vp, vp],
            "hm_store_fork_submit": [vp, u32, vp, vp, vp, vp, vp, u32, vp],
            "hm_docset_fork": [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp],
            "hm_store_merge_from_submit": [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp],
            "hm_docset_merge_from": [vp, u32, vp, vp, vp, vp, vp, vp, vp], "hm_docset_merge_stats": [vp, vp],
            "hm_materialize_work_bytes": [u32],
            "hm_docset_materialize": [vp, u32, vp, vp, vp, vp, vp, vp, vp],
            "hm_materialize_device": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), u32, vp, vp, vp, vp, vp, vp, vp],
            "hm_docset_materialize_patch": [vp, u32, vp, vp, vp],
            "hm_store_op_diff_sizes": [vp, u32, vp, vp, vp, vp, vp, vp],
            "hm_store_op_diffs": [vp, u32, vp, vp, vp, vp, vp],
            "hm_op_diffs_work_bytes": [ctypes.POINTER(CBatch), u32],
            "hm_op_diffs_device": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), u32, vp, vp, vp, vp, vp, vp, vp],
            "hm_op_diffs_host": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), u32, vp, vp, vp, vp, vp],
            "hm_docset_materialize_patch_ex": [vp, u32, vp, vp, u32, vp],
            "hm_store_state_sizes": [vp, u32, vp, vp, vp, vp],
            "hm_store_state": [vp, u32, vp, vp, vp, vp, vp],
            "hm_state_work_bytes": [u32],
            "hm_state_device": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), u32, vp, vp, vp, vp, vp, vp, vp],
            "hm_state_host": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), u32, vp, vp, vp, vp, vp],
            "hm_docset_views": [vp, u32, vp, ctypes.POINTER(vp)],
            "hm_docset_get_patch": [vp, u32, vp, ctypes.POINTER(vp)],
            "hm_store_op_diff_sizes_ex": [vp, u32, vp, vp, vp, vp, vp, vp, u32],
            "hm_store_op_diffs_ex": [vp, u32, vp, vp, vp, vp, vp, vp, u32],
            "hm_op_diffs_work_bytes_ex": [ctypes.POINTER(CBatch), u32, u32],
            "hm_op_diffs_device_ex": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), u32, vp, vp, vp, vp, vp, vp, vp, vp, u32],
            "hm_op_diffs_host_ex": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), u32, vp, vp, vp, vp, vp, vp, u32],
            "hm_store_op_diff_sizes_at": [vp, u32, vp, vp, vp, vp, vp, u32],
            "hm_store_op_diffs_at": [vp, u32, vp, vp, vp, vp, vp, u32],
            "hm_op_diffs_at_work_bytes": [ctypes.POINTER(CBatch), u32, u32],
            "hm_op_diffs_at_device": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), u32, vp, vp, vp, vp, vp, vp, vp, u32],
            "hm_op_diffs_at_host": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), u32, vp, vp, vp, vp, vp, u32],
            "hm_docset_materialize_patch_at": [vp, u32, vp, vp, vp, vp, vp, u32, vp],
            "hm_store_fields": [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp],
            "hm_fields_device": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), vp, vp, vp, u32, vp, vp, u32,
                                 vp, vp, vp, vp, u32, vp, vp, vp],
            "hm_fields_host": [vp, ctypes.POINTER(CBatch), ctypes.POINTER(CResults), vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp],
            "hm_docset_fields": [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        }
        for f, a in sig.items():
            getattr(L, f).argtypes = a
        L.hm_store_destroy.restype = None
        L.hm_cursors_destroy.restype = None
        L.hm_comm_destroy.restype = None
        L.hm_decoded_status.restype = ctypes.POINTER(ctypes.c_int32)
        L.hm_decoded_n_strings.restype = ctypes.c_uint32
        L.hm_decoded_string.restype = ctypes.c_void_p
        L.hm_decoded_actor.restype = ctypes.c_void_p
        L.hm_decoded_obj.restype = ctypes.c_void_p
        L.hm_decoded_reg.restype = ctypes.c_void_p
        L.hm_decoded_free.restype = None
        L.hm_clock_records_scratch_bytes.restype = ctypes.c_size_t
        L.hm_materialize_work_bytes.restype = ctypes.c_size_t
        L.hm_op_diffs_work_bytes.restype = ctypes.c_size_t
        L.hm_op_diffs_work_bytes_ex.restype = ctypes.c_size_t
        L.hm_op_diffs_at_work_bytes.restype = ctypes.c_size_t
        L.hm_state_work_bytes.restype = ctypes.c_size_t
        L.hm_docset_destroy.restype = None
        L.hm_docset_engine.restype = ctypes.c_void_p
        L.hm_text_data.restype = ctypes.c_void_p
        L.hm_text_results.restype = ctypes.c_void_p
        L.hm_text_free.restype = None
        _lib = L
    return _lib


MC_RAW, MC_ONLY_LISTED = 1, 2   # HM_MC_*


class CPastOut(ctypes.Structure):
    """struct hm_past_out"""
    _fields_ = [("cap_changes", ctypes.c_uint32), ("cap_deps", ctypes.c_uint32), ("cap_ops", ctypes.c_uint32),
                ("cap_regs", ctypes.c_uint32), ("docs", ctypes.c_void_p), ("changes", ctypes.c_void_p),
                ("deps", ctypes.c_void_p), ("ops", ctypes.c_void_p), ("change_log", ctypes.c_void_p),
                ("op_log", ctypes.c_void_p), ("res", CResults)]


class CPastSummary(ctypes.Structure):
    """struct hm_past_summary"""
    _fields_ = [("totals", ctypes.c_uint64 * 4)] + [(f, ctypes.c_uint32) for f in (
        "max_changes", "max_ops", "max_regs", "max_objs", "max_deps", "doc_flags", "bad", "pad")]


assert ctypes.sizeof(CPastSummary) == 64


OD_CREATE, OD_SET, OD_REMOVE = 0, 1, 2   # HM_OD_* row kinds
OD_LISTS = 1                              # HM_OD_LISTS request flag
OD_ELEM_INSERT, OD_ELEM_SET, OD_ELEM_REMOVE = 3, 4, 5   # HM_OD_ELEM_* row kinds (ODF_LISTS)
ODF_LISTS = 1                             # HM_ODF_LISTS option: answer list / text element assigns
ODF_ONCE = 2                              # HM_ODF_ONCE option (hm_store_op_diffs_ex): one walk into guessed tables
OP_DIFF_DT = np.dtype([("op", "<u4"), ("kind", "<u4"), ("n_surv", "<u4"), ("surv_off", "<u4")])


class COpDiffOut(ctypes.Structure):
    """struct hm_op_diff_out"""
    _fields_ = [("cap_rows", ctypes.c_uint32), ("cap_surv", ctypes.c_uint32), ("rows", ctypes.c_void_p),
                ("surv", ctypes.c_void_p), ("range", ctypes.c_void_p), ("flags", ctypes.c_void_p)]


class COpDiffSummary(ctypes.Structure):
    """struct hm_op_diff_summary"""
    _fields_ = [("totals", ctypes.c_uint64 * 4), ("max_rows", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3),
                ("max_surv", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("bad", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


assert ctypes.sizeof(COpDiffSummary) == 64 and OP_DIFF_DT.itemsize == 16


ST_BAD_ROWS = 1                           # HM_ST_BAD_ROWS request flag
STATE_ROW_DT = np.dtype([("reg", "<u4"), ("obj", "<u4"), ("index", "<i4"), ("n_surv", "<u4"), ("surv_off", "<u4")])


class CStateOut(ctypes.Structure):
    """struct hm_state_out"""
    _fields_ = [("cap_rows", ctypes.c_uint32), ("cap_surv", ctypes.c_uint32), ("rows", ctypes.c_void_p),
                ("surv", ctypes.c_void_p), ("range", ctypes.c_void_p), ("flags", ctypes.c_void_p)]


class CStateSummary(ctypes.Structure):
    """struct hm_state_summary"""
    _fields_ = [("totals", ctypes.c_uint64 * 2), ("reserved64", ctypes.c_uint64 * 2), ("max_rows", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 3), ("max_surv", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("bad", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


assert ctypes.sizeof(CStateSummary) == 64 and STATE_ROW_DT.itemsize == 20


FLD_NOT_READY, FLD_BAD_ROWS = 1, 2          # HM_FLD_* request flags
FIELD_OP_DT = np.dtype([("op", "<u4"), ("seq", "<u4"), ("actor", "<u2"), ("action", "u1"), ("datatype", "u1"),
                        ("vtag", "u1"), ("covered", "u1"), ("pad", "<u2"), ("value", "<u8")])   # struct hm_field_op
assert FIELD_OP_DT.itemsize == 24


def pack_fields(fields, n: int):
    """Per request a sequence of registers as the C-ABI's field tables (field_off [n + 1] u32,
    field_reg u32)."""
    assert len(fields) == n, len(fields)
    off = np.zeros(n + 1, np.uint32)
    regs: list = []
    for i, f in enumerate(fields):
        regs.extend(int(r) for r in f)
        off[i + 1] = len(regs)
    return off, np.array(regs + [0], np.uint32)


def unpack_fields(n, foff, flags, rng, rows):
    """The tables of a fields call as, per request, (ready, [rows of each field])."""
    out = []
    for i in range(n):
        fl = [rows[int(rng[f, 0]):int(rng[f, 0]) + int(rng[f, 1])].copy() for f in range(int(foff[i]), int(foff[i + 1]))]
        out.append((not int(flags[i]) & FLD_NOT_READY, fl))
    return out


def pack_entries(have, n: int):
    """have-clocks as the C-ABI's entry tables (entry_off [n + 1] u32, entry_actor u16, entry_seq u32):
    `have` is an [n, S] array of rank-indexed rows (its non-zero columns become entries, in rank
    order) or per request a sequence of (actor rank, seq) in the clock's key order."""
    off = np.zeros(n + 1, np.uint32)
    ea: list = []
    es: list = []
    if isinstance(have, np.ndarray) and have.ndim == 2:
        assert have.shape[0] == n, have.shape
        for i in range(n):
            nz = np.flatnonzero(have[i])
            ea.extend(int(a) for a in nz)
            es.extend(int(have[i, a]) for a in nz)
            off[i + 1] = len(ea)
    else:
        assert len(have) == n, len(have)
        for i, ents in enumerate(have):
            for a, q in ents:
                ea.append(int(a))
                es.append(min(max(int(q), 0), 0xFFFFFFFF))
            off[i + 1] = len(ea)
    return off, np.array(ea + [0], np.uint16), np.array(es + [0], np.uint32)


class _Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("flags", ctypes.c_int)]


GENERAL_ONLY = 1   # HM_CFG_GENERAL_ONLY


class Engine:
    def __init__(self, device: int = 0, flags: int = 0):
        L = lib()
        h = ctypes.c_void_p()
        cfg = _Config(device, flags)
        st = L.hm_engine_create(ctypes.byref(cfg), ctypes.byref(h))
        if st != 0:
            raise EngineError(f"hm_engine_create failed: {L.hm_status_message(st).decode()}")
        self._h = h
        self._L = L
        self.device = device

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.hm_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        # (at interpreter exit finalizers run in any order: the engine may be gone, and the
        # process releases the device anyway)
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int, what: str) -> None:
        if st != 0:
            msg = self._L.hm_engine_last_error(self._h).decode()
            raise EngineError(f"{what}: {self._L.hm_status_message(st).decode()} ({msg})")

    def merge(self, batch: Batch, results: Optional[Results] = None) -> Results:
        """Host batch -> GPU merge -> host results (synchronous)."""
        if results is None:
            results = Results.alloc(batch)
        cb, cr = batch.c_struct(), results.c_struct()
        self._check(self._L.hm_merge_host(self._h, ctypes.byref(cb), ctypes.byref(cr)), "hm_merge_host")
        return results

    def merge_device(self, cbatch: CBatch, cresults: CResults, stream: int = 0) -> None:
        """Device-resident merge: every pointer in the structs is a device pointer."""
        self._check(self._L.hm_merge_device(self._h, ctypes.byref(cbatch), ctypes.byref(cresults), None,
                                            ctypes.c_void_p(stream) if stream else None), "hm_merge_device")

    def missing_deps(self, batch: Batch, results: Results) -> np.ndarray:
        """getMissingDeps of every document of a merged batch: [n_docs, a_stride], per actor rank the
        largest seq a queued change needs that opSet.clock has not reached (0 = no entry); a
        document whose merge threw gets a zero row."""
        out = np.zeros((batch.n_docs, batch.a_stride), np.uint32)
        cb, cr = batch.c_struct(), results.c_struct()
        self._check(self._L.hm_missing_deps_host(self._h, ctypes.byref(cb), ctypes.byref(cr), out.ctypes.data),
                    "hm_missing_deps_host")
        return out

    def missing_deps_device(self, cbatch: CBatch, cresults: CResults, out_ptr: int, stream: int = 0) -> None:
        """The same with every table and the [n_docs * a_stride] u32 output in device memory
        (enqueued on the stream, not synchronised)."""
        self._check(self._L.hm_missing_deps_device(self._h, ctypes.byref(cbatch), ctypes.byref(cresults),
                                                   ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream) if stream else None),
                    "hm_missing_deps_device")

    def missing_changes(self, batch: Batch, results: Results, have, flags: int = 0, closure: bool = False):
        """getMissingChanges of every document of a merged batch: per document the document-local
        log indices, in history order, of the applied changes a peer with the clock `have` lacks.
        have: an [n_docs, a_stride] array of rank-indexed rows (0 = no entry; the entries are taken
        in rank order), or per document a sequence of (actor rank, seq) in the clock's key order.
        closure=True: also the [n_docs, a_stride] transitiveDeps rows.  A document whose merge threw
        offers nothing."""
        n, S = batch.n_docs, batch.a_stride
        off, ea, es = pack_entries(have, n)
        rng = np.zeros((max(n, 1), 2), np.uint32)
        clo = np.zeros((max(n, 1), S), np.uint32)
        cb, cr = batch.c_struct(), results.c_struct()
        cap = len(batch.changes)                       # (no document offers more than its own rows)
        out = np.zeros(max(cap, 1), np.uint32)
        tot = ctypes.c_uint32()
        self._check(self._L.hm_missing_changes_host(self._h, ctypes.byref(cb), ctypes.byref(cr), off.ctypes.data,
                                                    ea.ctypes.data, es.ctypes.data, flags, clo.ctypes.data,
                                                    rng.ctypes.data, out.ctypes.data, cap, ctypes.byref(tot)),
                    "hm_missing_changes_host")
        lists = [[int(x) for x in out[int(o):int(o) + int(c)]] for o, c in rng[:n]]
        return (lists, clo[:n]) if closure else lists

    def missing_changes_device(self, cbatch: CBatch, cresults: CResults, entry_off: int, entry_actor: int, entry_seq: int,
                               n_entries: int, flags: int, out_closure: int, out_range: int, out_log: int, cap: int,
                               out_total: int, out_bad: int, stream: int = 0) -> None:
        """The same with every table, the entry arrays and the outputs in device memory (pointers;
        out_total / out_bad are device words zeroed by the caller; enqueued, not synchronised)."""
        p = lambda x: ctypes.c_void_p(x) if x else None
        self._check(self._L.hm_missing_changes_device(self._h, ctypes.byref(cbatch), ctypes.byref(cresults), p(entry_off),
                                                      p(entry_actor), p(entry_seq), n_entries, flags, p(out_closure),
                                                      p(out_range), p(out_log), cap, p(out_total), p(out_bad), p(stream)),
                    "hm_missing_changes_device")

    def fields(self, batch: Batch, results: Results, have, fields, cap: Optional[int] = None, closure: bool = False):
        """hm_fields_host: the fields a proposed change touches, for every document of a merged batch.
        have: per document the would-be change's base clock as pack_entries takes it (its deps in key
        order with its own actor at seq - 1); fields: per document a sequence of registers.  Returns
        per document (ready, [FIELD_OP_DT rows of each field, winner first]); closure=True: also the
        [n_docs, a_stride] transitiveDeps rows.  A document whose merge threw offers nothing."""
        n, S = batch.n_docs, batch.a_stride
        off, ea, es = pack_entries(have, n)
        foff, freg = pack_fields(fields, n)
        nf = int(foff[-1])
        flags = np.zeros(max(n, 1), np.uint32)
        rng = np.zeros((nf + 1, 2), np.uint32)
        clo = np.zeros((max(n, 1), S), np.uint32)
        cb, cr = batch.c_struct(), results.c_struct()
        grow, cap = cap is None, max(64, 2 * nf) if cap is None else cap
        tot = ctypes.c_uint32()
        rows = np.zeros(max(cap, 1), FIELD_OP_DT)
        args = (self._h, ctypes.byref(cb), ctypes.byref(cr), off.ctypes.data, ea.ctypes.data, es.ctypes.data,
                foff.ctypes.data, freg.ctypes.data, flags.ctypes.data, clo.ctypes.data, rng.ctypes.data)
        st = self._L.hm_fields_host(*args, rows.ctypes.data, cap, ctypes.byref(tot))
        if grow and st == 34 and tot.value > cap:     # HM_ERR_NOMEM: tot = the rows needed
            cap = tot.value
            rows = np.zeros(cap, FIELD_OP_DT)
            st = self._L.hm_fields_host(*args, rows.ctypes.data, cap, ctypes.byref(tot))
        self._check(st, "hm_fields_host")
        out = unpack_fields(n, foff, flags, rng, rows)
        return (out, clo[:n]) if closure else out

    def fields_device(self, cbatch: CBatch, cresults: CResults, entry_off: int, entry_actor: int, entry_seq: int,
                      n_entries: int, field_off: int, field_reg: int, n_fields: int, out_flags: int, out_closure: int,
                      out_range: int, out_rows: int, cap: int, out_total: int, out_bad: int, stream: int = 0) -> None:
        """The same with every table, the request arrays and the outputs in device memory (pointers;
        out_total / out_bad are device words zeroed by the caller; enqueued, not synchronised)."""
        p = lambda x: ctypes.c_void_p(x) if x else None
        self._check(self._L.hm_fields_device(self._h, ctypes.byref(cbatch), ctypes.byref(cresults), p(entry_off),
                                             p(entry_actor), p(entry_seq), n_entries, p(field_off), p(field_reg), n_fields,
                                             p(out_flags), p(out_closure), p(out_range), p(out_rows), cap, p(out_total),
                                             p(out_bad), p(stream)), "hm_fields_device")

    def materialize_device(self, cbatch: CBatch, cresults: CResults, n: int, doc_index: int, hist_len: int,
                           clock_rows: int, out: "CPastOut", out_summary: int, work: int, stream: int = 0) -> None:
        """hm_materialize_device: documents of a merged cold batch gathered as they were at a history
        length or a clock, every table in device memory (pointers; `out` a CPastOut of device tables,
        `work` of work_bytes(n) bytes; enqueued, not synchronised)."""
        p = lambda x: ctypes.c_void_p(x) if x else None
        self._check(self._L.hm_materialize_device(self._h, ctypes.byref(cbatch), ctypes.byref(cresults), n, p(doc_index),
                                                  p(hist_len), p(clock_rows), ctypes.byref(out), p(out_summary), p(work),
                                                  p(stream)), "hm_materialize_device")

    def op_diffs_host(self, batch: Batch, results: Results, docs, frm, to, cap=None, lists=False):
        """hm_op_diffs_host: what each applied op of the history slices [frm[i], to[i]) of documents
        docs[i] of a merged batch did (None: every document, one request each).  Returns (rows
        OP_DIFF_DT, survivors SURV_RESULT_DT, ranges [n, 2] = first row and rows per request, flags [n]);
        a request flagged OD_LISTS has no rows.  cap = (rows, survivors) the tables hold (None: every
        op of the batch per request, which no slice exceeds in rows; survivors are sized by a first
        call's totals when that is too small).  lists=True (hm_op_diffs_host_ex with ODF_LISTS): list /
        text element assigns are answered as OD_ELEM_* rows and the rows' index table ([rows] u32, NONE
        where a row has none) is returned as a fifth element."""
        from .columnar import SURV_RESULT_DT
        opts = ODF_LISTS if lists else 0
        idx = None if docs is None else np.ascontiguousarray(docs, np.uint32)
        n = batch.n_docs if idx is None else len(idx)
        f, t = np.ascontiguousarray(frm, np.uint32), np.ascontiguousarray(to, np.uint32)
        assert len(f) == n and len(t) == n
        cb, cr = batch.c_struct(), results.c_struct()
        tot = (ctypes.c_uint64 * 2)()
        caps = cap if cap is not None else (0, 0)
        for _ in range(2):
            rows, surv = np.zeros(max(caps[0], 1), OP_DIFF_DT), np.zeros(max(caps[1], 1), SURV_RESULT_DT)
            rng, fl = np.zeros((max(n, 1), 2), np.uint32), np.zeros(max(n, 1), np.uint32)
            index = np.zeros(max(caps[0], 1), np.uint32)
            out = COpDiffOut(caps[0], caps[1], rows.ctypes.data, surv.ctypes.data, rng.ctypes.data, fl.ctypes.data)
            st = self._L.hm_op_diffs_host_ex(self._h, ctypes.byref(cb), ctypes.byref(cr), n,
                                             idx.ctypes.data if idx is not None and n else None,
                                             f.ctypes.data if n else None, t.ctypes.data if n else None, ctypes.byref(out),
                                             index.ctypes.data if lists else None, tot, opts)
            if st == 34 and cap is None and (tot[0] > caps[0] or tot[1] > caps[1]):   # HM_ERR_NOMEM: sized by the totals
                caps = (int(tot[0]), int(tot[1]))
                continue
            break
        self._check(st, "hm_op_diffs_host")
        base = (rows[:int(tot[0])], surv[:int(tot[1])], rng[:n], fl[:n])
        return base + (index[:int(tot[0])],) if lists else base

    def op_diffs_work_bytes(self, cbatch: CBatch, n: int, lists=False) -> int:
        return int(self._L.hm_op_diffs_work_bytes_ex(ctypes.byref(cbatch), n, ODF_LISTS if lists else 0))

    def op_diffs_device(self, cbatch: CBatch, cresults: CResults, n: int, doc_index: int, frm: int, to: int,
                        out: "COpDiffOut", out_summary: int, work: int, stream: int = 0, lists=False, out_index: int = 0) -> None:
        """hm_op_diffs_device: the same with every table in device memory (pointers; `out` a COpDiffOut of
        device tables, `work` of op_diffs_work_bytes(cbatch, n) bytes; enqueued, not synchronised).
        lists=True (hm_op_diffs_device_ex with ODF_LISTS): out_index = the device table of out.cap_rows
        u32 the rows' indexes go to, `work` of op_diffs_work_bytes(cbatch, n, lists=True) bytes."""
        p = lambda x: ctypes.c_void_p(x) if x else None
        self._check(self._L.hm_op_diffs_device_ex(self._h, ctypes.byref(cbatch), ctypes.byref(cresults), n, p(doc_index),
                                                  p(frm), p(to), ctypes.byref(out), p(out_index), p(out_summary), p(work),
                                                  p(stream), ODF_LISTS if lists else 0),
                    "hm_op_diffs_device")

    def op_diffs_at_host(self, batch: Batch, results: Results, docs, clocks, cap=None, lists=False):
        """hm_op_diffs_at_host: the per-op patch of documents docs[i] of a merged batch (None: every
        document, one request each) as they stood at the clocks clocks[i] ([n, a_stride] rank rows): what
        op_diffs_host returns, for the changes applied at each clock, from the empty document."""
        from .columnar import SURV_RESULT_DT
        opts = ODF_LISTS if lists else 0
        idx = None if docs is None else np.ascontiguousarray(docs, np.uint32)
        n = batch.n_docs if idx is None else len(idx)
        crow = np.ascontiguousarray(clocks, np.uint32).reshape(n, batch.a_stride)
        cb, cr = batch.c_struct(), results.c_struct()
        tot = (ctypes.c_uint64 * 2)()
        caps = cap if cap is not None else (0, 0)
        for _ in range(2):
            rows, surv = np.zeros(max(caps[0], 1), OP_DIFF_DT), np.zeros(max(caps[1], 1), SURV_RESULT_DT)
            rng, fl = np.zeros((max(n, 1), 2), np.uint32), np.zeros(max(n, 1), np.uint32)
            index = np.zeros(max(caps[0], 1), np.uint32)
            out = COpDiffOut(caps[0], caps[1], rows.ctypes.data, surv.ctypes.data, rng.ctypes.data, fl.ctypes.data)
            st = self._L.hm_op_diffs_at_host(self._h, ctypes.byref(cb), ctypes.byref(cr), n,
                                             idx.ctypes.data if idx is not None and n else None,
                                             crow.ctypes.data if n else None, ctypes.byref(out),
                                             index.ctypes.data if lists else None, tot, opts)
            if st == 34 and cap is None and (tot[0] > caps[0] or tot[1] > caps[1]):   # HM_ERR_NOMEM: sized by the totals
                caps = (int(tot[0]), int(tot[1]))
                continue
            break
        self._check(st, "hm_op_diffs_at_host")
        base = (rows[:int(tot[0])], surv[:int(tot[1])], rng[:n], fl[:n])
        return base + (index[:int(tot[0])],) if lists else base

    def op_diffs_at_work_bytes(self, cbatch: CBatch, n: int, lists=False) -> int:
        return int(self._L.hm_op_diffs_at_work_bytes(ctypes.byref(cbatch), n, ODF_LISTS if lists else 0))

    def op_diffs_at_device(self, cbatch: CBatch, cresults: CResults, n: int, doc_index: int, clock_rows: int,
                           out: "COpDiffOut", out_summary: int, work: int, stream: int = 0, lists=False, out_index: int = 0) -> None:
        """hm_op_diffs_at_device: the same with every table and the clock rows in device memory (pointers;
        `work` of op_diffs_at_work_bytes(cbatch, n, lists) bytes; enqueued, not synchronised)."""
        p = lambda x: ctypes.c_void_p(x) if x else None
        self._check(self._L.hm_op_diffs_at_device(self._h, ctypes.byref(cbatch), ctypes.byref(cresults), n, p(doc_index),
                                                  p(clock_rows), ctypes.byref(out), p(out_index), p(out_summary), p(work),
                                                  p(stream), ODF_LISTS if lists else 0),
                    "hm_op_diffs_at_device")

    def state_host(self, batch: Batch, results: Results, docs=None, cap=None, clocks=False):
        """hm_state_host: the current state of documents docs[i] of a merged batch (None: every document,
        one request each): per live register (n_surv > 0, obj known) one STATE_ROW_DT row in ascending
        register id, the survivors in row order.  Returns (rows, survivors SURV_RESULT_DT, ranges [n, 4] =
        first row, rows, first survivor, survivors per request, flags [n]); a request flagged ST_BAD_ROWS
        has no rows, as has a document whose status is not OK.  cap = (rows, survivors) the tables hold
        (None: sized by a first call's totals).  clocks=True: the requests' clock and heads rows
        ([n, a_stride] each) as a fifth and sixth element."""
        from .columnar import SURV_RESULT_DT
        idx = None if docs is None else np.ascontiguousarray(docs, np.uint32)
        n = batch.n_docs if idx is None else len(idx)
        S = batch.a_stride
        cb, cr = batch.c_struct(), results.c_struct()
        tot = (ctypes.c_uint64 * 2)()
        caps = cap if cap is not None else (0, 0)
        for _ in range(2):
            rows, surv = np.zeros(max(caps[0], 1), STATE_ROW_DT), np.zeros(max(caps[1], 1), SURV_RESULT_DT)
            rng, fl = np.zeros((max(n, 1), 4), np.uint32), np.zeros(max(n, 1), np.uint32)
            ck, hd = np.zeros((max(n, 1), S), np.uint32), np.zeros((max(n, 1), S), np.uint32)
            out = CStateOut(caps[0], caps[1], rows.ctypes.data, surv.ctypes.data, rng.ctypes.data, fl.ctypes.data)
            st = self._L.hm_state_host(self._h, ctypes.byref(cb), ctypes.byref(cr), n,
                                       idx.ctypes.data if idx is not None and n else None, ctypes.byref(out),
                                       ck.ctypes.data if clocks else None, hd.ctypes.data if clocks else None, tot)
            if st == 34 and cap is None and (tot[0] > caps[0] or tot[1] > caps[1]):   # HM_ERR_NOMEM: sized by the totals
                caps = (int(tot[0]), int(tot[1]))
                continue
            break
        self._check(st, "hm_state_host")
        base = (rows[:int(tot[0])], surv[:int(tot[1])], rng[:n], fl[:n])
        return base + (ck[:n], hd[:n]) if clocks else base

    def state_work_bytes(self, n: int) -> int:
        return int(self._L.hm_state_work_bytes(n))

    def state_device(self, cbatch: CBatch, cresults: CResults, n: int, doc_index: int, out: "CStateOut", out_summary: int,
                     work: int, stream: int = 0, out_clock: int = 0, out_heads: int = 0) -> None:
        """hm_state_device: the same with every table in device memory (pointers; `out` a CStateOut of
        device tables, `work` of state_work_bytes(n) bytes; enqueued, not synchronised)."""
        p = lambda x: ctypes.c_void_p(x) if x else None
        self._check(self._L.hm_state_device(self._h, ctypes.byref(cbatch), ctypes.byref(cresults), n, p(doc_index),
                                            ctypes.byref(out), p(out_clock), p(out_heads), p(out_summary), p(work), p(stream)),
                    "hm_state_device")

    def small_occupancy(self, batch: Batch) -> Sequence[int]:
        """(resident one-wave workgroups per CU, CUs, op rows per lane, size class, lists, counters) of
        merge_small_kernel's launch for a host batch: the persistent grid is the product of the first
        two (at most n_docs), the other four name the instantiation."""
        out = (ctypes.c_uint32 * 6)()
        cb = batch.c_struct()
        self._check(self._L.hm_debug_small_occupancy(self._h, ctypes.byref(cb), out), "hm_debug_small_occupancy")
        return tuple(int(x) for x in out)

    def last_kernel_ms(self) -> Sequence[float]:
        buf = (ctypes.c_float * 4)()
        n = self._L.hm_last_kernel_ms(self._h, buf, 4)
        return [float(buf[i]) for i in range(n)]

    def last_deferred(self, n_docs: int) -> np.ndarray:
        """Launch rows the last launch handed to the general kernel (hand-over order)."""
        out = np.zeros(max(n_docs, 1), np.uint32)
        n = self._L.hm_last_deferred(self._h, out.ctypes.data, len(out))
        if n < 0:
            self._check(-n, "hm_last_deferred")
        return out[:min(n, len(out))].copy()

    def clock_op(self, which: str, a_ptr: int, b_ptr: int, out_ptr: int, n_docs: int, a_stride: int,
                 stream: int = 0) -> None:
        f = {"cmp": self._L.hm_clock_cmp_device, "union": self._L.hm_clock_union_device,
             "intersection": self._L.hm_clock_intersection_device}[which]
        self._check(f(self._h, a_ptr, b_ptr, out_ptr, n_docs, a_stride, stream or None), f"clock_{which}")
