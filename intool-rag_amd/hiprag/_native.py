"""
ctypes binding of libhiprag.so (include/hiprag.h).  No fallbacks: if the library or a symbol is missing this
module raises -- the product path never computes on the CPU.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("HIPRAG_LIB", os.path.join(_PKG_DIR, "lib", "libhiprag.so"))

METRIC_IP = 0
METRIC_L2 = 1
PROBE_ANY = 0      # HIPIVF_PROBE_ANY
PROBE_SCOPE = 1    # HIPIVF_PROBE_SCOPE


class HipRagError(RuntimeError):
    """Raised for any non-zero status from libhiprag (message from hiprag_last_error)."""

    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} failed (status {code}): {msg}")
        self.code = code


class HipIdxStats(ctypes.Structure):
    _fields_ = [("passes", c_int64), ("queries", c_int64), ("fallback_queries", c_int64),
                ("bytes_per_pass", c_int64), ("timed_passes", c_int64), ("avg_scan_ms", c_float),
                ("avg_scan_wall_ms", c_float), ("avg_scan_gap_ms", c_float), ("launches", c_int64), ("roundb_queries", c_int64),
                ("list_entries", c_int64), ("ranked_entries", c_int64), ("rescored_groups", c_int64),
                ("wide_launches", c_int64), ("wide_theta_folds", c_int64)]


class HipIdxScanShape(ctypes.Structure):
    """hipidx_scan_shape_t: all the scan's launch policy depends on"""
    _fields_ = [("nblocks", c_int64), ("P", c_int32), ("mode", c_int32), ("wide_env", c_int32), ("n_cu", c_int32),
                ("launch_env", c_int32)]


class HipIdxScanPlan(ctypes.Structure):
    """hipidx_scan_plan_t: the launch hiprag_scan_plan gives (shape, nq, k, cus)"""
    _fields_ = [("run", c_int32), ("wide", c_int32), ("waves", c_int32), ("ring", c_int32), ("multi_pass", c_int32),
                ("filter", c_int32), ("ncls", c_int32), ("qtile_image", c_int32), ("lds_bytes", c_int64),
                ("launch_queries", c_int32), ("pipe_spare_cus", c_int32), ("bytes_per_pass_ip", c_int64),
                ("bytes_per_pass_l2", c_int64)]


class HipEncShape(ctypes.Structure):
    """hipenc_shape_t: all the encoder's forward policy depends on"""
    _fields_ = [("hidden", c_int32), ("ffn", c_int32), ("n_cu", c_int32), ("small_rows", c_int32), ("use256", c_int32)]


class HipEncPlan(ctypes.Structure):
    """hipenc_plan_t: the forward hipenc_forward_plan gives (shape, nseq, S)"""
    _fields_ = [("T", c_int32), ("M", c_int32), ("path", c_int32), ("osplit", c_int32), ("dsplit", c_int32), ("fsplit", c_int32),
                ("head_split", c_int32), ("pre_bytes", c_int64)]


ENC_PATH_SMALL, ENC_PATH_BIG, ENC_PATH_TILED = 0, 1, 2     # HIPENC_PATH_*


class HipBm25Stats(ctypes.Structure):
    _fields_ = [("queries", c_int64), ("postings_touched", c_int64), ("bytes_algorithmic", c_int64)]


f32p, f64p, i64p, i32p, u32p, u64p = (POINTER(c_float), POINTER(c_double), POINTER(c_int64), POINTER(c_int32),
                                      POINTER(c_uint32), POINTER(c_uint64))

# name -> argtypes; every function returns int32 status except the two noted below
SIGNATURES = {
    "hiprag_device_count": [i32p],
    "hiprag_device_sync": [c_int32],
    "hiprag_scan_stream": [c_int32, c_void_p],
    "hiprag_tail_stream": [c_int32, c_int32, c_void_p],
    "hiprag_init": [c_int32],
    "hiprag_shutdown": [],
    "hiphybrid_search": [c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float,
                         c_float, c_void_p, c_void_p],
    "hiphybrid_search_dev": [c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float,
                             c_float, c_void_p, c_void_p, c_void_p, c_void_p],
    "hiphybrid_search_scoped": [c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float,
                                c_float, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    "hiphybrid_search_scoped_dev": [c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_float, c_float,
                                    c_float, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "hiphybrid_search_ivf_scoped": [c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                    c_float, c_float, c_float, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    "hiphybrid_search_ivf_scoped_dev": [c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                        c_float, c_float, c_float, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p],
    "hiphybrid_shard_begin_dev": [c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                  c_void_p, c_void_p],
    "hiphybrid_shard_end_dev": [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_float, c_float, c_float, c_void_p,
                                c_void_p, c_void_p, c_void_p],
    "hiprag_event_create": [u64p],
    "hiprag_event_record": [c_uint64, c_void_p],
    "hiprag_probe_read_gbps": [c_int32, c_int64, c_int32, POINTER(c_double)],
    "hiprag_event_elapsed_ms": [c_uint64, c_uint64, f32p],
    "hiprag_event_destroy": [c_uint64],
    "hipidx_create": [c_int32, c_int32, c_int32, u64p],
    "hipidx_destroy": [c_uint64],
    "hipidx_add": [c_uint64, c_void_p, c_int64],
    "hipidx_add_dev": [c_uint64, c_void_p, c_int64, c_void_p],
    "hipidx_ntotal": [c_uint64, i64p],
    "hipidx_dim": [c_uint64, i32p],
    "hipidx_metric": [c_uint64, i32p],
    "hipidx_set_id_base": [c_uint64, c_int64],
    "hipidx_search": [c_uint64, c_void_p, c_int32, c_int32, c_void_p, c_void_p],
    "hipidx_search_dev": [c_uint64, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipidx_search_scoped_dev": [c_uint64, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p],
    "hipidx_search_scoped": [c_uint64, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                             c_void_p],
    "hipidx_scoped_info": [c_uint64, c_void_p],
    "hiprag_scope_plan": [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int64],
    "hiprag_slice_items": [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int32, c_int32, c_void_p, c_int64, c_void_p],
    "hipidx_score_ids_dev": [c_uint64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p],
    "hipidx_score_ids": [c_uint64, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p],
    "hipidx_score_info": [c_uint64, c_void_p],
    "hipidx_remove_ranges": [c_uint64, c_void_p, c_int32],
    "hipidx_remove_info": [c_uint64, c_void_p],
    "hipidx_row_bounds": [c_uint64, c_void_p],
    "hipidx_search_begin_dev": [c_uint64, c_void_p, c_int32, c_int32, c_int32, c_void_p],
    "hipidx_search_finish_dev": [c_uint64, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipidx_pass_queries": [c_uint64, i32p],
    "hipidx_launch_queries": [c_uint64, i32p],
    "hipidx_set_spare_cus": [c_uint64, c_int32],
    "hipidx_get_spare_cus": [c_uint64, c_void_p],
    "hipidx_pipe_spare_cus": [c_uint64, c_void_p],
    "hipidx_gate_tail_dev": [c_uint64, c_int32, c_void_p],
    "hiprag_scan_plan": [POINTER(HipIdxScanShape), c_int32, c_int32, c_int32, POINTER(HipIdxScanPlan)],
    "hipidx_scan_shape": [c_uint64, POINTER(HipIdxScanShape)],
    "hiprag_wide_walk": [c_int64, c_int32, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p],
    "hiprag_wide_fold": [c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p],
    "hiprag_compaction_plan": [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p],
    "hipidx_reserve_search": [c_uint64, c_int32],
    "hipidx_reserve_rows": [c_uint64, c_int64],
    "hipidx_reconstruct": [c_uint64, c_int64, c_void_p],
    "hipidx_save": [c_uint64, c_char_p],
    "hipidx_load": [c_char_p, c_int32, u64p],
    "hipidx_get_stats": [c_uint64, POINTER(HipIdxStats)],
    "hipidx_enable_timing": [c_uint64, c_int32],
    "hipivf_create": [c_uint64, c_uint64, c_void_p, c_void_p, c_int32, u64p],
    "hipivf_destroy": [c_uint64],
    "hipivf_search_dev": [c_uint64, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipivf_info": [c_uint64, i32p, i64p, i64p],
    "hipivf_search_batch_dev": [c_uint64, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipivf_batch_info": [c_uint64, c_void_p],
    "hipivf_search_scoped_dev": [c_uint64, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p],
    "hipivf_search_scoped": [c_uint64, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                             c_void_p, c_void_p],
    "hipivf_scoped_info": [c_uint64, c_void_p],
    "hipivf_search_scoped_probe_dev": [c_uint64, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p],
    "hipivf_search_scoped_probe": [c_uint64, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                   c_void_p, c_void_p, c_void_p],
    "hipivf_scope_probe_info": [c_uint64, c_void_p],
    "hipivf_build_dev": [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_uint64, c_int64, c_int32, c_void_p, u64p],
    "hipivf_build": [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_uint64, c_int64, c_int32, c_void_p, u64p],
    "hipivf_save": [c_uint64, c_char_p],
    "hipivf_load": [c_char_p, c_int32, u64p],
    "hipivf_get_centroids": [c_uint64, c_void_p],
    "hipivf_get_lists": [c_uint64, c_void_p, c_void_p],
    "hipivf_meta": [c_uint64, i32p, i32p, i64p],
    "hipivf_build_times": [c_uint64, c_void_p],
    "hipivf_from_centroids": [c_void_p, c_int32, c_int32, c_int32, c_int32, u64p],
    "hipivf_add_dev": [c_uint64, c_void_p, c_int64, c_void_p],
    "hipivf_add": [c_uint64, c_void_p, c_int64],
    "hipivf_remove_ranges": [c_uint64, c_void_p, c_int32],
    "hipivf_update_info": [c_uint64, c_void_p],
    "hiprag_merge_topk_dev": [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int64, c_int32, c_void_p,
                              c_void_p, c_void_p, c_void_p],
    "hipbm25_create": [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int32, u64p],
    "hipbm25_destroy": [c_uint64],
    "hipbm25_set_id_base": [c_uint64, c_int64],
    "hipbm25_search": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p],
    "hipbm25_search_dev": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipbm25_search_scoped": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                              c_void_p],
    "hipbm25_search_scoped_dev": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p],
    "hipbm25_scoped_info": [c_uint64, c_void_p],
    "hipbm25_search_weighted": [c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p],
    "hipbm25_search_weighted_dev": [c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipbm25_search_scoped_weighted": [c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                       c_void_p, c_void_p],
    "hipbm25_search_scoped_weighted_dev": [c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p],
    "hipbm25_score_ids_dev": [c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p],
    "hipbm25_score_ids": [c_uint64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p],
    "hipbm25_score_info": [c_uint64, c_void_p],
    "hipbm25_get_stats": [c_uint64, POINTER(HipBm25Stats)],
    "hipbm25_create_tf": [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_int32, u64p],
    "hipbm25_append": [c_uint64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipbm25_remove_ranges": [c_uint64, c_void_p, c_int32],
    "hipbm25_reweigh": [c_uint64, c_void_p],
    "hipbm25_export": [c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipbm25_sizes": [c_uint64, c_void_p],
    "hipbm25_update_info": [c_uint64, c_void_p],
    "hipbm25_impacts_host": [c_void_p, c_void_p, c_void_p, c_int64, c_double, c_double, c_double, c_void_p],
    "hipbm25_create_impacts": [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int32, u64p],
    "hipbm25_append_impacts": [c_uint64, c_int64, c_int64, c_void_p, c_void_p, c_void_p],
    "hipbm25_append_rows_dev": [c_uint64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p],
    "hipenc_create": [c_void_p, c_void_p, c_int32, u64p],
    "hipenc_destroy": [c_uint64],
    "hipenc_forward": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p],
    "hipenc_score_pairs": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p],
    "hipenc_last_flops": [c_uint64, f64p],
    "hipenc_forward_plan": [POINTER(HipEncShape), c_int32, c_int32, POINTER(HipEncPlan)],
    "hipenc_shape": [c_uint64, POINTER(HipEncShape)],
    "hipenc_forward_packed": [c_uint64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],
    "hipenc_score_pairs_packed": [c_uint64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],
    "hipenc_forward_hidden_packed": [c_uint64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],
    "hipenc_packed_layout": [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipenc_packed_info": [c_uint64, c_void_p],
    "hipenc_attention_packed": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                c_void_p, c_void_p],
    "hipenc_set_lexical_head": [c_uint64, c_void_p, c_void_p, c_void_p, c_int32],
    "hipenc_forward_lexical": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipenc_set_colbert_head": [c_uint64, c_void_p, c_void_p],
    "hipenc_forward_colbert": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipenc_forward_m3": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                          c_void_p],
    "hipenc_colbert_rows": [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                            c_void_p],
    "hipenc_forward_hidden":[c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p],
    "hipenc_attention": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p],
    "hipenc_linear": [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                      c_void_p, c_int32, c_int32, c_int32, c_void_p],
    "hipenc_linear_ex": [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, i32p, c_void_p],
    "hipenc_layernorm": [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_float, c_int32, c_int32, c_void_p,
                         c_void_p, c_void_p],
    "hiptok_create": [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, u64p],
    "hiptok_destroy": [c_uint64],
    "hiptok_append": [c_uint64, c_void_p, c_void_p, c_int64],
    "hiptok_remove_ranges": [c_uint64, c_void_p, c_int32],
    "hiptok_export": [c_uint64, c_void_p, c_void_p],
    "hiptok_sizes": [c_uint64, c_void_p],
    "hiprerank_dev": [c_uint64, c_uint64, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int64,
                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "hiprerank_host": [c_uint64, c_uint64, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int64,
                  c_void_p, c_void_p, c_void_p, c_void_p],
    "hiprerank_info": [c_uint64, c_void_p],
    "hiprerank_assemble": [c_uint64, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p,
                           c_void_p],
    "hiprerank_packed_dev": [c_uint64, c_uint64, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int64,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "hiprerank_packed_host": [c_uint64, c_uint64, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int32, c_int32, c_int64,
                              c_void_p, c_void_p, c_void_p, c_void_p],
    "hiprerank_packed_info": [c_uint64, c_void_p],
    "hiprerank_assemble_packed": [c_uint64, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p,
                                  c_void_p, c_void_p],
    "hipmv_create": [c_int32, c_int32, c_int32, u64p],
    "hipmv_destroy": [c_uint64],
    "hipmv_append_dev": [c_uint64, c_void_p, c_int32, c_void_p, c_int64, c_void_p],
    "hipmv_append": [c_uint64, c_void_p, c_void_p, c_int64],
    "hipmv_remove_ranges": [c_uint64, c_void_p, c_int32],
    "hipmv_save": [c_uint64, c_char_p],
    "hipmv_load": [c_char_p, c_int32, u64p],
    "hipmv_export": [c_uint64, c_void_p, c_void_p],
    "hipmv_sizes": [c_uint64, c_void_p],
    "hipmv_create_ex": [c_int32, c_int32, c_int32, c_int32, u64p],
    "hipmv_export_fp8": [c_uint64, c_void_p, c_void_p, c_void_p],
    "hipmv_format_info": [c_uint64, c_void_p],
    "hipmv_to_fp8": [c_uint64, u64p],
    "hipmv_export_mxfp4": [c_uint64, c_void_p, c_void_p, c_void_p],
    "hipmv_to_mxfp4": [c_uint64, u64p],
    "hipmaxsim_dev": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p,
                      c_void_p, c_void_p, c_void_p],
    "hipmaxsim_host": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int64, c_int32, c_void_p, c_void_p,
                       c_void_p, c_void_p],
    "hipmaxsim_info": [c_uint64, c_void_p],
    "hipm3_score_dev": [c_uint64, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                        c_void_p, c_int32, c_int32, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                        c_void_p],
    "hipm3_score_host": [c_uint64, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                         c_void_p, c_int32, c_int32, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipmaxsim_search_scoped_dev": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                    c_int64, c_void_p, c_void_p, c_void_p],
    "hipmaxsim_search_scoped": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                c_int64, c_void_p, c_void_p],
    "hipmaxsim_search_info": [c_uint64, c_void_p],
    "hipmv_attach_centroids": [c_uint64, c_void_p, c_int32],
    "hipmv_detach_centroids": [c_uint64],
    "hipmv_export_centroids": [c_uint64, c_void_p],
    "hipmv_export_codes": [c_uint64, c_void_p],
    "hipmv_centroid_info": [c_uint64, c_void_p],
    "hipmv_gather_f32_dev": [c_uint64, c_void_p, c_int64, c_void_p],
    "hipmaxsim_search_pruned_dev": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                    c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipmaxsim_search_pruned": [c_uint64, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p],
    "hipmaxsim_pruned_info": [c_uint64, c_void_p],
    "hippage_create": [c_int32, u64p],
    "hippage_destroy": [c_uint64],
    "hippage_append": [c_uint64, c_void_p, c_void_p, c_int64],
    "hippage_remove_ranges": [c_uint64, c_void_p, c_int32],
    "hippage_export": [c_uint64, c_void_p, c_void_p],
    "hippage_sizes": [c_uint64, c_void_p],
    "hippage_rank_dev": [c_uint64, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_int32, c_int32, c_void_p,
                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "hiprrf_fuse": [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_float, c_float, c_void_p,
                    c_void_p],
    "hiprrf_fuse_dev": [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_float, c_float, c_void_p,
                        c_void_p, c_void_p],
}
NON_STATUS = {"hiprag_version": ([], c_int32), "hiprag_last_error": ([], c_char_p)}

_lib = None


def load() -> ctypes.CDLL:
    """Load libhiprag.so and type every symbol the header declares.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipRagError("load", -1, f"{LIB_PATH} not found: build it with `make -C intool-rag_amd` "
                                      "(__graft_entry__.build()); there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (args, res) in NON_STATUS.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, res
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)        # AttributeError here = header/library mismatch: fail loudly
        fn.argtypes, fn.restype = args, c_int32
    _lib = lib
    return lib


def call(name: str, *args) -> None:
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.hiprag_last_error()
        raise HipRagError(name, rc, msg.decode("utf-8", "replace") if msg else "")


def exported_symbols():
    return list(NON_STATUS) + list(SIGNATURES)
