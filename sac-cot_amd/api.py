"""Host-side mirror of the C ABI in include/saccot.h (ctypes over libsaccot.so).

The reference has no operator/plugin interface to mirror (/root/reference/README.md:1-2 is the whole tree), so the
names follow SURVEY.md §8(b): `register()` is the drop-in entry point — correspondences in, (R, t, inlier mask)
out — and the `compat` / `triangles` / `kabsch` / `score` / `mask` methods are the per-stage hooks the parity
tests drive.  Everything computes on the GPU through libsaccot.so; if the library or a HIP device is missing
this module raises — there is no CPU fallback (the CPU restatement lives in oracle/ and is test-only).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsaccot.so")

SC_OK, SC_EINVAL, SC_ENOMEM, SC_EHIP, SC_ERCCL, SC_ENOHYP, SC_ETOOMANY, SC_ERETRY, SC_EBOUND = 0, -1, -2, -3, -4, -5, -6, -7, -8
SC_FLAG_SHARD_AB = 4096  # sc_register_multi: shard stages A and B at every size (default: replicated below 8192 correspondences)
SC_FLAG_EST_BOUND = 128  # phase API sc_shard_*: prune by an estimated bound, no histogram all-reduce, SC_EBOUND -> repeat without it
SC_AOS, SC_SOA = 0, 1
SC_RANK_WEIGHT, SC_RANK_DEGREE = 0, 1
SC_SCORE_COUNT, SC_SCORE_MSE, SC_SCORE_MAE = 0, 1, 2
SC_FLAG_TIMING, SC_FLAG_EXACT_TOTAL, SC_FLAG_NO_PRUNE, SC_FLAG_REFINE, SC_FLAG_TIMING_HOT, SC_FLAG_NO_DENSE_S = 1, 2, 4, 8, 16, 32
SC_FLAG_TIMING_ONE = 64
SC_MATCH_MUTUAL = 1  # sc_match_params.flags: keep (i, j) only if each is the other's nearest (knn == 1)


def SC_TIMING_STAGE(k: int) -> int:
    """flags bits selecting the one bracket of SC_FLAG_TIMING_ONE: 0 staging, 1 compat, 2 triangles, 3 kabsch, 4 score,
    5 argmax, 6 mask"""
    return (k & 15) << 8


SC_HIST_WORDS = 256  # u32 words of the pruning-sample histogram (sc_hypothesize_begin_device)

EXPORTS = ["sc_version", "sc_strerror", "sc_default_params", "sc_create", "sc_destroy", "sc_set_stream",
           "sc_last_error", "sc_set_debug", "sc_debug_last", "sc_register", "sc_register_device", "sc_register_device_async", "sc_wait",
           "sc_register_batch", "sc_register_batch_device",
           "sc_peel", "sc_peel_device", "sc_register_instances",
           "sc_polish_default_params", "sc_polish_device", "sc_polish",
           "sc_match_default_params", "sc_match_device", "sc_match", "sc_register_features",
           "sc_guide_default_params", "sc_match_guided_device", "sc_match_guided", "sc_register_guided_features",
           "sc_match_batch", "sc_match_batch_device", "sc_register_batch_features", "sc_register_batch_features_device",
           "sc_polish_batch", "sc_polish_batch_device", "sc_polish_batch_slots_device",
           "sc_register_instances_batch", "sc_register_instances_batch_device", "sc_register_instances_batch_features_device",
           "sc_pairs_layout", "sc_match_pairs", "sc_match_pairs_device", "sc_register_pairs_features", "sc_register_pairs_features_device",
           "sc_polish_pairs_slots_device",
           "sc_match_guided_batch", "sc_match_guided_batch_device", "sc_register_guided_batch_features_device",
           "sc_match_guided_pairs", "sc_match_guided_pairs_device", "sc_register_guided_pairs_features_device",
           "sc_match_guided_poses", "sc_match_guided_poses_device", "sc_register_guided_poses_features",
           "sc_pose_info_batch", "sc_pose_info_batch_device", "sc_pose_info_batch_slots_device", "sc_pose_info_pairs_slots_device",
           "sc_pose_info_default_params", "sc_pose_info_frame", "sc_pose_info_frame_device",
           "sc_polish_poses_default_params", "sc_polish_poses", "sc_polish_poses_device",
           "sc_assign_default_params", "sc_assign_poses_frame", "sc_assign_poses_frame_device", "sc_assign_poses_batch",
           "sc_assign_poses_batch_device",
           "sc_settle_default_params", "sc_settle_poses_frame", "sc_settle_poses_frame_device", "sc_settle_poses_batch",
           "sc_settle_poses_batch_device",
           "sc_hypothesize_device", "sc_finalize_device",
           "sc_hypothesize_begin_device", "sc_hypothesize_end_device", "sc_finalize_gathered_device", "sc_finalize_gathered_device_async",
           "sc_shard_plan_query", "sc_shard_compat_device", "sc_shard_edges_device", "sc_shard_select_device",
           "sc_shard_score_device", "sc_create_multi", "sc_create_multi_loopback", "sc_destroy_multi",
           "sc_multi_last_error", "sc_register_multi",
           "sc_compat_host", "sc_triangles_host", "sc_kabsch_host", "sc_score_host", "sc_mask_host"]


class ScParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("sigma", C.c_float), ("t_cmp", C.c_float), ("tau", C.c_float),
                ("min_len", C.c_float), ("max_triangles", C.c_uint32), ("rank_mode", C.c_int32),
                ("layout", C.c_int32), ("shard_rank", C.c_int32), ("shard_world", C.c_int32),
                ("shard_block", C.c_uint32), ("flags", C.c_uint32), ("max_workspace", C.c_uint64),
                ("score_mode", C.c_int32), ("shard_cand_level", C.c_int32)]


class ScStats(C.Structure):
    _fields_ = [("size", C.c_uint32), ("n", C.c_uint32), ("edges", C.c_uint64), ("tri_total", C.c_uint64),
                ("tri_kept", C.c_uint32), ("tri_scored", C.c_uint32), ("best_rank", C.c_uint32),
                ("best_count", C.c_uint32), ("us_stage", C.c_float), ("us_compat", C.c_float), ("us_triangles", C.c_float),
                ("us_trikeys", C.c_float),
                ("us_kabsch", C.c_float), ("us_score", C.c_float), ("us_argmax", C.c_float), ("us_mask", C.c_float),
                ("us_total", C.c_float),
                ("workspace_bytes", C.c_uint64), ("bytes_moved", C.c_uint64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


class ScMatchParams(C.Structure):
    """Mirror of `sc_match_params` (include/saccot.h): descriptor length, neighbours per row (1 .. 4), SC_MATCH_* flags, ratio test."""
    _fields_ = [("size", C.c_uint32), ("dim", C.c_uint32), ("knn", C.c_uint32), ("flags", C.c_uint32), ("ratio", C.c_float),
                ("reserved", C.c_uint32 * 3)]


class ScGuideParams(C.Structure):
    """Mirror of `sc_guide_params` (include/saccot.h): the layout of the keypoints (SC_AOS / SC_SOA) and the gate radius of
    sc_match_guided."""
    _fields_ = [("size", C.c_uint32), ("layout", C.c_uint32), ("gate", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class ScPolishParams(C.Structure):
    """Mirror of `sc_polish_params` (include/saccot.h): hypotheses polished (1 .. 64), refits per candidate at most (1 .. 64)."""
    _fields_ = [("size", C.c_uint32), ("candidates", C.c_uint32), ("max_iter", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class ScPolishCand(C.Structure):
    """Mirror of `sc_polish_cand` (include/saccot.h), 64 bytes: a candidate's last iterate, its position in the ranked list, its frame
    score, the score of the iterate, the refits that changed (R, t)."""
    _fields_ = [("Rt", C.c_float * 12), ("rank", C.c_uint32), ("score0", C.c_uint32), ("score", C.c_uint32), ("iters", C.c_uint16),
                ("reserved", C.c_uint16)]


POLISH_CAND_DTYPE = np.dtype([("Rt", np.float32, 12), ("rank", np.uint32), ("score0", np.uint32), ("score", np.uint32),
                              ("iters", np.uint16), ("reserved", np.uint16)])  # sc_polish_cand as a numpy record


class ScBatchResult(C.Structure):
    """Mirror of `sc_batch_result` (include/saccot.h), 80 bytes: one problem's record of sc_register_batch."""
    _fields_ = [("Rt", C.c_float * 12), ("status", C.c_int32), ("n", C.c_uint32), ("edges", C.c_uint32), ("tri_kept", C.c_uint32),
                ("tri_total", C.c_uint64), ("best_rank", C.c_uint32), ("best_count", C.c_uint32)]


BATCH_RESULT_DTYPE = np.dtype([("Rt", np.float32, 12), ("status", np.int32), ("n", np.uint32), ("edges", np.uint32),
                               ("tri_kept", np.uint32), ("tri_total", np.uint64), ("best_rank", np.uint32),
                               ("best_count", np.uint32)])  # sc_batch_result as a numpy record
SC_BATCH_MAX_N = 512


class ScPolishBatchResult(C.Structure):
    """Mirror of `sc_polish_batch_result` (include/saccot.h), 64 bytes: one problem's record of sc_polish_batch."""
    _fields_ = [("Rt", C.c_float * 12), ("status", C.c_int32), ("score0", C.c_uint32), ("score", C.c_uint32), ("iters", C.c_uint16),
                ("stop", C.c_uint16)]


POLISH_BATCH_RESULT_DTYPE = np.dtype([("Rt", np.float32, 12), ("status", np.int32), ("score0", np.uint32), ("score", np.uint32),
                                      ("iters", np.uint16), ("stop", np.uint16)])  # sc_polish_batch_result as a numpy record
SC_POLISH_STOP_FIXED, SC_POLISH_STOP_DECLINED, SC_POLISH_STOP_MAX_ITER = 0, 1, 2


class ScPoseInfoResult(C.Structure):
    """Mirror of `sc_pose_info_result` (include/saccot.h), 320 bytes: one problem's record of sc_pose_info_batch."""
    _fields_ = [("info", C.c_double * 36), ("sse", C.c_double), ("status", C.c_int32), ("inliers", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


POSE_INFO_RESULT_DTYPE = np.dtype([("info", np.float64, 36), ("sse", np.float64), ("status", np.int32), ("inliers", np.uint32),
                                   ("reserved", np.uint32, 4)])  # sc_pose_info_result as a numpy record


class ScPoseInfoParams(C.Structure):
    """Mirror of `sc_pose_info_params` (include/saccot.h), 32 bytes: which correspondences of the frame take part (SC_POSE_INFO_SEL_*),
    the label of pose 0 (SEL_LABEL), SC_POSE_INFO_STATUS or 0."""
    _fields_ = [("size", C.c_uint32), ("sel_mode", C.c_uint32), ("label0", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


SC_POSE_INFO_MAX_POSES = 1024
SC_POSE_INFO_SEL_NONE, SC_POSE_INFO_SEL_MASK, SC_POSE_INFO_SEL_LABEL = 0, 1, 2
SC_POSE_INFO_STATUS = 1


class ScPolishPosesParams(C.Structure):
    """Mirror of `sc_polish_poses_params` (include/saccot.h), 32 bytes: refits per pose at most (1 .. 64), which correspondences of
    the frame take part (SC_POLISH_POSES_SEL_*), the label of pose 0 (SEL_LABEL / SEL_ALIVE), SC_POLISH_POSES_STATUS or 0."""
    _fields_ = [("size", C.c_uint32), ("max_iter", C.c_uint32), ("sel_mode", C.c_uint32), ("label0", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


SC_POLISH_POSES_MAX = 1024
SC_POLISH_POSES_SEL_NONE, SC_POLISH_POSES_SEL_MASK, SC_POLISH_POSES_SEL_LABEL, SC_POLISH_POSES_SEL_ALIVE = 0, 1, 2, 3
SC_POLISH_POSES_STATUS = 1


class ScAssignParams(C.Structure):
    """Mirror of `sc_assign_params` (include/saccot.h), 32 bytes: SC_ASSIGN_BEST / _FIRST, which correspondences take part
    (SC_ASSIGN_SEL_*), SC_ASSIGN_STATUS or 0."""
    _fields_ = [("size", C.c_uint32), ("mode", C.c_uint32), ("sel_mode", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class ScAssignResult(C.Structure):
    """Mirror of `sc_assign_result` (include/saccot.h), 32 bytes: one pose's record of sc_assign_poses."""
    _fields_ = [("status", C.c_int32), ("count", C.c_uint32), ("score", C.c_uint64), ("reserved", C.c_uint32 * 4)]


ASSIGN_RESULT_DTYPE = np.dtype([("status", np.int32), ("count", np.uint32), ("score", np.uint64),
                                ("reserved", np.uint32, 4)])  # sc_assign_result as a numpy record
SC_ASSIGN_MAX_POSES, SC_ASSIGN_BATCH_MAX_POSES = 1024, 64
SC_ASSIGN_BEST, SC_ASSIGN_FIRST = 0, 1
SC_ASSIGN_SEL_NONE, SC_ASSIGN_SEL_MASK = 0, 1
SC_ASSIGN_STATUS = 1


class ScSettleParams(C.Structure):
    """Mirror of `sc_settle_params` (include/saccot.h), 32 bytes: counted rounds at most (1 .. 64), which correspondences take part
    (SC_ASSIGN_SEL_*), SC_SETTLE_STATUS or 0."""
    _fields_ = [("size", C.c_uint32), ("max_iter", C.c_uint32), ("sel_mode", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


SC_SETTLE_MAX_POSES, SC_SETTLE_BATCH_MAX_POSES = 64, 16
SC_SETTLE_STATUS = 1
SC_GUIDE_POSE_STATUS = 1  # sc_guide_params.flags, the sc_match_guided_batch / _poses entries only: the pose records hold an int32 status at byte 48
SC_GUIDE_MAX_POSES = 64  # pose records per call of sc_match_guided_poses at most
SC_MATCH_BATCH_MAX_N = 4096  # rows a side of one problem of sc_match_batch
SC_INSTANCES_BATCH_MAX = 16  # motions per problem of sc_register_instances_batch at most


class ScShardPlan(C.Structure):
    """Mirror of `sc_shard_plan` (include/saccot.h): sizes of the buffers the ranks exchange when A and B are sharded."""
    _fields_ = [("size", C.c_uint32), ("rows_per_rank", C.c_uint32), ("words_per_row", C.c_uint32),
                ("reserved", C.c_uint32), ("bits_bytes_per_rank", C.c_uint64), ("bits_bytes_total", C.c_uint64),
                ("cand_bytes_per_rank", C.c_uint64)]


class ScDebug(C.Structure):
    """Mirror of `sc_debug` (include/saccot_debug.h): test / tuning hook, 0 = default (-1 for the *_self_max fields).  The two
    arrays are set through the names of their slots (`_ALIASES`): set_debug(tg_count=4, cnt_blocks=37)."""
    _fields_ = [("size", C.c_uint32), ("no_events", C.c_uint32), ("event_cap", C.c_uint64),
                ("compact_self_max", C.c_int64), ("scan_self_max", C.c_int64),
                ("grid_blocks", C.c_uint32 * 4), ("lanes_per_edge", C.c_uint32 * 4),
                ("sample_edges", C.c_uint64), ("score_split", C.c_uint32), ("compat_one_phase", C.c_uint32),
                ("compat_rows", C.c_uint32), ("compat_store_mode", C.c_uint32), ("compat_linear_order", C.c_uint32),
                ("sample_mode", C.c_uint32), ("rows_unfused", C.c_uint32), ("no_edge_build", C.c_uint32),
                ("no_estimate", C.c_uint32), ("est_margin_pct", C.c_uint32), ("no_fast", C.c_uint32),
                ("score_filter", C.c_uint32), ("filter_splits", C.c_uint32), ("filter_queue_cap", C.c_uint32),
                ("filter_lds_queue", C.c_uint32), ("filter_blind", C.c_uint32), ("gram_kappa_q4", C.c_uint32),
                ("gram_ref_late", C.c_uint32), ("gram_guard_fail", C.c_uint32), ("no_lane", C.c_uint32),
                ("scan_ordinals", C.c_uint32), ("ord_chunk_max", C.c_uint32)]
    _ALIASES = {"cnt_blocks": ("grid_blocks", 0), "keys_blocks": ("grid_blocks", 1), "sel_blocks": ("grid_blocks", 2),
                "sample_blocks": ("grid_blocks", 3), "tg_count": ("lanes_per_edge", 0), "tg_keys": ("lanes_per_edge", 1),
                "tg_sample": ("lanes_per_edge", 2), "tg_events": ("lanes_per_edge", 3)}


class ScDebugLab(C.Structure):
    """`sc_debug` of a library built with -DSC_ABLATIONS (sac-cot_amd/build.py --ablations): one knob more."""
    _fields_ = ScDebug._fields_ + [("filter_variant", C.c_uint32), ("lab_pad_", C.c_uint32)]
    _ALIASES = ScDebug._ALIASES


class ScDebugInfo(C.Structure):
    """Mirror of `sc_debug_info` (include/saccot_debug.h): which C2 kernel the last call ran, the filter's hand-overs,
    how the call was enqueued (fast_path: 0 waited, 1 host-free, 2 host-free then repeated; lane: 1 = on the context's lane beside
    the caller's stream, n_lane: such frames so far), the matrix-pipe probe."""
    _fields_ = [("size", C.c_uint32), ("c2_kernel", C.c_uint32), ("filter_undecided", C.c_uint64),
                ("filter_recounts", C.c_uint64), ("filter_splits", C.c_uint32), ("fast_path", C.c_uint32),
                ("gram_guard", C.c_uint32), ("prune_bound", C.c_uint32), ("gram_guard_worst", C.c_float),
                ("lane", C.c_uint32), ("gram_near_corr", C.c_uint32), ("gram_near_hyp", C.c_uint32),
                ("gram_rows", C.c_uint32), ("gram_ref", C.c_uint32), ("gram_ref_votes_q8", C.c_uint32),
                ("us_c2_filter", C.c_float),
                ("n_frames", C.c_uint64), ("n_fast_ok", C.c_uint64), ("n_fast_repeat", C.c_uint64),
                ("n_est_ok", C.c_uint64), ("n_est_fail", C.c_uint64), ("cover_edges", C.c_uint64), ("cover_triangles", C.c_uint64), ("n_hostfree_grow", C.c_uint64), ("n_lane", C.c_uint64),
                ("ordinals", C.c_uint32), ("strong_edges", C.c_uint32)]


class SacCotError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"libsaccot status {status}: {msg}")
        self.status = status


_LIB = None


def load_library() -> C.CDLL:
    """dlopen libsaccot.so and declare every prototype.  Raises if it was not built (run __graft_entry__.build())."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's), and the
    # copy that is loaded first serves every later DT_NEEDED.  torch cannot run on the system copy ("No HIP GPUs
    # are available"), libsaccot.so runs on either — so when torch is present, let it load first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
                                "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, f32p, u8p, u32p, u64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    pp, sp = C.POINTER(ScParams), C.POINTER(ScStats)
    L.sc_version.restype = C.c_int
    L.sc_strerror.argtypes = [C.c_int]; L.sc_strerror.restype = C.c_char_p
    L.sc_default_params.argtypes = [pp]; L.sc_default_params.restype = None
    L.sc_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.sc_destroy.argtypes = [vp]; L.sc_destroy.restype = None
    L.sc_set_stream.argtypes = [vp, vp]
    L.sc_last_error.argtypes = [vp]; L.sc_last_error.restype = C.c_char_p
    L.sc_set_debug.argtypes = [vp, C.POINTER(ScDebug)]
    L.sc_debug_last.argtypes = [vp, C.POINTER(ScDebugInfo)]
    L.sc_register.argtypes = [vp, f32p, f32p, C.c_int64, pp, f32p, f32p, u8p, sp]
    L.sc_register_device.argtypes = [vp, vp, vp, C.c_int64, pp, vp, vp, sp]
    L.sc_register_device_async.argtypes = [vp, vp, vp, C.c_int64, pp, vp, vp]
    L.sc_wait.argtypes = [vp, sp]
    L.sc_register_batch.argtypes = [vp, f32p, f32p, u32p, C.c_uint32, pp, vp, u8p]
    L.sc_register_batch_device.argtypes = [vp, vp, vp, u32p, C.c_uint32, pp, vp, vp]
    L.sc_peel.argtypes = [vp, f32p, f32p, u8p, sp]
    L.sc_peel_device.argtypes = [vp, vp, vp, sp]
    L.sc_register_instances.argtypes = [vp, f32p, f32p, C.c_int64, pp, C.c_uint32, C.c_uint32, f32p, u32p, C.POINTER(C.c_int32),
                                        u32p, sp]
    qp = C.POINTER(ScPolishParams)
    L.sc_polish_default_params.argtypes = [qp]
    L.sc_polish_device.argtypes = [vp, qp, vp, vp, vp, vp, sp]
    L.sc_polish.argtypes = [vp, qp, f32p, f32p, u8p, C.c_void_p, u32p, sp]
    mp, i32p = C.POINTER(ScMatchParams), C.POINTER(C.c_int32)
    L.sc_match_default_params.argtypes = [mp]
    L.sc_match_device.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, mp, vp, vp, vp]
    L.sc_match.argtypes = [vp, f32p, C.c_int64, f32p, C.c_int64, mp, i32p, f32p, u32p]
    L.sc_register_features.argtypes = [vp, f32p, f32p, C.c_int64, f32p, f32p, C.c_int64, mp, pp, f32p, f32p, i32p, f32p, u32p, u8p, sp]
    gp = C.POINTER(ScGuideParams)
    L.sc_guide_default_params.argtypes = [gp]
    L.sc_match_guided_device.argtypes = [vp, vp, vp, C.c_int64, vp, vp, C.c_int64, mp, gp, vp, vp, vp, vp, vp]
    L.sc_match_guided.argtypes = [vp, f32p, f32p, C.c_int64, f32p, f32p, C.c_int64, mp, gp, f32p, i32p, f32p, f32p, u32p]
    L.sc_register_guided_features.argtypes = [vp, f32p, f32p, C.c_int64, f32p, f32p, C.c_int64, mp, gp, f32p, pp, f32p, f32p, i32p, f32p,
                                              f32p, u32p, u8p, sp]
    L.sc_match_guided_poses_device.argtypes = [vp, vp, vp, C.c_int64, vp, vp, C.c_int64, mp, gp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
    L.sc_match_guided_poses.argtypes = [vp, f32p, f32p, C.c_int64, f32p, f32p, C.c_int64, mp, gp, vp, C.c_uint32, C.c_uint32, i32p, f32p,
                                        f32p, i32p, u32p]
    L.sc_register_guided_poses_features.argtypes = [vp, f32p, f32p, C.c_int64, f32p, f32p, C.c_int64, mp, gp, vp, C.c_uint32, C.c_uint32,
                                                    pp, f32p, f32p, i32p, f32p, f32p, i32p, u32p, u8p, sp]
    L.sc_match_batch_device.argtypes = [vp, vp, u32p, vp, u32p, C.c_uint32, mp, vp, vp, vp]
    L.sc_match_batch.argtypes = [vp, f32p, u32p, f32p, u32p, C.c_uint32, mp, i32p, f32p, u32p]
    L.sc_register_batch_features_device.argtypes = [vp, vp, vp, u32p, vp, vp, u32p, C.c_uint32, mp, pp, vp, vp, vp, vp, vp]
    L.sc_register_batch_features.argtypes = [vp, f32p, f32p, u32p, f32p, f32p, u32p, C.c_uint32, mp, pp, vp, i32p, f32p, u32p, u8p]
    L.sc_polish_batch.argtypes = [vp, f32p, f32p, u32p, C.c_uint32, pp, qp, vp, vp, u8p]
    L.sc_polish_batch_device.argtypes = [vp, vp, vp, u32p, C.c_uint32, pp, qp, vp, vp, vp]
    L.sc_polish_batch_slots_device.argtypes = [vp, vp, u32p, vp, u32p, C.c_uint32, C.c_uint32, pp, qp, vp, vp, vp, vp, vp]
    L.sc_register_instances_batch.argtypes = [vp, f32p, f32p, u32p, C.c_uint32, pp, C.c_uint32, C.c_uint32, vp, i32p, u32p]
    L.sc_register_instances_batch_device.argtypes = [vp, vp, vp, u32p, C.c_uint32, pp, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sc_register_instances_batch_features_device.argtypes = [vp, vp, vp, u32p, vp, vp, u32p, C.c_uint32, mp, pp, C.c_uint32, C.c_uint32,
                                                              vp, vp, vp, vp, vp, vp]
    L.sc_pairs_layout.argtypes = [u32p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, u32p]
    L.sc_match_pairs_device.argtypes = [vp, vp, u32p, C.c_uint32, u32p, C.c_uint32, mp, vp, vp, vp]
    L.sc_match_pairs.argtypes = [vp, f32p, u32p, C.c_uint32, u32p, C.c_uint32, mp, i32p, f32p, u32p]
    L.sc_register_pairs_features_device.argtypes = [vp, vp, vp, u32p, C.c_uint32, u32p, C.c_uint32, mp, pp, vp, vp, vp, vp, vp]
    L.sc_register_pairs_features.argtypes = [vp, f32p, f32p, u32p, C.c_uint32, u32p, C.c_uint32, mp, pp, vp, i32p, f32p, u32p, u8p]
    L.sc_polish_pairs_slots_device.argtypes = [vp, vp, u32p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, pp, qp, vp, vp, vp, vp, vp]
    u32 = C.c_uint32
    L.sc_match_guided_batch_device.argtypes = [vp, vp, vp, u32p, vp, vp, u32p, u32, mp, gp, vp, u32, vp, vp, vp, vp]
    L.sc_match_guided_batch.argtypes = [vp, f32p, f32p, u32p, f32p, f32p, u32p, u32, mp, gp, vp, u32, i32p, f32p, f32p, u32p]
    L.sc_register_guided_batch_features_device.argtypes = [vp, vp, vp, u32p, vp, vp, u32p, u32, mp, gp, vp, u32, pp, vp, vp, vp, vp, vp, vp]
    L.sc_match_guided_pairs_device.argtypes = [vp, vp, vp, u32p, u32, u32p, u32, mp, gp, vp, u32, vp, vp, vp, vp]
    L.sc_match_guided_pairs.argtypes = [vp, f32p, f32p, u32p, u32, u32p, u32, mp, gp, vp, u32, i32p, f32p, f32p, u32p]
    L.sc_register_guided_pairs_features_device.argtypes = [vp, vp, vp, u32p, u32, u32p, u32, mp, gp, vp, u32, pp, vp, vp, vp, vp, vp, vp]
    L.sc_pose_info_batch.argtypes = [vp, f32p, f32p, u32p, C.c_uint32, pp, vp, C.c_uint32, vp]
    L.sc_pose_info_batch_device.argtypes = [vp, vp, vp, u32p, C.c_uint32, pp, vp, C.c_uint32, vp]
    L.sc_pose_info_batch_slots_device.argtypes = [vp, vp, u32p, vp, u32p, C.c_uint32, C.c_uint32, pp, vp, vp, vp, C.c_uint32, vp]
    L.sc_pose_info_pairs_slots_device.argtypes = [vp, vp, u32p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, pp, vp, vp, vp, C.c_uint32, vp]
    ip = C.POINTER(ScPoseInfoParams)
    L.sc_pose_info_default_params.argtypes = [ip]
    L.sc_pose_info_frame.argtypes = [vp, ip, vp, C.c_uint32, C.c_uint32, vp, vp]
    L.sc_pose_info_frame_device.argtypes = [vp, ip, vp, C.c_uint32, C.c_uint32, vp, vp]
    zp = C.POINTER(ScPolishPosesParams)
    L.sc_polish_poses_default_params.argtypes = [zp]
    L.sc_polish_poses.argtypes = [vp, zp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sc_polish_poses_device.argtypes = [vp, zp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    ap = C.POINTER(ScAssignParams)
    L.sc_assign_default_params.argtypes = [ap]
    L.sc_assign_poses_frame.argtypes = [vp, ap, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.sc_assign_poses_frame_device.argtypes = [vp, ap, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.sc_assign_poses_batch.argtypes = [vp, f32p, f32p, u32p, C.c_uint32, pp, ap, vp, C.c_uint32, C.c_uint32, vp, vp]
    L.sc_assign_poses_batch_device.argtypes = [vp, vp, vp, u32p, C.c_uint32, pp, ap, vp, C.c_uint32, C.c_uint32, vp, vp]
    tp = C.POINTER(ScSettleParams)
    L.sc_settle_default_params.argtypes = [tp]
    L.sc_settle_poses_frame.argtypes = [vp, tp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
    L.sc_settle_poses_frame_device.argtypes = [vp, tp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
    L.sc_settle_poses_batch.argtypes = [vp, f32p, f32p, u32p, C.c_uint32, pp, tp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sc_settle_poses_batch_device.argtypes = [vp, vp, vp, u32p, C.c_uint32, pp, tp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.sc_hypothesize_device.argtypes = [vp, vp, vp, C.c_int64, pp, vp, sp]
    L.sc_finalize_device.argtypes = [vp, vp, vp, vp, sp]
    L.sc_hypothesize_begin_device.argtypes = [vp, vp, vp, C.c_int64, pp, vp, sp]
    L.sc_hypothesize_end_device.argtypes = [vp, vp, vp, sp]
    L.sc_finalize_gathered_device.argtypes = [vp, vp, C.c_int, vp, vp, sp]
    L.sc_finalize_gathered_device_async.argtypes = [vp, vp, C.c_int, vp, vp]
    L.sc_shard_plan_query.argtypes = [pp, C.c_int64, C.POINTER(ScShardPlan)]
    L.sc_shard_compat_device.argtypes = [vp, vp, vp, C.c_int64, pp, vp]
    L.sc_shard_edges_device.argtypes = [vp, vp]
    L.sc_shard_select_device.argtypes = [vp, vp, vp]
    L.sc_shard_score_device.argtypes = [vp, vp, vp, sp]
    L.sc_create_multi.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.sc_create_multi_loopback.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.sc_destroy_multi.argtypes = [vp]; L.sc_destroy_multi.restype = None
    L.sc_multi_last_error.argtypes = [vp]; L.sc_multi_last_error.restype = C.c_char_p
    L.sc_register_multi.argtypes = [vp, f32p, f32p, C.c_int64, pp, f32p, f32p, u8p, sp]
    L.sc_compat_host.argtypes = [vp, f32p, f32p, C.c_int64, pp, f32p, u64p, u32p]
    L.sc_triangles_host.argtypes = [vp, f32p, f32p, C.c_int64, pp, u32p, u32p, u32p, u64p, u64p]
    L.sc_kabsch_host.argtypes = [vp, f32p, f32p, C.c_int64, pp, u32p, C.c_uint32, f32p]
    L.sc_score_host.argtypes = [vp, f32p, f32p, C.c_int64, pp, f32p, C.c_uint32, u32p, u64p]
    L.sc_mask_host.argtypes = [vp, f32p, f32p, C.c_int64, pp, f32p, u8p]
    _LIB = L
    return L


def make_params(sigma=0.1, t_cmp=0.9, tau=0.1, min_len=0.1, max_triangles=50000, rank_mode=SC_RANK_WEIGHT,
                layout=SC_AOS, shard_rank=0, shard_world=1, shard_block=1024, flags=0, max_workspace=0,
                score_mode=0, shard_cand_level=0) -> ScParams:
    return ScParams(C.sizeof(ScParams), sigma, t_cmp, tau, min_len, max_triangles, rank_mode, layout, shard_rank,
                    shard_world, shard_block, flags, max_workspace, score_mode, shard_cand_level)


def make_match_params(dim: int, knn: int = 1, mutual: bool = False, ratio: float = 0.0, flags: int = 0) -> ScMatchParams:
    """sc_match_params for descriptors of length `dim`: knn 1 .. 4; mutual / ratio (in (0, 1), 0 = off) with knn == 1 only."""
    return ScMatchParams(C.sizeof(ScMatchParams), dim, knn, flags | (SC_MATCH_MUTUAL if mutual else 0), ratio)


def make_guide_params(gate: float, layout: int = SC_AOS, flags: int = 0) -> ScGuideParams:
    """sc_guide_params: the gate radius (finite, > 0) and the layout of the keypoint arrays of sc_match_guided; flags: 0, or — the
    batch and pairs entries only — SC_GUIDE_POSE_STATUS."""
    return ScGuideParams(C.sizeof(ScGuideParams), layout, gate, flags)


def make_polish_params(candidates: int = 8, max_iter: int = 16, flags: int = 0) -> ScPolishParams:
    """sc_polish_params: the best `candidates` hypotheses of the frame (1 .. 64), at most `max_iter` refits each (1 .. 64)."""
    return ScPolishParams(C.sizeof(ScPolishParams), candidates, max_iter, flags)


def make_pose_info_params(sel_mode: int = SC_POSE_INFO_SEL_NONE, label0: int = 0, flags: int = 0) -> ScPoseInfoParams:
    """sc_pose_info_params: sel_mode SC_POSE_INFO_SEL_*, label0 (SEL_LABEL only), flags SC_POSE_INFO_STATUS or 0."""
    return ScPoseInfoParams(C.sizeof(ScPoseInfoParams), sel_mode, label0, flags)


def make_polish_poses_params(max_iter: int = 16, sel_mode: int = SC_POLISH_POSES_SEL_NONE, label0: int = 0, flags: int = 0) -> ScPolishPosesParams:
    """sc_polish_poses_params: max_iter 1 .. 64, sel_mode SC_POLISH_POSES_SEL_*, label0 (SEL_LABEL / SEL_ALIVE only), flags
    SC_POLISH_POSES_STATUS or 0."""
    return ScPolishPosesParams(C.sizeof(ScPolishPosesParams), max_iter, sel_mode, label0, flags)


def make_assign_params(mode: int = SC_ASSIGN_BEST, sel_mode: int = SC_ASSIGN_SEL_NONE, flags: int = 0) -> ScAssignParams:
    """sc_assign_params: mode SC_ASSIGN_BEST / _FIRST, sel_mode SC_ASSIGN_SEL_*, flags SC_ASSIGN_STATUS or 0."""
    return ScAssignParams(C.sizeof(ScAssignParams), mode, sel_mode, flags)


def make_settle_params(max_iter: int = 16, sel_mode: int = SC_ASSIGN_SEL_NONE, flags: int = 0) -> ScSettleParams:
    """sc_settle_params: max_iter 1 .. 64 counted rounds, sel_mode SC_ASSIGN_SEL_*, flags SC_SETTLE_STATUS or 0."""
    return ScSettleParams(C.sizeof(ScSettleParams), max_iter, sel_mode, flags)


def shard_plan(params: ScParams, n: int) -> ScShardPlan:
    """sc_shard_plan_query: sizes of d_bits_all / the candidate blobs for `params` (shard_world) and n correspondences."""
    plan = ScShardPlan(size=C.sizeof(ScShardPlan))
    rc = load_library().sc_shard_plan_query(C.byref(params), n, C.byref(plan))
    if rc != SC_OK:
        raise SacCotError(rc, "sc_shard_plan_query")
    return plan


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _f32c(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _pack_problems(problems, layout):
    """A list of (src (n_b, 3), tgt (n_b, 3)) problems -> the packed (src, tgt, offset) of the batch entries, the points in `layout`."""
    sizes = [np.shape(s)[0] for s, _ in problems]
    src = np.concatenate([_f32c(s).reshape(-1, 3) for s, _ in problems]) if sizes else np.zeros((0, 3), np.float32)
    tgt = np.concatenate([_f32c(t).reshape(-1, 3) for _, t in problems]) if sizes else np.zeros((0, 3), np.float32)
    if layout == SC_SOA:
        src, tgt = np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)
    return src, tgt, Registrar._offsets(sizes)


def _record_dict(r) -> dict:
    """A BATCH_RESULT_DTYPE record as dict(status, R, t, stats)."""
    stats = {k: int(r[k]) for k in ("n", "edges", "tri_total", "tri_kept", "best_rank", "best_count")}
    return dict(status=int(r["status"]), R=r["Rt"][:9].reshape(3, 3).copy(), t=r["Rt"][9:].copy(), stats=stats)


class Registrar:
    """One GPU context (`sc_ctx`): one process, one GPU, one stream."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.sc_create(device, C.byref(h))
        if rc != SC_OK:
            raise SacCotError(rc, "sc_create failed (no usable HIP device? this library has no CPU fallback): "
                              + self._lib.sc_strerror(rc).decode())
        self._h = h
        self.device = device
        self._frame_n = 0  # correspondences of the last register* call: what peel() sizes its mask by

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, allow=()):
        if rc != SC_OK and rc not in allow:
            raise SacCotError(rc, self._lib.sc_strerror(rc).decode() + " — " + self._lib.sc_last_error(self._h).decode())
        return rc

    def set_stream(self, stream_ptr: int | None):
        """Enqueue on a caller stream: pass `torch.cuda.current_stream().cuda_stream` (0 = the default stream, mapped
        to SC_STREAM_DEFAULT here).  None restores the context's private, NON-blocking stream — nothing the caller
        enqueues elsewhere (an all-reduce of the key, a copy of the mask) is ordered against it."""
        if stream_ptr is None:
            ptr = 0
        elif stream_ptr == 0:
            ptr = 1  # SC_STREAM_DEFAULT
        else:
            ptr = stream_ptr
        self._check(self._lib.sc_set_stream(self._h, C.c_void_p(ptr)))

    def set_debug(self, **knobs):
        """sc_set_debug: scheduling knobs / forced fallbacks for tests and sweeps (field names of `sc_debug`); no
        arguments restores the defaults.  The library itself reads no environment variable."""
        if not knobs:
            self._check(self._lib.sc_set_debug(self._h, None))
            return
        cls = ScDebugLab if "filter_variant" in knobs else ScDebug   # (lab builds have a field more; the product rejects the lab struct's size)
        d = cls(size=C.sizeof(cls), compact_self_max=-1, scan_self_max=-1)
        names = dict(cls._fields_)
        for k, v in knobs.items():
            if k in cls._ALIASES:
                arr, slot = cls._ALIASES[k]
                getattr(d, arr)[slot] = int(v)
            elif k in names and k not in ("size", "grid_blocks", "lanes_per_edge", "lab_pad_"):
                setattr(d, k, int(v))
            else:
                raise KeyError(f"sc_debug has no field {k!r}")
        self._check(self._lib.sc_set_debug(self._h, C.cast(C.byref(d), C.POINTER(ScDebug))))

    def debug_last(self) -> dict:
        """sc_debug_last: which stage C2 kernel the last call ran (0 plain fp32, 1 linear filter + exact pass, 2 Gram
        filter + exact pass), what the filter handed to the exact pass, how the call was enqueued (fast_path) and the result
        of the matrix-pipe probe (gram_guard).  Synchronises the context's stream."""
        d = ScDebugInfo(size=C.sizeof(ScDebugInfo))
        self._check(self._lib.sc_debug_last(self._h, C.byref(d)))
        return {k: getattr(d, k) for k, _ in ScDebugInfo._fields_ if k not in ("size", "reserved", "reserved2")}

    # ---- drop-in entry point ----------------------------------------------------------------------------
    def register(self, src, tgt, params: ScParams | None = None, **kw):
        """(n,3) src/tgt correspondences -> dict(status, R (3,3), t (3,), mask (n,) uint8, stats)."""
        p = params or make_params(**kw)
        src, tgt = _f32c(src), _f32c(tgt)
        n = src.shape[0] if p.layout == SC_AOS else src.shape[1]
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32); mask = np.zeros(n, np.uint8)
        st = ScStats(C.sizeof(ScStats))
        self._frame_n = n
        rc = self._check(self._lib.sc_register(self._h, _p(src, C.c_float), _p(tgt, C.c_float), n, C.byref(p),
                                               _p(R, C.c_float), _p(t, C.c_float), _p(mask, C.c_uint8), C.byref(st)),
                         allow=(SC_ENOHYP,))
        return dict(status=rc, R=R.reshape(3, 3), t=t, mask=mask, stats=st.as_dict())

    # ---- device-resident forms (pointers are ints: torch .data_ptr()) -------------------------------------
    def register_device(self, d_src: int, d_tgt: int, n: int, params: ScParams, d_Rt: int, d_mask: int):
        st = ScStats(C.sizeof(ScStats))
        self._frame_n = n
        rc = self._check(self._lib.sc_register_device(self._h, d_src, d_tgt, n, C.byref(params), d_Rt, d_mask,
                                                      C.byref(st)), allow=(SC_ENOHYP,))
        return rc, st.as_dict()

    def register_device_async(self, d_src: int, d_tgt: int, n: int, params: ScParams, d_Rt: int, d_mask: int):
        """sc_register_device_async: enqueue the whole path and return; `wait()` delivers status and statistics.  At most
        one call outstanding per Registrar; inputs must stay valid until wait() returns."""
        self._frame_n = n
        self._check(self._lib.sc_register_device_async(self._h, d_src, d_tgt, n, C.byref(params), d_Rt, d_mask))

    def wait(self):
        """sc_wait: the second half of register_device_async / finalize_gathered_device_async."""
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_wait(self._h, C.byref(st)), allow=(SC_ENOHYP, SC_ERETRY, SC_EBOUND))
        return rc, st.as_dict()

    # ---- many small registrations in one launch (include/saccot.h, sc_register_batch) ------------------------------
    def register_batch_raw(self, src, tgt, offset, params: ScParams):
        """sc_register_batch on packed arrays: src / tgt (total, 3) — or (3, total) with SC_SOA —, offset (B + 1,) uint32 ->
        (records (B,) of BATCH_RESULT_DTYPE, mask (total,) uint8).  A problem's status is a field of its record."""
        src, tgt = _f32c(src), _f32c(tgt)
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        nb = max(len(offset) - 1, 0)
        total = int(offset[-1]) if len(offset) else 0
        res = np.zeros(max(nb, 1), BATCH_RESULT_DTYPE); mask = np.zeros(max(total, 1), np.uint8)
        self._frame_n = 0
        self._check(self._lib.sc_register_batch(self._h, _p(src, C.c_float), _p(tgt, C.c_float), _p(offset, C.c_uint32), nb,
                                                C.byref(params), res.ctypes.data_as(C.c_void_p), _p(mask, C.c_uint8)))
        return res[:nb], mask[:total]

    def register_batch(self, problems, params: ScParams | None = None, **kw):
        """sc_register_batch: many small problems (3 .. SC_BATCH_MAX_N correspondences each), one launch.  problems: a list of
        (src (n_b, 3), tgt (n_b, 3)) pairs, or the packed (src, tgt, offset) themselves (in params' layout).  -> a list of
        dict(status, R, t, mask, stats) with register()'s keys, one per problem; stats holds n, edges, tri_total, tri_kept, best_rank,
        best_count.  A problem's SC_ENOHYP / SC_EINVAL (a non-finite coordinate) is its status, not an exception."""
        p = params or make_params(**kw)
        if isinstance(problems, tuple) and len(problems) == 3 and not isinstance(problems[0], tuple):
            src, tgt, offset = problems
        else:
            src, tgt, offset = _pack_problems(problems, p.layout)
        res, mask = self.register_batch_raw(src, tgt, offset, p)
        return [dict(_record_dict(r), mask=mask[int(offset[b]): int(offset[b + 1])].copy()) for b, r in enumerate(res)]

    def register_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, d_res: int, d_mask: int):
        """sc_register_batch_device: points, records (80 bytes each) and mask in HBM, offset a HOST array (B + 1,) uint32; enqueues
        on the context's stream and returns without waiting."""
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_register_batch_device(self._h, d_src, d_tgt, _p(offset, C.c_uint32), max(len(offset) - 1, 0),
                                                       C.byref(params), d_res, d_mask))

    # ---- further rigid motions from the frame the last register* call left (include/saccot.h, sc_peel) ------
    def peel(self):
        """sc_peel: the next round on the frame in this context -> dict(status, R, t, mask, stats) like register()'s; SC_ENOHYP
        (no hypothesis explains an unclaimed correspondence) is a status, not an exception.  The frame's n sizes the mask."""
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32)
        n = self._frame_n
        mask = np.zeros(max(n, 1), np.uint8)
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_peel(self._h, _p(R, C.c_float), _p(t, C.c_float), _p(mask, C.c_uint8), C.byref(st)),
                         allow=(SC_ENOHYP,))
        return dict(status=rc, R=R.reshape(3, 3), t=t, mask=mask[:n], stats=st.as_dict())

    def peel_device(self, d_Rt: int, d_mask: int):
        """sc_peel_device: the same with the outputs in HBM (d_Rt: 12 floats, d_mask: n bytes) -> (status, stats)."""
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_peel_device(self._h, d_Rt, d_mask, C.byref(st)), allow=(SC_ENOHYP,))
        return rc, st.as_dict()

    # ---- refits iterated to a fixed point on that frame (include/saccot.h, sc_polish) --------------------------------
    def polish(self, pparams: ScPolishParams | None = None, **kw):
        """sc_polish: the frame's best hypotheses, each refitted over its own inliers until nothing changes; the best of them ->
        dict(status, R, t, mask, n_cand, cand (candidates,) records of POLISH_CAND_DTYPE — those past n_cand zeroed —, stats).  stats["best_count"] is the polished
        score and may be below the frame's.  kw: candidates, max_iter (make_polish_params)."""
        q = pparams or make_polish_params(**kw)
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32)
        n = self._frame_n
        mask = np.zeros(max(n, 1), np.uint8)
        cand = np.zeros(max(int(q.candidates), 1), POLISH_CAND_DTYPE); k = C.c_uint32(0)
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_polish(self._h, C.byref(q), _p(R, C.c_float), _p(t, C.c_float), _p(mask, C.c_uint8),
                                             cand.ctypes.data_as(C.c_void_p), C.byref(k), C.byref(st)), allow=(SC_ENOHYP,))
        return dict(status=rc, R=R.reshape(3, 3), t=t, mask=mask[:n], n_cand=int(k.value), cand=cand, stats=st.as_dict())

    def polish_device(self, pparams: ScPolishParams, d_Rt: int, d_mask: int, d_cand: int = 0, d_ncand: int = 0):
        """sc_polish_device: the same with the outputs in HBM (d_Rt: 12 floats, d_mask: n bytes, d_cand: `candidates` records of
        64 bytes or 0, d_ncand: one uint32 or 0) -> (status, stats)."""
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_polish_device(self._h, C.byref(pparams), d_Rt, d_mask, d_cand or None, d_ncand or None,
                                                    C.byref(st)), allow=(SC_ENOHYP,))
        return rc, st.as_dict()

    def register_instances(self, src, tgt, max_instances: int = 8, min_score: int = 0, params: ScParams | None = None, **kw):
        """sc_register_instances: the frame and its rounds in one call -> dict(status, Rt (k,12), score (k,), label (n,) int32:
        the motion that claimed each correspondence, -1 for none; stats: the frame's)."""
        p = params or make_params(**kw)
        src, tgt = _f32c(src), _f32c(tgt)
        n = src.shape[0] if p.layout == SC_AOS else src.shape[1]
        Rt = np.zeros((max_instances, 12), np.float32); score = np.zeros(max_instances, np.uint32)
        label = np.full(n, -1, np.int32); found = C.c_uint32(0)
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_register_instances(self._h, _p(src, C.c_float), _p(tgt, C.c_float), n, C.byref(p),
                                                         max_instances, min_score, _p(Rt, C.c_float), _p(score, C.c_uint32),
                                                         _p(label, C.c_int32), C.byref(found), C.byref(st)), allow=(SC_ENOHYP,))
        self._frame_n = n
        k = int(found.value)
        return dict(status=rc, Rt=Rt[:k].copy(), score=score[:k].copy(), label=label, stats=st.as_dict())

    # ---- descriptor matching (include/saccot.h, sc_match) ------------------------------------------------------
    def match(self, fsrc, ftgt, mparams: ScMatchParams | None = None, **kw):
        """sc_match: (ns, D) and (nt, D) descriptors -> dict(n, corr (n, 2) int32: source row, target row, in ascending (row, rank)
        order; d2 (n,) float32: the canonical squared distances).  kw: knn, mutual, ratio (make_match_params)."""
        fsrc, ftgt = _f32c(fsrc), _f32c(ftgt)
        if fsrc.ndim != 2 or ftgt.ndim != 2 or fsrc.shape[1] != ftgt.shape[1]:
            raise ValueError("match: fsrc (ns, D) and ftgt (nt, D) with one D")
        m = mparams or make_match_params(fsrc.shape[1], **kw)
        cap = max(fsrc.shape[0] * max(int(m.knn), 1), 1)
        corr = np.zeros((cap, 2), np.int32); d2 = np.zeros(cap, np.float32); n = C.c_uint32(0)
        self._check(self._lib.sc_match(self._h, _p(fsrc, C.c_float), fsrc.shape[0], _p(ftgt, C.c_float), ftgt.shape[0], C.byref(m),
                                       _p(corr, C.c_int32), _p(d2, C.c_float), C.byref(n)))
        k = int(n.value)
        return dict(n=k, corr=corr[:k].copy(), d2=d2[:k].copy())

    def match_device(self, d_fsrc: int, ns: int, d_ftgt: int, nt: int, mparams: ScMatchParams, d_corr: int, d_d2: int, d_count: int):
        """sc_match_device: everything in HBM (d_corr: ns * knn x 2 int32, d_d2: ns * knn float32, d_count: 2 x uint32 — the
        count, and 1 if a non-finite descriptor was read); enqueues on the context's stream and returns without waiting."""
        self._check(self._lib.sc_match_device(self._h, d_fsrc, ns, d_ftgt, nt, C.byref(mparams), d_corr, d_d2, d_count))

    def register_features(self, src_pts, fsrc, tgt_pts, ftgt, mparams: ScMatchParams | None = None, params: ScParams | None = None,
                          knn: int = 1, mutual: bool = False, ratio: float = 0.0, **kw):
        """sc_register_features: keypoints and their descriptors in -> dict(status, R, t, n, corr (n, 2), d2 (n,), mask (n,), stats):
        sc_match on the descriptors, then sc_register on the matched points, gathered on the device.  Fewer than 3 matches:
        SC_ENOHYP, R = I.  Leaves a frame of n correspondences: peel() may follow."""
        p = params or make_params(**kw)
        src_pts, tgt_pts, fsrc, ftgt = _f32c(src_pts), _f32c(tgt_pts), _f32c(fsrc), _f32c(ftgt)
        m = mparams or make_match_params(fsrc.shape[1], knn, mutual, ratio)
        ns, nt = fsrc.shape[0], ftgt.shape[0]
        if (src_pts.shape[0] if p.layout == SC_AOS else src_pts.shape[1]) != ns or \
                (tgt_pts.shape[0] if p.layout == SC_AOS else tgt_pts.shape[1]) != nt or fsrc.shape[1] != ftgt.shape[1]:
            raise ValueError("register_features: one descriptor row per point, one D")
        cap = max(ns * max(int(m.knn), 1), 1)
        corr = np.zeros((cap, 2), np.int32); d2 = np.zeros(cap, np.float32); n = C.c_uint32(0)
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32); mask = np.zeros(cap, np.uint8)
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_register_features(self._h, _p(src_pts, C.c_float), _p(fsrc, C.c_float), ns, _p(tgt_pts, C.c_float),
                                                        _p(ftgt, C.c_float), nt, C.byref(m), C.byref(p), _p(R, C.c_float),
                                                        _p(t, C.c_float), _p(corr, C.c_int32), _p(d2, C.c_float), C.byref(n),
                                                        _p(mask, C.c_uint8), C.byref(st)), allow=(SC_ENOHYP,))
        k = int(n.value)
        self._frame_n = k
        return dict(status=rc, R=R.reshape(3, 3), t=t, n=k, corr=corr[:k].copy(), d2=d2[:k].copy(), mask=mask[:k].copy(),
                    stats=st.as_dict())

    # ---- descriptor matching gated by a pose prior (include/saccot.h, sc_match_guided) --------------------------
    @staticmethod
    def _guided_inputs(who, src_pts, fsrc, tgt_pts, ftgt, layout):
        src_pts, tgt_pts, fsrc, ftgt = _f32c(src_pts), _f32c(tgt_pts), _f32c(fsrc), _f32c(ftgt)
        if fsrc.ndim != 2 or ftgt.ndim != 2 or fsrc.shape[1] != ftgt.shape[1] or src_pts.ndim != 2 or tgt_pts.ndim != 2:
            raise ValueError(who + ": fsrc (ns, D) and ftgt (nt, D) with one D, points (n, 3) or, SC_SOA, (3, n)")
        ax = 1 if layout == SC_SOA else 0
        if src_pts.shape[ax] != fsrc.shape[0] or tgt_pts.shape[ax] != ftgt.shape[0] or src_pts.shape[1 - ax] != 3 or tgt_pts.shape[1 - ax] != 3:
            raise ValueError(who + ": one descriptor row per point")
        return src_pts, fsrc, tgt_pts, ftgt

    def match_guided(self, src_pts, fsrc, tgt_pts, ftgt, Rt, gate: float | None = None, layout: int = SC_AOS,
                     mparams: ScMatchParams | None = None, gparams: ScGuideParams | None = None, **kw):
        """sc_match_guided: keypoints and descriptors of both sets, the pose prior Rt (12 floats: R row-major, then t) and the gate
        radius -> dict(n, corr (n, 2) int32, d2 (n,), g2 (n,): the gate residual of every entry).  Row i may only pair with the
        targets within `gate` of where Rt puts point i.  kw: knn, mutual, ratio (make_match_params)."""
        g = gparams or make_guide_params(gate, layout)
        src_pts, fsrc, tgt_pts, ftgt = self._guided_inputs("match_guided", src_pts, fsrc, tgt_pts, ftgt, g.layout)
        Rt = _f32c(Rt).reshape(12)
        m = mparams or make_match_params(fsrc.shape[1], **kw)
        cap = max(fsrc.shape[0] * max(int(m.knn), 1), 1)
        corr = np.zeros((cap, 2), np.int32); d2 = np.zeros(cap, np.float32); g2 = np.zeros(cap, np.float32); n = C.c_uint32(0)
        self._check(self._lib.sc_match_guided(self._h, _p(src_pts, C.c_float), _p(fsrc, C.c_float), fsrc.shape[0], _p(tgt_pts, C.c_float),
                                              _p(ftgt, C.c_float), ftgt.shape[0], C.byref(m), C.byref(g), _p(Rt, C.c_float),
                                              _p(corr, C.c_int32), _p(d2, C.c_float), _p(g2, C.c_float), C.byref(n)))
        k = int(n.value)
        return dict(n=k, corr=corr[:k].copy(), d2=d2[:k].copy(), g2=g2[:k].copy())

    def match_guided_device(self, d_src_pts: int, d_fsrc: int, ns: int, d_tgt_pts: int, d_ftgt: int, nt: int, mparams: ScMatchParams,
                            gparams: ScGuideParams, d_Rt: int, d_corr: int, d_d2: int, d_g2: int | None, d_count: int):
        """sc_match_guided_device: everything in HBM (d_Rt: 12 floats, read in stream order; d_corr, d_d2, d_count as match_device's;
        d_g2: ns * knn float32 or None); three stream operations on the context's stream, returns without waiting."""
        self._check(self._lib.sc_match_guided_device(self._h, d_src_pts, d_fsrc, ns, d_tgt_pts, d_ftgt, nt, C.byref(mparams),
                                                     C.byref(gparams), d_Rt, d_corr, d_d2, d_g2, d_count))

    def register_guided_features(self, src_pts, fsrc, tgt_pts, ftgt, Rt_prior, gate: float | None = None,
                                 mparams: ScMatchParams | None = None, gparams: ScGuideParams | None = None,
                                 params: ScParams | None = None, knn: int = 1, mutual: bool = False, ratio: float = 0.0, **kw):
        """sc_register_guided_features: register_features with the guided match under Rt_prior in front -> dict(status, R, t, n,
        corr (n, 2), d2 (n,), g2 (n,), mask (n,), stats).  Fewer than 3 matches: SC_ENOHYP, R = I.  Leaves a frame of n
        correspondences: peel(), polish() ... may follow."""
        p = params or make_params(**kw)
        g = gparams or make_guide_params(gate, p.layout)
        src_pts, fsrc, tgt_pts, ftgt = self._guided_inputs("register_guided_features", src_pts, fsrc, tgt_pts, ftgt, g.layout)
        Rt = _f32c(Rt_prior).reshape(12)
        m = mparams or make_match_params(fsrc.shape[1], knn, mutual, ratio)
        ns, nt = fsrc.shape[0], ftgt.shape[0]
        cap = max(ns * max(int(m.knn), 1), 1)
        corr = np.zeros((cap, 2), np.int32); d2 = np.zeros(cap, np.float32); g2 = np.zeros(cap, np.float32); n = C.c_uint32(0)
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32); mask = np.zeros(cap, np.uint8)
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_register_guided_features(
            self._h, _p(src_pts, C.c_float), _p(fsrc, C.c_float), ns, _p(tgt_pts, C.c_float), _p(ftgt, C.c_float), nt, C.byref(m),
            C.byref(g), _p(Rt, C.c_float), C.byref(p), _p(R, C.c_float), _p(t, C.c_float), _p(corr, C.c_int32), _p(d2, C.c_float),
            _p(g2, C.c_float), C.byref(n), _p(mask, C.c_uint8), C.byref(st)), allow=(SC_ENOHYP,))
        k = int(n.value)
        self._frame_n = k
        return dict(status=rc, R=R.reshape(3, 3), t=t, n=k, corr=corr[:k].copy(), d2=d2[:k].copy(), g2=g2[:k].copy(),
                    mask=mask[:k].copy(), stats=st.as_dict())

    # ---- descriptor matching gated by several poses (include/saccot.h, sc_match_guided_poses) -------------------
    def match_guided_poses(self, src_pts, fsrc, tgt_pts, ftgt, pose, gate: float | None = None, layout: int = SC_AOS, flags: int = 0,
                           mparams: ScMatchParams | None = None, gparams: ScGuideParams | None = None, **kw):
        """sc_match_guided_poses: match_guided under the union of K poses.  pose: K records (_pose_records: a (K, 12) float array, or
        records of a dtype that starts with float Rt[12] and, with SC_GUIDE_POSE_STATUS in flags, holds an int32 status at byte 48)
        -> dict(n, corr (n, 2) int32, d2 (n,), g2 (n,): the smallest gate residual of every entry, label (n,) int32: the record
        it belongs to).  kw: knn, mutual, ratio (make_match_params)."""
        g = gparams or make_guide_params(gate, layout, flags)
        src_pts, fsrc, tgt_pts, ftgt = self._guided_inputs("match_guided_poses", src_pts, fsrc, tgt_pts, ftgt, g.layout)
        pose, stride = self._pose_records(pose)
        m = mparams or make_match_params(fsrc.shape[1], **kw)
        cap = max(fsrc.shape[0] * max(int(m.knn), 1), 1)
        corr = np.zeros((cap, 2), np.int32); d2 = np.zeros(cap, np.float32); g2 = np.zeros(cap, np.float32); n = C.c_uint32(0)
        label = np.zeros(cap, np.int32)
        self._check(self._lib.sc_match_guided_poses(self._h, _p(src_pts, C.c_float), _p(fsrc, C.c_float), fsrc.shape[0],
                                                    _p(tgt_pts, C.c_float), _p(ftgt, C.c_float), ftgt.shape[0], C.byref(m), C.byref(g),
                                                    pose.ctypes.data_as(C.c_void_p), stride, len(pose), _p(corr, C.c_int32),
                                                    _p(d2, C.c_float), _p(g2, C.c_float), _p(label, C.c_int32), C.byref(n)))
        k = int(n.value)
        return dict(n=k, corr=corr[:k].copy(), d2=d2[:k].copy(), g2=g2[:k].copy(), label=label[:k].copy())

    def match_guided_poses_device(self, d_src_pts: int, d_fsrc: int, ns: int, d_tgt_pts: int, d_ftgt: int, nt: int, mparams: ScMatchParams,
                                  gparams: ScGuideParams, d_pose: int, pose_stride: int, n_poses: int, d_corr: int, d_d2: int,
                                  d_g2: int | None, d_label: int | None, d_count: int):
        """sc_match_guided_poses_device: everything in HBM (d_pose: n_poses records pose_stride bytes apart, read in stream order;
        d_corr, d_d2, d_g2, d_count as match_guided_device's; d_label: ns * knn int32 or None); three stream operations on the
        context's stream, returns without waiting."""
        self._check(self._lib.sc_match_guided_poses_device(self._h, d_src_pts, d_fsrc, ns, d_tgt_pts, d_ftgt, nt, C.byref(mparams),
                                                           C.byref(gparams), d_pose, pose_stride, n_poses, d_corr, d_d2, d_g2, d_label,
                                                           d_count))

    def register_guided_poses_features(self, src_pts, fsrc, tgt_pts, ftgt, pose, gate: float | None = None, flags: int = 0,
                                       mparams: ScMatchParams | None = None, gparams: ScGuideParams | None = None,
                                       params: ScParams | None = None, knn: int = 1, mutual: bool = False, ratio: float = 0.0, **kw):
        """sc_register_guided_poses_features: register_features with the several-pose match in front -> dict(status, R, t, n,
        corr (n, 2), d2 (n,), g2 (n,), label (n,), mask (n,), stats).  Fewer than 3 matches: SC_ENOHYP, R = I.  Leaves a frame of n
        correspondences: polish_poses / pose_info_frame with SEL_LABEL and the returned labels may follow."""
        p = params or make_params(**kw)
        g = gparams or make_guide_params(gate, p.layout, flags)
        src_pts, fsrc, tgt_pts, ftgt = self._guided_inputs("register_guided_poses_features", src_pts, fsrc, tgt_pts, ftgt, g.layout)
        pose, stride = self._pose_records(pose)
        m = mparams or make_match_params(fsrc.shape[1], knn, mutual, ratio)
        ns, nt = fsrc.shape[0], ftgt.shape[0]
        cap = max(ns * max(int(m.knn), 1), 1)
        corr = np.zeros((cap, 2), np.int32); d2 = np.zeros(cap, np.float32); g2 = np.zeros(cap, np.float32); n = C.c_uint32(0)
        label = np.zeros(cap, np.int32)
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32); mask = np.zeros(cap, np.uint8)
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_register_guided_poses_features(
            self._h, _p(src_pts, C.c_float), _p(fsrc, C.c_float), ns, _p(tgt_pts, C.c_float), _p(ftgt, C.c_float), nt, C.byref(m),
            C.byref(g), pose.ctypes.data_as(C.c_void_p), stride, len(pose), C.byref(p), _p(R, C.c_float), _p(t, C.c_float),
            _p(corr, C.c_int32), _p(d2, C.c_float), _p(g2, C.c_float), _p(label, C.c_int32), C.byref(n), _p(mask, C.c_uint8), C.byref(st)),
            allow=(SC_ENOHYP,))
        k = int(n.value)
        self._frame_n = k
        return dict(status=rc, R=R.reshape(3, 3), t=t, n=k, corr=corr[:k].copy(), d2=d2[:k].copy(), g2=g2[:k].copy(),
                    label=label[:k].copy(), mask=mask[:k].copy(), stats=st.as_dict())

    # ---- descriptor matching for a batch of small problems (include/saccot.h, sc_match_batch) -------------------
    @staticmethod
    def _offsets(sizes):
        return np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.uint32)

    def match_batch_raw(self, fsrc, src_off, ftgt, tgt_off, mparams: ScMatchParams):
        """sc_match_batch on packed arrays: fsrc (total_s, D), ftgt (total_t, D), both offset arrays (B + 1,) uint32 ->
        (corr (total_s * knn, 2) int32, d2 (total_s * knn,) float32, count (B, 2) uint32).  Problem b's slot starts at entry
        src_off[b] * knn; count[b] = (n_b, 1 if the problem read a non-finite descriptor)."""
        fsrc, ftgt = _f32c(fsrc), _f32c(ftgt)
        src_off, tgt_off = np.ascontiguousarray(src_off, dtype=np.uint32), np.ascontiguousarray(tgt_off, dtype=np.uint32)
        nb = max(len(src_off) - 1, 0)
        slots = (int(src_off[-1]) if len(src_off) else 0) * max(int(mparams.knn), 1)
        corr = np.zeros((max(slots, 1), 2), np.int32); d2 = np.zeros(max(slots, 1), np.float32); count = np.zeros((max(nb, 1), 2), np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_match_batch(self._h, _p(fsrc, C.c_float), _p(src_off, C.c_uint32), _p(ftgt, C.c_float),
                                             _p(tgt_off, C.c_uint32), nb, C.byref(mparams), _p(corr, C.c_int32), _p(d2, C.c_float),
                                             _p(count, C.c_uint32)))
        return corr[:slots], d2[:slots], count[:nb]

    def match_batch(self, problems, mparams: ScMatchParams | None = None, **kw):
        """sc_match_batch: problems, a list of (fsrc (ns_b, D), ftgt (nt_b, D)) with one D and 1 .. SC_MATCH_BATCH_MAX_N rows a side ->
        a list of dict(n, corr (n, 2) int32 local to the problem, d2 (n,), nonfinite) — match() of every problem alone, in two
        launches for the whole batch.  kw: knn, mutual, ratio (make_match_params).  A non-finite descriptor flags its own problem
        (nonfinite True, n 0), not the call."""
        fs = [_f32c(a) for a, _ in problems]; ft = [_f32c(b) for _, b in problems]
        if not fs or any(a.ndim != 2 or b.ndim != 2 or a.shape[1] != fs[0].shape[1] or b.shape[1] != fs[0].shape[1] for a, b in zip(fs, ft)):
            raise ValueError("match_batch: at least one problem, fsrc (ns, D) and ftgt (nt, D) with one D for all")
        m = mparams or make_match_params(fs[0].shape[1], **kw)
        so, to = self._offsets([len(a) for a in fs]), self._offsets([len(b) for b in ft])
        corr, d2, count = self.match_batch_raw(np.concatenate(fs), so, np.concatenate(ft), to, m)
        out = []
        for b in range(len(fs)):
            lo, k = int(so[b]) * int(m.knn), int(count[b, 0])
            out.append(dict(n=k, corr=corr[lo: lo + k].copy(), d2=d2[lo: lo + k].copy(), nonfinite=bool(count[b, 1])))
        return out

    def match_batch_device(self, d_fsrc: int, src_off, d_ftgt: int, tgt_off, mparams: ScMatchParams, d_corr: int, d_d2: int, d_count: int):
        """sc_match_batch_device: descriptors and outputs in HBM (d_corr total_s * knn x 2 int32, d_d2 total_s * knn float32, d_count
        2 x B uint32), the offsets HOST arrays (B + 1,) uint32; enqueues on the context's stream and returns without waiting."""
        src_off, tgt_off = np.ascontiguousarray(src_off, dtype=np.uint32), np.ascontiguousarray(tgt_off, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_match_batch_device(self._h, d_fsrc, _p(src_off, C.c_uint32), d_ftgt, _p(tgt_off, C.c_uint32),
                                                    max(len(src_off) - 1, 0), C.byref(mparams), d_corr, d_d2, d_count))

    def register_batch_features_raw(self, src_pts, fsrc, src_off, tgt_pts, ftgt, tgt_off, mparams: ScMatchParams, params: ScParams):
        """sc_register_batch_features on packed arrays (points in params' layout) -> (records (B,), corr, d2, count (B, 2), mask
        (total_s * knn,)), the last four slot-positioned as in match_batch_raw."""
        src_pts, fsrc, tgt_pts, ftgt = _f32c(src_pts), _f32c(fsrc), _f32c(tgt_pts), _f32c(ftgt)
        src_off, tgt_off = np.ascontiguousarray(src_off, dtype=np.uint32), np.ascontiguousarray(tgt_off, dtype=np.uint32)
        nb = max(len(src_off) - 1, 0)
        slots = (int(src_off[-1]) if len(src_off) else 0) * max(int(mparams.knn), 1)
        res = np.zeros(max(nb, 1), BATCH_RESULT_DTYPE); mask = np.zeros(max(slots, 1), np.uint8)
        corr = np.zeros((max(slots, 1), 2), np.int32); d2 = np.zeros(max(slots, 1), np.float32); count = np.zeros((max(nb, 1), 2), np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_register_batch_features(self._h, _p(src_pts, C.c_float), _p(fsrc, C.c_float), _p(src_off, C.c_uint32),
                                                         _p(tgt_pts, C.c_float), _p(ftgt, C.c_float), _p(tgt_off, C.c_uint32), nb,
                                                         C.byref(mparams), C.byref(params), res.ctypes.data_as(C.c_void_p),
                                                         _p(corr, C.c_int32), _p(d2, C.c_float), _p(count, C.c_uint32), _p(mask, C.c_uint8)))
        return res[:nb], corr[:slots], d2[:slots], count[:nb], mask[:slots]

    def register_batch_features(self, problems, mparams: ScMatchParams | None = None, params: ScParams | None = None, knn: int = 1,
                                mutual: bool = False, ratio: float = 0.0, **kw):
        """sc_register_batch_features: problems, a list of (src_pts (ns_b, 3), fsrc (ns_b, D), tgt_pts (nt_b, 3), ftgt (nt_b, D)) -> one
        dict per problem shaped like register_batch's (status, R, t, mask, stats) plus corr (n, 2), d2 (n,) and n: the match of
        every problem, then sc_register_batch's kernel on the matched points, and nothing crosses the host in between.  Fewer than 3
        matches: SC_ENOHYP; a non-finite descriptor or matched point: SC_EINVAL — a problem's status, not an exception."""
        p = params or make_params(**kw)
        ps = [_f32c(a).reshape(-1, 3) for a, _, _, _ in problems]; fs = [_f32c(a) for _, a, _, _ in problems]
        pt = [_f32c(a).reshape(-1, 3) for _, _, a, _ in problems]; ft = [_f32c(a) for _, _, _, a in problems]
        if not fs or any(len(a) != len(b) for a, b in zip(ps, fs)) or any(len(a) != len(b) for a, b in zip(pt, ft)) or \
                any(a.ndim != 2 or a.shape[1] != fs[0].shape[1] for a in fs + ft):
            raise ValueError("register_batch_features: at least one problem, one descriptor row per point, one D for all")
        m = mparams or make_match_params(fs[0].shape[1], knn, mutual, ratio)
        so, to = self._offsets([len(a) for a in fs]), self._offsets([len(a) for a in ft])
        src, tgt = np.concatenate(ps), np.concatenate(pt)
        if p.layout == SC_SOA:
            src, tgt = np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)
        res, corr, d2, count, mask = self.register_batch_features_raw(src, np.concatenate(fs), so, tgt, np.concatenate(ft), to, m, p)
        out = []
        for b, r in enumerate(res):
            lo, k = int(so[b]) * int(m.knn), int(count[b, 0])
            out.append(dict(_record_dict(r), mask=mask[lo: lo + k].copy(), n=k, corr=corr[lo: lo + k].copy(), d2=d2[lo: lo + k].copy()))
        return out

    def register_batch_features_device(self, d_src_pts: int, d_fsrc: int, src_off, d_tgt_pts: int, d_ftgt: int, tgt_off,
                                       mparams: ScMatchParams, params: ScParams, d_res: int, d_corr: int, d_d2: int, d_count: int,
                                       d_mask: int):
        """sc_register_batch_features_device: everything but the offsets in HBM (d_res B records of 80 bytes, d_mask total_s * knn
        bytes, the rest as match_batch_device); enqueues on the context's stream and returns without waiting."""
        src_off, tgt_off = np.ascontiguousarray(src_off, dtype=np.uint32), np.ascontiguousarray(tgt_off, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_register_batch_features_device(self._h, d_src_pts, d_fsrc, _p(src_off, C.c_uint32), d_tgt_pts, d_ftgt,
                                                                _p(tgt_off, C.c_uint32), max(len(src_off) - 1, 0), C.byref(mparams),
                                                                C.byref(params), d_res, d_corr, d_d2, d_count, d_mask))

    # ---- iterated fp64 refits for a batch's winners (include/saccot.h, sc_polish_batch) ------------------------------
    def polish_batch_raw(self, src, tgt, offset, params: ScParams, pparams: ScPolishParams, res):
        """sc_polish_batch on packed arrays: src / tgt / offset as register_batch_raw's, res (B,) records of BATCH_RESULT_DTYPE (the
        input poses and statuses; read only) -> (records (B,) of POLISH_BATCH_RESULT_DTYPE, mask (total,) uint8)."""
        src, tgt = _f32c(src), _f32c(tgt)
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        res = np.ascontiguousarray(res, dtype=BATCH_RESULT_DTYPE)
        nb = max(len(offset) - 1, 0)
        if len(res) != nb:
            raise ValueError("polish_batch_raw: one input record per problem")
        total = int(offset[-1]) if len(offset) else 0
        pol = np.zeros(max(nb, 1), POLISH_BATCH_RESULT_DTYPE); mask = np.zeros(max(total, 1), np.uint8)
        self._frame_n = 0
        self._check(self._lib.sc_polish_batch(self._h, _p(src, C.c_float), _p(tgt, C.c_float), _p(offset, C.c_uint32), nb,
                                              C.byref(params), C.byref(pparams), res.ctypes.data_as(C.c_void_p),
                                              pol.ctypes.data_as(C.c_void_p), _p(mask, C.c_uint8)))
        return pol[:nb], mask[:total]

    def polish_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, pparams: ScPolishParams, d_res: int, d_pol: int,
                            d_mask: int):
        """sc_polish_batch_device: points, input records (80 bytes each, read only), output records (64 bytes each) and mask in HBM,
        offset a HOST array (B + 1,) uint32; enqueues on the context's stream and returns without waiting.  d_mask may be the
        buffer register_batch_device wrote."""
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_polish_batch_device(self._h, d_src, d_tgt, _p(offset, C.c_uint32), max(len(offset) - 1, 0),
                                                     C.byref(params), C.byref(pparams), d_res, d_pol, d_mask))

    def polish_batch_slots_device(self, d_src_pts: int, src_off, d_tgt_pts: int, tgt_off, knn: int, params: ScParams,
                                  pparams: ScPolishParams, d_corr: int, d_count: int, d_res: int, d_pol: int, d_mask: int):
        """sc_polish_batch_slots_device: behind register_batch_features_device — its points, offsets, d_corr, d_count and d_res; d_pol
        B records of 64 bytes, d_mask total_s * knn bytes; enqueues on the context's stream and returns without waiting."""
        src_off, tgt_off = np.ascontiguousarray(src_off, dtype=np.uint32), np.ascontiguousarray(tgt_off, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_polish_batch_slots_device(self._h, d_src_pts, _p(src_off, C.c_uint32), d_tgt_pts, _p(tgt_off, C.c_uint32),
                                                           max(len(src_off) - 1, 0), knn, C.byref(params), C.byref(pparams), d_corr,
                                                           d_count, d_res, d_pol, d_mask))

    def register_batch_polished(self, problems, params: ScParams | None = None, pparams: ScPolishParams | None = None, max_iter: int = 16,
                                **kw):
        """sc_register_batch, then sc_polish_batch on its records.  problems: a list of (src (n_b, 3), tgt (n_b, 3)) pairs -> one dict
        per problem: register_batch's (status, R, t, mask, stats: the batch record) plus polished = dict(status, R, t, mask, score0,
        score, iters, stop) — the winner refitted over its own inliers until nothing changes (at most max_iter refits)."""
        p = params or make_params(**kw)
        q = pparams or make_polish_params(candidates=1, max_iter=max_iter)
        src, tgt, offset = _pack_problems(problems, p.layout)
        res, mask = self.register_batch_raw(src, tgt, offset, p)
        pol, pmask = self.polish_batch_raw(src, tgt, offset, p, q, res)
        out = []
        for b, (r, o) in enumerate(zip(res, pol)):
            lo, hi = int(offset[b]), int(offset[b + 1])
            polished = dict(status=int(o["status"]), R=o["Rt"][:9].reshape(3, 3).copy(), t=o["Rt"][9:].copy(), mask=pmask[lo:hi].copy(),
                            score0=int(o["score0"]), score=int(o["score"]), iters=int(o["iters"]), stop=int(o["stop"]))
            out.append(dict(_record_dict(r), mask=mask[lo:hi].copy(), polished=polished))
        return out

    # ---- several rigid motions per batch problem (include/saccot.h, sc_register_instances_batch) --------------------
    def register_instances_batch_raw(self, src, tgt, offset, params: ScParams, max_instances: int = 8, min_score: int = 0):
        """sc_register_instances_batch on packed arrays (src / tgt / offset as register_batch_raw's) -> (records (max_instances, B)
        of BATCH_RESULT_DTYPE, motion-major: records[k, b] is motion k of problem b; label (total,) int32, the motion that claimed a
        correspondence, -1 for none; nfound (B,) uint32)."""
        src, tgt = _f32c(src), _f32c(tgt)
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        nb = max(len(offset) - 1, 0)
        total = int(offset[-1]) if len(offset) else 0
        planes = min(max(int(max_instances), 1), SC_INSTANCES_BATCH_MAX)  # (room; the library refuses what is out of range)
        res = np.zeros((planes, max(nb, 1)), BATCH_RESULT_DTYPE); label = np.zeros(max(total, 1), np.int32)
        nfound = np.zeros(max(nb, 1), np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_register_instances_batch(self._h, _p(src, C.c_float), _p(tgt, C.c_float), _p(offset, C.c_uint32), nb,
                                                          C.byref(params), max_instances, min_score, res.ctypes.data_as(C.c_void_p),
                                                          _p(label, C.c_int32), _p(nfound, C.c_uint32)))
        return res[:, :nb], label[:total], nfound[:nb]

    def register_instances_batch(self, problems, max_instances: int = 8, min_score: int = 0, params: ScParams | None = None, **kw):
        """sc_register_instances_batch: problems, a list of (src (n_b, 3), tgt (n_b, 3)) pairs -> one dict per problem: status (plane
        0's: sc_register_batch's for the problem), Rt (found, 12), score (found,), label (n_b,) int32, stats (plane 0's counts) — the
        keys of register_instances(), a problem's SC_ENOHYP / SC_EINVAL being its status, not an exception."""
        p = params or make_params(**kw)
        src, tgt, offset = _pack_problems(problems, p.layout)
        res, label, nfound = self.register_instances_batch_raw(src, tgt, offset, p, max_instances, min_score)
        out = []
        for b in range(len(offset) - 1):
            k, r0 = int(nfound[b]), _record_dict(res[0, b])
            out.append(dict(status=r0["status"], Rt=res[:k, b]["Rt"].copy(), score=res[:k, b]["best_count"].copy(),
                            label=label[int(offset[b]): int(offset[b + 1])].copy(), stats=r0["stats"]))
        return out

    def register_instances_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, max_instances: int, min_score: int,
                                        d_res: int, d_label: int, d_nfound: int):
        """sc_register_instances_batch_device: points, records (max_instances x B of 80 bytes, motion-major), labels (total int32) and
        nfound (B uint32) in HBM, offset a HOST array (B + 1,) uint32; enqueues on the context's stream and returns without waiting."""
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_register_instances_batch_device(self._h, d_src, d_tgt, _p(offset, C.c_uint32), max(len(offset) - 1, 0),
                                                                 C.byref(params), max_instances, min_score, d_res, d_label, d_nfound))

    def register_instances_batch_features_device(self, d_src_pts: int, d_fsrc: int, src_off, d_tgt_pts: int, d_ftgt: int, tgt_off,
                                                 mparams: ScMatchParams, params: ScParams, max_instances: int, min_score: int, d_res: int,
                                                 d_corr: int, d_d2: int, d_count: int, d_label: int, d_nfound: int):
        """sc_register_instances_batch_features_device: register_batch_features_device with rounds — d_res max_instances x B records,
        d_label total_s * knn int32 positioned like that entry's mask, d_nfound B uint32; returns without waiting."""
        src_off, tgt_off = np.ascontiguousarray(src_off, dtype=np.uint32), np.ascontiguousarray(tgt_off, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_register_instances_batch_features_device(
            self._h, d_src_pts, d_fsrc, _p(src_off, C.c_uint32), d_tgt_pts, d_ftgt, _p(tgt_off, C.c_uint32), max(len(src_off) - 1, 0),
            C.byref(mparams), C.byref(params), max_instances, min_score, d_res, d_corr, d_d2, d_count, d_label, d_nfound))

    # ---- listed pairs of shared keypoint sets (include/saccot.h, sc_match_pairs) ------------------------------------
    @staticmethod
    def _table(set_off, pairs):
        set_off = np.ascontiguousarray(set_off, dtype=np.uint32).reshape(-1)
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1)
        return set_off, pairs, max(len(set_off) - 1, 0), len(pairs) // 2

    @staticmethod
    def pairs_layout(set_off, pairs, knn: int = 1) -> np.ndarray:
        """sc_pairs_layout (host only, no context): set_off (S + 1,) uint32, pairs (P, 2) set indices -> slot (P + 1,) uint32,
        slot[p] the first output entry of pair p and slot[P] the entries in all.  Raises SacCotError for a table or a list the
        pairs entries refuse."""
        set_off, pairs, ns, npairs = Registrar._table(set_off, pairs)
        slot = np.zeros(npairs + 1, np.uint32)
        rc = load_library().sc_pairs_layout(_p(set_off, C.c_uint32), ns, _p(pairs, C.c_uint32), npairs, knn, _p(slot, C.c_uint32))
        if rc != SC_OK:
            raise SacCotError(rc, "sc_pairs_layout")
        return slot

    def match_pairs(self, feat, set_off, pairs, mparams: ScMatchParams | None = None, **kw):
        """sc_match_pairs: feat (total, D) the descriptors of a table of sets, set s rows set_off[s] .. set_off[s + 1]; pairs (P, 2),
        pair p matching source set pairs[p, 0] against target set pairs[p, 1] -> (corr (slots, 2) int32 local to the pair's sets,
        d2 (slots,), count (P, 2) uint32, slot (P + 1,)): pair p's entries start at slot[p], count[p] = (n_p, 1 if one of its
        sets holds a non-finite descriptor).  kw: knn, mutual, ratio (make_match_params)."""
        feat = _f32c(feat)
        m = mparams or make_match_params(feat.shape[1], **kw)
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        slot = self.pairs_layout(set_off, pairs, int(m.knn))
        slots = int(slot[-1])
        corr = np.zeros((max(slots, 1), 2), np.int32); d2 = np.zeros(max(slots, 1), np.float32); count = np.zeros((max(npairs, 1), 2), np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_match_pairs(self._h, _p(feat, C.c_float), _p(set_off, C.c_uint32), ns, _p(pairs, C.c_uint32), npairs,
                                             C.byref(m), _p(corr, C.c_int32), _p(d2, C.c_float), _p(count, C.c_uint32)))
        return corr[:slots], d2[:slots], count[:npairs], slot

    def match_pairs_device(self, d_feat: int, set_off, pairs, mparams: ScMatchParams, d_corr: int, d_d2: int, d_count: int):
        """sc_match_pairs_device: the table's descriptors and the outputs in HBM (d_corr slot[P] x 2 int32, d_d2 slot[P] float32,
        d_count 2 x P uint32), set_off and pairs HOST arrays; enqueues on the context's stream and returns without waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_match_pairs_device(self._h, d_feat, _p(set_off, C.c_uint32), ns, _p(pairs, C.c_uint32), npairs,
                                                    C.byref(mparams), d_corr, d_d2, d_count))

    def register_pairs_features(self, pts, feat, set_off, pairs, mparams: ScMatchParams | None = None, params: ScParams | None = None,
                                knn: int = 1, mutual: bool = False, ratio: float = 0.0, **kw):
        """sc_register_pairs_features: pts the table's points in params' layout ((total, 3), or (3, total) with SC_SOA), feat
        (total, D), set_off, pairs as match_pairs' -> (records (P,) of BATCH_RESULT_DTYPE, corr, d2, count (P, 2), mask (slots,),
        slot (P + 1,)): the match of every pair, then sc_register_batch's kernel on the matched points."""
        pts, feat = _f32c(pts), _f32c(feat)
        p = params or make_params(**kw)
        m = mparams or make_match_params(feat.shape[1], knn, mutual, ratio)
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        slot = self.pairs_layout(set_off, pairs, int(m.knn))
        slots = int(slot[-1])
        res = np.zeros(max(npairs, 1), BATCH_RESULT_DTYPE); mask = np.zeros(max(slots, 1), np.uint8)
        corr = np.zeros((max(slots, 1), 2), np.int32); d2 = np.zeros(max(slots, 1), np.float32); count = np.zeros((max(npairs, 1), 2), np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_register_pairs_features(self._h, _p(pts, C.c_float), _p(feat, C.c_float), _p(set_off, C.c_uint32), ns,
                                                         _p(pairs, C.c_uint32), npairs, C.byref(m), C.byref(p),
                                                         res.ctypes.data_as(C.c_void_p), _p(corr, C.c_int32), _p(d2, C.c_float),
                                                         _p(count, C.c_uint32), _p(mask, C.c_uint8)))
        return res[:npairs], corr[:slots], d2[:slots], count[:npairs], mask[:slots], slot

    def register_pairs_features_device(self, d_pts: int, d_feat: int, set_off, pairs, mparams: ScMatchParams, params: ScParams,
                                       d_res: int, d_corr: int, d_d2: int, d_count: int, d_mask: int):
        """sc_register_pairs_features_device: everything but set_off and pairs in HBM (d_res P records of 80 bytes, d_mask slot[P]
        bytes, the rest as match_pairs_device); enqueues on the context's stream and returns without waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_register_pairs_features_device(self._h, d_pts, d_feat, _p(set_off, C.c_uint32), ns, _p(pairs, C.c_uint32),
                                                                npairs, C.byref(mparams), C.byref(params), d_res, d_corr, d_d2, d_count,
                                                                d_mask))

    def polish_pairs_slots_device(self, d_pts: int, set_off, pairs, knn: int, params: ScParams, pparams: ScPolishParams, d_corr: int,
                                  d_count: int, d_res: int, d_pol: int, d_mask: int):
        """sc_polish_pairs_slots_device: behind register_pairs_features_device — its points, set_off, pairs, d_corr, d_count and
        d_res; d_pol P records of 64 bytes, d_mask slot[P] bytes; enqueues on the context's stream and returns without waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_polish_pairs_slots_device(self._h, d_pts, _p(set_off, C.c_uint32), ns, _p(pairs, C.c_uint32), npairs, knn,
                                                           C.byref(params), C.byref(pparams), d_corr, d_count, d_res, d_pol, d_mask))

    # ---- pose-gated matching for batches and pairs (include/saccot.h, sc_match_guided_batch) ---------------------------
    @staticmethod
    def _pose_records(pose, n=None):
        """pose records as the entries take them: an (n, 12) float array (stride 48), or n records of any dtype whose items start
        with float Rt[12] (and, with SC_GUIDE_POSE_STATUS, an int32 status at byte 48) -> (contiguous array, stride); n = None:
        as many as there are"""
        pose = np.ascontiguousarray(pose)
        if pose.dtype.fields is None:
            pose = np.ascontiguousarray(pose, np.float32).reshape(-1, 12)
            stride = 48
        else:
            pose = pose.reshape(-1)
            stride = pose.dtype.itemsize
        if n is not None and len(pose) != n:
            raise ValueError("one pose record per problem")
        return pose, stride

    def match_guided_batch(self, src_pts, fsrc, src_off, tgt_pts, ftgt, tgt_off, pose, gate: float | None = None, layout: int = SC_AOS,
                           flags: int = 0, mparams: ScMatchParams | None = None, gparams: ScGuideParams | None = None, want_g2: bool = True,
                           **kw):
        """sc_match_guided_batch on packed arrays: points in `layout` ((total, 3), or (3, total) with SC_SOA) beside the descriptors
        and offsets of match_batch_raw; pose: one record per problem (_pose_records) -> (corr (total_s * knn, 2), d2, g2 or None,
        count (B, 2)), slot-positioned as match_batch_raw's: problem b's entries are match_guided() of problem b alone under pose b.
        count[b] = (n_b, 1 if a descriptor, a point or the pose of b is not finite); with SC_GUIDE_POSE_STATUS in flags a record
        whose status is not SC_OK skips its problem: (0, 0)."""
        g = gparams or make_guide_params(gate, layout, flags)
        src_pts, fsrc, tgt_pts, ftgt = _f32c(src_pts), _f32c(fsrc), _f32c(tgt_pts), _f32c(ftgt)
        src_off, tgt_off = np.ascontiguousarray(src_off, dtype=np.uint32), np.ascontiguousarray(tgt_off, dtype=np.uint32)
        m = mparams or make_match_params(fsrc.shape[1], **kw)
        nb = max(len(src_off) - 1, 0)
        pose, stride = self._pose_records(pose, nb)
        slots = (int(src_off[-1]) if len(src_off) else 0) * max(int(m.knn), 1)
        corr = np.zeros((max(slots, 1), 2), np.int32); d2 = np.zeros(max(slots, 1), np.float32); count = np.zeros((max(nb, 1), 2), np.uint32)
        g2 = np.zeros(max(slots, 1), np.float32) if want_g2 else None
        self._frame_n = 0
        self._check(self._lib.sc_match_guided_batch(self._h, _p(src_pts, C.c_float), _p(fsrc, C.c_float), _p(src_off, C.c_uint32),
                                                    _p(tgt_pts, C.c_float), _p(ftgt, C.c_float), _p(tgt_off, C.c_uint32), nb, C.byref(m),
                                                    C.byref(g), pose.ctypes.data_as(C.c_void_p), stride, _p(corr, C.c_int32),
                                                    _p(d2, C.c_float), _p(g2, C.c_float), _p(count, C.c_uint32)))
        return corr[:slots], d2[:slots], (g2[:slots] if want_g2 else None), count[:nb]

    def match_guided_batch_device(self, d_src_pts: int, d_fsrc: int, src_off, d_tgt_pts: int, d_ftgt: int, tgt_off, mparams: ScMatchParams,
                                  gparams: ScGuideParams, d_pose: int, pose_stride: int, d_corr: int, d_d2: int, d_g2: int | None,
                                  d_count: int):
        """sc_match_guided_batch_device: everything but the offsets in HBM (d_pose: B records pose_stride bytes apart, read in stream
        order; d_g2: total_s * knn float32 or None; the rest as match_batch_device); returns without waiting."""
        src_off, tgt_off = np.ascontiguousarray(src_off, dtype=np.uint32), np.ascontiguousarray(tgt_off, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_match_guided_batch_device(self._h, d_src_pts, d_fsrc, _p(src_off, C.c_uint32), d_tgt_pts, d_ftgt,
                                                           _p(tgt_off, C.c_uint32), max(len(src_off) - 1, 0), C.byref(mparams),
                                                           C.byref(gparams), d_pose, pose_stride, d_corr, d_d2, d_g2, d_count))

    def register_guided_batch_features_device(self, d_src_pts: int, d_fsrc: int, src_off, d_tgt_pts: int, d_ftgt: int, tgt_off,
                                              mparams: ScMatchParams, gparams: ScGuideParams, d_pose: int, pose_stride: int,
                                              params: ScParams, d_res: int, d_corr: int, d_d2: int, d_g2: int | None, d_count: int,
                                              d_mask: int):
        """sc_register_guided_batch_features_device: match_guided_batch_device, then the registration on the slots (d_res, d_mask as
        register_batch_features_device's).  d_pose may be d_res; returns without waiting."""
        src_off, tgt_off = np.ascontiguousarray(src_off, dtype=np.uint32), np.ascontiguousarray(tgt_off, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_register_guided_batch_features_device(
            self._h, d_src_pts, d_fsrc, _p(src_off, C.c_uint32), d_tgt_pts, d_ftgt, _p(tgt_off, C.c_uint32), max(len(src_off) - 1, 0),
            C.byref(mparams), C.byref(gparams), d_pose, pose_stride, C.byref(params), d_res, d_corr, d_d2, d_g2, d_count, d_mask))

    def match_guided_pairs(self, pts, feat, set_off, pairs, pose, gate: float | None = None, layout: int = SC_AOS, flags: int = 0,
                           mparams: ScMatchParams | None = None, gparams: ScGuideParams | None = None, want_g2: bool = True, **kw):
        """sc_match_guided_pairs: the table (pts in `layout`, feat) and the list of match_pairs; pose: one record per PAIR ->
        (corr, d2, g2 or None, count (P, 2), slot (P + 1,)) as match_pairs', every pair matched under its own pose."""
        g = gparams or make_guide_params(gate, layout, flags)
        pts, feat = _f32c(pts), _f32c(feat)
        m = mparams or make_match_params(feat.shape[1], **kw)
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        pose, stride = self._pose_records(pose, npairs)
        slot = self.pairs_layout(set_off, pairs, int(m.knn))
        slots = int(slot[-1])
        corr = np.zeros((max(slots, 1), 2), np.int32); d2 = np.zeros(max(slots, 1), np.float32); count = np.zeros((max(npairs, 1), 2), np.uint32)
        g2 = np.zeros(max(slots, 1), np.float32) if want_g2 else None
        self._frame_n = 0
        self._check(self._lib.sc_match_guided_pairs(self._h, _p(pts, C.c_float), _p(feat, C.c_float), _p(set_off, C.c_uint32), ns,
                                                    _p(pairs, C.c_uint32), npairs, C.byref(m), C.byref(g), pose.ctypes.data_as(C.c_void_p),
                                                    stride, _p(corr, C.c_int32), _p(d2, C.c_float), _p(g2, C.c_float),
                                                    _p(count, C.c_uint32)))
        return corr[:slots], d2[:slots], (g2[:slots] if want_g2 else None), count[:npairs], slot

    def match_guided_pairs_device(self, d_pts: int, d_feat: int, set_off, pairs, mparams: ScMatchParams, gparams: ScGuideParams,
                                  d_pose: int, pose_stride: int, d_corr: int, d_d2: int, d_g2: int | None, d_count: int):
        """sc_match_guided_pairs_device: the table, the pose records (one per pair) and the outputs in HBM, set_off and pairs HOST
        arrays; returns without waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_match_guided_pairs_device(self._h, d_pts, d_feat, _p(set_off, C.c_uint32), ns, _p(pairs, C.c_uint32),
                                                           npairs, C.byref(mparams), C.byref(gparams), d_pose, pose_stride, d_corr, d_d2,
                                                           d_g2, d_count))

    def register_guided_pairs_features_device(self, d_pts: int, d_feat: int, set_off, pairs, mparams: ScMatchParams,
                                              gparams: ScGuideParams, d_pose: int, pose_stride: int, params: ScParams, d_res: int,
                                              d_corr: int, d_d2: int, d_g2: int | None, d_count: int, d_mask: int):
        """sc_register_guided_pairs_features_device: match_guided_pairs_device, then the registration on the slots.  d_pose may be
        d_res; returns without waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_register_guided_pairs_features_device(
            self._h, d_pts, d_feat, _p(set_off, C.c_uint32), ns, _p(pairs, C.c_uint32), npairs, C.byref(mparams), C.byref(gparams), d_pose,
            pose_stride, C.byref(params), d_res, d_corr, d_d2, d_g2, d_count, d_mask))

    # ---- the fp64 information matrix of a batch's poses (include/saccot.h, sc_pose_info_batch) -------------------------
    def pose_info_batch_raw(self, src, tgt, offset, params: ScParams, pose):
        """sc_pose_info_batch on packed arrays: src / tgt / offset as register_batch_raw's; pose (B,) records of any dtype whose
        items start with float Rt[12] and int32 status — BATCH_RESULT_DTYPE, POLISH_BATCH_RESULT_DTYPE, a plane of
        register_instances_batch_raw's records — read only -> records (B,) of POSE_INFO_RESULT_DTYPE."""
        src, tgt = _f32c(src), _f32c(tgt)
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        pose = np.ascontiguousarray(pose)
        nb = max(len(offset) - 1, 0)
        if pose.ndim != 1 or len(pose) != nb:
            raise ValueError("pose_info_batch_raw: one pose record per problem")
        info = np.zeros(max(nb, 1), POSE_INFO_RESULT_DTYPE)
        self._frame_n = 0
        self._check(self._lib.sc_pose_info_batch(self._h, _p(src, C.c_float), _p(tgt, C.c_float), _p(offset, C.c_uint32), nb,
                                                 C.byref(params), pose.ctypes.data_as(C.c_void_p), pose.dtype.itemsize,
                                                 info.ctypes.data_as(C.c_void_p)))
        return info[:nb]

    def pose_info_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, d_pose: int, pose_stride: int, d_info: int):
        """sc_pose_info_batch_device: points, pose records (pose_stride bytes each, read only) and output records (320 bytes each) in
        HBM, offset a HOST array (B + 1,) uint32; enqueues on the context's stream and returns without waiting."""
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_pose_info_batch_device(self._h, d_src, d_tgt, _p(offset, C.c_uint32), max(len(offset) - 1, 0),
                                                        C.byref(params), d_pose, pose_stride, d_info))

    def pose_info_batch_slots_device(self, d_src_pts: int, src_off, d_tgt_pts: int, tgt_off, knn: int, params: ScParams, d_corr: int,
                                     d_count: int, d_pose: int, pose_stride: int, d_info: int):
        """sc_pose_info_batch_slots_device: behind register_batch_features_device — its points, offsets, d_corr and d_count; d_pose B
        records of pose_stride bytes, d_info B records of 320 bytes; enqueues on the context's stream and returns without waiting."""
        src_off, tgt_off = np.ascontiguousarray(src_off, dtype=np.uint32), np.ascontiguousarray(tgt_off, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_pose_info_batch_slots_device(self._h, d_src_pts, _p(src_off, C.c_uint32), d_tgt_pts, _p(tgt_off, C.c_uint32),
                                                              max(len(src_off) - 1, 0), knn, C.byref(params), d_corr, d_count, d_pose,
                                                              pose_stride, d_info))

    def pose_info_pairs_slots_device(self, d_pts: int, set_off, pairs, knn: int, params: ScParams, d_corr: int, d_count: int, d_pose: int,
                                     pose_stride: int, d_info: int):
        """sc_pose_info_pairs_slots_device: behind register_pairs_features_device — its points, set_off, pairs, d_corr and d_count;
        d_pose P records of pose_stride bytes, d_info P records of 320 bytes; enqueues on the context's stream and returns without
        waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_pose_info_pairs_slots_device(self._h, d_pts, _p(set_off, C.c_uint32), ns, _p(pairs, C.c_uint32), npairs, knn,
                                                              C.byref(params), d_corr, d_count, d_pose, pose_stride, d_info))

    # ---- the same on the frame the last register* call left (include/saccot.h, sc_pose_info_frame) ---------------------------
    def pose_info_frame(self, pose, iparams: ScPoseInfoParams | None = None, sel=None, **kw):
        """sc_pose_info_frame: pose (K,) records of any dtype whose items start with float Rt[12] (and, with SC_POSE_INFO_STATUS, an
        int32 status behind it) — or a float32 array (K, 12) / (12,) —; sel None, (n,) uint8 (SEL_MASK) or (n,) int32 (SEL_LABEL), read
        only -> records (K,) of POSE_INFO_RESULT_DTYPE.  The frame stays.  kw: sel_mode, label0, flags (make_pose_info_params)."""
        q = iparams or make_pose_info_params(**kw)
        pose = np.ascontiguousarray(pose)
        if pose.dtype.fields is None:
            pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(-1, 12)
            stride = 48
        else:
            pose = pose.reshape(-1)
            stride = pose.dtype.itemsize
        k = len(pose)
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.int32 if q.sel_mode == SC_POSE_INFO_SEL_LABEL else np.uint8)
            if sel.size != self._frame_n:
                raise ValueError("pose_info_frame: sel holds one entry per correspondence of the frame")
        info = np.zeros(max(k, 1), POSE_INFO_RESULT_DTYPE)
        self._check(self._lib.sc_pose_info_frame(self._h, C.byref(q), pose.ctypes.data_as(C.c_void_p), stride, k,
                                                 None if sel is None else sel.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)))
        return info[:k]

    def pose_info_frame_device(self, iparams: ScPoseInfoParams, d_pose: int, pose_stride: int, n_poses: int, d_sel: int, d_info: int):
        """sc_pose_info_frame_device: pose records (pose_stride bytes each, read only), the selection (0: none) and the output
        records (320 bytes each) in HBM; enqueues on the context's stream and returns without waiting.  The frame stays."""
        self._check(self._lib.sc_pose_info_frame_device(self._h, C.byref(iparams), d_pose, pose_stride, n_poses, d_sel or None, d_info))

    # ---- caller-supplied poses refitted on that frame (include/saccot.h, sc_polish_poses) -------------------------------------
    def polish_poses(self, pose, pparams: ScPolishPosesParams | None = None, sel=None, want_mask: bool = True, **kw):
        """sc_polish_poses: pose (K,) records of any dtype whose items start with float Rt[12] (and, with SC_POLISH_POSES_STATUS, an
        int32 status behind it) — or a float32 array (K, 12) / (12,) —; sel None, (n,) uint8 (SEL_MASK) or (n,) int32 (SEL_LABEL,
        SEL_ALIVE), read only -> (records (K,) of POLISH_BATCH_RESULT_DTYPE, masks (K, n) uint8 or None).  The frame stays.
        kw: max_iter, sel_mode, label0, flags (make_polish_poses_params)."""
        q = pparams or make_polish_poses_params(**kw)
        pose = np.ascontiguousarray(pose)
        if pose.dtype.fields is None:
            pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(-1, 12)
            stride = 48
        else:
            pose = pose.reshape(-1)
            stride = pose.dtype.itemsize
        k = len(pose)
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.uint8 if q.sel_mode == SC_POLISH_POSES_SEL_MASK else np.int32)
            if sel.size != self._frame_n:
                raise ValueError("polish_poses: sel holds one entry per correspondence of the frame")
        pol = np.zeros(max(k, 1), POLISH_BATCH_RESULT_DTYPE)
        mask = np.zeros((max(k, 1), max(self._frame_n, 1)), np.uint8) if want_mask else None
        self._check(self._lib.sc_polish_poses(self._h, C.byref(q), pose.ctypes.data_as(C.c_void_p), stride, k,
                                              None if sel is None else sel.ctypes.data_as(C.c_void_p), pol.ctypes.data_as(C.c_void_p),
                                              None if mask is None else mask.ctypes.data_as(C.c_void_p)))
        return pol[:k], (None if mask is None else mask[:k, :self._frame_n])

    def polish_poses_device(self, pparams: ScPolishPosesParams, d_pose: int, pose_stride: int, n_poses: int, d_sel: int, d_pol: int,
                            d_mask: int = 0):
        """sc_polish_poses_device: pose records (pose_stride bytes each, read only), the selection (0: none), the output records (64
        bytes each) and the masks (n_poses x n bytes; 0: none) in HBM; enqueues on the context's stream and returns without waiting.
        The frame stays."""
        self._check(self._lib.sc_polish_poses_device(self._h, C.byref(pparams), d_pose, pose_stride, n_poses, d_sel or None, d_pol,
                                                     d_mask or None))

    # ---- correspondences labelled by the pose that fits best (include/saccot.h, sc_assign_poses) ---------------------------------
    def assign_poses_frame(self, pose, aparams: ScAssignParams | None = None, sel=None, want_d2: bool = True, **kw):
        """sc_assign_poses_frame: pose (K,) records of any dtype whose items start with float Rt[12] (and, with SC_ASSIGN_STATUS, an
        int32 status behind it) — or a float32 array (K, 12) / (12,) —; sel None or (n,) uint8 (SC_ASSIGN_SEL_MASK), read only ->
        (label (n,) int32, d2 (n,) float32 or None, records (K,) of ASSIGN_RESULT_DTYPE).  The frame stays.
        kw: mode, sel_mode, flags (make_assign_params)."""
        q = aparams or make_assign_params(**kw)
        pose = np.ascontiguousarray(pose)
        if pose.dtype.fields is None:
            pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(-1, 12)
            stride = 48
        else:
            pose = pose.reshape(-1)
            stride = pose.dtype.itemsize
        k, n = len(pose), self._frame_n
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.uint8)
            if sel.size != n:
                raise ValueError("assign_poses_frame: sel holds one entry per correspondence of the frame")
        label = np.zeros(max(n, 1), np.int32)
        d2 = np.zeros(max(n, 1), np.float32) if want_d2 else None
        asg = np.zeros(max(k, 1), ASSIGN_RESULT_DTYPE)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._check(self._lib.sc_assign_poses_frame(self._h, C.byref(q), vp(pose), stride, k, vp(sel), vp(label), vp(d2), vp(asg)))
        return label[:n], (None if d2 is None else d2[:n]), asg[:k]

    def assign_poses_frame_device(self, aparams: ScAssignParams, d_pose: int, pose_stride: int, n_poses: int, d_sel: int, d_label: int,
                                  d_d2: int, d_asg: int):
        """sc_assign_poses_frame_device: pose records (pose_stride bytes each, read only), the selection (0: none), the labels (n
        int32), the residuals (n floats; 0: none) and the records (32 bytes each) in HBM; enqueues on the context's stream and returns
        without waiting.  The frame stays."""
        self._check(self._lib.sc_assign_poses_frame_device(self._h, C.byref(aparams), d_pose, pose_stride, n_poses, d_sel or None, d_label,
                                                           d_d2 or None, d_asg))

    def assign_poses_batch(self, src, tgt, offset, params: ScParams, pose, aparams: ScAssignParams | None = None, **kw):
        """sc_assign_poses_batch on packed arrays: src / tgt / offset as register_batch_raw's; pose (K, B) records, motion-major, of any
        dtype whose items start with float Rt[12] and int32 status — register_instances_batch_raw's records — read only ->
        (label (total,) int32, records (K, B) of ASSIGN_RESULT_DTYPE).  kw: mode, flags (make_assign_params)."""
        q = aparams or make_assign_params(**kw)
        src, tgt = _f32c(src), _f32c(tgt)
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        pose = np.ascontiguousarray(pose)
        nb = max(len(offset) - 1, 0)
        total = int(offset[-1]) if len(offset) else 0
        if pose.ndim != 2 or pose.shape[1] != nb:
            raise ValueError("assign_poses_batch: pose holds (n_poses, n_problems) records")
        k = pose.shape[0]
        label = np.zeros(max(total, 1), np.int32)
        asg = np.zeros((max(k, 1), max(nb, 1)), ASSIGN_RESULT_DTYPE)
        self._frame_n = 0
        self._check(self._lib.sc_assign_poses_batch(self._h, _p(src, C.c_float), _p(tgt, C.c_float), _p(offset, C.c_uint32), nb,
                                                    C.byref(params), C.byref(q), pose.ctypes.data_as(C.c_void_p), pose.dtype.itemsize, k,
                                                    label.ctypes.data_as(C.c_void_p), asg.ctypes.data_as(C.c_void_p)))
        return label[:total], asg[:k, :nb]

    def assign_poses_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, aparams: ScAssignParams, d_pose: int,
                                  pose_stride: int, n_poses: int, d_label: int, d_asg: int):
        """sc_assign_poses_batch_device: points, pose records (n_poses x B of pose_stride bytes, motion-major, read only), labels
        (total int32) and records (n_poses x B of 32 bytes, motion-major) in HBM, offset a HOST array (B + 1,) uint32; enqueues on the
        context's stream and returns without waiting."""
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_assign_poses_batch_device(self._h, d_src, d_tgt, _p(offset, C.c_uint32), max(len(offset) - 1, 0),
                                                           C.byref(params), C.byref(aparams), d_pose, pose_stride, n_poses, d_label, d_asg))

    # ---- poses relabelled and refitted until stable (include/saccot.h, sc_settle_poses) -----------------------------------------
    def settle_poses_frame(self, pose, sparams: ScSettleParams | None = None, sel=None, want_d2: bool = True, want_rounds: bool = True,
                           **kw):
        """sc_settle_poses_frame: pose (K,) records of any dtype whose items start with float Rt[12] (and, with SC_SETTLE_STATUS, an
        int32 status behind it) — or a float32 array (K, 12) / (12,) —; sel None or (n,) uint8 (SC_ASSIGN_SEL_MASK), read only ->
        (records (K,) of POLISH_BATCH_RESULT_DTYPE, label (n,) int32, d2 (n,) float32 or None, rounds (2,) uint32 — counted rounds,
        stop — or None).  The frame stays.  kw: max_iter, sel_mode, flags (make_settle_params)."""
        q = sparams or make_settle_params(**kw)
        pose = np.ascontiguousarray(pose)
        if pose.dtype.fields is None:
            pose = np.ascontiguousarray(pose, dtype=np.float32).reshape(-1, 12)
            stride = 48
        else:
            pose = pose.reshape(-1)
            stride = pose.dtype.itemsize
        k, n = len(pose), self._frame_n
        if sel is not None:
            sel = np.ascontiguousarray(sel, dtype=np.uint8)
            if sel.size != n:
                raise ValueError("settle_poses_frame: sel holds one entry per correspondence of the frame")
        pol = np.zeros(max(k, 1), POLISH_BATCH_RESULT_DTYPE)
        label = np.zeros(max(n, 1), np.int32)
        d2 = np.zeros(max(n, 1), np.float32) if want_d2 else None
        rounds = np.zeros(2, np.uint32) if want_rounds else None
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._check(self._lib.sc_settle_poses_frame(self._h, C.byref(q), vp(pose), stride, k, vp(sel), vp(pol), vp(label), vp(d2),
                                                    vp(rounds)))
        return pol[:k], label[:n], (None if d2 is None else d2[:n]), rounds

    def settle_poses_frame_device(self, sparams: ScSettleParams, d_pose: int, pose_stride: int, n_poses: int, d_sel: int, d_pol: int,
                                  d_label: int, d_d2: int = 0, d_rounds: int = 0):
        """sc_settle_poses_frame_device: pose records (pose_stride bytes each, read only), the selection (0: none), the output
        records (64 bytes each), the labels (n int32), the residuals (n floats; 0: none) and the two words (0: none) in HBM;
        enqueues ONE launch on the context's stream and returns without waiting.  The frame stays."""
        self._check(self._lib.sc_settle_poses_frame_device(self._h, C.byref(sparams), d_pose, pose_stride, n_poses, d_sel or None, d_pol,
                                                           d_label, d_d2 or None, d_rounds or None))

    def settle_poses_batch(self, src, tgt, offset, params: ScParams, pose, sparams: ScSettleParams | None = None, **kw):
        """sc_settle_poses_batch on packed arrays: src / tgt / offset as register_batch_raw's; pose (K, B) records, motion-major, of any
        dtype whose items start with float Rt[12] and int32 status — register_instances_batch_raw's records — read only ->
        (records (K, B) of POLISH_BATCH_RESULT_DTYPE, label (total,) int32, rounds (B, 2) uint32).  kw: max_iter, flags
        (make_settle_params)."""
        q = sparams or make_settle_params(**kw)
        src, tgt = _f32c(src), _f32c(tgt)
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        pose = np.ascontiguousarray(pose)
        nb = max(len(offset) - 1, 0)
        total = int(offset[-1]) if len(offset) else 0
        if pose.ndim != 2 or pose.shape[1] != nb:
            raise ValueError("settle_poses_batch: pose holds (n_poses, n_problems) records")
        k = pose.shape[0]
        pol = np.zeros((max(k, 1), max(nb, 1)), POLISH_BATCH_RESULT_DTYPE)
        label = np.zeros(max(total, 1), np.int32)
        rounds = np.zeros((max(nb, 1), 2), np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_settle_poses_batch(self._h, _p(src, C.c_float), _p(tgt, C.c_float), _p(offset, C.c_uint32), nb,
                                                    C.byref(params), C.byref(q), pose.ctypes.data_as(C.c_void_p), pose.dtype.itemsize, k,
                                                    pol.ctypes.data_as(C.c_void_p), label.ctypes.data_as(C.c_void_p),
                                                    rounds.ctypes.data_as(C.c_void_p)))
        return pol[:k, :nb], label[:total], rounds[:nb]

    def settle_poses_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, sparams: ScSettleParams, d_pose: int,
                                  pose_stride: int, n_poses: int, d_pol: int, d_label: int, d_rounds: int = 0):
        """sc_settle_poses_batch_device: points, pose records (n_poses x B of pose_stride bytes, motion-major, read only), output
        records (n_poses x B of 64 bytes, motion-major), labels (total int32) and the word pairs (2 x B; 0: none) in HBM, offset a
        HOST array (B + 1,) uint32; enqueues on the context's stream and returns without waiting."""
        offset = np.ascontiguousarray(offset, dtype=np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_settle_poses_batch_device(self._h, d_src, d_tgt, _p(offset, C.c_uint32), max(len(offset) - 1, 0),
                                                           C.byref(params), C.byref(sparams), d_pose, pose_stride, n_poses, d_pol, d_label,
                                                           d_rounds or None))

    def hypothesize_device(self, d_src: int, d_tgt: int, n: int, params: ScParams, d_key: int):
        st = ScStats(C.sizeof(ScStats))
        self._check(self._lib.sc_hypothesize_device(self._h, d_src, d_tgt, n, C.byref(params), d_key, C.byref(st)))
        return st.as_dict()

    def hypothesize_begin_device(self, d_src: int, d_tgt: int, n: int, params: ScParams, d_hist: int):
        """Phase 1, first half (include/saccot.h): A, edges, and this rank's share of the pruning sample into
        d_hist (SC_HIST_WORDS u32 on the device, zeroed by the call).  Sum d_hist over the ranks
        (shard.allreduce_hist), then call hypothesize_end_device."""
        st = ScStats(C.sizeof(ScStats))
        self._check(self._lib.sc_hypothesize_begin_device(self._h, d_src, d_tgt, n, C.byref(params), d_hist, C.byref(st)))
        return st.as_dict()

    def hypothesize_end_device(self, d_hist: int, d_key: int):
        st = ScStats(C.sizeof(ScStats))
        self._check(self._lib.sc_hypothesize_end_device(self._h, d_hist, d_key, C.byref(st)))
        return st.as_dict()

    def finalize_device(self, d_key: int, d_Rt: int, d_mask: int):
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_finalize_device(self._h, d_key, d_Rt, d_mask, C.byref(st)), allow=(SC_ENOHYP,))
        return rc, st.as_dict()

    def finalize_gathered_device(self, d_keys: int, n_pairs: int, d_Rt: int, d_mask: int):
        """Phase 2 on n_pairs all-gathered key pairs (shard.allgather_best): the reduction runs in the kernel."""
        st = ScStats(C.sizeof(ScStats))
        rc = self._check(self._lib.sc_finalize_gathered_device(self._h, d_keys, n_pairs, d_Rt, d_mask, C.byref(st)),
                         allow=(SC_ENOHYP, SC_ERETRY, SC_EBOUND))  # SC_ERETRY (sharded A + B): repeat with shard_cand_level + 1; SC_EBOUND: repeat without SC_FLAG_EST_BOUND
        return rc, st.as_dict()

    def finalize_gathered_device_async(self, d_keys: int, n_pairs: int, d_Rt: int, d_mask: int):
        """sc_finalize_gathered_device_async: the finalize kernel is enqueued; `wait()` delivers status and statistics."""
        self._check(self._lib.sc_finalize_gathered_device_async(self._h, d_keys, n_pairs, d_Rt, d_mask))

    # ---- stages A and B sharded too (include/saccot.h "phase API") ----------------------------
    def shard_compat_device(self, d_src: int, d_tgt: int, n: int, params: ScParams, d_bits_all: int):
        """Phase 1: this rank's row block of the adjacency bit rows into the shared d_bits_all -> all-gather in place."""
        self._check(self._lib.sc_shard_compat_device(self._h, d_src, d_tgt, n, C.byref(params), d_bits_all))

    def shard_edges_device(self, d_hist: int):
        """Phase 2 (bit rows gathered): degrees, edge list, this rank's share of the pruning sample -> all-reduce SUM."""
        self._check(self._lib.sc_shard_edges_device(self._h, d_hist))

    def shard_select_device(self, d_hist: int, d_cand_mine: int):
        """Phase 3: this rank's own top-T triangles (its contiguous row range) into its candidate blob -> all-gather."""
        self._check(self._lib.sc_shard_select_device(self._h, d_hist, d_cand_mine))

    def shard_score_device(self, d_cand_all: int, d_key: int):
        """Phase 4: merge of the gathered blobs, then C1 + C2 on this rank's blocks -> key pair -> all-gather, finalize."""
        st = ScStats(C.sizeof(ScStats))
        self._check(self._lib.sc_shard_score_device(self._h, d_cand_all, d_key, C.byref(st)))
        return st.as_dict()

    # ---- stage hooks -----------------------------------------------------------------------------------------
    def compat(self, src, tgt, params: ScParams, want_S=True):
        src, tgt = _f32c(src), _f32c(tgt)
        n = src.shape[0] if params.layout == SC_AOS else src.shape[1]
        W = (n + 63) // 64
        S = np.empty((n, n), np.float32) if want_S else None
        bits = np.zeros((n, W), np.uint64); deg = np.zeros(n, np.uint32)
        self._check(self._lib.sc_compat_host(self._h, _p(src, C.c_float), _p(tgt, C.c_float), n, C.byref(params),
                                             _p(S, C.c_float), _p(bits, C.c_uint64), _p(deg, C.c_uint32)))
        return S, bits, deg

    def triangles(self, src, tgt, params: ScParams):
        src, tgt = _f32c(src), _f32c(tgt)
        n = src.shape[0] if params.layout == SC_AOS else src.shape[1]
        T = params.max_triangles
        tri = np.zeros((T, 3), np.uint32); key = np.zeros(T, np.uint32)
        t_eff = C.c_uint32(0); total = C.c_uint64(0); edges = C.c_uint64(0)
        self._check(self._lib.sc_triangles_host(self._h, _p(src, C.c_float), _p(tgt, C.c_float), n, C.byref(params),
                                                _p(tri, C.c_uint32), _p(key, C.c_uint32), C.byref(t_eff),
                                                C.byref(total), C.byref(edges)))
        return tri[: t_eff.value].copy(), key[: t_eff.value].copy(), int(total.value), int(edges.value)

    def kabsch(self, src, tgt, params: ScParams, tri):
        src, tgt = _f32c(src), _f32c(tgt)
        n = src.shape[0] if params.layout == SC_AOS else src.shape[1]
        tri = np.ascontiguousarray(tri, dtype=np.uint32)
        Rt = np.zeros((tri.shape[0], 12), np.float32)
        self._check(self._lib.sc_kabsch_host(self._h, _p(src, C.c_float), _p(tgt, C.c_float), n, C.byref(params),
                                             _p(tri, C.c_uint32), tri.shape[0], _p(Rt, C.c_float)))
        return Rt

    def score(self, src, tgt, params: ScParams, Rt):
        src, tgt = _f32c(src), _f32c(tgt)
        n = src.shape[0] if params.layout == SC_AOS else src.shape[1]
        Rt = _f32c(Rt)
        cnt = np.zeros(Rt.shape[0], np.uint32); key = C.c_uint64(0)
        self._check(self._lib.sc_score_host(self._h, _p(src, C.c_float), _p(tgt, C.c_float), n, C.byref(params),
                                            _p(Rt, C.c_float), Rt.shape[0], _p(cnt, C.c_uint32), C.byref(key)))
        return cnt, int(key.value)

    def mask(self, src, tgt, params: ScParams, Rt12):
        src, tgt = _f32c(src), _f32c(tgt)
        n = src.shape[0] if params.layout == SC_AOS else src.shape[1]
        Rt12 = _f32c(Rt12).reshape(12)
        m = np.zeros(n, np.uint8)
        self._check(self._lib.sc_mask_host(self._h, _p(src, C.c_float), _p(tgt, C.c_float), n, C.byref(params),
                                           _p(Rt12, C.c_float), _p(m, C.c_uint8)))
        return m


class MultiRegistrar:
    """sc_multi (include/saccot.h): one process, several GPUs, RCCL inside the library.  `devices`: distinct device
    ids; `loopback_ranks` > 0 instead runs that many ranks on devices[0] with device copies in place of RCCL (test
    hook: the whole orchestration on a one-GPU box)."""

    def __init__(self, devices=(0,), loopback_ranks: int = 0):
        self._lib = load_library()
        h = C.c_void_p()
        if loopback_ranks:
            rc = self._lib.sc_create_multi_loopback(int(devices[0]), loopback_ranks, C.byref(h))
        else:
            ids = (C.c_int * len(devices))(*devices)
            rc = self._lib.sc_create_multi(ids, len(devices), C.byref(h))
        if rc != SC_OK:
            raise SacCotError(rc, "sc_create_multi failed: " + self._lib.sc_strerror(rc).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sc_destroy_multi(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def register(self, src, tgt, params: ScParams | None = None, **kw):
        p = params or make_params(**kw)
        src, tgt = _f32c(src), _f32c(tgt)
        n = src.shape[0] if p.layout == SC_AOS else src.shape[1]
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32); mask = np.zeros(n, np.uint8)
        st = ScStats(C.sizeof(ScStats))
        rc = self._lib.sc_register_multi(self._h, _p(src, C.c_float), _p(tgt, C.c_float), n, C.byref(p),
                                         _p(R, C.c_float), _p(t, C.c_float), _p(mask, C.c_uint8), C.byref(st))
        if rc not in (SC_OK, SC_ENOHYP):
            raise SacCotError(rc, self._lib.sc_strerror(rc).decode() + " — " + self._lib.sc_multi_last_error(self._h).decode())
        return dict(status=rc, R=R.reshape(3, 3), t=t, mask=mask, stats=st.as_dict())


def register(src, tgt, device: int = 0, **kw):
    """One-shot convenience: create a context, run the whole path, destroy the context."""
    r = Registrar(device)
    try:
        return r.register(src, tgt, **kw)
    finally:
        r.close()
