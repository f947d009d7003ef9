"""Host-side mirror of the C ABI in include/saccot.h (ctypes over libsaccot.so).

The reference has no operator/plugin interface to mirror, so the names follow SURVEY.md §8(b): `register()` is the
drop-in entry point — correspondences in, (R, t, inlier mask) out — and the `compat` / `triangles` / `kabsch` /
`score` / `mask` methods are the per-stage hooks the parity tests drive.  Everything computes on the GPU through
libsaccot.so; if the library or a HIP device is missing this module raises — there is no CPU fallback (the CPU
restatement lives in oracle/ and is test-only).

A new entry point of the header is added in two places: its prototype in `_PROTOTYPES` (`EXPORTS` and `load_library()`
follow from the table; tests/test_api_mirror.py holds it against the header) and its method, which reads "prepare, one
library call, slice" on the helpers below `load_library()`: `_p` / `_vp` (pointers), `_u32c` / `_total` (host offset
arrays), `_n_points`, `_frame_sel`, `_frame_out` / `_frame_cut` and `_slot_out` / `_slot_cut` (the matchers' outputs),
`_sized` (size-first structures), `_motion_out` / `_result` (one motion and its dict) and `Registrar._pose_records`.
A record the library writes is declared once, as a `ctypes.Structure`; its numpy dtype is made from that.  The device
forms on the benchmark's timed path (register_device[_async], wait, hypothesize_*, finalize_*, shard_*, set_stream)
spell their one call out and go through no helper.
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


POLISH_CAND_DTYPE = np.dtype(ScPolishCand)  # sc_polish_cand as a numpy record


class ScBatchResult(C.Structure):
    """Mirror of `sc_batch_result` (include/saccot.h), 80 bytes: one problem's record of sc_register_batch."""
    _fields_ = [("Rt", C.c_float * 12), ("status", C.c_int32), ("n", C.c_uint32), ("edges", C.c_uint32), ("tri_kept", C.c_uint32),
                ("tri_total", C.c_uint64), ("best_rank", C.c_uint32), ("best_count", C.c_uint32)]


BATCH_RESULT_DTYPE = np.dtype(ScBatchResult)  # sc_batch_result as a numpy record
SC_BATCH_MAX_N = 512


class ScPolishBatchResult(C.Structure):
    """Mirror of `sc_polish_batch_result` (include/saccot.h), 64 bytes: one problem's record of sc_polish_batch."""
    _fields_ = [("Rt", C.c_float * 12), ("status", C.c_int32), ("score0", C.c_uint32), ("score", C.c_uint32), ("iters", C.c_uint16),
                ("stop", C.c_uint16)]


POLISH_BATCH_RESULT_DTYPE = np.dtype(ScPolishBatchResult)  # sc_polish_batch_result as a numpy record
SC_POLISH_STOP_FIXED, SC_POLISH_STOP_DECLINED, SC_POLISH_STOP_MAX_ITER = 0, 1, 2


class ScPoseInfoResult(C.Structure):
    """Mirror of `sc_pose_info_result` (include/saccot.h), 320 bytes: one problem's record of sc_pose_info_batch."""
    _fields_ = [("info", C.c_double * 36), ("sse", C.c_double), ("status", C.c_int32), ("inliers", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


POSE_INFO_RESULT_DTYPE = np.dtype(ScPoseInfoResult)  # sc_pose_info_result as a numpy record


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


ASSIGN_RESULT_DTYPE = np.dtype(ScAssignResult)  # sc_assign_result as a numpy record
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


class ScMergeParams(C.Structure):
    """Mirror of `sc_merge_params` (include/saccot.h), 32 bytes: the measure (SC_MERGE_OVER_*), the fraction num / den (1 <= num <= den
    <= 65536), the inlier count below which a valid pose is dropped, which correspondences take part (SC_ASSIGN_SEL_*),
    SC_MERGE_STATUS | SC_MERGE_COMPACT or 0."""
    _fields_ = [("size", C.c_uint32), ("measure", C.c_uint32), ("num", C.c_uint32), ("den", C.c_uint32), ("min_count", C.c_uint32),
                ("sel_mode", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 1)]


class ScMergePose(C.Structure):
    """Mirror of `sc_merge_pose` (include/saccot.h), 64 bytes: one pose's record of sc_merge_poses — itself a pose record, the status
    at byte 48."""
    _fields_ = [("Rt", C.c_float * 12), ("status", C.c_int32), ("index", C.c_int32), ("count", C.c_uint32), ("score", C.c_uint32)]


MERGE_POSE_DTYPE = np.dtype(ScMergePose)  # sc_merge_pose as a numpy record
SC_MERGE_MAX_POSES, SC_MERGE_BATCH_MAX_POSES = 1024, 64
SC_MERGE_OVER_MIN, SC_MERGE_OVER_UNION = 0, 1
SC_MERGE_STATUS, SC_MERGE_COMPACT = 1, 2


class ScCycleParams(C.Structure):
    """Mirror of `sc_cycle_params` (include/saccot.h), 32 bytes: the consistent loops an unprotected pair must close, the rounds at
    most (1 .. 64), SC_CYCLES_STATUS or 0, the rotation tolerance (radians, in [0, pi]) and the translation tolerance (>= 0)."""
    _fields_ = [("size", C.c_uint32), ("min_ok", C.c_uint32), ("max_rounds", C.c_uint32), ("flags", C.c_uint32), ("rot_tol", C.c_float),
                ("trans_tol", C.c_float), ("reserved", C.c_uint32 * 2)]


class ScCycleResult(C.Structure):
    """Mirror of `sc_cycle_result` (include/saccot.h), 48 bytes: one pair's record of sc_pairs_cycles."""
    _fields_ = [("status", C.c_int32), ("cycles", C.c_uint32), ("ok", C.c_uint32), ("ok_alive", C.c_uint32), ("alive", C.c_uint32),
                ("dropped_round", C.c_uint32), ("min_trace", C.c_double), ("max_e2", C.c_double), ("reserved", C.c_uint32 * 2)]


class ScCycleSummary(C.Structure):
    """Mirror of `sc_cycle_summary` (include/saccot.h), 32 bytes: the rounds run, whether the list is stable, the pairs alive at the
    end and at the start, the triangles of the start and the consistent ones among them."""
    _fields_ = [("rounds", C.c_uint32), ("stable", C.c_uint32), ("alive", C.c_uint32), ("edges", C.c_uint32), ("triangles", C.c_uint64),
                ("consistent", C.c_uint64)]


CYCLE_RESULT_DTYPE = np.dtype(ScCycleResult)    # sc_cycle_result as a numpy record
CYCLE_SUMMARY_DTYPE = np.dtype(ScCycleSummary)  # sc_cycle_summary as a numpy record
SC_CYCLES_STATUS, SC_CYCLES_MAX_PAIRS, SC_CYCLES_MAX_DEGREE = 1, 1 << 22, 65535
class ScSyncParams(C.Structure):
    """Mirror of `sc_sync_params` (include/saccot.h), 32 bytes: the anchor set, the rounds at most (1 .. 256), SC_SYNC_STATUS or 0, the
    rotation tolerance (radians, in [0, pi]) and the translation tolerance (>= 0) of the stopping rule."""
    _fields_ = [("size", C.c_uint32), ("anchor", C.c_uint32), ("max_rounds", C.c_uint32), ("flags", C.c_uint32), ("rot_tol", C.c_float),
                ("trans_tol", C.c_float), ("reserved", C.c_uint32 * 2)]


class ScSyncSet(C.Structure):
    """Mirror of `sc_sync_set` (include/saccot.h), 160 bytes: one set's record of sc_pairs_sync — a legal pose record with a status
    (Rt, status) in front of the tallies and the fp64 pose."""
    _fields_ = [("Rt", C.c_float * 12), ("status", C.c_int32), ("known_round", C.c_uint32), ("used", C.c_uint32), ("degenerate", C.c_uint32),
                ("X", C.c_double * 12)]


class ScSyncPair(C.Structure):
    """Mirror of `sc_sync_pair` (include/saccot.h), 32 bytes: one pair's status, whether it was used, and its residual."""
    _fields_ = [("status", C.c_int32), ("used", C.c_uint32), ("r2", C.c_double), ("e2", C.c_double), ("reserved", C.c_uint32 * 2)]


class ScSyncSummary(C.Structure):
    """Mirror of `sc_sync_summary` (include/saccot.h), 32 bytes: the rounds run, whether they converged, the sets known and the pairs
    used at the end, the sets the last round changed."""
    _fields_ = [("rounds", C.c_uint32), ("converged", C.c_uint32), ("known", C.c_uint32), ("used", C.c_uint32), ("changed_last", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


SYNC_SET_DTYPE = np.dtype(ScSyncSet)          # sc_sync_set as a numpy record
SYNC_PAIR_DTYPE = np.dtype(ScSyncPair)        # sc_sync_pair as a numpy record
SYNC_SUMMARY_DTYPE = np.dtype(ScSyncSummary)  # sc_sync_summary as a numpy record
SC_SYNC_STATUS = 1
class ScSolveParams(C.Structure):
    """Mirror of `sc_solve_params` (include/saccot.h), 32 bytes: the anchor set, the Gauss-Newton steps at most (1 .. 32), the iterations
    of a step's solve at most (1 .. 256; their product at most 2048), SC_SOLVE_STATUS | SC_SOLVE_INFO_STATUS or 0, the two tolerances
    of the stopping rule and the relative tolerance of the inner solve (in [0, 1))."""
    _fields_ = [("size", C.c_uint32), ("anchor", C.c_uint32), ("max_outer", C.c_uint32), ("max_inner", C.c_uint32), ("flags", C.c_uint32),
                ("rot_tol", C.c_float), ("trans_tol", C.c_float), ("cg_tol", C.c_float)]


class ScSolveSet(C.Structure):
    """Mirror of `sc_solve_set` (include/saccot.h), 160 bytes, the layout of sc_sync_set: a legal pose record with a status (Rt,
    status) in front of the set's state, its tally and the fp64 pose."""
    _fields_ = [("Rt", C.c_float * 12), ("status", C.c_int32), ("state", C.c_uint32), ("degenerate", C.c_uint32), ("reserved", C.c_uint32),
                ("X", C.c_double * 12)]


class ScSolvePair(C.Structure):
    """Mirror of `sc_solve_pair` (include/saccot.h), 48 bytes: one pair's status, whether it was used, its cost and the two parts of
    its error at the result."""
    _fields_ = [("status", C.c_int32), ("used", C.c_uint32), ("cost", C.c_double), ("w2", C.c_double), ("v2", C.c_double), ("reserved", C.c_uint32 * 4)]


class ScSolveSummary(C.Structure):
    """Mirror of `sc_solve_summary` (include/saccot.h), 64 bytes: the steps kept, why the call stopped, the inner iterations, the free
    sets and used pairs, the sets held in the last step, the cost at the start and at the result, rz_0 of the last step."""
    _fields_ = [("outer", C.c_uint32), ("stop", C.c_uint32), ("inner_total", C.c_uint32), ("inner_last", C.c_uint32), ("free_sets", C.c_uint32),
                ("used_pairs", C.c_uint32), ("held_last", C.c_uint32), ("reserved", C.c_uint32), ("cost0", C.c_double), ("cost", C.c_double),
                ("rz0", C.c_double), ("reserved2", C.c_double)]


SOLVE_SET_DTYPE = np.dtype(ScSolveSet)          # sc_solve_set as a numpy record
SOLVE_PAIR_DTYPE = np.dtype(ScSolvePair)        # sc_solve_pair as a numpy record
SOLVE_SUMMARY_DTYPE = np.dtype(ScSolveSummary)  # sc_solve_summary as a numpy record
SC_SOLVE_STATUS, SC_SOLVE_INFO_STATUS = 1, 2
SC_SOLVE_FREE, SC_SOLVE_ANCHOR, SC_SOLVE_UNKNOWN, SC_SOLVE_ISOLATED = 0, 1, 2, 3
SC_SOLVE_STOP_CONVERGED, SC_SOLVE_STOP_ROSE, SC_SOLVE_STOP_MAX_OUTER = 1, 2, 3
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


# ---- the prototypes of include/saccot.h and include/saccot_debug.h, once: name -> argtypes, or (argtypes, restype) where the
# function does not return int.  A new export gets its line here and nowhere else. --------------------------------------------
_INT, _I64, _U32, _VP = C.c_int, C.c_int64, C.c_uint32, C.c_void_p
_F32P, _U8P, _I32P, _U32P, _U64P = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_int32, C.c_uint32, C.c_uint64))
_PP, _SP, _QP, _MP, _GP = (C.POINTER(t) for t in (ScParams, ScStats, ScPolishParams, ScMatchParams, ScGuideParams))
_IP, _ZP, _AP, _TP, _RP = (C.POINTER(t) for t in (ScPoseInfoParams, ScPolishPosesParams, ScAssignParams, ScSettleParams, ScMergeParams))
_CP = C.POINTER(ScCycleParams)
_YP = C.POINTER(ScSyncParams)
_VSP = C.POINTER(ScSolveParams)
_PROTOTYPES = {
    "sc_version": [],
    "sc_strerror": ([_INT], C.c_char_p),
    "sc_default_params": ([_PP], None),
    "sc_create": [_INT, C.POINTER(_VP)],
    "sc_destroy": ([_VP], None),
    "sc_set_stream": [_VP, _VP],
    "sc_last_error": ([_VP], C.c_char_p),
    "sc_set_debug": [_VP, C.POINTER(ScDebug)],
    "sc_debug_last": [_VP, C.POINTER(ScDebugInfo)],
    "sc_register": [_VP, _F32P, _F32P, _I64, _PP, _F32P, _F32P, _U8P, _SP],
    "sc_register_device": [_VP, _VP, _VP, _I64, _PP, _VP, _VP, _SP],
    "sc_register_device_async": [_VP, _VP, _VP, _I64, _PP, _VP, _VP],
    "sc_wait": [_VP, _SP],
    "sc_register_batch": [_VP, _F32P, _F32P, _U32P, _U32, _PP, _VP, _U8P],
    "sc_register_batch_device": [_VP, _VP, _VP, _U32P, _U32, _PP, _VP, _VP],
    "sc_peel": [_VP, _F32P, _F32P, _U8P, _SP],
    "sc_peel_device": [_VP, _VP, _VP, _SP],
    "sc_register_instances": [_VP, _F32P, _F32P, _I64, _PP, _U32, _U32, _F32P, _U32P, _I32P, _U32P, _SP],
    "sc_polish_default_params": [_QP],
    "sc_polish_device": [_VP, _QP, _VP, _VP, _VP, _VP, _SP],
    "sc_polish": [_VP, _QP, _F32P, _F32P, _U8P, _VP, _U32P, _SP],
    "sc_match_default_params": [_MP],
    "sc_match_device": [_VP, _VP, _I64, _VP, _I64, _MP, _VP, _VP, _VP],
    "sc_match": [_VP, _F32P, _I64, _F32P, _I64, _MP, _I32P, _F32P, _U32P],
    "sc_register_features": [_VP, _F32P, _F32P, _I64, _F32P, _F32P, _I64, _MP, _PP, _F32P, _F32P, _I32P, _F32P, _U32P, _U8P, _SP],
    "sc_guide_default_params": [_GP],
    "sc_match_guided_device": [_VP, _VP, _VP, _I64, _VP, _VP, _I64, _MP, _GP, _VP, _VP, _VP, _VP, _VP],
    "sc_match_guided": [_VP, _F32P, _F32P, _I64, _F32P, _F32P, _I64, _MP, _GP, _F32P, _I32P, _F32P, _F32P, _U32P],
    "sc_register_guided_features": [_VP, _F32P, _F32P, _I64, _F32P, _F32P, _I64, _MP, _GP, _F32P, _PP, _F32P, _F32P, _I32P, _F32P,
                                    _F32P, _U32P, _U8P, _SP],
    "sc_match_batch": [_VP, _F32P, _U32P, _F32P, _U32P, _U32, _MP, _I32P, _F32P, _U32P],
    "sc_match_batch_device": [_VP, _VP, _U32P, _VP, _U32P, _U32, _MP, _VP, _VP, _VP],
    "sc_register_batch_features": [_VP, _F32P, _F32P, _U32P, _F32P, _F32P, _U32P, _U32, _MP, _PP, _VP, _I32P, _F32P, _U32P, _U8P],
    "sc_register_batch_features_device": [_VP, _VP, _VP, _U32P, _VP, _VP, _U32P, _U32, _MP, _PP, _VP, _VP, _VP, _VP, _VP],
    "sc_polish_batch": [_VP, _F32P, _F32P, _U32P, _U32, _PP, _QP, _VP, _VP, _U8P],
    "sc_polish_batch_device": [_VP, _VP, _VP, _U32P, _U32, _PP, _QP, _VP, _VP, _VP],
    "sc_polish_batch_slots_device": [_VP, _VP, _U32P, _VP, _U32P, _U32, _U32, _PP, _QP, _VP, _VP, _VP, _VP, _VP],
    "sc_register_instances_batch": [_VP, _F32P, _F32P, _U32P, _U32, _PP, _U32, _U32, _VP, _I32P, _U32P],
    "sc_register_instances_batch_device": [_VP, _VP, _VP, _U32P, _U32, _PP, _U32, _U32, _VP, _VP, _VP],
    "sc_register_instances_batch_features_device": [_VP, _VP, _VP, _U32P, _VP, _VP, _U32P, _U32, _MP, _PP, _U32, _U32,
                                                    _VP, _VP, _VP, _VP, _VP, _VP],
    "sc_pairs_layout": [_U32P, _U32, _U32P, _U32, _U32, _U32P],
    "sc_match_pairs": [_VP, _F32P, _U32P, _U32, _U32P, _U32, _MP, _I32P, _F32P, _U32P],
    "sc_match_pairs_device": [_VP, _VP, _U32P, _U32, _U32P, _U32, _MP, _VP, _VP, _VP],
    "sc_register_pairs_features": [_VP, _F32P, _F32P, _U32P, _U32, _U32P, _U32, _MP, _PP, _VP, _I32P, _F32P, _U32P, _U8P],
    "sc_register_pairs_features_device": [_VP, _VP, _VP, _U32P, _U32, _U32P, _U32, _MP, _PP, _VP, _VP, _VP, _VP, _VP],
    "sc_polish_pairs_slots_device": [_VP, _VP, _U32P, _U32, _U32P, _U32, _U32, _PP, _QP, _VP, _VP, _VP, _VP, _VP],
    "sc_match_guided_batch": [_VP, _F32P, _F32P, _U32P, _F32P, _F32P, _U32P, _U32, _MP, _GP, _VP, _U32, _I32P, _F32P, _F32P, _U32P],
    "sc_match_guided_batch_device": [_VP, _VP, _VP, _U32P, _VP, _VP, _U32P, _U32, _MP, _GP, _VP, _U32, _VP, _VP, _VP, _VP],
    "sc_register_guided_batch_features_device": [_VP, _VP, _VP, _U32P, _VP, _VP, _U32P, _U32, _MP, _GP, _VP, _U32, _PP, _VP, _VP, _VP,
                                                 _VP, _VP, _VP],
    "sc_match_guided_pairs": [_VP, _F32P, _F32P, _U32P, _U32, _U32P, _U32, _MP, _GP, _VP, _U32, _I32P, _F32P, _F32P, _U32P],
    "sc_match_guided_pairs_device": [_VP, _VP, _VP, _U32P, _U32, _U32P, _U32, _MP, _GP, _VP, _U32, _VP, _VP, _VP, _VP],
    "sc_register_guided_pairs_features_device": [_VP, _VP, _VP, _U32P, _U32, _U32P, _U32, _MP, _GP, _VP, _U32, _PP, _VP, _VP, _VP, _VP,
                                                 _VP, _VP],
    "sc_match_guided_poses": [_VP, _F32P, _F32P, _I64, _F32P, _F32P, _I64, _MP, _GP, _VP, _U32, _U32, _I32P, _F32P, _F32P, _I32P, _U32P],
    "sc_match_guided_poses_device": [_VP, _VP, _VP, _I64, _VP, _VP, _I64, _MP, _GP, _VP, _U32, _U32, _VP, _VP, _VP, _VP, _VP],
    "sc_register_guided_poses_features": [_VP, _F32P, _F32P, _I64, _F32P, _F32P, _I64, _MP, _GP, _VP, _U32, _U32, _PP, _F32P, _F32P,
                                          _I32P, _F32P, _F32P, _I32P, _U32P, _U8P, _SP],
    "sc_pose_info_batch": [_VP, _F32P, _F32P, _U32P, _U32, _PP, _VP, _U32, _VP],
    "sc_pose_info_batch_device": [_VP, _VP, _VP, _U32P, _U32, _PP, _VP, _U32, _VP],
    "sc_pose_info_batch_slots_device": [_VP, _VP, _U32P, _VP, _U32P, _U32, _U32, _PP, _VP, _VP, _VP, _U32, _VP],
    "sc_pose_info_pairs_slots_device": [_VP, _VP, _U32P, _U32, _U32P, _U32, _U32, _PP, _VP, _VP, _VP, _U32, _VP],
    "sc_pose_info_default_params": [_IP],
    "sc_pose_info_frame": [_VP, _IP, _VP, _U32, _U32, _VP, _VP],
    "sc_pose_info_frame_device": [_VP, _IP, _VP, _U32, _U32, _VP, _VP],
    "sc_polish_poses_default_params": [_ZP],
    "sc_polish_poses": [_VP, _ZP, _VP, _U32, _U32, _VP, _VP, _VP],
    "sc_polish_poses_device": [_VP, _ZP, _VP, _U32, _U32, _VP, _VP, _VP],
    "sc_assign_default_params": [_AP],
    "sc_assign_poses_frame": [_VP, _AP, _VP, _U32, _U32, _VP, _VP, _VP, _VP],
    "sc_assign_poses_frame_device": [_VP, _AP, _VP, _U32, _U32, _VP, _VP, _VP, _VP],
    "sc_assign_poses_batch": [_VP, _F32P, _F32P, _U32P, _U32, _PP, _AP, _VP, _U32, _U32, _VP, _VP],
    "sc_assign_poses_batch_device": [_VP, _VP, _VP, _U32P, _U32, _PP, _AP, _VP, _U32, _U32, _VP, _VP],
    "sc_settle_default_params": [_TP],
    "sc_settle_poses_frame": [_VP, _TP, _VP, _U32, _U32, _VP, _VP, _VP, _VP, _VP],
    "sc_settle_poses_frame_device": [_VP, _TP, _VP, _U32, _U32, _VP, _VP, _VP, _VP, _VP],
    "sc_settle_poses_batch": [_VP, _F32P, _F32P, _U32P, _U32, _PP, _TP, _VP, _U32, _U32, _VP, _VP, _VP],
    "sc_settle_poses_batch_device": [_VP, _VP, _VP, _U32P, _U32, _PP, _TP, _VP, _U32, _U32, _VP, _VP, _VP],
    "sc_merge_default_params": [_RP],
    "sc_merge_poses_frame": [_VP, _RP, _VP, _U32, _U32, _VP, _VP, _VP, _VP, _VP],
    "sc_merge_poses_frame_device": [_VP, _RP, _VP, _U32, _U32, _VP, _VP, _VP, _VP, _VP],
    "sc_merge_poses_batch": [_VP, _F32P, _F32P, _U32P, _U32, _PP, _RP, _VP, _U32, _U32, _VP, _VP, _VP],
    "sc_merge_poses_batch_device": [_VP, _VP, _VP, _U32P, _U32, _PP, _RP, _VP, _U32, _U32, _VP, _VP, _VP],
    "sc_cycles_default_params": [_CP],
    "sc_cycles_thresholds": [_CP, C.POINTER(C.c_double)],
    "sc_pairs_cycles": [_VP, _U32, _U32P, _U32, _CP, _VP, _U32, _U8P, _VP, _VP],
    "sc_pairs_cycles_device": [_VP, _U32, _U32P, _U32, _CP, _VP, _U32, _VP, _VP, _VP],
    "sc_sync_default_params": [_YP],
    "sc_sync_thresholds": [_YP, C.POINTER(C.c_double)],
    "sc_pairs_sync": [_VP, _U32, _U32P, _U32, _YP, _VP, _U32, _VP, _U32, _F32P, _VP, _VP, _VP],
    "sc_pairs_sync_device": [_VP, _U32, _U32P, _U32, _YP, _VP, _U32, _VP, _U32, _VP, _VP, _VP, _VP],
    "sc_solve_default_params": [_VSP],
    "sc_solve_thresholds": [_VSP, C.POINTER(C.c_double)],
    "sc_pairs_solve": [_VP, _U32, _U32P, _U32, _VSP, _VP, _U32, _VP, _U32, _VP, _U32, _VP, _U32, _VP, _VP, _VP],
    "sc_pairs_solve_device": [_VP, _U32, _U32P, _U32, _VSP, _VP, _U32, _VP, _U32, _VP, _U32, _VP, _U32, _VP, _VP, _VP],
    "sc_hypothesize_device": [_VP, _VP, _VP, _I64, _PP, _VP, _SP],
    "sc_finalize_device": [_VP, _VP, _VP, _VP, _SP],
    "sc_hypothesize_begin_device": [_VP, _VP, _VP, _I64, _PP, _VP, _SP],
    "sc_hypothesize_end_device": [_VP, _VP, _VP, _SP],
    "sc_finalize_gathered_device": [_VP, _VP, _INT, _VP, _VP, _SP],
    "sc_finalize_gathered_device_async": [_VP, _VP, _INT, _VP, _VP],
    "sc_shard_plan_query": [_PP, _I64, C.POINTER(ScShardPlan)],
    "sc_shard_compat_device": [_VP, _VP, _VP, _I64, _PP, _VP],
    "sc_shard_edges_device": [_VP, _VP],
    "sc_shard_select_device": [_VP, _VP, _VP],
    "sc_shard_score_device": [_VP, _VP, _VP, _SP],
    "sc_create_multi": [C.POINTER(_INT), _INT, C.POINTER(_VP)],
    "sc_create_multi_loopback": [_INT, _INT, C.POINTER(_VP)],
    "sc_destroy_multi": ([_VP], None),
    "sc_multi_last_error": ([_VP], C.c_char_p),
    "sc_register_multi": [_VP, _F32P, _F32P, _I64, _PP, _F32P, _F32P, _U8P, _SP],
    "sc_compat_host": [_VP, _F32P, _F32P, _I64, _PP, _F32P, _U64P, _U32P],
    "sc_triangles_host": [_VP, _F32P, _F32P, _I64, _PP, _U32P, _U32P, _U32P, _U64P, _U64P],
    "sc_kabsch_host": [_VP, _F32P, _F32P, _I64, _PP, _U32P, _U32, _F32P],
    "sc_score_host": [_VP, _F32P, _F32P, _I64, _PP, _F32P, _U32, _U32P, _U64P],
    "sc_mask_host": [_VP, _F32P, _F32P, _I64, _PP, _F32P, _U8P],
}
EXPORTS = list(_PROTOTYPES)

_LIB = None


def load_library() -> C.CDLL:
    """dlopen libsaccot.so and give every export of `_PROTOTYPES` its argtypes and restype.  Raises if it was not built (run
    __graft_entry__.build()).  A new entry point: a line in the table, a method on the class — nothing here."""
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
    for name, proto in _PROTOTYPES.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = proto if isinstance(proto, tuple) else (proto, _INT)
    _LIB = L
    return L


def _sized(cls, *fields, **named):
    """A structure of the ABI whose first field is its own size."""
    return cls(C.sizeof(cls), *fields, **named)


def make_params(sigma=0.1, t_cmp=0.9, tau=0.1, min_len=0.1, max_triangles=50000, rank_mode=SC_RANK_WEIGHT,
                layout=SC_AOS, shard_rank=0, shard_world=1, shard_block=1024, flags=0, max_workspace=0,
                score_mode=0, shard_cand_level=0) -> ScParams:
    return _sized(ScParams, sigma, t_cmp, tau, min_len, max_triangles, rank_mode, layout, shard_rank, shard_world, shard_block,
                  flags, max_workspace, score_mode, shard_cand_level)


def make_match_params(dim: int, knn: int = 1, mutual: bool = False, ratio: float = 0.0, flags: int = 0) -> ScMatchParams:
    """sc_match_params for descriptors of length `dim`: knn 1 .. 4; mutual / ratio (in (0, 1), 0 = off) with knn == 1 only."""
    return _sized(ScMatchParams, dim, knn, flags | (SC_MATCH_MUTUAL if mutual else 0), ratio)


def make_guide_params(gate: float, layout: int = SC_AOS, flags: int = 0) -> ScGuideParams:
    """sc_guide_params: the gate radius (finite, > 0) and the layout of the keypoint arrays of sc_match_guided; flags: 0, or — the
    batch and pairs entries only — SC_GUIDE_POSE_STATUS."""
    return _sized(ScGuideParams, layout, gate, flags)


def make_polish_params(candidates: int = 8, max_iter: int = 16, flags: int = 0) -> ScPolishParams:
    """sc_polish_params: the best `candidates` hypotheses of the frame (1 .. 64), at most `max_iter` refits each (1 .. 64)."""
    return _sized(ScPolishParams, candidates, max_iter, flags)


def make_pose_info_params(sel_mode: int = SC_POSE_INFO_SEL_NONE, label0: int = 0, flags: int = 0) -> ScPoseInfoParams:
    """sc_pose_info_params: sel_mode SC_POSE_INFO_SEL_*, label0 (SEL_LABEL only), flags SC_POSE_INFO_STATUS or 0."""
    return _sized(ScPoseInfoParams, sel_mode, label0, flags)


def make_polish_poses_params(max_iter: int = 16, sel_mode: int = SC_POLISH_POSES_SEL_NONE, label0: int = 0, flags: int = 0) -> ScPolishPosesParams:
    """sc_polish_poses_params: max_iter 1 .. 64, sel_mode SC_POLISH_POSES_SEL_*, label0 (SEL_LABEL / SEL_ALIVE only), flags
    SC_POLISH_POSES_STATUS or 0."""
    return _sized(ScPolishPosesParams, max_iter, sel_mode, label0, flags)


def make_assign_params(mode: int = SC_ASSIGN_BEST, sel_mode: int = SC_ASSIGN_SEL_NONE, flags: int = 0) -> ScAssignParams:
    """sc_assign_params: mode SC_ASSIGN_BEST / _FIRST, sel_mode SC_ASSIGN_SEL_*, flags SC_ASSIGN_STATUS or 0."""
    return _sized(ScAssignParams, mode, sel_mode, flags)


def make_settle_params(max_iter: int = 16, sel_mode: int = SC_ASSIGN_SEL_NONE, flags: int = 0) -> ScSettleParams:
    """sc_settle_params: max_iter 1 .. 64 counted rounds, sel_mode SC_ASSIGN_SEL_*, flags SC_SETTLE_STATUS or 0."""
    return _sized(ScSettleParams, max_iter, sel_mode, flags)


def make_merge_params(measure: int = SC_MERGE_OVER_MIN, num: int = 1, den: int = 2, min_count: int = 0, sel_mode: int = SC_ASSIGN_SEL_NONE,
                      flags: int = 0) -> ScMergeParams:
    """sc_merge_params: measure SC_MERGE_OVER_*, the fraction num / den (1 <= num <= den <= 65536), min_count, sel_mode
    SC_ASSIGN_SEL_*, flags SC_MERGE_STATUS | SC_MERGE_COMPACT or 0."""
    return _sized(ScMergeParams, measure, num, den, min_count, sel_mode, flags)


def make_cycle_params(rot_tol: float, trans_tol: float, min_ok: int = 1, max_rounds: int = 16, flags: int = 0) -> ScCycleParams:
    """sc_cycle_params: the tolerances (rot_tol in radians, in [0, pi]; trans_tol >= 0) are the caller's; min_ok, max_rounds 1 .. 64,
    flags SC_CYCLES_STATUS or 0."""
    return _sized(ScCycleParams, min_ok, max_rounds, flags, rot_tol, trans_tol)


def cycles_thresholds(cparams: ScCycleParams) -> tuple[float, float]:
    """sc_cycles_thresholds: (tr_min, e2_max), exactly the two values a call with these parameters uses."""
    out = (C.c_double * 2)()
    rc = load_library().sc_cycles_thresholds(C.byref(cparams), out)
    if rc != SC_OK:
        raise SacCotError(rc, "sc_cycles_thresholds")
    return out[0], out[1]


def make_sync_params(rot_tol: float = 0.0, trans_tol: float = 0.0, anchor: int = 0, max_rounds: int = 32, flags: int = 0) -> ScSyncParams:
    """sc_sync_params: the tolerances of the stopping rule (rot_tol in radians, in [0, pi]; trans_tol >= 0) are the caller's; anchor
    < n_sets, max_rounds 1 .. 256, flags SC_SYNC_STATUS or 0."""
    return _sized(ScSyncParams, anchor, max_rounds, flags, rot_tol, trans_tol)


def sync_thresholds(sparams: ScSyncParams) -> tuple[float, float]:
    """sc_sync_thresholds: (r2_max, e2_max), exactly the two values a call with these parameters uses."""
    out = (C.c_double * 2)()
    rc = load_library().sc_sync_thresholds(C.byref(sparams), out)
    if rc != SC_OK:
        raise SacCotError(rc, "sc_sync_thresholds")
    return out[0], out[1]


def make_solve_params(rot_tol: float = 0.0, trans_tol: float = 0.0, cg_tol: float = 0.0, anchor: int = 0, max_outer: int = 8, max_inner: int = 64,
                      flags: int = 0) -> ScSolveParams:
    """sc_solve_params: the tolerances of the stopping rule (rot_tol in radians, in [0, pi]; trans_tol >= 0) and of the inner solve
    (cg_tol in [0, 1)) are the caller's; anchor < n_sets, max_outer 1 .. 32, max_inner 1 .. 256, max_outer * max_inner <= 2048, flags
    SC_SOLVE_STATUS | SC_SOLVE_INFO_STATUS or 0."""
    return _sized(ScSolveParams, anchor, max_outer, max_inner, flags, rot_tol, trans_tol, cg_tol)


def solve_thresholds(vparams: ScSolveParams) -> tuple[float, float, float]:
    """sc_solve_thresholds: (r2_max, e2_max, cg2), exactly the three values a call with these parameters uses."""
    out = (C.c_double * 3)()
    rc = load_library().sc_solve_thresholds(C.byref(vparams), out)
    if rc != SC_OK:
        raise SacCotError(rc, "sc_solve_thresholds")
    return float(out[0]), float(out[1]), float(out[2])


def shard_plan(params: ScParams, n: int) -> ScShardPlan:
    """sc_shard_plan_query: sizes of d_bits_all / the candidate blobs for `params` (shard_world) and n correspondences."""
    plan = _sized(ScShardPlan)
    rc = load_library().sc_shard_plan_query(C.byref(params), n, C.byref(plan))
    if rc != SC_OK:
        raise SacCotError(rc, "sc_shard_plan_query")
    return plan


# ---- marshalling, each step said once ------------------------------------------------------------------------------------
_POINTER_OF = {np.dtype(d): p for d, p in ((np.float32, _F32P), (np.uint8, _U8P), (np.int32, _I32P), (np.uint32, _U32P),
                                            (np.uint64, _U64P))}


def _p(a):
    """An array as the typed pointer its dtype calls for (a dtype the ABI has no pointer for is a KeyError); None stays NULL."""
    return None if a is None else a.ctypes.data_as(_POINTER_OF[a.dtype])


def _vp(a):
    """An array of records, or one a `void*` parameter takes, as that; None stays NULL."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32c(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _u32c(off):
    """A host offset array (B + 1,) as the entries take it -> (contiguous uint32 array, B); B = 0 for an empty one."""
    off = np.ascontiguousarray(off, dtype=np.uint32)
    return off, max(len(off) - 1, 0)


def _total(off) -> int:
    """The rows an offset array spans: its last entry, 0 for an empty one."""
    return int(off[-1]) if len(off) else 0


def _n_points(a, layout) -> int:
    """The points of an (n, 3) array, or of a (3, n) one with SC_SOA."""
    return a.shape[0] if layout == SC_AOS else a.shape[1]


def _frame_sel(who, sel, dtype, n):
    """The selection of a frame entry: None, or n entries of the dtype the entry's sel_mode reads (the caller names it)."""
    if sel is None:
        return None
    sel = np.ascontiguousarray(sel, dtype=dtype)
    if sel.size != n:
        raise ValueError(who + ": sel holds one entry per correspondence of the frame")
    return sel


def _frame_out(ns, knn, g2=False, label=False, mask=False):
    """Room for what a frame matcher writes, ns * knn entries and never fewer than 1 -> (arrays by their result key — corr, d2, then
    g2 / label / mask where asked for —, the count word)."""
    cap = max(ns * max(int(knn), 1), 1)
    out = dict(corr=np.zeros((cap, 2), np.int32), d2=np.zeros(cap, np.float32))
    for key, wanted, dtype in (("g2", g2, np.float32), ("label", label, np.int32), ("mask", mask, np.uint8)):
        if wanted:
            out[key] = np.zeros(cap, dtype)
    return out, C.c_uint32(0)


def _frame_cut(out, count) -> dict:
    """_frame_out's arrays cut to the entries the call counted, each a copy, behind n."""
    k = int(count.value)
    return dict(n=k, **{key: a[:k].copy() for key, a in out.items()})


def _slot_out(slots, nb, g2=False, registered=False) -> dict:
    """Room for what a batch or pairs matcher writes: corr, d2 and (g2, else None) of `slots` entries, count of nb problems; with a
    registration behind the match also res (nb records) and mask (slots bytes).  Never fewer than 1 of either."""
    s, b = max(slots, 1), max(nb, 1)
    out = dict(corr=np.zeros((s, 2), np.int32), d2=np.zeros(s, np.float32), g2=np.zeros(s, np.float32) if g2 else None,
               count=np.zeros((b, 2), np.uint32))
    if registered:
        out.update(res=np.zeros(b, BATCH_RESULT_DTYPE), mask=np.zeros(s, np.uint8))
    return out


def _slot_cut(out, slots, nb, *keys) -> tuple:
    """_slot_out's arrays named by `keys`, in that order, as views: count and res cut to nb problems, the others to `slots`
    entries; None stays None."""
    return tuple(None if out[k] is None else out[k][:nb if k in ("count", "res") else slots] for k in keys)


def _motion_out():
    """Room for the one motion an entry returns and for its statistics -> (R (9,), t (3,), sc_stats)."""
    return np.zeros(9, np.float32), np.zeros(3, np.float32), _sized(ScStats)


def _result(rc, R, t, st, **more) -> dict:
    """dict(status, R (3, 3), t, ..., stats) of the entries that return one motion; `more` (mask, n, corr, ...) goes in between."""
    return dict(status=rc, R=R.reshape(3, 3), t=t, **more, stats=st.as_dict())


def _register(self, fn, src, tgt, params, kw) -> dict:
    """Registrar.register and MultiRegistrar.register: (n, 3) src / tgt through `fn` of self's handle -> _result with the mask.  The
    frame's n is stored before the call."""
    p = params or make_params(**kw)
    src, tgt = _f32c(src), _f32c(tgt)
    n = _n_points(src, p.layout)
    (R, t, st), mask = _motion_out(), np.zeros(n, np.uint8)
    self._frame_n = n
    rc = self._check(fn(self._h, _p(src), _p(tgt), n, C.byref(p), _p(R), _p(t), _p(mask), C.byref(st)), allow=(SC_ENOHYP,))
    return _result(rc, R, t, st, mask=mask)


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
        d = _sized(cls, compact_self_max=-1, scan_self_max=-1)
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
        d = _sized(ScDebugInfo)
        self._check(self._lib.sc_debug_last(self._h, C.byref(d)))
        return {k: getattr(d, k) for k, _ in ScDebugInfo._fields_ if k != "size"}

    # ---- drop-in entry point ----------------------------------------------------------------------------
    def register(self, src, tgt, params: ScParams | None = None, **kw):
        """(n,3) src/tgt correspondences -> dict(status, R (3,3), t (3,), mask (n,) uint8, stats)."""
        return _register(self, self._lib.sc_register, src, tgt, params, kw)

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
        offset, nb = _u32c(offset)
        total = _total(offset)
        res = np.zeros(max(nb, 1), BATCH_RESULT_DTYPE); mask = np.zeros(max(total, 1), np.uint8)
        self._frame_n = 0
        self._check(self._lib.sc_register_batch(self._h, _p(src), _p(tgt), _p(offset), nb, C.byref(params), _vp(res), _p(mask)))
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
        offset, nb = _u32c(offset)
        self._frame_n = 0
        self._check(self._lib.sc_register_batch_device(self._h, d_src, d_tgt, _p(offset), nb, C.byref(params), d_res, d_mask))

    # ---- further rigid motions from the frame the last register* call left (include/saccot.h, sc_peel) ------
    def peel(self):
        """sc_peel: the next round on the frame in this context -> dict(status, R, t, mask, stats) like register()'s; SC_ENOHYP
        (no hypothesis explains an unclaimed correspondence) is a status, not an exception.  The frame's n sizes the mask."""
        n = self._frame_n
        (R, t, st), mask = _motion_out(), np.zeros(max(n, 1), np.uint8)
        rc = self._check(self._lib.sc_peel(self._h, _p(R), _p(t), _p(mask), C.byref(st)), allow=(SC_ENOHYP,))
        return _result(rc, R, t, st, mask=mask[:n])

    def peel_device(self, d_Rt: int, d_mask: int):
        """sc_peel_device: the same with the outputs in HBM (d_Rt: 12 floats, d_mask: n bytes) -> (status, stats)."""
        st = _sized(ScStats)
        rc = self._check(self._lib.sc_peel_device(self._h, d_Rt, d_mask, C.byref(st)), allow=(SC_ENOHYP,))
        return rc, st.as_dict()

    # ---- refits iterated to a fixed point on that frame (include/saccot.h, sc_polish) --------------------------------
    def polish(self, pparams: ScPolishParams | None = None, **kw):
        """sc_polish: the frame's best hypotheses, each refitted over its own inliers until nothing changes; the best of them ->
        dict(status, R, t, mask, n_cand, cand (candidates,) records of POLISH_CAND_DTYPE — those past n_cand zeroed —, stats).  stats["best_count"] is the polished
        score and may be below the frame's.  kw: candidates, max_iter (make_polish_params)."""
        q = pparams or make_polish_params(**kw)
        n = self._frame_n
        (R, t, st), mask = _motion_out(), np.zeros(max(n, 1), np.uint8)
        cand = np.zeros(max(int(q.candidates), 1), POLISH_CAND_DTYPE); k = C.c_uint32(0)
        rc = self._check(self._lib.sc_polish(self._h, C.byref(q), _p(R), _p(t), _p(mask), _vp(cand), C.byref(k), C.byref(st)),
                         allow=(SC_ENOHYP,))
        return _result(rc, R, t, st, mask=mask[:n], n_cand=int(k.value), cand=cand)

    def polish_device(self, pparams: ScPolishParams, d_Rt: int, d_mask: int, d_cand: int = 0, d_ncand: int = 0):
        """sc_polish_device: the same with the outputs in HBM (d_Rt: 12 floats, d_mask: n bytes, d_cand: `candidates` records of
        64 bytes or 0, d_ncand: one uint32 or 0) -> (status, stats)."""
        st = _sized(ScStats)
        rc = self._check(self._lib.sc_polish_device(self._h, C.byref(pparams), d_Rt, d_mask, d_cand or None, d_ncand or None,
                                                    C.byref(st)), allow=(SC_ENOHYP,))
        return rc, st.as_dict()

    def register_instances(self, src, tgt, max_instances: int = 8, min_score: int = 0, params: ScParams | None = None, **kw):
        """sc_register_instances: the frame and its rounds in one call -> dict(status, Rt (k,12), score (k,), label (n,) int32:
        the motion that claimed each correspondence, -1 for none; stats: the frame's)."""
        p = params or make_params(**kw)
        src, tgt = _f32c(src), _f32c(tgt)
        n = _n_points(src, p.layout)
        Rt = np.zeros((max_instances, 12), np.float32); score = np.zeros(max_instances, np.uint32)
        label = np.full(n, -1, np.int32); found = C.c_uint32(0)
        st = _sized(ScStats)
        rc = self._check(self._lib.sc_register_instances(self._h, _p(src), _p(tgt), n, C.byref(p), max_instances, min_score, _p(Rt),
                                                         _p(score), _p(label), C.byref(found), C.byref(st)), allow=(SC_ENOHYP,))
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
        out, n = _frame_out(fsrc.shape[0], m.knn)
        self._check(self._lib.sc_match(self._h, _p(fsrc), fsrc.shape[0], _p(ftgt), ftgt.shape[0], C.byref(m), _p(out["corr"]),
                                       _p(out["d2"]), C.byref(n)))
        return _frame_cut(out, n)

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
        if _n_points(src_pts, p.layout) != ns or _n_points(tgt_pts, p.layout) != nt or fsrc.shape[1] != ftgt.shape[1]:
            raise ValueError("register_features: one descriptor row per point, one D")
        out, n = _frame_out(ns, m.knn, mask=True)
        R, t, st = _motion_out()
        rc = self._check(self._lib.sc_register_features(self._h, _p(src_pts), _p(fsrc), ns, _p(tgt_pts), _p(ftgt), nt, C.byref(m),
                                                        C.byref(p), _p(R), _p(t), _p(out["corr"]), _p(out["d2"]), C.byref(n),
                                                        _p(out["mask"]), C.byref(st)), allow=(SC_ENOHYP,))
        return self._features_result(rc, R, t, st, out, n)

    def _features_result(self, rc, R, t, st, out, count):
        """What the *_features frame entries return, and their rule for the frame: it holds the matches counted, noted after the call."""
        cut = _frame_cut(out, count)
        self._frame_n = cut["n"]
        return _result(rc, R, t, st, **cut)

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
        out, n = _frame_out(fsrc.shape[0], m.knn, g2=True)
        self._check(self._lib.sc_match_guided(self._h, _p(src_pts), _p(fsrc), fsrc.shape[0], _p(tgt_pts), _p(ftgt), ftgt.shape[0],
                                              C.byref(m), C.byref(g), _p(Rt), _p(out["corr"]), _p(out["d2"]), _p(out["g2"]),
                                              C.byref(n)))
        return _frame_cut(out, n)

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
        out, n = _frame_out(ns, m.knn, g2=True, mask=True)
        R, t, st = _motion_out()
        rc = self._check(self._lib.sc_register_guided_features(
            self._h, _p(src_pts), _p(fsrc), ns, _p(tgt_pts), _p(ftgt), nt, C.byref(m), C.byref(g), _p(Rt), C.byref(p), _p(R), _p(t),
            _p(out["corr"]), _p(out["d2"]), _p(out["g2"]), C.byref(n), _p(out["mask"]), C.byref(st)), allow=(SC_ENOHYP,))
        return self._features_result(rc, R, t, st, out, n)

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
        out, n = _frame_out(fsrc.shape[0], m.knn, g2=True, label=True)
        self._check(self._lib.sc_match_guided_poses(self._h, _p(src_pts), _p(fsrc), fsrc.shape[0], _p(tgt_pts), _p(ftgt), ftgt.shape[0],
                                                    C.byref(m), C.byref(g), _vp(pose), stride, len(pose), _p(out["corr"]),
                                                    _p(out["d2"]), _p(out["g2"]), _p(out["label"]), C.byref(n)))
        return _frame_cut(out, n)

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
        out, n = _frame_out(ns, m.knn, g2=True, label=True, mask=True)
        R, t, st = _motion_out()
        rc = self._check(self._lib.sc_register_guided_poses_features(
            self._h, _p(src_pts), _p(fsrc), ns, _p(tgt_pts), _p(ftgt), nt, C.byref(m), C.byref(g), _vp(pose), stride, len(pose),
            C.byref(p), _p(R), _p(t), _p(out["corr"]), _p(out["d2"]), _p(out["g2"]), _p(out["label"]), C.byref(n), _p(out["mask"]),
            C.byref(st)), allow=(SC_ENOHYP,))
        return self._features_result(rc, R, t, st, out, n)

    # ---- descriptor matching for a batch of small problems (include/saccot.h, sc_match_batch) -------------------
    @staticmethod
    def _offsets(sizes):
        return np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.uint32)

    def match_batch_raw(self, fsrc, src_off, ftgt, tgt_off, mparams: ScMatchParams):
        """sc_match_batch on packed arrays: fsrc (total_s, D), ftgt (total_t, D), both offset arrays (B + 1,) uint32 ->
        (corr (total_s * knn, 2) int32, d2 (total_s * knn,) float32, count (B, 2) uint32).  Problem b's slot starts at entry
        src_off[b] * knn; count[b] = (n_b, 1 if the problem read a non-finite descriptor)."""
        fsrc, ftgt = _f32c(fsrc), _f32c(ftgt)
        (src_off, nb), (tgt_off, _) = _u32c(src_off), _u32c(tgt_off)
        slots = _total(src_off) * max(int(mparams.knn), 1)
        o = _slot_out(slots, nb)
        self._frame_n = 0
        self._check(self._lib.sc_match_batch(self._h, _p(fsrc), _p(src_off), _p(ftgt), _p(tgt_off), nb, C.byref(mparams), _p(o["corr"]),
                                             _p(o["d2"]), _p(o["count"])))
        return _slot_cut(o, slots, nb, "corr", "d2", "count")

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
        (src_off, nb), (tgt_off, _) = _u32c(src_off), _u32c(tgt_off)
        self._frame_n = 0
        self._check(self._lib.sc_match_batch_device(self._h, d_fsrc, _p(src_off), d_ftgt, _p(tgt_off), nb, C.byref(mparams), d_corr, d_d2,
                                                    d_count))

    def register_batch_features_raw(self, src_pts, fsrc, src_off, tgt_pts, ftgt, tgt_off, mparams: ScMatchParams, params: ScParams):
        """sc_register_batch_features on packed arrays (points in params' layout) -> (records (B,), corr, d2, count (B, 2), mask
        (total_s * knn,)), the last four slot-positioned as in match_batch_raw."""
        src_pts, fsrc, tgt_pts, ftgt = _f32c(src_pts), _f32c(fsrc), _f32c(tgt_pts), _f32c(ftgt)
        (src_off, nb), (tgt_off, _) = _u32c(src_off), _u32c(tgt_off)
        slots = _total(src_off) * max(int(mparams.knn), 1)
        o = _slot_out(slots, nb, registered=True)
        self._frame_n = 0
        self._check(self._lib.sc_register_batch_features(self._h, _p(src_pts), _p(fsrc), _p(src_off), _p(tgt_pts), _p(ftgt), _p(tgt_off),
                                                         nb, C.byref(mparams), C.byref(params), _vp(o["res"]), _p(o["corr"]),
                                                         _p(o["d2"]), _p(o["count"]), _p(o["mask"])))
        return _slot_cut(o, slots, nb, "res", "corr", "d2", "count", "mask")

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
        (src_off, nb), (tgt_off, _) = _u32c(src_off), _u32c(tgt_off)
        self._frame_n = 0
        self._check(self._lib.sc_register_batch_features_device(self._h, d_src_pts, d_fsrc, _p(src_off), d_tgt_pts, d_ftgt, _p(tgt_off), nb,
                                                                C.byref(mparams), C.byref(params), d_res, d_corr, d_d2, d_count, d_mask))

    # ---- iterated fp64 refits for a batch's winners (include/saccot.h, sc_polish_batch) ------------------------------
    def polish_batch_raw(self, src, tgt, offset, params: ScParams, pparams: ScPolishParams, res):
        """sc_polish_batch on packed arrays: src / tgt / offset as register_batch_raw's, res (B,) records of BATCH_RESULT_DTYPE (the
        input poses and statuses; read only) -> (records (B,) of POLISH_BATCH_RESULT_DTYPE, mask (total,) uint8)."""
        src, tgt = _f32c(src), _f32c(tgt)
        offset, nb = _u32c(offset)
        res = np.ascontiguousarray(res, dtype=BATCH_RESULT_DTYPE)
        if len(res) != nb:
            raise ValueError("polish_batch_raw: one input record per problem")
        total = _total(offset)
        pol = np.zeros(max(nb, 1), POLISH_BATCH_RESULT_DTYPE); mask = np.zeros(max(total, 1), np.uint8)
        self._frame_n = 0
        self._check(self._lib.sc_polish_batch(self._h, _p(src), _p(tgt), _p(offset), nb, C.byref(params), C.byref(pparams), _vp(res),
                                              _vp(pol), _p(mask)))
        return pol[:nb], mask[:total]

    def polish_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, pparams: ScPolishParams, d_res: int, d_pol: int,
                            d_mask: int):
        """sc_polish_batch_device: points, input records (80 bytes each, read only), output records (64 bytes each) and mask in HBM,
        offset a HOST array (B + 1,) uint32; enqueues on the context's stream and returns without waiting.  d_mask may be the
        buffer register_batch_device wrote."""
        offset, nb = _u32c(offset)
        self._frame_n = 0
        self._check(self._lib.sc_polish_batch_device(self._h, d_src, d_tgt, _p(offset), nb, C.byref(params), C.byref(pparams), d_res,
                                                     d_pol, d_mask))

    def polish_batch_slots_device(self, d_src_pts: int, src_off, d_tgt_pts: int, tgt_off, knn: int, params: ScParams,
                                  pparams: ScPolishParams, d_corr: int, d_count: int, d_res: int, d_pol: int, d_mask: int):
        """sc_polish_batch_slots_device: behind register_batch_features_device — its points, offsets, d_corr, d_count and d_res; d_pol
        B records of 64 bytes, d_mask total_s * knn bytes; enqueues on the context's stream and returns without waiting."""
        (src_off, nb), (tgt_off, _) = _u32c(src_off), _u32c(tgt_off)
        self._frame_n = 0
        self._check(self._lib.sc_polish_batch_slots_device(self._h, d_src_pts, _p(src_off), d_tgt_pts, _p(tgt_off), nb, knn,
                                                           C.byref(params), C.byref(pparams), d_corr, d_count, d_res, d_pol, d_mask))

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
        offset, nb = _u32c(offset)
        total = _total(offset)
        planes = min(max(int(max_instances), 1), SC_INSTANCES_BATCH_MAX)  # (room; the library refuses what is out of range)
        res = np.zeros((planes, max(nb, 1)), BATCH_RESULT_DTYPE); label = np.zeros(max(total, 1), np.int32)
        nfound = np.zeros(max(nb, 1), np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_register_instances_batch(self._h, _p(src), _p(tgt), _p(offset), nb, C.byref(params), max_instances,
                                                          min_score, _vp(res), _p(label), _p(nfound)))
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
        offset, nb = _u32c(offset)
        self._frame_n = 0
        self._check(self._lib.sc_register_instances_batch_device(self._h, d_src, d_tgt, _p(offset), nb, C.byref(params), max_instances,
                                                                 min_score, d_res, d_label, d_nfound))

    def register_instances_batch_features_device(self, d_src_pts: int, d_fsrc: int, src_off, d_tgt_pts: int, d_ftgt: int, tgt_off,
                                                 mparams: ScMatchParams, params: ScParams, max_instances: int, min_score: int, d_res: int,
                                                 d_corr: int, d_d2: int, d_count: int, d_label: int, d_nfound: int):
        """sc_register_instances_batch_features_device: register_batch_features_device with rounds — d_res max_instances x B records,
        d_label total_s * knn int32 positioned like that entry's mask, d_nfound B uint32; returns without waiting."""
        (src_off, nb), (tgt_off, _) = _u32c(src_off), _u32c(tgt_off)
        self._frame_n = 0
        self._check(self._lib.sc_register_instances_batch_features_device(
            self._h, d_src_pts, d_fsrc, _p(src_off), d_tgt_pts, d_ftgt, _p(tgt_off), nb, C.byref(mparams), C.byref(params), max_instances,
            min_score, d_res, d_corr, d_d2, d_count, d_label, d_nfound))

    # ---- listed pairs of shared keypoint sets (include/saccot.h, sc_match_pairs) ------------------------------------
    @staticmethod
    def _table(set_off, pairs):
        """set_off (S + 1,) and pairs (P, 2) as the pairs entries take them -> (set_off, pairs, S, P), both flat uint32"""
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
        rc = load_library().sc_pairs_layout(_p(set_off), ns, _p(pairs), npairs, knn, _p(slot))
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
        o = _slot_out(slots, npairs)
        self._frame_n = 0
        self._check(self._lib.sc_match_pairs(self._h, _p(feat), _p(set_off), ns, _p(pairs), npairs, C.byref(m), _p(o["corr"]), _p(o["d2"]),
                                             _p(o["count"])))
        return _slot_cut(o, slots, npairs, "corr", "d2", "count") + (slot,)

    def match_pairs_device(self, d_feat: int, set_off, pairs, mparams: ScMatchParams, d_corr: int, d_d2: int, d_count: int):
        """sc_match_pairs_device: the table's descriptors and the outputs in HBM (d_corr slot[P] x 2 int32, d_d2 slot[P] float32,
        d_count 2 x P uint32), set_off and pairs HOST arrays; enqueues on the context's stream and returns without waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_match_pairs_device(self._h, d_feat, _p(set_off), ns, _p(pairs), npairs, C.byref(mparams), d_corr, d_d2,
                                                    d_count))

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
        o = _slot_out(slots, npairs, registered=True)
        self._frame_n = 0
        self._check(self._lib.sc_register_pairs_features(self._h, _p(pts), _p(feat), _p(set_off), ns, _p(pairs), npairs, C.byref(m),
                                                         C.byref(p), _vp(o["res"]), _p(o["corr"]), _p(o["d2"]), _p(o["count"]),
                                                         _p(o["mask"])))
        return _slot_cut(o, slots, npairs, "res", "corr", "d2", "count", "mask") + (slot,)

    def register_pairs_features_device(self, d_pts: int, d_feat: int, set_off, pairs, mparams: ScMatchParams, params: ScParams,
                                       d_res: int, d_corr: int, d_d2: int, d_count: int, d_mask: int):
        """sc_register_pairs_features_device: everything but set_off and pairs in HBM (d_res P records of 80 bytes, d_mask slot[P]
        bytes, the rest as match_pairs_device); enqueues on the context's stream and returns without waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_register_pairs_features_device(self._h, d_pts, d_feat, _p(set_off), ns, _p(pairs), npairs,
                                                                C.byref(mparams), C.byref(params), d_res, d_corr, d_d2, d_count, d_mask))

    def polish_pairs_slots_device(self, d_pts: int, set_off, pairs, knn: int, params: ScParams, pparams: ScPolishParams, d_corr: int,
                                  d_count: int, d_res: int, d_pol: int, d_mask: int):
        """sc_polish_pairs_slots_device: behind register_pairs_features_device — its points, set_off, pairs, d_corr, d_count and
        d_res; d_pol P records of 64 bytes, d_mask slot[P] bytes; enqueues on the context's stream and returns without waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_polish_pairs_slots_device(self._h, d_pts, _p(set_off), ns, _p(pairs), npairs, knn, C.byref(params),
                                                           C.byref(pparams), d_corr, d_count, d_res, d_pol, d_mask))

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
        (src_off, nb), (tgt_off, _) = _u32c(src_off), _u32c(tgt_off)
        m = mparams or make_match_params(fsrc.shape[1], **kw)
        pose, stride = self._pose_records(pose, nb)
        slots = _total(src_off) * max(int(m.knn), 1)
        o = _slot_out(slots, nb, g2=want_g2)
        self._frame_n = 0
        self._check(self._lib.sc_match_guided_batch(self._h, _p(src_pts), _p(fsrc), _p(src_off), _p(tgt_pts), _p(ftgt), _p(tgt_off), nb,
                                                    C.byref(m), C.byref(g), _vp(pose), stride, _p(o["corr"]), _p(o["d2"]), _p(o["g2"]),
                                                    _p(o["count"])))
        return _slot_cut(o, slots, nb, "corr", "d2", "g2", "count")

    def match_guided_batch_device(self, d_src_pts: int, d_fsrc: int, src_off, d_tgt_pts: int, d_ftgt: int, tgt_off, mparams: ScMatchParams,
                                  gparams: ScGuideParams, d_pose: int, pose_stride: int, d_corr: int, d_d2: int, d_g2: int | None,
                                  d_count: int):
        """sc_match_guided_batch_device: everything but the offsets in HBM (d_pose: B records pose_stride bytes apart, read in stream
        order; d_g2: total_s * knn float32 or None; the rest as match_batch_device); returns without waiting."""
        (src_off, nb), (tgt_off, _) = _u32c(src_off), _u32c(tgt_off)
        self._frame_n = 0
        self._check(self._lib.sc_match_guided_batch_device(self._h, d_src_pts, d_fsrc, _p(src_off), d_tgt_pts, d_ftgt, _p(tgt_off), nb,
                                                           C.byref(mparams), C.byref(gparams), d_pose, pose_stride, d_corr, d_d2, d_g2,
                                                           d_count))

    def register_guided_batch_features_device(self, d_src_pts: int, d_fsrc: int, src_off, d_tgt_pts: int, d_ftgt: int, tgt_off,
                                              mparams: ScMatchParams, gparams: ScGuideParams, d_pose: int, pose_stride: int,
                                              params: ScParams, d_res: int, d_corr: int, d_d2: int, d_g2: int | None, d_count: int,
                                              d_mask: int):
        """sc_register_guided_batch_features_device: match_guided_batch_device, then the registration on the slots (d_res, d_mask as
        register_batch_features_device's).  d_pose may be d_res; returns without waiting."""
        (src_off, nb), (tgt_off, _) = _u32c(src_off), _u32c(tgt_off)
        self._frame_n = 0
        self._check(self._lib.sc_register_guided_batch_features_device(
            self._h, d_src_pts, d_fsrc, _p(src_off), d_tgt_pts, d_ftgt, _p(tgt_off), nb, C.byref(mparams), C.byref(gparams), d_pose,
            pose_stride, C.byref(params), d_res, d_corr, d_d2, d_g2, d_count, d_mask))

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
        o = _slot_out(slots, npairs, g2=want_g2)
        self._frame_n = 0
        self._check(self._lib.sc_match_guided_pairs(self._h, _p(pts), _p(feat), _p(set_off), ns, _p(pairs), npairs, C.byref(m), C.byref(g),
                                                    _vp(pose), stride, _p(o["corr"]), _p(o["d2"]), _p(o["g2"]), _p(o["count"])))
        return _slot_cut(o, slots, npairs, "corr", "d2", "g2", "count") + (slot,)

    def match_guided_pairs_device(self, d_pts: int, d_feat: int, set_off, pairs, mparams: ScMatchParams, gparams: ScGuideParams,
                                  d_pose: int, pose_stride: int, d_corr: int, d_d2: int, d_g2: int | None, d_count: int):
        """sc_match_guided_pairs_device: the table, the pose records (one per pair) and the outputs in HBM, set_off and pairs HOST
        arrays; returns without waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_match_guided_pairs_device(self._h, d_pts, d_feat, _p(set_off), ns, _p(pairs), npairs, C.byref(mparams),
                                                           C.byref(gparams), d_pose, pose_stride, d_corr, d_d2, d_g2, d_count))

    def register_guided_pairs_features_device(self, d_pts: int, d_feat: int, set_off, pairs, mparams: ScMatchParams,
                                              gparams: ScGuideParams, d_pose: int, pose_stride: int, params: ScParams, d_res: int,
                                              d_corr: int, d_d2: int, d_g2: int | None, d_count: int, d_mask: int):
        """sc_register_guided_pairs_features_device: match_guided_pairs_device, then the registration on the slots.  d_pose may be
        d_res; returns without waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_register_guided_pairs_features_device(
            self._h, d_pts, d_feat, _p(set_off), ns, _p(pairs), npairs, C.byref(mparams), C.byref(gparams), d_pose, pose_stride,
            C.byref(params), d_res, d_corr, d_d2, d_g2, d_count, d_mask))

    # ---- the fp64 information matrix of a batch's poses (include/saccot.h, sc_pose_info_batch) -------------------------
    def pose_info_batch_raw(self, src, tgt, offset, params: ScParams, pose):
        """sc_pose_info_batch on packed arrays: src / tgt / offset as register_batch_raw's; pose (B,) records of any dtype whose
        items start with float Rt[12] and int32 status — BATCH_RESULT_DTYPE, POLISH_BATCH_RESULT_DTYPE, a plane of
        register_instances_batch_raw's records — read only -> records (B,) of POSE_INFO_RESULT_DTYPE."""
        src, tgt = _f32c(src), _f32c(tgt)
        offset, nb = _u32c(offset)
        pose = np.ascontiguousarray(pose)
        if pose.ndim != 1 or len(pose) != nb:
            raise ValueError("pose_info_batch_raw: one pose record per problem")
        info = np.zeros(max(nb, 1), POSE_INFO_RESULT_DTYPE)
        self._frame_n = 0
        self._check(self._lib.sc_pose_info_batch(self._h, _p(src), _p(tgt), _p(offset), nb, C.byref(params), _vp(pose),
                                                 pose.dtype.itemsize, _vp(info)))
        return info[:nb]

    def pose_info_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, d_pose: int, pose_stride: int, d_info: int):
        """sc_pose_info_batch_device: points, pose records (pose_stride bytes each, read only) and output records (320 bytes each) in
        HBM, offset a HOST array (B + 1,) uint32; enqueues on the context's stream and returns without waiting."""
        offset, nb = _u32c(offset)
        self._frame_n = 0
        self._check(self._lib.sc_pose_info_batch_device(self._h, d_src, d_tgt, _p(offset), nb, C.byref(params), d_pose, pose_stride,
                                                        d_info))

    def pose_info_batch_slots_device(self, d_src_pts: int, src_off, d_tgt_pts: int, tgt_off, knn: int, params: ScParams, d_corr: int,
                                     d_count: int, d_pose: int, pose_stride: int, d_info: int):
        """sc_pose_info_batch_slots_device: behind register_batch_features_device — its points, offsets, d_corr and d_count; d_pose B
        records of pose_stride bytes, d_info B records of 320 bytes; enqueues on the context's stream and returns without waiting."""
        (src_off, nb), (tgt_off, _) = _u32c(src_off), _u32c(tgt_off)
        self._frame_n = 0
        self._check(self._lib.sc_pose_info_batch_slots_device(self._h, d_src_pts, _p(src_off), d_tgt_pts, _p(tgt_off), nb, knn,
                                                              C.byref(params), d_corr, d_count, d_pose, pose_stride, d_info))

    def pose_info_pairs_slots_device(self, d_pts: int, set_off, pairs, knn: int, params: ScParams, d_corr: int, d_count: int, d_pose: int,
                                     pose_stride: int, d_info: int):
        """sc_pose_info_pairs_slots_device: behind register_pairs_features_device — its points, set_off, pairs, d_corr and d_count;
        d_pose P records of pose_stride bytes, d_info P records of 320 bytes; enqueues on the context's stream and returns without
        waiting."""
        set_off, pairs, ns, npairs = self._table(set_off, pairs)
        self._frame_n = 0
        self._check(self._lib.sc_pose_info_pairs_slots_device(self._h, d_pts, _p(set_off), ns, _p(pairs), npairs, knn, C.byref(params),
                                                              d_corr, d_count, d_pose, pose_stride, d_info))

    # ---- the same on the frame the last register* call left (include/saccot.h, sc_pose_info_frame) ---------------------------
    def pose_info_frame(self, pose, iparams: ScPoseInfoParams | None = None, sel=None, **kw):
        """sc_pose_info_frame: pose (K,) records of any dtype whose items start with float Rt[12] (and, with SC_POSE_INFO_STATUS, an
        int32 status behind it) — or a float32 array (K, 12) / (12,) —; sel None, (n,) uint8 (SEL_MASK) or (n,) int32 (SEL_LABEL), read
        only -> records (K,) of POSE_INFO_RESULT_DTYPE.  The frame stays.  kw: sel_mode, label0, flags (make_pose_info_params)."""
        q = iparams or make_pose_info_params(**kw)
        pose, stride = self._pose_records(pose)
        k = len(pose)
        sel = _frame_sel("pose_info_frame", sel, np.int32 if q.sel_mode == SC_POSE_INFO_SEL_LABEL else np.uint8, self._frame_n)
        info = np.zeros(max(k, 1), POSE_INFO_RESULT_DTYPE)
        self._check(self._lib.sc_pose_info_frame(self._h, C.byref(q), _vp(pose), stride, k, _vp(sel), _vp(info)))
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
        pose, stride = self._pose_records(pose)
        k, n = len(pose), self._frame_n
        sel = _frame_sel("polish_poses", sel, np.uint8 if q.sel_mode == SC_POLISH_POSES_SEL_MASK else np.int32, n)
        pol = np.zeros(max(k, 1), POLISH_BATCH_RESULT_DTYPE)
        mask = np.zeros((max(k, 1), max(n, 1)), np.uint8) if want_mask else None
        self._check(self._lib.sc_polish_poses(self._h, C.byref(q), _vp(pose), stride, k, _vp(sel), _vp(pol), _vp(mask)))
        return pol[:k], (None if mask is None else mask[:k, :n])

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
        pose, stride = self._pose_records(pose)
        k, n = len(pose), self._frame_n
        sel = _frame_sel("assign_poses_frame", sel, np.uint8, n)
        label = np.zeros(max(n, 1), np.int32)
        d2 = np.zeros(max(n, 1), np.float32) if want_d2 else None
        asg = np.zeros(max(k, 1), ASSIGN_RESULT_DTYPE)
        self._check(self._lib.sc_assign_poses_frame(self._h, C.byref(q), _vp(pose), stride, k, _vp(sel), _vp(label), _vp(d2), _vp(asg)))
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
        offset, nb = _u32c(offset)
        pose = np.ascontiguousarray(pose)
        total = _total(offset)
        if pose.ndim != 2 or pose.shape[1] != nb:
            raise ValueError("assign_poses_batch: pose holds (n_poses, n_problems) records")
        k = pose.shape[0]
        label = np.zeros(max(total, 1), np.int32)
        asg = np.zeros((max(k, 1), max(nb, 1)), ASSIGN_RESULT_DTYPE)
        self._frame_n = 0
        self._check(self._lib.sc_assign_poses_batch(self._h, _p(src), _p(tgt), _p(offset), nb, C.byref(params), C.byref(q), _vp(pose),
                                                    pose.dtype.itemsize, k, _vp(label), _vp(asg)))
        return label[:total], asg[:k, :nb]

    def assign_poses_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, aparams: ScAssignParams, d_pose: int,
                                  pose_stride: int, n_poses: int, d_label: int, d_asg: int):
        """sc_assign_poses_batch_device: points, pose records (n_poses x B of pose_stride bytes, motion-major, read only), labels
        (total int32) and records (n_poses x B of 32 bytes, motion-major) in HBM, offset a HOST array (B + 1,) uint32; enqueues on the
        context's stream and returns without waiting."""
        offset, nb = _u32c(offset)
        self._frame_n = 0
        self._check(self._lib.sc_assign_poses_batch_device(self._h, d_src, d_tgt, _p(offset), nb, C.byref(params), C.byref(aparams),
                                                           d_pose, pose_stride, n_poses, d_label, d_asg))

    # ---- poses relabelled and refitted until stable (include/saccot.h, sc_settle_poses) -----------------------------------------
    def settle_poses_frame(self, pose, sparams: ScSettleParams | None = None, sel=None, want_d2: bool = True, want_rounds: bool = True,
                           **kw):
        """sc_settle_poses_frame: pose (K,) records of any dtype whose items start with float Rt[12] (and, with SC_SETTLE_STATUS, an
        int32 status behind it) — or a float32 array (K, 12) / (12,) —; sel None or (n,) uint8 (SC_ASSIGN_SEL_MASK), read only ->
        (records (K,) of POLISH_BATCH_RESULT_DTYPE, label (n,) int32, d2 (n,) float32 or None, rounds (2,) uint32 — counted rounds,
        stop — or None).  The frame stays.  kw: max_iter, sel_mode, flags (make_settle_params)."""
        q = sparams or make_settle_params(**kw)
        pose, stride = self._pose_records(pose)
        k, n = len(pose), self._frame_n
        sel = _frame_sel("settle_poses_frame", sel, np.uint8, n)
        pol = np.zeros(max(k, 1), POLISH_BATCH_RESULT_DTYPE)
        label = np.zeros(max(n, 1), np.int32)
        d2 = np.zeros(max(n, 1), np.float32) if want_d2 else None
        rounds = np.zeros(2, np.uint32) if want_rounds else None
        self._check(self._lib.sc_settle_poses_frame(self._h, C.byref(q), _vp(pose), stride, k, _vp(sel), _vp(pol), _vp(label), _vp(d2),
                                                    _vp(rounds)))
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
        offset, nb = _u32c(offset)
        pose = np.ascontiguousarray(pose)
        total = _total(offset)
        if pose.ndim != 2 or pose.shape[1] != nb:
            raise ValueError("settle_poses_batch: pose holds (n_poses, n_problems) records")
        k = pose.shape[0]
        pol = np.zeros((max(k, 1), max(nb, 1)), POLISH_BATCH_RESULT_DTYPE)
        label = np.zeros(max(total, 1), np.int32)
        rounds = np.zeros((max(nb, 1), 2), np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_settle_poses_batch(self._h, _p(src), _p(tgt), _p(offset), nb, C.byref(params), C.byref(q), _vp(pose),
                                                    pose.dtype.itemsize, k, _vp(pol), _vp(label), _vp(rounds)))
        return pol[:k, :nb], label[:total], rounds[:nb]

    def settle_poses_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, sparams: ScSettleParams, d_pose: int,
                                  pose_stride: int, n_poses: int, d_pol: int, d_label: int, d_rounds: int = 0):
        """sc_settle_poses_batch_device: points, pose records (n_poses x B of pose_stride bytes, motion-major, read only), output
        records (n_poses x B of 64 bytes, motion-major), labels (total int32) and the word pairs (2 x B; 0: none) in HBM, offset a
        HOST array (B + 1,) uint32; enqueues on the context's stream and returns without waiting."""
        offset, nb = _u32c(offset)
        self._frame_n = 0
        self._check(self._lib.sc_settle_poses_batch_device(self._h, d_src, d_tgt, _p(offset), nb, C.byref(params), C.byref(sparams),
                                                           d_pose, pose_stride, n_poses, d_pol, d_label, d_rounds or None))

    # ---- duplicate poses found and folded (include/saccot.h, sc_merge_poses) ---------------------------------------------------
    def merge_poses_frame(self, pose, mparams: ScMergeParams | None = None, sel=None, want_overlap: bool = True, want_count: bool = True,
                          **kw):
        """sc_merge_poses_frame: pose (K,) records of any dtype whose items start with float Rt[12] (and, with SC_MERGE_STATUS, an
        int32 status behind it) — or a float32 array (K, 12) / (12,) —; sel None or (n,) uint8 (SC_ASSIGN_SEL_MASK), read only ->
        (records (K,) of MERGE_POSE_DTYPE, parent (K,) int32, overlap (K, K) uint32 or None, count (2,) uint32 — the kept poses, the
        valid poses — or None).  The frame stays.  kw: measure, num, den, min_count, sel_mode, flags (make_merge_params)."""
        q = mparams or make_merge_params(**kw)
        pose, stride = self._pose_records(pose)
        k, n = len(pose), self._frame_n
        sel = _frame_sel("merge_poses_frame", sel, np.uint8, n)
        out = np.zeros(max(k, 1), MERGE_POSE_DTYPE)
        parent = np.zeros(max(k, 1), np.int32)
        overlap = np.zeros((max(k, 1), max(k, 1)), np.uint32) if want_overlap else None
        count = np.zeros(2, np.uint32) if want_count else None
        self._check(self._lib.sc_merge_poses_frame(self._h, C.byref(q), _vp(pose), stride, k, _vp(sel), _vp(out), _vp(parent), _vp(overlap),
                                                   _vp(count)))
        return out[:k], parent[:k], (None if overlap is None else overlap[:k, :k]), count

    def merge_poses_frame_device(self, mparams: ScMergeParams, d_pose: int, pose_stride: int, n_poses: int, d_sel: int, d_out: int,
                                 d_parent: int, d_overlap: int = 0, d_count: int = 0):
        """sc_merge_poses_frame_device: pose records (pose_stride bytes each, read only), the selection (0: none), the output records
        (64 bytes each), the parents (n_poses int32), the overlap table (n_poses x n_poses uint32; 0: none) and the two count words
        (0: none) in HBM; enqueues one memset and three launches on the context's stream and returns without waiting.  The frame
        stays."""
        self._check(self._lib.sc_merge_poses_frame_device(self._h, C.byref(mparams), d_pose, pose_stride, n_poses, d_sel or None, d_out,
                                                          d_parent, d_overlap or None, d_count or None))

    def merge_poses_batch(self, src, tgt, offset, params: ScParams, pose, mparams: ScMergeParams | None = None, **kw):
        """sc_merge_poses_batch on packed arrays: src / tgt / offset as register_batch_raw's; pose (K, B) records, motion-major, of any
        dtype whose items start with float Rt[12] and int32 status — register_instances_batch_raw's records — read only ->
        (records (K, B) of MERGE_POSE_DTYPE, parent (K, B) int32, count (B, 2) uint32).  kw: measure, num, den, min_count, flags
        (make_merge_params)."""
        q = mparams or make_merge_params(**kw)
        src, tgt = _f32c(src), _f32c(tgt)
        offset, nb = _u32c(offset)
        pose = np.ascontiguousarray(pose)
        if pose.ndim != 2 or pose.shape[1] != nb:
            raise ValueError("merge_poses_batch: pose holds (n_poses, n_problems) records")
        k = pose.shape[0]
        out = np.zeros((max(k, 1), max(nb, 1)), MERGE_POSE_DTYPE)
        parent = np.zeros((max(k, 1), max(nb, 1)), np.int32)
        count = np.zeros((max(nb, 1), 2), np.uint32)
        self._frame_n = 0
        self._check(self._lib.sc_merge_poses_batch(self._h, _p(src), _p(tgt), _p(offset), nb, C.byref(params), C.byref(q), _vp(pose),
                                                   pose.dtype.itemsize, k, _vp(out), _vp(parent), _vp(count)))
        return out[:k, :nb], parent[:k, :nb], count[:nb]

    def merge_poses_batch_device(self, d_src: int, d_tgt: int, offset, params: ScParams, mparams: ScMergeParams, d_pose: int,
                                 pose_stride: int, n_poses: int, d_out: int, d_parent: int, d_count: int = 0):
        """sc_merge_poses_batch_device: points, pose records (n_poses x B of pose_stride bytes, motion-major, read only), output
        records (n_poses x B of 64 bytes, motion-major), parents (n_poses x B int32, motion-major) and the word pairs (2 x B; 0: none)
        in HBM, offset a HOST array (B + 1,) uint32; enqueues ONE launch on the context's stream and returns without waiting."""
        offset, nb = _u32c(offset)
        self._frame_n = 0
        self._check(self._lib.sc_merge_poses_batch_device(self._h, d_src, d_tgt, _p(offset), nb, C.byref(params), C.byref(mparams),
                                                          d_pose, pose_stride, n_poses, d_out, d_parent, d_count or None))

    # ---- the entries on a pair list: what they take alike -----------------------------------------------------------------------
    @staticmethod
    def _pair_list(pairs):
        """pairs (P, 2) set indices as the pair-list entries take them -> (flat uint32 array, P)"""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1)
        return pairs, len(pairs) // 2

    @staticmethod
    def _use_words(use, npairs: int, who: str):
        """use as pairs_sync and pairs_solve take it: None, (P,) words, or (P,) records of CYCLE_RESULT_DTYPE whose `alive` words are
        read in place -> (the array to keep alive through the call, address of the first word or None, stride in bytes)"""
        if use is None:
            return None, None, 4
        use = np.ascontiguousarray(use)
        if use.dtype == CYCLE_RESULT_DTYPE:
            ptr, stride = use.ctypes.data + CYCLE_RESULT_DTYPE.fields["alive"][1], CYCLE_RESULT_DTYPE.itemsize
        else:
            use = np.ascontiguousarray(use, dtype=np.uint32).reshape(-1)
            ptr, stride = use.ctypes.data, 4
        if len(use) != npairs:
            raise ValueError(f"{who}: use holds one word (or one sc_cycle_result) per pair")
        return use, ptr, stride

    # ---- loop consistency of a pair list's poses (include/saccot.h, sc_pairs_cycles) --------------------------------------------
    def pairs_cycles(self, n_sets: int, pairs, pose, cparams: ScCycleParams | None = None, keep=None, **kw):
        """sc_pairs_cycles: pairs (P, 2) set indices (source, target); pose (P,) records of any dtype whose items start with float
        Rt[12] (and, with SC_CYCLES_STATUS, an int32 status at byte 48) — or a float32 array (P, 12); keep None or (P,) uint8, non-zero:
        never dropped -> (records (P,) of CYCLE_RESULT_DTYPE, summary: one record of CYCLE_SUMMARY_DTYPE).  kw: rot_tol, trans_tol,
        min_ok, max_rounds, flags (make_cycle_params)."""
        q = cparams or make_cycle_params(**kw)
        pairs, npairs = self._pair_list(pairs)
        pose, stride = self._pose_records(pose, npairs)
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8).reshape(-1)
            if len(keep) != npairs:
                raise ValueError("pairs_cycles: keep holds one byte per pair")
        res = np.zeros(max(npairs, 1), CYCLE_RESULT_DTYPE)
        summary = np.zeros(1, CYCLE_SUMMARY_DTYPE)
        self._frame_n = 0
        self._check(self._lib.sc_pairs_cycles(self._h, n_sets, _p(pairs), npairs, C.byref(q), _vp(pose), stride, _p(keep), _vp(res), _vp(summary)))
        return res[:npairs], summary[0]

    def pairs_cycles_device(self, n_sets: int, pairs, cparams: ScCycleParams, d_pose: int, pose_stride: int, d_keep: int, d_res: int,
                            d_sum: int):
        """sc_pairs_cycles_device: pairs a HOST array (P, 2); pose records (pose_stride bytes each, read only), the keep bytes (0:
        none), the output records (P of 48 bytes) and the summary (32 bytes) in HBM; enqueues on the context's stream — a number of
        operations that depends on max_rounds only — and returns without waiting."""
        pairs, npairs = self._pair_list(pairs)
        self._frame_n = 0
        self._check(self._lib.sc_pairs_cycles_device(self._h, n_sets, _p(pairs), npairs, C.byref(cparams), d_pose, pose_stride,
                                                     d_keep or None, d_res, d_sum))

    # ---- absolute poses of a pair list's sets (include/saccot.h, sc_pairs_sync) ---------------------------------------------------
    def pairs_sync(self, n_sets: int, pairs, pose, sparams: ScSyncParams | None = None, use=None, weight=None, **kw):
        """sc_pairs_sync: pairs (P, 2) set indices (source, target); pose (P,) records as pairs_cycles takes them; use None or (P,)
        uint32, non-zero: the pair may be used — or (P,) records of pairs_cycles (CYCLE_RESULT_DTYPE), whose `alive` words are read in
        place; weight None or (P,) float32 -> (sets (n_sets,) of SYNC_SET_DTYPE, pairs (P,) of SYNC_PAIR_DTYPE, summary: one record of
        SYNC_SUMMARY_DTYPE).  kw: rot_tol, trans_tol, anchor, max_rounds, flags (make_sync_params)."""
        q = sparams or make_sync_params(**kw)
        pairs, npairs = self._pair_list(pairs)
        pose, stride = self._pose_records(pose, npairs)
        use, use_ptr, use_stride = self._use_words(use, npairs, "pairs_sync")
        if weight is not None:
            weight = _f32c(weight).reshape(-1)
            if len(weight) != npairs:
                raise ValueError("pairs_sync: weight holds one float per pair")
        sets = np.zeros(max(n_sets, 1), SYNC_SET_DTYPE)
        res = np.zeros(max(npairs, 1), SYNC_PAIR_DTYPE)
        summary = np.zeros(1, SYNC_SUMMARY_DTYPE)
        self._frame_n = 0
        self._check(self._lib.sc_pairs_sync(self._h, n_sets, _p(pairs), npairs, C.byref(q), _vp(pose), stride, use_ptr, use_stride, _p(weight),
                                            _vp(sets), _vp(res), _vp(summary)))
        return sets[:n_sets], res[:npairs], summary[0]

    def pairs_sync_device(self, n_sets: int, pairs, sparams: ScSyncParams, d_pose: int, pose_stride: int, d_use: int, use_stride: int,
                          d_weight: int, d_set: int, d_pair: int, d_sum: int):
        """sc_pairs_sync_device: pairs a HOST array (P, 2); pose records (pose_stride bytes each), the use words (one every use_stride
        bytes; 0: every pair), the weights (P floats; 0: 1.0), the set records (n_sets of 160 bytes), the pair records (P of 32 bytes)
        and the summary (32 bytes) in HBM; enqueues on the context's stream — a number of operations that depends on max_rounds only —
        and returns without waiting."""
        pairs, npairs = self._pair_list(pairs)
        self._frame_n = 0
        self._check(self._lib.sc_pairs_sync_device(self._h, n_sets, _p(pairs), npairs, C.byref(sparams), d_pose, pose_stride,
                                                   d_use or None, use_stride, d_weight or None, d_set, d_pair, d_sum))

    # ---- Gauss-Newton pose-graph solve of a pair list's sets (include/saccot.h, sc_pairs_solve) ----------------------------------
    def pairs_solve(self, n_sets: int, pairs, pose, init, vparams: ScSolveParams | None = None, use=None, info=None, **kw):
        """sc_pairs_solve: pairs, pose and use as pairs_sync takes them; init (n_sets,) records of 160 bytes or more with an int32
        status at byte 48 and double X[12] at byte 64 — pairs_sync's sets, or an earlier call's own; info None (every matrix the
        identity), (P, 36) float64, or (P,) records with the 36 doubles at byte 0 (POSE_INFO_RESULT_DTYPE: pose_info's records as they
        stand) -> (sets (n_sets,) of SOLVE_SET_DTYPE, pairs (P,) of SOLVE_PAIR_DTYPE, summary: one record of SOLVE_SUMMARY_DTYPE).
        kw: rot_tol, trans_tol, cg_tol, anchor, max_outer, max_inner, flags (make_solve_params)."""
        q = vparams or make_solve_params(**kw)
        pairs, npairs = self._pair_list(pairs)
        pose, stride = self._pose_records(pose, npairs)
        use, use_ptr, use_stride = self._use_words(use, npairs, "pairs_solve")
        info_ptr, info_stride = None, 288
        if info is not None:
            info = np.ascontiguousarray(info)
            if info.dtype.fields is None:
                info = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 36)
            if len(info) != npairs:
                raise ValueError("pairs_solve: info holds 36 doubles (or one record) per pair")
            info_ptr, info_stride = info.ctypes.data, info.strides[0]
        init = np.ascontiguousarray(init)
        if init.dtype.fields is None or len(init) != n_sets:
            raise ValueError("pairs_solve: init holds one record (SYNC_SET_DTYPE, SOLVE_SET_DTYPE) per set")
        sets = np.zeros(max(n_sets, 1), SOLVE_SET_DTYPE)
        res = np.zeros(max(npairs, 1), SOLVE_PAIR_DTYPE)
        summary = np.zeros(1, SOLVE_SUMMARY_DTYPE)
        self._frame_n = 0
        self._check(self._lib.sc_pairs_solve(self._h, n_sets, _p(pairs), npairs, C.byref(q), _vp(pose), stride, use_ptr, use_stride, info_ptr,
                                             info_stride, init.ctypes.data, init.strides[0], _vp(sets), _vp(res), _vp(summary)))
        return sets[:n_sets], res[:npairs], summary[0]

    def pairs_solve_device(self, n_sets: int, pairs, vparams: ScSolveParams, d_pose: int, pose_stride: int, d_use: int, use_stride: int,
                           d_info: int, info_stride: int, d_init: int, init_stride: int, d_set: int, d_pair: int, d_sum: int):
        """sc_pairs_solve_device: pairs a HOST array (P, 2); pose records, the use words (0: every pair), the info records (0: the
        identity), the init records (n_sets), the set records (n_sets of 160 bytes), the pair records (P of 48 bytes) and the summary
        (64 bytes) in HBM; enqueues on the context's stream — a number of operations that depends on max_outer and max_inner only —
        and returns without waiting."""
        pairs, npairs = self._pair_list(pairs)
        self._frame_n = 0
        self._check(self._lib.sc_pairs_solve_device(self._h, n_sets, _p(pairs), npairs, C.byref(vparams), d_pose, pose_stride,
                                                    d_use or None, use_stride, d_info or None, info_stride, d_init, init_stride, d_set, d_pair,
                                                    d_sum))

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
        n = _n_points(src, params.layout)
        W = (n + 63) // 64
        S = np.empty((n, n), np.float32) if want_S else None
        bits = np.zeros((n, W), np.uint64); deg = np.zeros(n, np.uint32)
        self._check(self._lib.sc_compat_host(self._h, _p(src), _p(tgt), n, C.byref(params), _p(S), _p(bits), _p(deg)))
        return S, bits, deg

    def triangles(self, src, tgt, params: ScParams):
        src, tgt = _f32c(src), _f32c(tgt)
        n = _n_points(src, params.layout)
        T = params.max_triangles
        tri = np.zeros((T, 3), np.uint32); key = np.zeros(T, np.uint32)
        t_eff = C.c_uint32(0); total = C.c_uint64(0); edges = C.c_uint64(0)
        self._check(self._lib.sc_triangles_host(self._h, _p(src), _p(tgt), n, C.byref(params), _p(tri), _p(key), C.byref(t_eff),
                                                C.byref(total), C.byref(edges)))
        return tri[: t_eff.value].copy(), key[: t_eff.value].copy(), int(total.value), int(edges.value)

    def kabsch(self, src, tgt, params: ScParams, tri):
        src, tgt = _f32c(src), _f32c(tgt)
        n = _n_points(src, params.layout)
        tri = np.ascontiguousarray(tri, dtype=np.uint32)
        Rt = np.zeros((tri.shape[0], 12), np.float32)
        self._check(self._lib.sc_kabsch_host(self._h, _p(src), _p(tgt), n, C.byref(params), _p(tri), tri.shape[0], _p(Rt)))
        return Rt

    def score(self, src, tgt, params: ScParams, Rt):
        src, tgt = _f32c(src), _f32c(tgt)
        n = _n_points(src, params.layout)
        Rt = _f32c(Rt)
        cnt = np.zeros(Rt.shape[0], np.uint32); key = C.c_uint64(0)
        self._check(self._lib.sc_score_host(self._h, _p(src), _p(tgt), n, C.byref(params), _p(Rt), Rt.shape[0], _p(cnt), C.byref(key)))
        return cnt, int(key.value)

    def mask(self, src, tgt, params: ScParams, Rt12):
        src, tgt = _f32c(src), _f32c(tgt)
        n = _n_points(src, params.layout)
        Rt12 = _f32c(Rt12).reshape(12)
        m = np.zeros(n, np.uint8)
        self._check(self._lib.sc_mask_host(self._h, _p(src), _p(tgt), n, C.byref(params), _p(Rt12), _p(m)))
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

    def _check(self, rc: int, allow=()):
        if rc != SC_OK and rc not in allow:
            raise SacCotError(rc, self._lib.sc_strerror(rc).decode() + " — " + self._lib.sc_multi_last_error(self._h).decode())
        return rc

    def register(self, src, tgt, params: ScParams | None = None, **kw):
        """Registrar.register over the handle's GPUs.  (The n it notes in _frame_n serves nothing here: sc_multi keeps no frame.)"""
        return _register(self, self._lib.sc_register_multi, src, tgt, params, kw)


def register(src, tgt, device: int = 0, **kw):
    """One-shot convenience: create a context, run the whole path, destroy the context."""
    r = Registrar(device)
    try:
        return r.register(src, tgt, **kw)
    finally:
        r.close()
