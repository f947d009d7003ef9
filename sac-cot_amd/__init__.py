"""saccot_amd — MI355X-native SAC-COT compatibility-triangle sample-consensus hot path.

The directory is named `sac-cot_amd` (not importable by name); load it with `__graft_entry__.load_package()`,
which registers it as the module `saccot_amd`.
"""
from . import api, corrio, shard, synth  # noqa: F401
from .api import (MultiRegistrar, Registrar, SacCotError, ScParams, ScStats, ScShardPlan, ScPolishParams, ScPolishCand, ScBatchResult, BATCH_RESULT_DTYPE, ScPolishBatchResult, POLISH_BATCH_RESULT_DTYPE, ScPoseInfoResult, POSE_INFO_RESULT_DTYPE, ScPoseInfoParams, SC_POSE_INFO_MAX_POSES, SC_POSE_INFO_SEL_NONE, SC_POSE_INFO_SEL_MASK, SC_POSE_INFO_SEL_LABEL, SC_POSE_INFO_STATUS, make_pose_info_params, ScPolishPosesParams, SC_POLISH_POSES_MAX, SC_POLISH_POSES_SEL_NONE, SC_POLISH_POSES_SEL_MASK, SC_POLISH_POSES_SEL_LABEL, SC_POLISH_POSES_SEL_ALIVE, SC_POLISH_POSES_STATUS, make_polish_poses_params, ScGuideParams, make_guide_params, SC_GUIDE_POSE_STATUS, SC_GUIDE_MAX_POSES, ScSettleParams, make_settle_params, SC_SETTLE_MAX_POSES, SC_SETTLE_BATCH_MAX_POSES, SC_SETTLE_STATUS, ScAssignParams, ScAssignResult, ASSIGN_RESULT_DTYPE, SC_ASSIGN_MAX_POSES, SC_ASSIGN_BATCH_MAX_POSES, SC_ASSIGN_BEST, SC_ASSIGN_FIRST, SC_ASSIGN_SEL_NONE, SC_ASSIGN_SEL_MASK, SC_ASSIGN_STATUS, make_assign_params, SC_POLISH_STOP_FIXED, SC_POLISH_STOP_DECLINED, SC_POLISH_STOP_MAX_ITER, SC_BATCH_MAX_N, SC_MATCH_BATCH_MAX_N, SC_INSTANCES_BATCH_MAX, load_library, make_params, make_polish_params, register, shard_plan,  # noqa: F401
                  SC_AOS, SC_SOA, SC_RANK_WEIGHT, SC_RANK_DEGREE, SC_SCORE_COUNT, SC_SCORE_MSE, SC_SCORE_MAE, SC_FLAG_TIMING, SC_FLAG_EXACT_TOTAL, SC_FLAG_NO_PRUNE, SC_FLAG_REFINE, SC_FLAG_TIMING_HOT, SC_FLAG_NO_DENSE_S, SC_FLAG_TIMING_ONE, SC_TIMING_STAGE, SC_HIST_WORDS, SC_OK, SC_ENOHYP, SC_EINVAL, SC_ERETRY, SC_EBOUND, SC_FLAG_EST_BOUND, SC_FLAG_SHARD_AB)

__all__ = ["api", "corrio", "shard", "synth", "Registrar", "SacCotError", "ScParams", "ScStats", "load_library", "make_params",
           "register"]
