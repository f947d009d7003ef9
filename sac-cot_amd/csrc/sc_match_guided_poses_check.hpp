// sc_match_guided_poses_check.hpp — the host-only rules of sc_match_guided_poses (include/saccot.h) that are not sc_match_guided's:
// the guide block with the one flag these entries know, the stride of the pose records (both said once, in
// sc_match_guided_batch_check.hpp) and the number of records.  No HIP: sc_capi_match_guided_poses.hip includes it, and so does
// tests/native/match_guided_poses_check_main.cpp, a program of its own that runs these functions under the sanitizers on the CPU.
#pragma once
#include "sc_match_guided_batch_check.hpp"

namespace sc {

// What a several-pose call refuses of its guide block, its stride and its count, in that order — the rule that is broken, for the
// caller to put its name in front of; nullptr: they are fine.  Nothing behind a wrong guide->size is looked at.
inline const char* guide_poses_error(const sc_guide_params* gp, uint32_t pose_stride, uint32_t n_poses) {
  if (const char* why = guide_batch_params_error(gp)) return why;
  if (const char* why = guide_pose_stride_error(gp->flags, pose_stride)) return why;
  if (n_poses < 1u || n_poses > SC_GUIDE_MAX_POSES) return "n_poses must be 1 .. SC_GUIDE_MAX_POSES (64)";
  return nullptr;
}

}  // namespace sc
