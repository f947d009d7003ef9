// sc_match_guided_batch_check.hpp — the host-only rules of sc_match_guided_batch (include/saccot.h) that are not sc_match_guided's:
// the guide block with the one flag these entries know, and the stride of the pose records.  No HIP:
// sc_capi_match_guided_batch.hip includes it, and so does tests/native/match_guided_batch_check_main.cpp, a program of its own that
// runs these functions under the sanitizers on the CPU.
#pragma once
#include "sc_match_guided_check.hpp"
#include "sc_pose_check.hpp"

namespace sc {

// What a batch or pairs call refuses of its guide block: every rule of guide_params_error, but that flags may be
// SC_GUIDE_POSE_STATUS.  The rule that is broken, for the caller to put its name in front of; nullptr: it is fine.
inline const char* guide_batch_params_error(const sc_guide_params* gp) {
  if (gp->size != sizeof(sc_guide_params)) return guide_params_error(gp);  // (nothing behind a wrong size is looked at)
  if (gp->flags & ~SC_GUIDE_POSE_STATUS) return "guide->flags: SC_GUIDE_POSE_STATUS is the only flag";
  sc_guide_params plain = *gp;
  plain.flags = 0;
  return guide_params_error(&plain);
}

// The pose records (sc_pose_check.hpp), the status read with SC_GUIDE_POSE_STATUS: which part of the stride rule is broken.
inline const char* guide_pose_stride_error(uint32_t flags, uint32_t pose_stride) {
  if (pose_stride % 4u != 0u) return "pose_stride must be a multiple of 4";
  if (pose_stride < POSE_RT_BYTES) return "pose_stride must be at least 48 (float Rt[12])";
  if (!pose_stride_ok(pose_stride, (flags & SC_GUIDE_POSE_STATUS) != 0)) return "pose_stride must be at least 52 with SC_GUIDE_POSE_STATUS (the status at byte 48)";
  return nullptr;
}

}  // namespace sc
