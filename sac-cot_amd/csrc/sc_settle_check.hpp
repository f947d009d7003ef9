// sc_settle_check.hpp — the host-only rules of sc_settle_poses (include/saccot.h): what is refused of sc_settle_params, of the stride
// and of n_poses, and how many bytes of the pose array a call reads.  The pose records are every pose entry's: where a record sits
// and what of it is read is sc_pose_check.hpp's.  No HIP: sc_capi_settle.hip includes it, and so does
// tests/native/settle_check_main.cpp, a program of its own that runs these functions under the sanitizers on the CPU.
#pragma once
#include "sc_pose_check.hpp"

namespace sc {

// Does the call read the status at byte 48?  The frame form with the flag; the batch form always (as sc_assign_poses_batch).
inline bool settle_reads_status(const sc_settle_params* sp, bool batch) { return batch || (sp->flags & SC_SETTLE_STATUS) != 0; }

// What a call refuses of its parameter block, the stride and n_poses — the rule that is broken, for the caller to put its name in
// front of; nullptr: they are fine.  has_sel: the caller gave a selection (the frame form; the batch form has none to give).
inline const char* settle_params_error(const sc_settle_params* sp, uint32_t pose_stride, uint32_t n_poses, bool batch, bool has_sel) {
  if (sp->size != sizeof(sc_settle_params)) return "params->size is not sizeof(sc_settle_params)";
  if (sp->max_iter < 1 || sp->max_iter > 64) return "max_iter must be 1 .. 64";
  if (sp->sel_mode > SC_ASSIGN_SEL_MASK) return "sel_mode must be SC_ASSIGN_SEL_NONE or SC_ASSIGN_SEL_MASK";
  if (batch && sp->sel_mode != SC_ASSIGN_SEL_NONE) return "sel_mode must be SC_ASSIGN_SEL_NONE in the batch form";
  if (sp->sel_mode == SC_ASSIGN_SEL_MASK && !has_sel) return "sel is NULL with SC_ASSIGN_SEL_MASK";
  if ((sp->flags & ~SC_SETTLE_STATUS) || sp->reserved[0] || sp->reserved[1] || sp->reserved[2] || sp->reserved[3])
    return "an unknown flag, or a reserved field that is not 0";
  if (batch) {
    if (n_poses < 1 || n_poses > SC_SETTLE_BATCH_MAX_POSES) return "n_poses must be 1 .. SC_SETTLE_BATCH_MAX_POSES";
    if (!pose_stride_ok(pose_stride, true)) return "pose_stride must be a multiple of 4 and at least 52";
  } else {
    if (n_poses < 1 || n_poses > SC_SETTLE_MAX_POSES) return "n_poses must be 1 .. SC_SETTLE_MAX_POSES";
    if (!pose_stride_ok(pose_stride, settle_reads_status(sp, false)))
      return "pose_stride must be a multiple of 4 and at least 48 (52 with SC_SETTLE_STATUS)";
  }
  return nullptr;
}

}  // namespace sc
