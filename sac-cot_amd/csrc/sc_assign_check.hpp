// sc_assign_check.hpp — the host-only rules of sc_assign_poses (include/saccot.h): what is refused of sc_assign_params, of the stride
// and of n_poses.  What a pose record holds, where a record of the batch form sits and how many bytes of the pose array a call reads
// is sc_pose_check.hpp's.  No HIP: sc_capi_assign.hip includes it, and so does tests/native/assign_check_main.cpp, a program of its
// own that runs these functions under the sanitizers on the CPU.
#pragma once
#include "sc_pose_check.hpp"

namespace sc {

// Does the call read the status at byte 48?  The frame form with the flag; the batch form always (as sc_pose_info_batch).
inline bool assign_reads_status(const sc_assign_params* ap, bool batch) { return batch || (ap->flags & SC_ASSIGN_STATUS) != 0; }

// What a call refuses of its parameter block, the stride and n_poses — the rule that is broken, for the caller to put its name in
// front of; nullptr: they are fine.  has_sel: the caller gave a selection (the frame form; the batch form has none to give).
inline const char* assign_params_error(const sc_assign_params* ap, uint32_t pose_stride, uint32_t n_poses, bool batch, bool has_sel) {
  if (ap->size != sizeof(sc_assign_params)) return "params->size is not sizeof(sc_assign_params)";
  if (ap->mode > SC_ASSIGN_FIRST) return "mode must be SC_ASSIGN_BEST or SC_ASSIGN_FIRST";
  if (ap->sel_mode > SC_ASSIGN_SEL_MASK) return "sel_mode must be SC_ASSIGN_SEL_NONE or SC_ASSIGN_SEL_MASK";
  if (batch && ap->sel_mode != SC_ASSIGN_SEL_NONE) return "sel_mode must be SC_ASSIGN_SEL_NONE in the batch form";
  if (ap->sel_mode == SC_ASSIGN_SEL_MASK && !has_sel) return "sel is NULL with SC_ASSIGN_SEL_MASK";
  if ((ap->flags & ~SC_ASSIGN_STATUS) || ap->reserved[0] || ap->reserved[1] || ap->reserved[2] || ap->reserved[3])
    return "an unknown flag, or a reserved field that is not 0";
  if (batch) {
    if (n_poses < 1 || n_poses > SC_ASSIGN_BATCH_MAX_POSES) return "n_poses must be 1 .. SC_ASSIGN_BATCH_MAX_POSES";
    if (!pose_stride_ok(pose_stride, true)) return "pose_stride must be a multiple of 4 and at least 52";
  } else {
    if (n_poses < 1 || n_poses > SC_ASSIGN_MAX_POSES) return "n_poses must be 1 .. SC_ASSIGN_MAX_POSES";
    if (!pose_stride_ok(pose_stride, assign_reads_status(ap, false)))
      return "pose_stride must be a multiple of 4 and at least 48 (52 with SC_ASSIGN_STATUS)";
  }
  return nullptr;
}

}  // namespace sc
