// sc_assign_check.hpp — the host-only rules of sc_assign_poses (include/saccot.h): what is refused of sc_assign_params, of the stride
// and of n_poses, where a pose record and an output record of the batch form sit, and how many bytes of the pose array a call reads.
// No HIP: sc_capi_assign.hip includes it, and so does tests/native/assign_check_main.cpp, a program of its own that runs these
// functions under the sanitizers on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/saccot.h"

namespace sc {

constexpr uint32_t ASSIGN_POSE_BYTES = 48;    // float Rt[12]
constexpr uint32_t ASSIGN_STATUS_BYTES = 52;  // ... and the int32 status behind it

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
    if (pose_stride < ASSIGN_STATUS_BYTES || pose_stride % 4 != 0) return "pose_stride must be a multiple of 4 and at least 52";
  } else {
    if (n_poses < 1 || n_poses > SC_ASSIGN_MAX_POSES) return "n_poses must be 1 .. SC_ASSIGN_MAX_POSES";
    const uint32_t least = assign_reads_status(ap, false) ? ASSIGN_STATUS_BYTES : ASSIGN_POSE_BYTES;
    if (pose_stride < least || pose_stride % 4 != 0)
      return "pose_stride must be a multiple of 4 and at least 48 (52 with SC_ASSIGN_STATUS)";
  }
  return nullptr;
}

// Motion-major: record (pose k, problem b) of n_problems problems — the index of an output record, and with the stride the byte a
// pose record starts at.  64 bits: 64 x 2^31 / 3 records of 2^32 - 4 bytes do not fit 32.
inline uint64_t assign_record_index(uint32_t k, uint32_t b, uint32_t n_problems) { return (uint64_t)k * n_problems + b; }
inline uint64_t assign_pose_offset(uint32_t k, uint32_t b, uint32_t n_problems, uint32_t pose_stride) {
  return assign_record_index(k, b, n_problems) * pose_stride;
}
// Bytes of the pose array a call reads: nothing behind the last record's last word that is read.  n_records: n_poses (the frame
// form) or n_poses x n_problems.
inline uint64_t assign_pose_bytes(uint64_t n_records, uint32_t pose_stride, bool reads_status) {
  return n_records == 0 ? 0 : (n_records - 1) * pose_stride + (reads_status ? ASSIGN_STATUS_BYTES : ASSIGN_POSE_BYTES);
}

}  // namespace sc
