// sc_pose_check.hpp — the host-only rules of a caller's pose records, said once for every entry that takes them (sc_pose_info_batch,
// sc_pose_info_frame, sc_polish_poses, sc_assign_poses, sc_settle_poses, and the guides of sc_match_guided_batch / _poses): what a
// record holds, which strides are accepted, how many bytes of the array a call reads, and where a record of a batch form sits.
// Behind them the parameter rules of the two entries that have no check header of their own: sc_polish_poses and
// sc_pose_info_frame.  No HIP: the sc_capi_* files include it, and so do the programs under tests/native, which run these functions
// under the sanitizers on the CPU (pose_check_main.cpp walks this file).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/saccot.h"

namespace sc {

// A pose record: float Rt[12] at byte 0 and — where the entry reads it — an int32 status at byte 48.  Records lie pose_stride bytes
// apart; whatever else a record holds is never read.
constexpr uint32_t POSE_RT_BYTES = 48;
constexpr uint32_t POSE_STATUS_BYTES = 52;  // ... with the status behind it
constexpr uint32_t pose_record_bytes(bool reads_status) { return reads_status ? POSE_STATUS_BYTES : POSE_RT_BYTES; }

// The stride: a multiple of 4 that holds what is read of a record.
inline bool pose_stride_ok(uint32_t pose_stride, bool reads_status) {
  return pose_stride >= pose_record_bytes(reads_status) && pose_stride % 4 == 0;
}
// Bytes of the pose array a call reads: nothing behind the last record's last word that is read.  n_records: n_poses (a frame
// form), n_problems, or n_poses x n_problems.
inline uint64_t pose_bytes_read(uint64_t n_records, uint32_t pose_stride, bool reads_status) {
  return n_records == 0 ? 0 : (n_records - 1) * pose_stride + pose_record_bytes(reads_status);
}
// Motion-major: record (pose k, problem b) of n_problems problems — the index of an output record, and with the stride the byte a
// pose record starts at.  64 bits: 64 x 2^31 / 3 records of 2^32 - 4 bytes do not fit 32.
inline uint64_t pose_record_index(uint32_t k, uint32_t b, uint32_t n_problems) { return (uint64_t)k * n_problems + b; }
inline uint64_t pose_record_offset(uint32_t k, uint32_t b, uint32_t n_problems, uint32_t pose_stride) {
  return pose_record_index(k, b, n_problems) * pose_stride;
}

// ---- sc_polish_poses.  What a call refuses of its parameter block, the stride and n_poses — the rule that is broken, for the caller
// to put its name in front of; nullptr: they are fine.  has_sel: the caller gave a selection.
inline bool polish_poses_reads_status(const sc_polish_poses_params* qp) { return (qp->flags & SC_POLISH_POSES_STATUS) != 0; }
inline bool polish_poses_reads_sel(uint32_t sel_mode) { return sel_mode != SC_POLISH_POSES_SEL_NONE; }
inline bool polish_poses_sel_is_label(uint32_t sel_mode) { return sel_mode == SC_POLISH_POSES_SEL_LABEL || sel_mode == SC_POLISH_POSES_SEL_ALIVE; }
inline const char* polish_poses_params_error(const sc_polish_poses_params* qp, uint32_t pose_stride, uint32_t n_poses, bool has_sel) {
  if (qp->size != sizeof(sc_polish_poses_params)) return "params->size is not sizeof(sc_polish_poses_params)";
  if (qp->max_iter < 1 || qp->max_iter > 64) return "max_iter must be 1 .. 64";
  if (qp->sel_mode > SC_POLISH_POSES_SEL_ALIVE) return "sel_mode must be SC_POLISH_POSES_SEL_NONE, _MASK, _LABEL or _ALIVE";
  if (polish_poses_reads_sel(qp->sel_mode) && !has_sel) return "sel is NULL with a sel_mode that reads it";
  if (qp->label0 != 0 && !polish_poses_sel_is_label(qp->sel_mode)) return "label0 must be 0 unless sel_mode is SC_POLISH_POSES_SEL_LABEL or _ALIVE";
  if ((qp->flags & ~SC_POLISH_POSES_STATUS) || qp->reserved[0] || qp->reserved[1] || qp->reserved[2])
    return "an unknown flag, or a reserved field that is not 0";
  if (n_poses < 1 || n_poses > SC_POLISH_POSES_MAX) return "n_poses must be 1 .. SC_POLISH_POSES_MAX";
  if (!pose_stride_ok(pose_stride, polish_poses_reads_status(qp)))
    return "pose_stride must be a multiple of 4 and at least 48 (52 with SC_POLISH_POSES_STATUS)";
  return nullptr;
}

// ---- sc_pose_info_frame, the same way.
inline bool pose_info_reads_status(const sc_pose_info_params* ip) { return (ip->flags & SC_POSE_INFO_STATUS) != 0; }
inline const char* pose_info_params_error(const sc_pose_info_params* ip, uint32_t pose_stride, uint32_t n_poses, bool has_sel) {
  if (ip->size != sizeof(sc_pose_info_params)) return "params->size is not sizeof(sc_pose_info_params)";
  if (ip->sel_mode > SC_POSE_INFO_SEL_LABEL) return "sel_mode must be SC_POSE_INFO_SEL_NONE, _MASK or _LABEL";
  if (ip->sel_mode != SC_POSE_INFO_SEL_NONE && !has_sel) return "sel is NULL with a sel_mode that reads it";
  if (ip->label0 != 0 && ip->sel_mode != SC_POSE_INFO_SEL_LABEL) return "label0 must be 0 unless sel_mode is SC_POSE_INFO_SEL_LABEL";
  if ((ip->flags & ~SC_POSE_INFO_STATUS) || ip->reserved[0] || ip->reserved[1] || ip->reserved[2] || ip->reserved[3])
    return "an unknown flag, or a reserved field that is not 0";
  if (n_poses < 1 || n_poses > SC_POSE_INFO_MAX_POSES) return "n_poses must be 1 .. SC_POSE_INFO_MAX_POSES";
  if (!pose_stride_ok(pose_stride, pose_info_reads_status(ip)))
    return "pose_stride must be a multiple of 4 and at least 48 (52 with SC_POSE_INFO_STATUS)";
  return nullptr;
}

}  // namespace sc
