// sc_sync_check.hpp — the host-only rules of sc_pairs_sync (include/saccot.h) that sc_pairs_cycles does not already have: what is
// refused of sc_sync_params, of the two strides and of the anchor, the two thresholds, and where the staged words and the workspace
// areas lie.  The list's rules and the adjacency are sc_cycles_check.hpp's, the pose records every pose entry's
// (sc_pose_check.hpp).  No HIP: sc_capi_sync.hip includes it, and so does tests/native/sync_check_main.cpp, a program of its own
// that runs these functions under the sanitizers on the CPU.
#pragma once
#include "sc_cycles_check.hpp"

namespace sc {

constexpr uint32_t SYNC_ROUNDS_MAX = 256;

inline bool sync_reads_status(const sc_sync_params* sp) { return (sp->flags & SC_SYNC_STATUS) != 0; }

// What a call refuses of its parameter block, of the strides and of the anchor — the rule that is broken, for the caller to put its
// name in front of; nullptr: they are fine.
inline const char* sync_params_error(const sc_sync_params* sp) {
  if (sp->size != sizeof(sc_sync_params)) return "params->size is not sizeof(sc_sync_params)";
  if (sp->max_rounds < 1 || sp->max_rounds > SYNC_ROUNDS_MAX) return "max_rounds must be 1 .. 256";
  if (!(sp->rot_tol >= 0.f && sp->rot_tol <= CYCLES_ROT_TOL_MAX)) return "rot_tol must be finite and in [0, pi]";
  if (!(sp->trans_tol >= 0.f && sp->trans_tol < INFINITY)) return "trans_tol must be finite and >= 0";
  if ((sp->flags & ~SC_SYNC_STATUS) || sp->reserved[0] || sp->reserved[1]) return "an unknown flag, or a reserved field that is not 0";
  return nullptr;
}
inline const char* sync_stride_error(const sc_sync_params* sp, uint32_t pose_stride, bool has_use, uint32_t use_stride) {
  if (!pose_stride_ok(pose_stride, sync_reads_status(sp))) return "pose_stride must be a multiple of 4 and at least 48 (52 with SC_SYNC_STATUS)";
  if (has_use && (use_stride < 4 || use_stride % 4 != 0)) return "use_stride must be a multiple of 4 and at least 4";
  return nullptr;
}
inline const char* sync_anchor_error(const sc_sync_params* sp, uint32_t n_sets) {
  if (sp->anchor >= n_sets) return "anchor must be less than n_sets";
  return nullptr;
}

// The two thresholds a call uses (of parameters that sync_params_error accepts): r2_max, e2_max.  The first is on the squared
// Frobenius distance of two rotations, 2 theta^2 to first order — not on a trace: 1 + 2 cos(rot_tol) is exactly 3.0 below 2e-8.
inline void sync_thresholds(const sc_sync_params* sp, double out[2]) {
  out[0] = 2.0 * (double)sp->rot_tol * (double)sp->rot_tol;
  out[1] = (double)sp->trans_tol * (double)sp->trans_tol;
}

// Bytes of the use array a call reads: a word at byte p * use_stride.
inline uint64_t sync_use_bytes_read(uint64_t n_pairs, uint32_t use_stride) { return n_pairs == 0 ? 0 : (n_pairs - 1) * use_stride + 4; }

// ---- what a call stages for the device: the pairs' records and the entries as sc_pairs_cycles stages them, then the n_sets + 1
// list starts (the records and the entries are multiples of 8 bytes: the starts are aligned).
inline uint64_t sync_off_at(uint32_t n_pairs, uint64_t n_entries) { return cycles_meta_bytes(n_pairs, n_entries); }
inline uint64_t sync_meta_bytes(uint32_t n_sets, uint32_t n_pairs, uint64_t n_entries) { return sync_off_at(n_pairs, n_entries) + 4 * ((uint64_t)n_sets + 1); }

// ---- the device workspace behind the staged words.  wide: the oriented fp64 poses, 192 bytes a pair, then a double a pair — its
// weight, 0.0 where it is not usable.  state: the round words (SyncCtl, sc_kernels.hpp) in SYNC_CTL_BYTES, then the two buffers of
// the sets' states (SYNC_STATE_BYTES a set each), then what a set's wave keeps about it (SYNC_INFO_BYTES a set).
constexpr uint32_t SYNC_CTL_BYTES = 2048;
constexpr uint32_t SYNC_STATE_BYTES = 104;
constexpr uint32_t SYNC_INFO_BYTES = 16;
inline uint64_t sync_weight_at(uint32_t n_pairs) { return cycles_pose_bytes(n_pairs); }
inline uint64_t sync_wide_bytes(uint32_t n_pairs) { return sync_weight_at(n_pairs) + 8 * (uint64_t)n_pairs; }
inline uint64_t sync_info_at(uint32_t n_sets) { return SYNC_CTL_BYTES + 2 * (uint64_t)SYNC_STATE_BYTES * n_sets; }
inline uint64_t sync_state_bytes(uint32_t n_sets) { return sync_info_at(n_sets) + (uint64_t)SYNC_INFO_BYTES * n_sets; }

}  // namespace sc
