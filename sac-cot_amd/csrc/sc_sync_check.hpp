// sc_sync_check.hpp — the host-only rules of sc_pairs_sync (include/saccot.h) that sc_pairs_cycles does not already have: what is
// refused of sc_sync_params, of the two strides and of the anchor, the two thresholds, and where the workspace areas lie.  The
// list's rules, the adjacency, the staged image and the rules every pair-list entry shares are sc_cycles_check.hpp's, the pose
// records every pose entry's (sc_pose_check.hpp).  No HIP: sc_capi_sync.hip includes it, and so does
// tests/native/sync_check_main.cpp, a program of its own that runs these functions under the sanitizers on the CPU.
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
  if (const char* what = pairs_tol_error(sp->rot_tol, sp->trans_tol)) return what;
  if ((sp->flags & ~SC_SYNC_STATUS) || sp->reserved[0] || sp->reserved[1]) return "an unknown flag, or a reserved field that is not 0";
  return nullptr;
}
inline const char* sync_stride_error(const sc_sync_params* sp, uint32_t pose_stride, bool has_use, uint32_t use_stride) {
  if (!pose_stride_ok(pose_stride, sync_reads_status(sp))) return "pose_stride must be a multiple of 4 and at least 48 (52 with SC_SYNC_STATUS)";
  return pairs_use_stride_error(has_use, use_stride);
}
inline const char* sync_anchor_error(const sc_sync_params* sp, uint32_t n_sets) { return pairs_anchor_error(sp->anchor, n_sets); }

// The two thresholds a call uses (of parameters that sync_params_error accepts): r2_max, e2_max.
inline void sync_thresholds(const sc_sync_params* sp, double out[2]) {
  out[0] = pairs_r2_max(sp->rot_tol);
  out[1] = pairs_e2_max(sp->trans_tol);
}

// Bytes of the use array a call reads: a word at byte p * use_stride.
inline uint64_t sync_use_bytes_read(uint64_t n_pairs, uint32_t use_stride) { return n_pairs == 0 ? 0 : (n_pairs - 1) * use_stride + 4; }

// ---- the device workspace behind the staged image (sync_meta_bytes of it: sc_cycles_check.hpp).  wide: the oriented fp64 poses, 192 bytes a pair, then a double a pair — its
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
