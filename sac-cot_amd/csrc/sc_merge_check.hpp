// sc_merge_check.hpp — the host-only rules of sc_merge_poses (include/saccot.h): what is refused of sc_merge_params, of the stride
// and of n_poses, and how many words the frame form's bit rows take.  The pose records are every pose entry's: where a record sits
// and what of it is read is sc_pose_check.hpp's.  No HIP: sc_capi_merge.hip includes it, and so does
// tests/native/merge_check_main.cpp, a program of its own that runs these functions under the sanitizers on the CPU.
#pragma once
#include "sc_pose_check.hpp"

namespace sc {

constexpr uint32_t MERGE_DEN_MAX = 65536u;

// Does the call read the status at byte 48?  The frame form with the flag; the batch form always (as sc_assign_poses_batch).
inline bool merge_reads_status(const sc_merge_params* mp, bool batch) { return batch || (mp->flags & SC_MERGE_STATUS) != 0; }

// What a call refuses of its parameter block, the stride and n_poses — the rule that is broken, for the caller to put its name in
// front of; nullptr: they are fine.  has_sel: the caller gave a selection (the frame form; the batch form has none to give).
inline const char* merge_params_error(const sc_merge_params* mp, uint32_t pose_stride, uint32_t n_poses, bool batch, bool has_sel) {
  if (mp->size != sizeof(sc_merge_params)) return "params->size is not sizeof(sc_merge_params)";
  if (mp->measure > SC_MERGE_OVER_UNION) return "measure must be SC_MERGE_OVER_MIN or SC_MERGE_OVER_UNION";
  if (mp->num < 1 || mp->num > mp->den || mp->den > MERGE_DEN_MAX) return "num and den must keep 1 <= num <= den <= 65536";
  if (mp->sel_mode > SC_ASSIGN_SEL_MASK) return "sel_mode must be SC_ASSIGN_SEL_NONE or SC_ASSIGN_SEL_MASK";
  if (batch && mp->sel_mode != SC_ASSIGN_SEL_NONE) return "sel_mode must be SC_ASSIGN_SEL_NONE in the batch form";
  if (mp->sel_mode == SC_ASSIGN_SEL_MASK && !has_sel) return "sel is NULL with SC_ASSIGN_SEL_MASK";
  if ((mp->flags & ~(SC_MERGE_STATUS | SC_MERGE_COMPACT)) || mp->reserved[0]) return "an unknown flag, or a reserved field that is not 0";
  if (batch) {
    if (n_poses < 1 || n_poses > SC_MERGE_BATCH_MAX_POSES) return "n_poses must be 1 .. SC_MERGE_BATCH_MAX_POSES";
    if (!pose_stride_ok(pose_stride, true)) return "pose_stride must be a multiple of 4 and at least 52";
  } else {
    if (n_poses < 1 || n_poses > SC_MERGE_MAX_POSES) return "n_poses must be 1 .. SC_MERGE_MAX_POSES";
    if (!pose_stride_ok(pose_stride, merge_reads_status(mp, false)))
      return "pose_stride must be a multiple of 4 and at least 48 (52 with SC_MERGE_STATUS)";
  }
  return nullptr;
}

// The frame form's scratch: the bit rows, n_poses x ceil(n / 64) u64, and behind them the tally words, 2 x n_poses u32.
inline uint64_t merge_row_words_of(uint64_t n) { return (n + 63) / 64; }
inline uint64_t merge_rows_bytes(uint64_t n, uint32_t n_poses) { return (uint64_t)n_poses * merge_row_words_of(n) * 8; }
inline uint64_t merge_scratch_bytes(uint64_t n, uint32_t n_poses) { return merge_rows_bytes(n, n_poses) + (uint64_t)n_poses * 8; }
inline uint64_t merge_table_bytes(uint32_t n_poses) { return (uint64_t)n_poses * n_poses * 4; }

}  // namespace sc
