// sc_assign.hpp — what the two kernels of sc_assign_poses share (include/saccot.h; sc_assign_frame.hip, sc_assign_batch.hip), once
// each: how a pose record reaches LDS and what makes it valid, the selection, the per-correspondence best-of-K step of either mode,
// the score term of a residual that is already there, and the LDS tallies.
//
// An INVALID pose — a status other than SC_OK where one is read, a non-finite Rt — is staged as twelve NaNs: every fused
// multiply-add of the canonical chain then carries a NaN into d2, and the candidate test is a float '<', which a NaN never passes.
// The loop over the poses therefore holds no validity branch, and "an invalid pose claims nothing" is a property of the arithmetic.
#pragma once
#include "../../include/saccot.h"
#include "sc_arith.hpp"
#include "sc_winner.hpp"

namespace sc {

// 512, two correspondences a lane: measured against 256 and 1024 — a frame of 5 000 to 20 000 correspondences
// leaves most SIMDs idle, so the call takes as long as ONE wave needs for its K poses, and that grows with what a lane owns.
constexpr int ASSIGN_TILE = 512;     // correspondences of one workgroup of assign_frame_kernel: one tile per workgroup, no grid stride
constexpr int ASSIGN_THREADS = 256;  // its threads: four waves, a lane owns ASSIGN_TILE / ASSIGN_THREADS correspondences
constexpr int ASSIGN_POSE_FLOATS = 12;
constexpr uint32_t ASSIGN_NO_D2 = 0x7F800000u;  // the d2 output of a correspondence without a label: +inf

// Lane t stages pose record `rec` into Rt (LDS, 12 floats) and returns the record's status word: the one at byte 48 passed through
// if it is read and not SC_OK, SC_EINVAL for a non-finite Rt, else SC_OK.  One lane per pose: twelve dwords of one record.
__device__ __forceinline__ int assign_stage_pose(const void* rec, bool reads_status, float* Rt) {
  const uint32_t* const w = static_cast<const uint32_t*>(rec);
  float M[ASSIGN_POSE_FLOATS];
#pragma unroll
  for (int c = 0; c < ASSIGN_POSE_FLOATS; c++) M[c] = __uint_as_float(w[c]);
  int status = reads_status ? (int)w[12] : SC_OK;  // (without the flag nothing past byte 47 is read)
  if (status == SC_OK && !finite12(M)) status = SC_EINVAL;
#pragma unroll
  for (int c = 0; c < ASSIGN_POSE_FLOATS; c++) Rt[c] = status == SC_OK ? M[c] : __builtin_nanf("");
  return status;
}

// part(m): SC_ASSIGN_SEL_NONE (sel == nullptr) or SC_ASSIGN_SEL_MASK
__device__ __forceinline__ bool assign_part(const uint8_t* __restrict__ sel, int m) { return sel == nullptr || sel[m] != 0; }

// One correspondence's running choice among the poses seen so far.
struct Assigned {
  int label;  // -1: no candidate yet
  float d2;   // the residual under `label` (+inf without one)
};
__device__ __forceinline__ Assigned assign_none() { return Assigned{-1, __uint_as_float(ASSIGN_NO_D2)}; }

// Pose k (M: its twelve floats, NaN if invalid) against correspondence c that takes part: the step of either mode.  BEST: a strictly
// smaller residual takes the label, so ties stay with the lowest k; a.d2 starts at +inf and d2 < tau2 is finite, so the first
// candidate always takes it.  FIRST: only a correspondence without a label looks.
template <uint32_t MODE>
__device__ __forceinline__ void assign_step(Assigned& a, const float* M, const Corr& c, bool part, float tau2, int k) {
  const float d2 = resid2(M, c.v[0], c.v[1], c.v[2], c.v[3], c.v[4], c.v[5]);
  const bool cand = part && d2 < tau2;
  const bool take = MODE == SC_ASSIGN_BEST ? (cand && d2 < a.d2) : (cand && a.label < 0);
  a.label = take ? k : a.label;
  a.d2 = take ? d2 : a.d2;
}

// score_term's value (sc_arith.hpp) for a residual d2 < tau^2 that is already computed: the labelled correspondence's term.
__device__ __forceinline__ uint32_t assign_score(float d2, float thr, int mode) {
  if (mode == 0) return 1u;
  const float x = mode == 1 ? d2 : sqrt_rn(d2);
  return (uint32_t)(fmaxf(fma_(-x, thr, 1.0f), 0.0f) * 1024.0f);
}

// A pose's tally inside one workgroup: LDS atomics on integers (any order).  A workgroup holds at most ASSIGN_TILE correspondences
// of at most 1024 score units each: 32 bits are plenty.
__device__ __forceinline__ void assign_tally(uint32_t* cnt, uint32_t* score, const Assigned& a, float thr, int score_mode) {
  if (a.label < 0) return;
  atomicAdd(&cnt[a.label], 1u);
  if (score_mode != 0) atomicAdd(&score[a.label], assign_score(a.d2, thr, score_mode));
}

}  // namespace sc
