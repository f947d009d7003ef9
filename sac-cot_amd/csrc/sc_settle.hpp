// sc_settle.hpp — the round of sc_settle_poses (include/saccot.h), said once for its two kernels: settle_frame_kernel
// (sc_settle_frame.hip: a scored frame, planes and chunk scratch in global memory, ONE workgroup of 1024 threads) and
// settle_batch_kernel (sc_settle_batch.hip: a batch problem, everything in LDS, 256 threads).  A round is
//
//   label      sc_assign_poses's BEST step (assign_step, sc_assign.hpp) over the K poses in LDS.  A wave owns whole chunks of 64
//              consecutive ORIGINAL indices, so the member bits of pose k in a chunk are ONE ballot of "my label is k": the round
//              never reads a label back.  The label (and d2) of every pass is stored; the last pass's stores are the output.
//   refit      sc_polish_poses's single refit of EVERY pose over its own label, all poses sharing the round's barriers: the lanes
//              are dealt over (pose, chunk, component) for pass 1 and pass 2, over (pose, component) for the chunk-order sums, one
//              lane per pose for the centroids and the solve.  The fp64 chains are sc_refit.hpp's — refit_chain1, refit_centroids,
//              refit_chain2, refit_chunk_sum, refit_solve, the functions refit_iterate itself is made of — so a round equals
//              sc_assign_poses(BEST) followed by sc_polish_poses(SEL_LABEL, max_iter 1) bit for bit: a BEST label k implies
//              d2_k < tau^2, so "inlier of pose k AND labelled k" is "labelled k".
//   stop       no pose changed its bits (one __syncthreads_or): SC_POLISH_STOP_FIXED, the round is not counted.
//
// Nothing here waits for another workgroup.  Every loop is bounded by max_iter, K, n.
//
// Where the bit words and chunk sums live is the kernel's: a storage policy `Chunks` with
//   double& sum(int k, int ch, int slot)    slot of chunk ch of pose k (pass 1 writes slots < 7, pass 2 slots < 9)
//   uint64_t& bits(int k, int ch)           the 64 member bits of pose k in chunk ch
//   void publish()                          before a barrier behind which other lanes read what this one stored
// A (pose, chunk) without a member bit costs its lanes the load of the word and the store of a zero.
//
// The scores: in the inlier-count mode a pose's tally is its member count, which pass 1 sums anyway (S[k][0]); in the other modes
// the FIRST labelling (score0) and the LAST (score) are walked once more — a lane re-reads the labels it stored itself and adds the
// term of the labelled pose's residual into the pose's LDS word (integers: any order).
#pragma once
#include "../../include/saccot.h"
#include "sc_arith.hpp"
#include "sc_assign.hpp"
#include "sc_refit.hpp"
#include "sc_winner.hpp"

namespace sc {

constexpr int SETTLE_REC_WORDS = 16;  // sc_polish_batch_result in dwords

// The K poses of a workgroup and what a round keeps per pose: LDS.  KMAX = 64: 16 064 bytes; KMAX = 16: 4 016 (the compiler reports
// 256 bytes more of static LDS for either kernel).
template <int KMAX>
struct alignas(16) SettleState {
  float Rt[KMAX][ASSIGN_POSE_FLOATS];  // the current poses; NaN: an invalid pose (sc_assign.hpp)
  double S[KMAX][8];                   // pass 1's sums over the chunks ([7] unused)
  double H[KMAX][9];                   // pass 2's
  double C[KMAX][6];                   // the centroids pc, qc
  uint32_t cnt[KMAX];                  // members under the last labelling
  uint32_t score0[KMAX], score[KMAX];  // the tallies under (P_0, L_1) and under the final poses and labels
  int32_t st[KMAX];                    // the record's status word
  uint16_t iters[KMAX];                // counted rounds in which the pose's bits changed
  uint8_t declined[KMAX];              // the refit of the last executed round was declined
};

// What a workgroup settles: planes of n correspondences (ld floats apart), K poses staged in the state, the selection (nullptr:
// every index), and where the labels (n int32) and residuals (n floats or nullptr) go.
struct SettleIn {
  const float* planes;
  int ld, n, K;
  const uint8_t* sel;
  float tau2, thr;
  int score_mode;
  uint32_t max_iter;
  int32_t* label;
  float* d2;
};
struct Settled { uint32_t rounds, stop; };  // counted rounds; SC_POLISH_STOP_FIXED or _MAX_ITER

// Lane k stages pose record `rec` and clears what the rounds keep for it (the caller's barrier publishes it).
template <int KMAX>
__device__ __forceinline__ void settle_stage_pose(SettleState<KMAX>& L, int k, const void* rec, bool reads_status) {
  L.st[k] = assign_stage_pose(rec, reads_status, L.Rt[k]);
  L.cnt[k] = 0u; L.score0[k] = 0u; L.score[k] = 0u;
  L.iters[k] = 0; L.declined[k] = 1;
}

// BEST labels under the poses in L: label / d2 stored, the member bits of every (pose, chunk) written.  A wave owns U chunks a trip:
// their residual chains run side by side.
template <int THREADS, int KMAX, class Chunks>
__device__ __forceinline__ void settle_label(const SettleIn& in, const SettleState<KMAX>& L, Chunks ck) {
  constexpr int W = THREADS / 64, U = 2;
  const int lane = threadIdx.x & 63;
  const int nch = (in.n + 63) / 64;
  for (int ch0 = threadIdx.x >> 6; ch0 < nch; ch0 += U * W) {  // (uniform within a wave)
    Corr c[U];
    bool part[U];
    Assigned a[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int ch = ch0 + u * W, m = ch * 64 + lane;
      const bool live = ch < nch && m < in.n;
      c[u] = live ? load_corr(in.planes, in.ld, m) : Corr{};
      part[u] = live && assign_part(in.sel, m);
      a[u] = assign_none();
    }
    for (int k = 0; k < in.K; k++) {
      const float4* const p4 = reinterpret_cast<const float4*>(L.Rt[k]);
      const float4 r0 = p4[0], r1 = p4[1], r2 = p4[2];
      const float M[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
#pragma unroll
      for (int u = 0; u < U; u++) assign_step<SC_ASSIGN_BEST>(a[u], M, c[u], part[u], in.tau2, k);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int ch = ch0 + u * W, m = ch * 64 + lane;
      if (ch >= nch) continue;  // (uniform)
      if (m < in.n) {
        in.label[m] = a[u].label;
        if (in.d2) in.d2[m] = a[u].d2;
      }
      unsigned long long mine = 0ull;
      for (int k = 0; k < in.K; k++) {
        const unsigned long long bal = __ballot(a[u].label == k);
        mine = lane == k ? bal : mine;
      }
      if (lane < in.K) ck.bits(lane, ch) = mine;
    }
  }
}

// The score terms of the labels this thread stored in settle_label (m = threadIdx.x + i * THREADS is the same deal), under the
// poses in L, added into acc[label]: LDS atomics on integers.  The residual is assign_step's, recomputed: the same chain, the same bits.
template <int THREADS, int KMAX>
__device__ __forceinline__ void settle_scores(const SettleIn& in, const SettleState<KMAX>& L, uint32_t* acc) {
  for (int m = threadIdx.x; m < in.n; m += THREADS) {
    const int lab = in.label[m];
    if (lab < 0) continue;
    const Corr c = load_corr(in.planes, in.ld, m);
    const float d2 = resid2(L.Rt[lab], c.v[0], c.v[1], c.v[2], c.v[3], c.v[4], c.v[5]);
    atomicAdd(&acc[lab], assign_score(d2, in.thr, in.score_mode));
  }
}

// The rounds.  Called by all THREADS threads of the workgroup, uniformly, behind the barrier that publishes the staged poses.  When
// it returns a barrier has passed behind the last store to L: L.Rt holds the final poses, L.cnt / score0 / score the tallies
// (score0 / score only outside the inlier-count mode), label / d2 the BEST labels under the final poses.
template <int THREADS, int KMAX, class Chunks>
__device__ __forceinline__ Settled settle_run(const SettleIn& in, SettleState<KMAX>& L, Chunks ck) {
  static_assert(THREADS % 64 == 0 && KMAX <= 64 && KMAX <= THREADS, "a wave per chunk, a lane of it per pose");
  const int tid = threadIdx.x;
  const int K = in.K;
  const int nch = (in.n + 63) / 64;  // (9 K nch fits an int: K <= 64)
  Settled res{0u, SC_POLISH_STOP_MAX_ITER};
#pragma unroll 1
  for (uint32_t r = 0; r < in.max_iter; r++) {
    settle_label<THREADS>(in, L, ck);
    if (r == 0 && in.score_mode != 0) settle_scores<THREADS>(in, L, L.score0);
    ck.publish();
    __syncthreads();
    // pass 1: lane = (pose, chunk, component)
    for (int w = tid; w < K * nch * 7; w += THREADS) {
      const int k = w / (nch * 7), x = w - k * (nch * 7), ch = x / 7, s = x % 7;
      ck.sum(k, ch, s) = refit_chain1(in.planes, in.ld, ch, s, ck.bits(k, ch));
    }
    ck.publish();
    __syncthreads();
    for (int w = tid; w < K * 7; w += THREADS) {  // the chunk sums in chunk order, one lane per (pose, component)
      const int k = w / 7, s = w % 7;
      L.S[k][s] = refit_chunk_sum(nch, [&](int ch) { return ck.sum(k, ch, s); });
    }
    __syncthreads();
    if (tid < K && L.S[tid][0] >= 3.0) {  // the centroids, one lane per pose
      double pc[3], qc[3];
      refit_centroids(L.S[tid], L.S[tid][0], pc, qc);
#pragma unroll
      for (int i = 0; i < 3; i++) { L.C[tid][i] = pc[i]; L.C[tid][3 + i] = qc[i]; }
    }
    __syncthreads();
    // pass 2: lane = (pose, chunk, entry of H); a pose with fewer than 3 members is declined and has none
    for (int w = tid; w < K * nch * 9; w += THREADS) {
      const int k = w / (nch * 9), x = w - k * (nch * 9), ch = x / 9, e = x % 9;
      if (L.S[k][0] < 3.0) continue;
      const double pc[3] = {L.C[k][0], L.C[k][1], L.C[k][2]}, qc[3] = {L.C[k][3], L.C[k][4], L.C[k][5]};
      ck.sum(k, ch, e) = refit_chain2(in.planes, in.ld, ch, e, ck.bits(k, ch), pc, qc);
    }
    ck.publish();
    __syncthreads();
    for (int w = tid; w < K * 9; w += THREADS) {
      const int k = w / 9, e = w % 9;
      if (L.S[k][0] < 3.0) continue;
      L.H[k][e] = refit_chunk_sum(nch, [&](int ch) { return ck.sum(k, ch, e); });
    }
    __syncthreads();
    int changed = 0;
    if (tid < K) {  // the solve, one lane per pose
      const double cnt = L.S[tid][0];
      L.cnt[tid] = (uint32_t)cnt;
      if (r == 0 && in.score_mode == 0) L.score0[tid] = (uint32_t)cnt;
      uint32_t g = GO_DECLINED;
      if (L.st[tid] == SC_OK && cnt >= 3.0) {
        const double pc[3] = {L.C[tid][0], L.C[tid][1], L.C[tid][2]}, qc[3] = {L.C[tid][3], L.C[tid][4], L.C[tid][5]};
        float M[12];
#pragma unroll
        for (int c = 0; c < 12; c++) M[c] = L.Rt[tid][c];
        g = refit_solve(L.H[tid], pc, qc, M, L.Rt[tid]);
      }
      L.declined[tid] = g == GO_DECLINED ? 1 : 0;
      if (g == GO_CHANGED) { L.iters[tid]++; changed = 1; }
    }
    if (!__syncthreads_or(changed)) {  // (uniform) the fixed point: this round's labels are the labels under the final poses
      res.stop = SC_POLISH_STOP_FIXED;
      break;
    }
    res.rounds++;
  }
  if (res.stop == SC_POLISH_STOP_MAX_ITER) {  // (uniform) the last round moved a pose: the labels under the final poses
    settle_label<THREADS>(in, L, ck);
    ck.publish();
    __syncthreads();
    if (tid < K) {
      uint32_t cnt = 0u;
      for (int ch = 0; ch < nch; ch++) cnt += (uint32_t)__builtin_popcountll(ck.bits(tid, ch));
      L.cnt[tid] = cnt;
    }
  }
  if (in.score_mode != 0) settle_scores<THREADS>(in, L, L.score);
  __syncthreads();
  return res;
}

// Word w of pose k's record (sc_polish_batch_result).  dead: the whole problem is refused (a non-finite coordinate): SC_EINVAL.
template <int KMAX>
__device__ __forceinline__ uint32_t settle_record_word(const SettleState<KMAX>& L, int k, int w, const Settled& so, int score_mode, bool dead) {
  const bool ok = !dead && L.st[k] == SC_OK;
  if (w < 12) return __float_as_uint(ok ? L.Rt[k][w] : ((w == 0 || w == 4 || w == 8) ? 1.f : 0.f));
  if (w == 12) return (uint32_t)(dead ? SC_EINVAL : L.st[k]);
  if (!ok) return w == 15 ? (uint32_t)SC_POLISH_STOP_DECLINED << 16 : 0u;
  if (w == 13) return L.score0[k];
  if (w == 14) return score_mode == 0 ? L.cnt[k] : L.score[k];
  return (uint32_t)L.iters[k] | ((L.declined[k] ? (uint32_t)SC_POLISH_STOP_DECLINED : so.stop) << 16);
}

}  // namespace sc
