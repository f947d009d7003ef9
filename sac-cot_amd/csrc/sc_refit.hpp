// sc_refit.hpp — the refit iterated to a fixed point, said once: the loop of polish_kernel (sc_polish.hip: a candidate of a scored
// frame, planes in global memory, 1024 threads) and of polish_batch_kernel (sc_polish_batch.hip: a batch problem, planes in LDS, 256
// threads).  Both instantiate refit_iterate, so sc_polish_batch's promise — a problem's record equals what sc_register followed by
// sc_polish(candidates = 1) returns, bit for bit — holds because there is one set of fp64 chains, not two kept in step by hand.
//
// An iteration is the inlier test of the current (R, t) — a wave's ballot per chunk of 64: no n-sized mask — and so_refine's two
// passes (oracle/saccot_oracle.c) over the set bits.  The summation ORDER is the canonical one (64 consecutive indices sequentially,
// then the chunk sums sequentially); the lanes are dealt one per (chunk, component): 7 x ceil(n / 64) sums in pass 1, 9 x in pass 2,
// every chain of 64 independent of the others, and one lane per component adds the chunk sums.  The solve (sc_refine.hpp) stays one
// thread.
//
// Where a chunk's sums and its inlier word live is the caller's: a storage policy `Chunks` with
//   double& sum(int ch, int k)              slot k of chunk ch's sums (pass 1 writes k < 7, pass 2 k < 9)
//   uint64_t& bits(int ch)                  chunk ch's 64 inlier bits
//   void publish()                          before a barrier behind which other lanes read what this one stored: a block fence for
//                                           global memory, nothing for LDS
//
// Which correspondences may be inliers at all is the caller's as well: a participation policy `Part` with
//   bool operator()(int m) const            correspondence m (< n) takes part
// ANDed into the inlier bit in the ballot loop and nowhere else: the chains see the bit words only.  The default, EveryIndex, admits
// every index and folds away: polish_kernel and polish_batch_kernel compile to what they were without it
// (profiles/polish_poses.txt); polish_poses_kernel (sc_polish_poses.hip) passes the selection of sc_polish_poses.
#pragma once
#include "../../include/saccot.h"
#include "sc_arith.hpp"
#include "sc_refine.hpp"
#include "sc_winner.hpp"

namespace sc {

enum : uint32_t { GO_FIXED = 0u, GO_CHANGED = 1u, GO_DECLINED = 2u };  // what the solving thread tells the workgroup

// ---- the fp64 chains, once each: refit_iterate below runs them for one pose, the round of sc_settle_poses (sc_settle.hpp) for K poses
// at a time.  A chain sees a chunk's bit word and the planes, never who set the bits or where the sums are kept.
// pass 1, slot k of chunk ch: the count (k == 0), sum p (1 .. 3) or sum q (4 .. 6) of the chunk's set bits, sequentially in index order
__device__ __forceinline__ double refit_chain1(const float* __restrict__ planes, int ld, int ch, int k, unsigned long long b) {
  const float* __restrict__ own = planes + (size_t)(k ? k - 1 : 0) * ld + (size_t)ch * 64;
  double c = 0.0;
  while (b) {
    const int j = __builtin_ctzll(b);
    b &= b - 1ull;
    c += k ? (double)own[j] : 1.0;
  }
  return c;
}
// the centroids of pass 1's sums S[7] (cnt = S[0] >= 3)
__device__ __forceinline__ void refit_centroids(const double* S, double cnt, double (&pc)[3], double (&qc)[3]) {
  pc[0] = S[1] / cnt; pc[1] = S[2] / cnt; pc[2] = S[3] / cnt;
  qc[0] = S[4] / cnt; qc[1] = S[5] / cnt; qc[2] = S[6] / cnt;
}
// pass 2, entry e of H for chunk ch: h = fma(p_r - pc_r, q_c - qc_c, h) over the chunk's set bits
__device__ __forceinline__ double refit_chain2(const float* __restrict__ planes, int ld, int ch, int e, unsigned long long b,
                                               const double (&pc)[3], const double (&qc)[3]) {
  const int r = e / 3, cc = e % 3;
  const float* __restrict__ pr = planes + (size_t)r * ld + (size_t)ch * 64;
  const float* __restrict__ qr = planes + (size_t)(3 + cc) * ld + (size_t)ch * 64;
  const double pcr = r == 0 ? pc[0] : (r == 1 ? pc[1] : pc[2]), qcc = cc == 0 ? qc[0] : (cc == 1 ? qc[1] : qc[2]);
  double h = 0.0;
  while (b) {
    const int j = __builtin_ctzll(b);
    b &= b - 1ull;
    h = __builtin_fma((double)pr[j] - pcr, (double)qr[j] - qcc, h);
  }
  return h;
}
// the chunk sums in chunk order; at(ch): one slot of chunk ch
template <class At>
__device__ __forceinline__ double refit_chunk_sum(int nch, At at) {
  double s = 0.0;
  for (int ch = 0; ch < nch; ch++) s += at(ch);
  return s;
}
// The solve on H[9] and the centroids, against the iterate M it started from: GO_DECLINED (not finite), GO_FIXED (M's bits again) or
// GO_CHANGED, and then Rt holds the new iterate.  One thread.
__device__ __forceinline__ uint32_t refit_solve(const double* H, const double (&pc)[3], const double (&qc)[3], const float* M,
                                                float* Rt) {
  double Hs[9];
#pragma unroll
  for (int k = 0; k < 9; k++) Hs[k] = H[k];
  float out[12];
  uint32_t g = GO_DECLINED;
  if (refine_solve(Hs, pc, qc, out)) {  // (not finite: declined)
    g = GO_FIXED;
#pragma unroll
    for (int c = 0; c < 12; c++) g |= (__float_as_uint(out[c]) != __float_as_uint(M[c])) ? GO_CHANGED : GO_FIXED;
    if (g) {
#pragma unroll
      for (int c = 0; c < 12; c++) Rt[c] = out[c];
    }
  }
  return g;
}

// Refits of Rt[12] (LDS; the workgroup sees the caller's stores to it) over the n correspondences of `planes`, until one is declined
// (fewer than 3 inliers, a non-finite result: SC_POLISH_STOP_DECLINED), returns the bits it started from (_FIXED), or max_iter are
// done (_MAX_ITER).  Rt holds the last iterate when it returns, visible to every thread.  S[8], H[9], go: LDS words of the workgroup.
// Called by all THREADS threads of the workgroup, uniformly.
struct Refit { uint32_t iters, stop; };  // the refits that changed (R, t); why they stopped (SC_POLISH_STOP_*)
struct EveryIndex { __device__ __forceinline__ bool operator()(int) const { return true; } };
template <int THREADS, class Chunks, class Part = EveryIndex>
__device__ __forceinline__ Refit refit_iterate(const float* __restrict__ planes, int ld, int n, float tau2, uint32_t max_iter, Chunks ck,
                                               float* Rt, double* S, double* H, uint32_t* go, Part part = Part{}) {
  const int tid = threadIdx.x;
  const int nch = (n + 63) / 64;  // (9 nch fits an int whatever n)
  Refit res{0u, SC_POLISH_STOP_MAX_ITER};
#pragma unroll 1
  for (uint32_t it = 0; it < max_iter; it++) {
    float M[12];
#pragma unroll
    for (int c = 0; c < 12; c++) M[c] = Rt[c];
    const bool fin = finite12(M);
    // the inlier bits of (R, t), one 64-bit word per chunk (a wave's ballot)
    for (int ch = tid >> 6; ch < nch; ch += THREADS / 64) {
      const int m = ch * 64 + (tid & 63);
      bool inl = false;
      if (m < n) {
        const bool takes = part(m);  // (first: what it loads is in flight beside the correspondence's six)
        inl = fin && within_tau(M, load_corr(planes, ld, m), tau2) && takes;
      }
      const unsigned long long bal = __ballot(inl);
      if ((tid & 63) == 0) ck.bits(ch) = bal;
    }
    ck.publish();
    __syncthreads();
    // pass 1: lane = (chunk, component)
    for (int w = tid; w < nch * 7; w += THREADS) {
      const int ch = w / 7, k = w % 7;
      ck.sum(ch, k) = refit_chain1(planes, ld, ch, k, ck.bits(ch));
    }
    ck.publish();
    __syncthreads();
    if (tid < 7) S[tid] = refit_chunk_sum(nch, [&](int ch) { return ck.sum(ch, tid); });  // one lane per component
    __syncthreads();
    const double cnt = S[0];
    if (cnt < 3.0) { res.stop = SC_POLISH_STOP_DECLINED; break; }  // (uniform) the refit is declined: (R, t) stays
    double pc[3], qc[3];
    refit_centroids(S, cnt, pc, qc);
    // pass 2: lane = (chunk, entry of H)
    for (int w = tid; w < nch * 9; w += THREADS) {
      const int ch = w / 9, e = w % 9;
      ck.sum(ch, e) = refit_chain2(planes, ld, ch, e, ck.bits(ch), pc, qc);
    }
    ck.publish();
    __syncthreads();
    if (tid < 9) H[tid] = refit_chunk_sum(nch, [&](int ch) { return ck.sum(ch, tid); });
    __syncthreads();
    if (tid == 0) *go = refit_solve(H, pc, qc, M, Rt);
    __syncthreads();
    const uint32_t g = *go;
    if (g != GO_CHANGED) {  // (uniform) declined, or the fixed point: the refit returned the bits it started from
      res.stop = g == GO_FIXED ? SC_POLISH_STOP_FIXED : SC_POLISH_STOP_DECLINED;
      break;
    }
    res.iters++;
  }
  return res;
}

}  // namespace sc
