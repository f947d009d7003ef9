// sc_winner.hpp — what the kernels that name a winner and write its mask share (sc_final.hip, sc_peel.hip, sc_polish.hip), once each:
//   load_corr / within_tau / is_inlier     a correspondence's six coordinates and the masks' inlier test (C2's scoring bodies — inlier_bit,
//                                          score_term, score_exact_kernel — spell the chain for their own operand layouts)
//   outranks / rank_prefetch / rank_count  a hypothesis's rank index in the ranked list, and its grid-strided count over sel_key
//   reduce_pairs / winner_*                from the arg-max launch's pairs to the winner's position, its (R, t) in LDS and a mask byte
// The tail of such a launch is sc_block.hpp's last_workgroup_sum.  Workgroups of 256 threads.
#pragma once
#include "sc_arith.hpp"
#include "sc_block.hpp"

namespace sc {

// ---- the inlier test of a mask ------------------------------------------------------------------------------------------------
struct Corr { float v[6]; };  // p, then q

__device__ __forceinline__ Corr load_corr(const float* __restrict__ planes, int ld, int m) {  // m < n is the caller's
  Corr c;
#pragma unroll
  for (int k = 0; k < 6; k++) c.v[k] = planes[(size_t)k * ld + m];
  return c;
}
// the canonical chain against tau^2: the half of is_inlier that depends on the correspondence (a loop hoists finite12 and calls this)
__device__ __forceinline__ bool within_tau(const float* M, const Corr& c, float tau2) {
  return resid2(M, c.v[0], c.v[1], c.v[2], c.v[3], c.v[4], c.v[5]) < tau2;
}
// a hypothesis with a non-finite coefficient has no inliers
__device__ __forceinline__ bool is_inlier(const float* M, const Corr& c, float tau2) { return finite12(M) && within_tau(M, c, tau2); }

// ---- the rank index ---------------------------------------------------------------------------------------------------------------
// Does ranking key k at position t of the selection outrank key wk at position g?  The ranked list orders by key, descending, then by
// position, ascending; a hypothesis's rank index is the number of hypotheses that outrank it.
__device__ __forceinline__ bool outranks(uint32_t k, uint32_t t, uint32_t wk, uint32_t g) { return k > wk || (k == wk && t < g); }

__device__ __forceinline__ uint32_t outranks4(const uint4& v, uint32_t q, uint32_t wk, uint32_t g) {  // keys 4 q .. 4 q + 3
  const uint32_t t = q << 2;
  return (uint32_t)outranks(v.x, t, wk, g) + (uint32_t)outranks(v.y, t + 1, wk, g) + (uint32_t)outranks(v.z, t + 2, wk, g) +
         (uint32_t)outranks(v.w, t + 3, wk, g);
}

// This thread's share of the rank index of (wk, g) among sel_key[0, T): 16-byte loads, grid-strided, four in flight (a loop of
// dependent trips is that many round trips to hipcc), the last T % 4 keys on workgroup 0.  A sum of integers: any order.  The first
// vector does not depend on the winner: rank_prefetch has it on its way before the pairs are looked at.
__device__ __forceinline__ uint4 rank_prefetch(const uint32_t* __restrict__ sel_key, uint32_t T) {
  const uint32_t q_first = blockIdx.x * 256 + threadIdx.x;
  uint4 v_first = make_uint4(0u, 0u, 0u, 0u);
  if (sel_key != nullptr && q_first < (T >> 2)) v_first = reinterpret_cast<const uint4*>(sel_key)[q_first];
  return v_first;
}
__device__ __forceinline__ uint32_t rank_count(const uint32_t* __restrict__ sel_key, uint32_t T, const uint4& v_first, uint32_t wk, uint32_t g) {
  const uint4* __restrict__ k4 = reinterpret_cast<const uint4*>(sel_key);
  const uint32_t T4 = T >> 2, q_first = blockIdx.x * 256 + threadIdx.x, qs = gridDim.x * 256;
  uint32_t r = 0;
  if (q_first < T4) r += outranks4(v_first, q_first, wk, g);
  uint32_t q = q_first + qs;
  for (; q + 3 * qs < T4; q += 4 * qs) {
    const uint4 a0 = k4[q], a1 = k4[q + qs], a2 = k4[q + 2 * qs], a3 = k4[q + 3 * qs];
    r += outranks4(a0, q, wk, g) + outranks4(a1, q + qs, wk, g) + outranks4(a2, q + 2 * qs, wk, g) + outranks4(a3, q + 3 * qs, wk, g);
  }
  {
    uint4 w[3];
#pragma unroll
    for (uint32_t u = 0; u < 3; u++) w[u] = q + u * qs < T4 ? k4[q + u * qs] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (uint32_t u = 0; u < 3; u++) if (q + u * qs < T4) r += outranks4(w[u], q + u * qs, wk, g);
  }
  if (blockIdx.x == 0) {
    const uint32_t t = (T4 << 2) + threadIdx.x;  // the last T % 4 keys
    if (t < T) r += outranks(sel_key[t], t, wk, g);
  }
  return r;
}

// ---- from the pairs to the winner -----------------------------------------------------------------------------------------------
// Many pairs (the arg-max launch's own workgroups', or a large world's): a thread takes every 256th, the workgroup reduces; lds is free again
__device__ __forceinline__ void reduce_pairs(const unsigned long long* __restrict__ pairs, int npairs, unsigned long long* lds,
                                             unsigned long long& k0, unsigned long long& k1) {
  k0 = 0; k1 = 0;
  for (int w = threadIdx.x; w < npairs; w += 256) lexmax_take(k0, k1, pairs[2 * w], pairs[2 * w + 1]);
  block_lexmax_u64(k0, k1, lds);
  __syncthreads();
}

// key = (count << 32) | second, second = sel_key[g] (two_stage) or 0xFFFFFFFF - g; position = 0xFFFFFFFF - g (score_argmax_kernel).
// k0 == 0: no hypothesis.  bad: a position outside the selection — a stale pair, ranks that disagree on T (never this context's own
// arg-max) — which must not index sel_key, the hypotheses or the triangle lookup: treated as "no hypothesis", for the caller to report.
struct Winner { unsigned long long k0, k1; uint32_t g; bool bad; };
__device__ __forceinline__ Winner winner_decode(unsigned long long k0, unsigned long long k1, bool two_stage, uint32_t T) {
  Winner w{k0, k1, 0u, false};
  if (k0 != 0) w.g = 0xFFFFFFFFu - (uint32_t)((two_stage ? k1 : k0) & 0xFFFFFFFFull);
  w.bad = k0 != 0 && w.g >= T;
  if (w.bad) { w.k0 = 0; w.k1 = 0; w.g = 0; }
  return w;
}
// the reduced pair, for whoever reads it after the launch (one thread of the launch)
__device__ __forceinline__ void winner_key_store(unsigned long long* key_out, const Winner& w) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { key_out[0] = w.k0; key_out[1] = w.k0 ? w.k1 : 0ull; }
}

// Twelve threads load the winner's (R, t) — component c at Rt[c * stride] — or the identity into sRt (the next barrier publishes it);
// workgroup 0 writes it to Rt12 as well.
__device__ __forceinline__ void winner_rt_to_lds(const float* __restrict__ Rt, size_t stride, bool have, float* sRt, float* __restrict__ Rt12) {
  if (threadIdx.x < 12) {
    const float ident = (threadIdx.x == 0 || threadIdx.x == 4 || threadIdx.x == 8) ? 1.f : 0.f;
    const float v = have ? Rt[(size_t)threadIdx.x * stride] : ident;
    sRt[threadIdx.x] = v;
    if (blockIdx.x == 0) Rt12[threadIdx.x] = v;
  }
}

// a mask byte: is correspondence c an inlier of the winner's (R, t) (12 floats, in LDS or global memory), if there is a winner
__device__ __forceinline__ bool winner_inlier(const float* Rt, bool have, const Corr& c, float tau2) {
  float M[12];
#pragma unroll
  for (int k = 0; k < 12; k++) M[k] = Rt[k];
  return have && is_inlier(M, c, tau2);
}

// The winner kernels' grid: the mask's ceil(n / 256) workgroups; more only if the key list is long (>= 4 uint4 per thread each)
inline uint32_t winner_blocks(int n, uint32_t T) {
  uint32_t blocks = (uint32_t)((n + 255) / 256);
  const uint32_t for_keys = (T / 4 + 1023) / 1024;
  if (for_keys > blocks) blocks = for_keys < 1024u ? for_keys : 1024u;
  return blocks;
}

}  // namespace sc
