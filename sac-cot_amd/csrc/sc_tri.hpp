// sc_tri.hpp — stage B: triangles_topT on the GPU: what its three files share.  Device code only.
//
// Total order of the output: key descending, then (i,j,k) lexicographic ascending.  The trick that makes the
// tie-break free: triangles are enumerated edge by edge in CSR order (i asc, j asc) and, inside an edge, in
// ascending k, so a triangle's position in that enumeration — its *ordinal* — orders like (i,j,k).  So:
//   1. edge_fill       CSR list of upper-triangle edges (ei, ej, es = s_ij) from the bit rows
//   2. tri_count       per edge: popcount(row_i & row_j & bits above j)          -> scan -> ordinals
//   3. tri_keys        per triangle: key at wkey[ordinal]  (s_ik / s_jk come from the compact edge-weight
//                      array through prefix popcounts, not from the 4N^2-byte dense matrix)
//   4. select rounds   exact radix select of the T-th largest key over wkey (<= 3 histogram rounds)
//   5. compact         keys > k*, plus the first (T - #greater) keys == k* by ordinal, in ordinal order
//   6. sort (rocPRIM)  by (~key, position)    7. tri_decode  ordinal -> (i,j,k)
// Everything is integer / bit work except the two fp32 adds of the key; results do not depend on grid size
// or on the order atomics land in (atomics are only used for commutative integer sums, min and max).
//
// The files, in pipeline order (the section tags — 1, 1', 2, 2b/3', 2c, 3, 3b, 3c, 4, 5, 5b, 7 — head their sections there):
//   sc_tri_edges.hip   1 edge_fill, 1' edge_build and the row emitter they share
//   sc_tri_prune.hip   3b the certifying samples, 3c the estimating sample, hist_reduce, prune_bits, strong_rowcost, cost_split, sample_plan
//   sc_tri.hip         2 tri_count, 3 tri_keys, 2b/3' the event pair, 2c ordinals from the ordered strong list, zero_weak_counts, key_range;
//                      then selection and hand-over: 4 select rounds, 5 compaction, 5b cand_emit and the merge pair, 7 tri_decode, the
//                      rank-order hook.  (One translation unit: without the compaction kernels in its module hipcc compiles
//                      tri_keys_events_kernel<true> one instruction longer — profiles/stage_b_views.txt.)
#pragma once
#include <type_traits>

#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_kernels.hpp"

namespace sc {

// A run-time lanes-per-edge width (Tuning::tg_*, or a choice by row width) as a compile-time constant: f(std::integral_constant<int,
// TG>) for the one of TGS... that tg equals, or for DEF.  The kernels instantiated are those of DEF and TGS..., no more.
template <int DEF, int... TGS, class F>
inline void with_lanes(int tg, F&& f) {
  if (!((tg == TGS ? (f(std::integral_constant<int, TGS>{}), true) : false) || ...)) f(std::integral_constant<int, DEF>{});
}

// Pop up to four set bits of m (lowest first).  nb = how many were popped; b[] are their positions (0 for unused
// slots, so derived indices stay in range).  Lets a lane issue the gathers of four triangles before it consumes the
// first: a lane's triangles would otherwise cost one dependent L2 round trip each.
__device__ __forceinline__ int pop4(uint64_t& m, int b[4]) {
  int nb = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const bool has = m != 0;
    b[q] = has ? __builtin_ctzll(m) : 0;
    m = has ? (m & (m - 1)) : 0;
    nb += has ? 1 : 0;
  }
  return nb;
}

// One end of an edge at one 64-column word: the CSR index of the word's first edge (row base + wpre) and the full-graph
// word; edge (v, k) of that row then sits at first + popc(word & below k).
struct CsrWord { uint32_t first; uint64_t word; };

// The weights s_ik, s_jk of one pop4 batch.  All eight gathers are issued before the first use; idle slots read es[0]
// (their modular index may be out of range).
__device__ __forceinline__ void tri_weights4(const float* __restrict__ es, const int (&b)[4], int nbits, CsrWord ri,
                                             CsrWord rj, float (&s_ik)[4], float (&s_jk)[4]) {
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint64_t below = (1ull << b[q]) - 1ull;
    const bool live = q < nbits;
    s_ik[q] = es[live ? ri.first + (uint32_t)__popcll(ri.word & below) : 0u];
    s_jk[q] = es[live ? rj.first + (uint32_t)__popcll(rj.word & below) : 0u];
  }
}

// The extremes of a 256-thread block's keys -> one plain store per block (no same-address atomics: they serialise at
// ~12 ns each).  Every thread calls it.
__device__ __forceinline__ void block_minmax_store(uint32_t kmin, uint32_t kmax, uint32_t* __restrict__ blk_min,
                                                   uint32_t* __restrict__ blk_max) {
  __shared__ uint32_t lmin[4], lmax[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (uint32_t)__shfl_xor(kmin, o));
    kmax = max(kmax, (uint32_t)__shfl_xor(kmax, o));
  }
  if ((threadIdx.x & 63) == 0) { lmin[threadIdx.x >> 6] = kmin; lmax[threadIdx.x >> 6] = kmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    blk_min[blockIdx.x] = min(min(lmin[0], lmin[1]), min(lmin[2], lmin[3]));
    blk_max[blockIdx.x] = max(max(lmax[0], lmax[1]), max(lmax[2], lmax[3]));
  }
}

constexpr int PR_BINS = 256;   // coarse is enough: LB only needs to be a valid, reasonably tight lower bound
constexpr int PR_COPIES = 16;  // one private copy per lane-in-group: same-bin hits land on different LDS words
constexpr int EST_COPIES = 4;  // the estimating sample (one lane per edge, ~200 hits per workgroup): fewer copies to clear and to add up

// Weight -> bin, heavier = higher, LOGARITHMIC in 1 - s: the weights of good edges crowd against 1.0 (s = exp(-d^2 / 2
// sigma^2) with d << sigma), so linear bins would put tens of thousands of edges into the top one and the sample could
// not be sized.  1 - s is exact in fp32 for s >= 0.5; its exponent and top three mantissa bits give 8 bins per octave:
// 1 - s in [2^-24, 2^-3) -> bins 255 .. 80, s == 1 -> 255, lighter edges -> the low bins.  (wlo / wshift: unused.)
__device__ __forceinline__ uint32_t weight_bin(uint32_t wbits, uint32_t wlo, uint32_t wshift) {
  (void)wlo; (void)wshift;
  const uint32_t lb = __float_as_uint(1.0f - __uint_as_float(wbits)) >> 20;  // sign 0, exponent, 3 mantissa bits
  const int b = (int)(103u << 3) + 255 - (int)lb;                              // 2^-24 has exponent field 103
  return (uint32_t)(b < 0 ? 0 : (b > 255 ? 255 : b));
}

}  // namespace sc
