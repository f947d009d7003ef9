// sc_match_tile.hpp — what sc_match.hip (one pair of sets, sliced) and sc_match_batch.hip (many small pairs, one launch) have in
// common, said once: what makes a distance, a row's list and an output entry the same bits in both.
//   tile_step        one component of a register tile of 8 rows x 4 columns: subtract, multiply, add on pairs of adjacent columns — no
//                    fused multiply-add (this header turns contraction off for every file that includes it)
//   top_insert       the cascade of 64-bit minima that keeps a row's KP smallest keys in LDS
//   row_kept         a finish kernel's row decision: how many of a row's merged keys become entries (mutual / ratio / knn)
//   entry_write      one output entry: corr, d2 and the gathered points;  entry_resid: its gate residual under one pose
//   pose_record / pose_used   a pose record of either guide: 12 floats, and behind them a status when the caller says so
//   not_finite / scan_not_finite   the exponent test of the finiteness rule, and a strided share of an array under it
// A key is (bits of the squared distance) << 32 | index; KEY_NONE is above every real key.
// Per kernel stay: where a problem's rows, lists and minima start, the gate's evaluation loop, the look-back / running count — and
// the chunk loop, the selection block and the column-minimum flush around tile_step and top_insert (sc_match.hip says why).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sc_arith.hpp"
#include "sc_kernels.hpp"

#pragma clang fp contract(off)  // the canonical distance rounds the product and the sum separately

namespace sc {

constexpr int MT_KC = 16;                       // components of a chunk staged in LDS
constexpr unsigned long long KEY_NONE = ~0ull;  // above every real key: a real key's low half is an index < 2^24

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool not_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

// this thread's share of n floats, strided over the threads that share the scan (me of stride): is one of them not finite?
__device__ __forceinline__ bool scan_not_finite(const float* __restrict__ p, size_t n, size_t me, size_t stride) {
  bool bad = false;
  for (size_t e = me; e < n; e += stride) bad = bad || not_finite(p[e]);
  return bad;
}

// record k of a guide's pose list (MatchGuide, MatchBatchGuide): 12 floats, and behind them the status when the caller says there
// is one; a record whose status is not SC_OK is not used
template <class Guide>
__device__ __forceinline__ const float* pose_record(const Guide& gd, uint32_t k) {
  return reinterpret_cast<const float*>(static_cast<const char*>(gd.pose) + (size_t)k * gd.pose_stride);
}
template <class Guide>
__device__ __forceinline__ bool pose_used(const Guide& gd, const float* rec) {
  return gd.use_status == 0u || reinterpret_cast<const int32_t*>(rec)[12] == (int32_t)SC_OK;
}

// slot q keeps the smaller, the larger moves on: every key goes through slot 0, so slot 0 ends as the minimum of all; what slot 1
// sees is everything else; and so on — the KP smallest in order, whatever the interleaving
template <int KP>
__device__ __forceinline__ void top_insert(unsigned long long* list, unsigned long long key) {
#pragma unroll
  for (int q = 0; q < KP; q++) {
    const unsigned long long old = atomicMin(&list[q], key);
    if (old > key) key = old;
    if (key == KEY_NONE) break;  // (an empty slot was filled: nothing left to pass on)
  }
}

// one component: the thread's 8 rows (pa) against its 4 columns (pb), as two column pairs
__device__ __forceinline__ void tile_step(f2 (&acc)[8][2], const float* pa, const float* pb) {
  const float4 a0 = *reinterpret_cast<const float4*>(pa);
  const float4 a1 = *reinterpret_cast<const float4*>(pa + 4);
  const float4 b = *reinterpret_cast<const float4*>(pb);
  const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  const f2 b01 = f2{b.x, b.y}, b23 = f2{b.z, b.w};
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const f2 ar = f2{a[r], a[r]};
    const f2 d0 = ar - b01, d1 = ar - b23;
    acc[r][0] = acc[r][0] + d0 * d0;
    acc[r][1] = acc[r][1] + d1 * d1;
  }
}

// A finish kernel's row decision: key = row i's smallest keys in order (KEY_NONE: none).  With mutual / the ratio test (knn == 1) the
// first is kept or not; otherwise the first knn that exist.  colmin: the problem's column minima (mutual only), nt its columns.
__device__ __forceinline__ uint32_t row_kept(const unsigned long long (&key)[4], uint32_t i, uint32_t mutual, float r2, uint32_t knn,
                                             const unsigned long long* __restrict__ colmin, uint32_t nt) {
  uint32_t cnt = 0;
  if (mutual || r2 > 0.f) {
    bool keep = key[0] != KEY_NONE;
    const uint32_t j = (uint32_t)key[0];
    if (keep && mutual) keep = j < nt && colmin[j] == ((key[0] & 0xFFFFFFFF00000000ull) | i);
    if (keep && r2 > 0.f && key[1] != KEY_NONE)
      keep = __uint_as_float((uint32_t)(key[0] >> 32)) < __fmul_rn(r2, __uint_as_float((uint32_t)(key[1] >> 32)));
    cnt = keep ? 1u : 0u;
  } else {
#pragma unroll
    for (int w = 0; w < 4; w++) cnt += (w < (int)knn && key[w] != KEY_NONE) ? 1u : 0u;
  }
  return cnt;
}

// Output entry e: (row i, the key's column and distance), and the matched points beside it where the call gathers.  so / to: the
// problem's first point row, either side (the frame form: 0).
__device__ __forceinline__ void entry_write(size_t e, uint32_t i, unsigned long long key, int32_t* __restrict__ corr, float* __restrict__ d2,
                                            const MatchGather& g, uint32_t so, uint32_t to) {
  const uint32_t j = (uint32_t)key;
  corr[2 * e] = (int32_t)i;
  corr[2 * e + 1] = (int32_t)j;
  d2[e] = __uint_as_float((uint32_t)(key >> 32));
  if (g.gsrc) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      g.gsrc[3 * e + c] = g.src[((size_t)so + i) * g.s_elem + (size_t)c * g.s_comp];
      g.gtgt[3 * e + c] = g.tgt[((size_t)to + j) * g.t_elem + (size_t)c * g.t_comp];
    }
  }
}

// the points of an entry as a guide addresses them (MatchGuide, MatchBatchGuide): rows si / tj of its two sets
template <class Guide>
__device__ __forceinline__ void entry_points(const Guide& gd, size_t si, size_t tj, float (&p)[3], float (&q)[3]) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    p[c] = gd.src[si * gd.s_elem + (size_t)c * gd.s_comp];
    q[c] = gd.tgt[tj * gd.t_elem + (size_t)c * gd.t_comp];
  }
}
// the gate residual of an entry under pose M: the distance launch's chain on the same points
template <class Guide>
__device__ __forceinline__ float entry_resid(const float (&M)[12], const Guide& gd, size_t si, size_t tj) {
  float p[3], q[3];
  entry_points(gd, si, tj, p, q);
  return resid2(M, p[0], p[1], p[2], q[0], q[1], q[2]);
}

}  // namespace sc
