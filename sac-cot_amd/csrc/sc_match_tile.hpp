// sc_match_tile.hpp — the canonical arithmetic and the selection step of descriptor matching, shared by sc_match.hip (one pair of
// sets, sliced) and sc_match_batch.hip (many small pairs, one launch): what makes a distance and a row's list the same bits in both.
//   tile_step    one component of a register tile of 8 rows x 4 columns: subtract, multiply, add on pairs of adjacent columns — no
//                fused multiply-add (this header turns contraction off for every file that includes it)
//   top_insert   the cascade of 64-bit minima that keeps a row's KP smallest keys in LDS
//   not_finite   the exponent test of the finiteness rule
// A key is (bits of the squared distance) << 32 | index; KEY_NONE is above every real key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)  // the canonical distance rounds the product and the sum separately

namespace sc {

constexpr int MT_KC = 16;                       // components of a chunk staged in LDS
constexpr unsigned long long KEY_NONE = ~0ull;  // above every real key: a real key's low half is an index < 2^24

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool not_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

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

}  // namespace sc
