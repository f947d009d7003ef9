// sc_pose64.hpp — a rigid transform in fp64 and the three operations the pair-list entries define on it in include/saccot.h
// (sc_pairs_cycles, sc_pairs_sync, sc_pairs_solve): the inverse, the composition, and the widening of a caller's pose record into the pair's TWO
// oriented transforms — lower set -> higher set and back, one of them the record itself, the other its inverse by the header's
// formula.  Every operation is a plain rounded product or sum in the order written: the files that include this say
// `#pragma clang fp contract(off)` themselves, and the library is built with -ffp-contract=off.  Device code only; three users:
// sc_cycles.hip, sc_sync.hip and sc_solve.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "sc_cycles_check.hpp"

namespace sc {

struct T64 { double R[9], t[3]; };

__device__ __forceinline__ T64 load_t64(const double* __restrict__ w) {
  T64 T;
#pragma unroll
  for (int c = 0; c < 9; c++) T.R[c] = w[c];
#pragma unroll
  for (int c = 0; c < 3; c++) T.t[c] = w[9 + c];
  return T;
}
__device__ __forceinline__ void store_t64(double* __restrict__ w, const T64& T) {
#pragma unroll
  for (int c = 0; c < 9; c++) w[c] = T.R[c];
#pragma unroll
  for (int c = 0; c < 3; c++) w[9 + c] = T.t[c];
}
// M = B o A
__device__ __forceinline__ T64 compose_t64(const T64& B, const T64& A) {
  T64 M;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) M.R[3 * i + j] = ((B.R[3 * i] * A.R[j] + B.R[3 * i + 1] * A.R[3 + j]) + B.R[3 * i + 2] * A.R[6 + j]);
    M.t[i] = ((B.R[3 * i] * A.t[0] + B.R[3 * i + 1] * A.t[1]) + B.R[3 * i + 2] * A.t[2]) + B.t[i];
  }
  return M;
}

// a pose record's twelve floats, widened exactly
__device__ __forceinline__ T64 widen_t64(const float (&M)[12]) {
  T64 A;
#pragma unroll
  for (int c = 0; c < 9; c++) A.R[c] = (double)M[c];
#pragma unroll
  for (int c = 0; c < 3; c++) A.t[c] = (double)M[9 + c];
  return A;
}
// A widened pose record (finite) -> the pair's two oriented transforms, 2 x 12 doubles at wide + 24 p: lower -> higher set at 0,
// higher -> lower at 12.  rec: the pair's record (sc_cycles_check.hpp), which says whether the pair is stored (lower, higher) and the
// record therefore is lower -> higher; the other one is its inverse.
__device__ __forceinline__ void store_oriented_pair(const T64 A, const uint32_t* rec, double* wide, uint32_t p) {
  T64 I;  // (R^T, t'), t'_c = -((R_0c t_0 + R_1c t_1) + R_2c t_2)
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) I.R[3 * i + j] = A.R[3 * j + i];
#pragma unroll
  for (int c = 0; c < 3; c++) I.t[c] = -((A.R[c] * A.t[0] + A.R[3 + c] * A.t[1]) + A.R[6 + c] * A.t[2]);
  const bool fwd = rec[CW_FWD] != 0;
  double* const w = wide + (size_t)24 * p;
  store_t64(w, fwd ? A : I);
  store_t64(w + 12, fwd ? I : A);
}

}  // namespace sc
