// sc_pose64.hpp — a rigid transform in fp64 and the operations the pair-list entries define on it in include/saccot.h
// (sc_pairs_cycles, sc_pairs_sync, sc_pairs_solve): the inverse, the composition, and the widening of a caller's pose record into
// the pair's TWO oriented transforms — lower set -> higher set and back, one of them the record itself, the other its inverse by the
// header's formula.  With them what the three entries' kernels do alike: the PROLOGUE of a prepare kernel's pair (pair_prologue),
// the read of a pair's `use` word, a pair as the caller stored it, finite64 and a wave's integer sum.  Every operation is a plain
// rounded product or sum in the order written: the files that include this say `#pragma clang fp contract(off)` themselves, and the
// library is built with -ffp-contract=off.  Device code only; three users: sc_cycles.hip, sc_sync.hip and sc_solve.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "sc_arith.hpp"
#include "sc_cycles_check.hpp"

namespace sc {

__device__ __forceinline__ bool finite64(double x) { return __builtin_fabs(x) < __builtin_inf(); }  // false for inf and NaN
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

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

// the header's inverse of a transform: (R^T, t'), t'_c = -((R_0c t_0 + R_1c t_1) + R_2c t_2)
__device__ __forceinline__ T64 inverse_t64(const T64& A) {
  T64 I;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) I.R[3 * i + j] = A.R[3 * j + i];
#pragma unroll
  for (int c = 0; c < 3; c++) I.t[c] = -((A.R[c] * A.t[0] + A.R[3 + c] * A.t[1]) + A.R[6 + c] * A.t[2]);
  return I;
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
  const T64 I = inverse_t64(A);
  const bool fwd = rec[CW_FWD] != 0;
  double* const w = wide + (size_t)24 * p;
  store_t64(w, fwd ? A : I);
  store_t64(w + 12, fwd ? I : A);
}

// What a prepare kernel does first for pair p: the caller's pose record read, its status (the optional word at byte 48; a record
// that is not finite: SC_EINVAL), and — where the pair is an edge: a valid record on two different sets — its two oriented
// transforms stored.  recs: the staged records of all pairs.
__device__ __forceinline__ int pair_prologue(const void* pose, uint32_t pose_stride, bool reads_status, const uint32_t* recs, double* wide, uint32_t p,
                                             bool* edge) {
  const uint32_t* const w = reinterpret_cast<const uint32_t*>(static_cast<const char*>(pose) + (size_t)p * pose_stride);
  float M[12];
#pragma unroll
  for (int c = 0; c < 12; c++) M[c] = __uint_as_float(w[c]);
  int status = reads_status ? (int)w[12] : SC_OK;  // (without the flag nothing past byte 47 is read)
  if (status == SC_OK && !finite12(M)) status = SC_EINVAL;
  const uint32_t* const r = recs + (size_t)CYCLES_REC_WORDS * p;
  const bool e = status == SC_OK && r[CW_LO] != r[CW_HI];
  if (e) store_oriented_pair(widen_t64(M), r, wide, p);
  *edge = e;  // (behind the store: written in front of it, the prepare kernels compile to other code)
  return status;
}
// pair p's `use` word, a word at byte p * use_stride of an optional array: without the array every pair is to be used
__device__ __forceinline__ bool pair_use(const void* use, uint32_t use_stride, uint32_t p) {
  return !use || *reinterpret_cast<const uint32_t*>(static_cast<const char*>(use) + (size_t)p * use_stride) != 0;
}
// A pair as the caller stored it, (a, b), from its record r.  fwd: a is the lower set, and a -> b the first of its two transforms.
struct StoredPair { uint32_t a, b; bool fwd; };
__device__ __forceinline__ StoredPair stored_pair(const uint32_t* r) {
  StoredPair s;
  s.fwd = r[CW_FWD] != 0;
  s.a = s.fwd ? r[CW_LO] : r[CW_HI]; s.b = s.fwd ? r[CW_HI] : r[CW_LO];
  return s;
}

}  // namespace sc
