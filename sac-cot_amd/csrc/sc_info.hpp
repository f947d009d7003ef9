// sc_info.hpp — what the two kernels of the fp64 information matrix share (sc_info_batch.hip: a batch problem in LDS;
// sc_info_frame.hip: a pose of a scored frame, planes in global memory), once: the ten sums' order and the assembly of the matrix
// from them.  include/saccot.h (sc_pose_info_batch) spells the contract; both entries promise the same record for the same problem,
// bit for bit.  Which term rows a sum reads is spelled in each kernel: the batch kernel's chains read rows stored in LDS, the frame
// kernel's recompute them, and moving the batch kernel's table here changed its instruction schedule (its object must stay what it
// was), so the table is restated in sc_info_frame.hip and tests/test_gpu_pose_info_frame.py compares the two kernels bit for bit.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sc {

constexpr int INFO_NSUM = 10;  // s0 s1 s2 | m00 m01 m02 m11 m12 m22 | sse

// entry (i, j) of sum J^T J, J = [-[x]x | I], from the ten sums S and the inlier count c (include/saccot.h spells the assembly)
__device__ __forceinline__ double info_entry(const double* S, int i, int j, uint32_t c) {
  const double s[3] = {S[0], S[1], S[2]};
  const double m00 = S[3], m01 = S[4], m02 = S[5], m11 = S[6], m12 = S[7], m22 = S[8];
  if (i < 3 && j < 3) {
    if (i == j) return i == 0 ? m11 + m22 : (i == 1 ? m00 + m22 : m00 + m11);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return -(lo == 0 ? (hi == 1 ? m01 : m02) : m12);
  }
  if (i >= 3 && j >= 3) return i == j ? (double)c : 0.0;
  // [s]x, rows (0, -s2, s1), (s2, 0, -s0), (-s1, s0, 0): entry (r, k) for the upper right block, (k, r) for the lower left
  const int r = i < 3 ? i : j, k = i < 3 ? j - 3 : i - 3;
  if (r == k) return 0.0;
  const int o = 3 - r - k;  // the third index
  const double v = o == 0 ? s[0] : (o == 1 ? s[1] : s[2]);
  return ((r + 1) % 3 == k) ? -v : v;  // (0, 1), (1, 2), (2, 0) carry the minus
}

}  // namespace sc
