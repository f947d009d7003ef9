// sc_batch_frame.hpp — the frame around one problem of a batch kernel, shared by batch_register_kernel (sc_batch.hip),
// polish_batch_kernel (sc_polish_batch.hip) and pose_info_kernel (sc_info_batch.hip): a workgroup of THREADS threads owns the problem, stages its points into six LDS planes,
// and leaves a record — staged in LDS, stored one dword per lane — and a mask range.  Each kernel keeps its own LDS layout (BatchLds,
// PolishLds, InfoLds) and the words of its record behind the twelve of (R, t); only these functions are shared.
#pragma once
#include "sc_kernels.hpp"

namespace sc {

// The plain job inside either form of a kernel's argument (the slot forms wrap it, sc_kernels.hpp).
__device__ __forceinline__ const BatchJob& job_of(const BatchJob& a) { return a; }
__device__ __forceinline__ const BatchJob& job_of(const BatchSlotJob& a) { return a.job; }
__device__ __forceinline__ const BatchJob& job_of(const InstBatchJob& a) { return a.job; }
__device__ __forceinline__ const BatchJob& job_of(const InstBatchSlotJob& a) { return a.job; }
__device__ __forceinline__ const PolishBatchJob& job_of(const PolishBatchJob& a) { return a; }
__device__ __forceinline__ const PolishBatchJob& job_of(const PolishBatchSlotJob& a) { return a.job; }
__device__ __forceinline__ const PolishBatchJob& job_of(const PolishBatchPairsJob& a) { return a.job; }
__device__ __forceinline__ const PoseInfoJob& job_of(const PoseInfoJob& a) { return a; }
__device__ __forceinline__ const PoseInfoJob& job_of(const PoseInfoSlotJob& a) { return a.job; }
__device__ __forceinline__ const PoseInfoJob& job_of(const PoseInfoPairsJob& a) { return a.job; }

// Staging: rows [off, off + n) of src / tgt (n x 3 row-major, or with soa three planes of `total`) -> pt (px py pz qx qy qz).
// true: THIS thread read a non-finite coordinate (the caller ends the problem with SC_EINVAL).
template <int THREADS>
__device__ __forceinline__ bool stage_planes(float (&pt)[6][BATCH_MAX_N], const float* src, const float* tgt, int soa, uint32_t total,
                                             uint32_t off, int n) {
  bool bad = false;
  for (int x = threadIdx.x; x < 3 * n; x += THREADS) {
    int c, m;
    size_t g;
    if (soa) { c = x / n; m = x - c * n; g = (size_t)c * total + off + m; }
    else { m = x / 3; c = x - 3 * m; g = (size_t)off * 3 + x; }
    const float p = src[g], q = tgt[g];
    bad = bad || !(fabsf(p) < __builtin_inff()) || !(fabsf(q) < __builtin_inff());
    pt[c][m] = p; pt[3 + c][m] = q;
  }
  return bad;
}

// a record's first twelve words: identity unless Rt is given
__device__ __forceinline__ void record_pose(uint32_t* rec, const float* Rt) {
#pragma unroll
  for (int c = 0; c < 12; c++) rec[c] = __float_as_uint(Rt ? Rt[c] : ((c == 0 || c == 4 || c == 8) ? 1.f : 0.f));
}
// one dword of the record per lane (the barrier publishes what one thread filled)
template <int WORDS, class Record>
__device__ __forceinline__ void record_store(const uint32_t (&rec)[WORDS], Record* out) {
  static_assert(sizeof(Record) == 4 * WORDS, "the staged words are the record");
  __syncthreads();
  if (threadIdx.x < WORDS) reinterpret_cast<uint32_t*>(out + blockIdx.x)[threadIdx.x] = rec[threadIdx.x];
}
template <int THREADS>
__device__ __forceinline__ void mask_zero(uint8_t* mask, int n) {
  for (int m = threadIdx.x; m < n; m += THREADS) mask[m] = 0;
}

}  // namespace sc
