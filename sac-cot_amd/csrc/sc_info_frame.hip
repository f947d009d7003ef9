// sc_info_frame.hip — the fp64 information matrix of poses on a scored frame (include/saccot.h, sc_pose_info_frame): the kernel.
//
// ONE launch, one workgroup of 1024 threads per pose, grid = n_poses — polish_kernel's shape, for sc_capi_polish.hip's reasons: a
// further dependent launch costs more than a pose's tail at the headline size, and the number of stream operations depends neither on
// n nor on n_poses.  The frame's planes live in global memory; nothing of the frame is written.  Per pose, the contract of
// sc_pose_info_batch (sc_info_batch.hip) word for word:
//
//   bits       a wave's ballot per chunk of 64 — the masks' inlier test, within_tau, ANDed with the selection — writes the chunk's
//              64-bit inlier word (refit_iterate's first loop).  The count is the sum of the words' popcounts.
//   chains     lane = (chunk, sum): the ten sums s_r, m_rs (r <= s), sse over the chunk's set bits, sequentially in index order from
//              0.0: 10 x ceil(n / 64) chains of at most 64 dependent adds, in as many rounds of the deal as that needs.  A chain
//              RECOMPUTES x_r (and the residual term) from the planes instead of reading four stored term rows per correspondence:
//              the same operations on the same operands, hence the same bits — the translation unit is compiled with
//              -ffp-contract=off and uses no fma builtin, so nothing fuses — and the scratch is the chunk sums only.
//   result     ten lanes add the chunk sums in chunk order; 36 lanes assemble the matrix (info_entry, sc_info.hpp); the record, staged
//              in LDS, is stored one dword per lane.
//
// A chunk's ten sums and its bit word live in global scratch as ChunkScratch keeps them (sc_chunks.hpp).  DESIGN §5.8d has the
// resources and the measured cost.
#include <cstddef>

#include "../../include/saccot.h"
#include "sc_arith.hpp"
#include "sc_batch_frame.hpp"
#include "sc_block.hpp"
#include "sc_chunks.hpp"
#include "sc_info.hpp"
#include "sc_kernels.hpp"
#include "sc_winner.hpp"

namespace sc {

namespace {

constexpr int FT = 1024;                               // threads of a workgroup: 16 waves ballot 16 chunks a round, 1024 chains a round
constexpr int REC_WORDS = sizeof(PoseInfoRecord) / 4;
static_assert(sizeof(PoseInfoRecord) == sizeof(sc_pose_info_result), "PoseInfoRecord is sc_pose_info_result");

// the record and nothing else: zero but the status
__device__ __forceinline__ void record_zero(uint32_t* rec, int status) {
#pragma unroll 1
  for (int w = 0; w < REC_WORDS; w++) rec[w] = 0u;
  rec[offsetof(PoseInfoRecord, status) / 4] = (uint32_t)status;
}
__device__ __forceinline__ void record_double(uint32_t* rec, int k, double v) {  // double k of the record
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  rec[2 * k] = (uint32_t)u; rec[2 * k + 1] = (uint32_t)(u >> 32);
}

// x_r of correspondence p under row r of (R, t), in fp64 with the contract's parentheses: products of two fp32 values (exact), three
// rounded sums
struct Row { double a, b, c, t; };
__device__ __forceinline__ Row row_of(const float* Rt, int r) {
  return Row{(double)Rt[3 * r], (double)Rt[3 * r + 1], (double)Rt[3 * r + 2], (double)Rt[9 + r]};
}
__device__ __forceinline__ double x_of(const Row& w, double p0, double p1, double p2) { return ((w.a * p0 + w.b * p1) + w.c * p2) + w.t; }

__global__ __launch_bounds__(FT) void pose_info_frame_kernel(const PoseInfoFrameJob job) {
  __shared__ float sRt[12];
  __shared__ double sS[INFO_NSUM];
  __shared__ uint64_t s_red[FT / 64];
  __shared__ uint32_t s_rec[REC_WORDS];
  const int tid = threadIdx.x;
  const int n = job.pts.n, ld = job.pts.ld;
  const float* __restrict__ planes = job.pts.planes;
  const uint32_t* const pose = reinterpret_cast<const uint32_t*>(static_cast<const char*>(job.pose) + (size_t)blockIdx.x * job.pose_stride);
  const int st_in = job.status ? (int)pose[12] : SC_OK;  // (without the flag nothing past byte 47 is read)
  if (st_in != SC_OK) {  // (uniform) no pose: the input's status is the result's
    if (tid == 0) record_zero(s_rec, st_in);
    record_store(s_rec, job.out);
    return;
  }
  if (tid < 12) sRt[tid] = __uint_as_float(pose[tid]);
  __syncthreads();
  float M[12];
#pragma unroll
  for (int c = 0; c < 12; c++) M[c] = sRt[c];
  if (!finite12(M)) {  // (uniform; the frame's points are finite: staging checked them)
    if (tid == 0) record_zero(s_rec, SC_EINVAL);
    record_store(s_rec, job.out);
    return;
  }
  const int nch = (n + 63) / 64;  // (10 nch fits an int whatever n <= 2^24)
  const auto ck = ChunkScratch<INFO_NSUM>::of_pose(job.scratch, blockIdx.x, n);
  const uint8_t* const sel_mask = static_cast<const uint8_t*>(job.sel);
  const int32_t* const sel_label = static_cast<const int32_t*>(job.sel);
  const int32_t want = (int32_t)((uint32_t)job.label0 + blockIdx.x);

  // ---- the inlier bits, one 64-bit word per chunk (a wave's ballot), with the selection ANDed in; their count
  uint64_t mine = 0;
  for (int ch = tid >> 6; ch < nch; ch += FT / 64) {
    const int m = ch * 64 + (tid & 63);
    bool inl = false;
    if (m < n) {
      bool part = true;
      if (job.sel_mode == SC_POSE_INFO_SEL_MASK) part = sel_mask[m] != 0;
      else if (job.sel_mode == SC_POSE_INFO_SEL_LABEL) part = sel_label[m] == want;
      inl = part && within_tau(M, load_corr(planes, ld, m), job.tau2);
    }
    const unsigned long long bal = __ballot(inl);
    if ((tid & 63) == 0) { ck.bits(ch) = bal; mine += (uint64_t)__builtin_popcountll(bal); }
  }
  ck.publish();
  const uint32_t cnt = (uint32_t)block_reduce_u64(mine, s_red);  // (its barriers publish the bit words as well)

  // ---- the chains: lane = (chunk, sum), the chunk's inliers sequentially in index order, from 0.0
  for (int w = tid; w < nch * INFO_NSUM; w += FT) {
    const int ch = w / INFO_NSUM, k = w % INFO_NSUM;
    // what a sum reads (sc_info_batch.hip's table, restated): s_r: x_r; m_rs: x_r * x_s; sse: the residual term, of all three x_r
    const bool sse = k == 9, product = k >= 3 && k < 9;
    int ia, ib;
    if (k < 3) { ia = k; ib = k; }
    else if (sse) { ia = 0; ib = 1; }
    else { ia = k < 6 ? 0 : (k < 8 ? 1 : 2); ib = k < 6 ? k - 3 : (k < 8 ? k - 5 : 2); }
    const Row ra = row_of(sRt, ia), rb = row_of(sRt, ib), rc = row_of(sRt, 2);
    const float* __restrict__ base = planes + (size_t)ch * 64;
    unsigned long long b = ck.bits(ch);
    double c = 0.0;
    while (b) {
      const int j = __builtin_ctzll(b);
      b &= b - 1ull;
      const double p0 = (double)base[j], p1 = (double)base[(size_t)ld + j], p2 = (double)base[2 * (size_t)ld + j];
      const double va = x_of(ra, p0, p1, p2), vb = x_of(rb, p0, p1, p2);
      double v;
      if (sse) {
        const double e0 = va - (double)base[3 * (size_t)ld + j], e1 = vb - (double)base[4 * (size_t)ld + j];
        const double e2 = x_of(rc, p0, p1, p2) - (double)base[5 * (size_t)ld + j];
        v = (e0 * e0 + e1 * e1) + e2 * e2;
      } else {
        v = product ? va * vb : va;
      }
      c += v;
    }
    ck.sum(ch, k) = c;
  }
  ck.publish();
  __syncthreads();
  if (tid < INFO_NSUM) {  // the chunk sums in chunk order, one lane per sum
    double s = 0.0;
    for (int ch = 0; ch < nch; ch++) s += ck.sum(ch, tid);
    sS[tid] = s;
  }
  __syncthreads();

  // ---- the record: 36 entries of the matrix, sse, the count
  // (no inlier: every byte of the record is zero — an exact negation of 0.0 would set a sign bit)
  constexpr int W_STATUS = offsetof(PoseInfoRecord, status) / 4, W_INLIERS = offsetof(PoseInfoRecord, inliers) / 4;
  static_assert(SC_OK == 0 && W_STATUS == 74 && W_INLIERS == 75 && REC_WORDS == 80, "doubles 0 .. 36, then status, inliers and four reserved words");
  if (tid < 36) record_double(s_rec, tid, cnt ? info_entry(sS, tid / 6, tid % 6, cnt) : 0.0);
  else if (tid == 36) record_double(s_rec, 36, cnt ? sS[9] : 0.0);
  else if (tid >= W_STATUS && tid < REC_WORDS) s_rec[tid] = tid == W_INLIERS ? cnt : 0u;
  record_store(s_rec, job.out);
}

}  // namespace

void launch_pose_info_frame(const PoseInfoFrameJob& job, hipStream_t st) {
  hipLaunchKernelGGL(pose_info_frame_kernel, dim3(job.n_poses), dim3(FT), 0, st, job);
}

}  // namespace sc
