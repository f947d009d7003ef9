// sc_polish_poses.hip — caller-supplied poses refitted to a fixed point on a scored frame (include/saccot.h, sc_polish_poses): the kernel.
//
// ONE launch, one workgroup of 1024 threads per pose, grid = n_poses — polish_kernel's shape, for sc_capi_polish.hip's and
// sc_info_frame.hip's reasons: a further dependent launch costs more than a pose's tail at the headline size, and the number of stream
// operations depends neither on n nor on n_poses.  The frame's planes live in global memory; nothing of the frame is written.  Per pose:
//
//   pose       read as pose_info_frame_kernel reads it: word 12 only with the flag; a status other than SC_OK and a non-finite Rt end
//              the workgroup (uniformly) with the identity record and a zero mask.
//   score0     the input pose's score over the correspondences that take part (score_term, a sum of integers: any order).
//   iteration  refit_iterate (sc_refit.hpp) — the ONE definition of the fp64 chains, the function polish_kernel and polish_batch_kernel
//              run — with the selection as its participation policy: ANDed into every inlier bit in the ballot loop, so the chains
//              see the chunks of 64 consecutive ORIGINAL indices with the bits of the others cleared.  A chunk's sums and its bit
//              word live in global scratch as ChunkScratch keeps them (sc_chunks.hpp).
//   result     the last iterate's score over the same correspondences, its mask when one is asked for, and the record — staged in
//              LDS, stored one dword per lane.
//
// The policy evaluates sel[m] per index in every iteration: a coalesced load of 1 or 4 bytes a lane, in flight beside the six of the
// correspondence.  DESIGN §5.6b has the resources and the measured cost.
#include <cstddef>

#include "../../include/saccot.h"
#include "sc_arith.hpp"
#include "sc_batch_frame.hpp"
#include "sc_block.hpp"
#include "sc_chunks.hpp"
#include "sc_kernels.hpp"
#include "sc_refit.hpp"
#include "sc_winner.hpp"

namespace sc {

static_assert(sizeof(PolishBatchRecord) == sizeof(sc_polish_batch_result) && sizeof(PolishBatchRecord) == 64,
              "PolishBatchRecord is sc_polish_batch_result, 64 bytes");

namespace {

constexpr int QT = 1024;                               // threads of a workgroup: 16 waves ballot 16 chunks a round, 1024 chains a round
constexpr int REC_WORDS = sizeof(PolishBatchRecord) / 4;

// refit_iterate's participation policy: the selection of sc_polish_poses for THIS pose (want = label0 + k, a wrapping 32-bit add)
struct Selection {
  const void* sel;
  uint32_t mode;
  int32_t label0, want;
  __device__ __forceinline__ bool operator()(int m) const {
    if (mode == SC_POLISH_POSES_SEL_MASK) return static_cast<const uint8_t*>(sel)[m] != 0;
    if (mode == SC_POLISH_POSES_SEL_LABEL) return static_cast<const int32_t*>(sel)[m] == want;
    if (mode == SC_POLISH_POSES_SEL_ALIVE) {
      const int32_t v = static_cast<const int32_t*>(sel)[m];
      return v < label0 || v >= want;
    }
    return true;
  }
};

// the record and nothing else: identity unless Rt is given
__device__ __forceinline__ void record_fill(uint32_t* rec, const float* Rt, int status, uint32_t score0, uint32_t score, uint32_t iters,
                                            uint32_t stop) {
  record_pose(rec, Rt);
  rec[12] = (uint32_t)status; rec[13] = score0; rec[14] = score; rec[15] = iters | (stop << 16);
}

// The score of (R, t) over the correspondences that take part, in the frame's score mode (a sum of integers: any order), and — with
// mask — their mask bytes.  A lane loads four correspondences before it scores the first: the walk is ceil(n / 4096) rounds of memory
// latency, not ceil(n / 1024) (profiles/polish_poses.txt has what that is worth at K = 8).
__device__ __forceinline__ uint32_t score_walk(const float* M, bool fin, const float* __restrict__ planes, int ld, int n, const Selection& part,
                                               float thr, int score_mode, float tau2, uint8_t* mask, uint64_t* red) {
  constexpr int U = 4;
  uint64_t s = 0;
  for (int m0 = threadIdx.x; m0 < n; m0 += U * QT) {
    Corr c[U];
    bool takes[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int m = m0 + u * QT;
      takes[u] = m < n && fin && part(m);
      c[u] = m < n ? load_corr(planes, ld, m) : Corr{};
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int m = m0 + u * QT;
      if (takes[u]) s += score_term(M, c[u].v[0], c[u].v[1], c[u].v[2], c[u].v[3], c[u].v[4], c[u].v[5], thr, score_mode);
      if (mask && m < n) mask[m] = (takes[u] && within_tau(M, c[u], tau2)) ? 1 : 0;
    }
  }
  return (uint32_t)block_reduce_u64(s, red);
}

__global__ __launch_bounds__(QT) void polish_poses_kernel(const PolishPosesJob job) {
  __shared__ float sRt[12];
  __shared__ double sS[8], sH[9];
  __shared__ uint32_t s_go;
  __shared__ uint64_t s_red[QT / 64];
  __shared__ uint32_t s_rec[REC_WORDS];
  const int tid = threadIdx.x;
  const int n = job.pts.n, ld = job.pts.ld;
  const float* __restrict__ planes = job.pts.planes;
  uint8_t* const mask = job.mask ? job.mask + (size_t)blockIdx.x * (size_t)n : nullptr;
  const uint32_t* const pose = reinterpret_cast<const uint32_t*>(static_cast<const char*>(job.pose) + (size_t)blockIdx.x * job.pose_stride);
  const int st_in = job.status ? (int)pose[12] : SC_OK;  // (without the flag nothing past byte 47 is read)
  if (st_in != SC_OK) {  // (uniform) no pose to start from: the input's status is the result's
    if (mask) mask_zero<QT>(mask, n);
    if (tid == 0) record_fill(s_rec, nullptr, st_in, 0u, 0u, 0u, SC_POLISH_STOP_DECLINED);
    record_store(s_rec, job.out);
    return;
  }
  if (tid < 12) sRt[tid] = __uint_as_float(pose[tid]);
  __syncthreads();
  float M[12];
#pragma unroll
  for (int c = 0; c < 12; c++) M[c] = sRt[c];
  if (!finite12(M)) {  // (uniform; the frame's points are finite: staging checked them)
    if (mask) mask_zero<QT>(mask, n);
    if (tid == 0) record_fill(s_rec, nullptr, SC_EINVAL, 0u, 0u, 0u, SC_POLISH_STOP_DECLINED);
    record_store(s_rec, job.out);
    return;
  }
  const Selection part{job.sel, job.sel_mode, job.label0, (int32_t)((uint32_t)job.label0 + blockIdx.x)};
  const auto ck = ChunkScratch<REFIT_NSUM>::of_pose(job.scratch, blockIdx.x, n);  // refit_iterate's chunk storage

  // ---- the input pose's score
  const uint32_t score0 = score_walk(M, true, planes, ld, n, part, job.thr, job.score_mode, job.tau2, nullptr, s_red);

  // ---- the iteration
  const Refit refit = refit_iterate<QT>(planes, ld, n, job.tau2, job.max_iter, ck, sRt, sS, sH, &s_go, part);

  // ---- the last iterate's score, its mask, the record
#pragma unroll
  for (int c = 0; c < 12; c++) M[c] = sRt[c];
  const bool fin = finite12(M);  // (an accepted refit is finite: refine_solve declines the others)
  const uint32_t score = score_walk(M, fin, planes, ld, n, part, job.thr, job.score_mode, job.tau2, mask, s_red);
  if (tid == 0) record_fill(s_rec, M, SC_OK, score0, score, refit.iters, refit.stop);
  record_store(s_rec, job.out);
}

}  // namespace

void launch_polish_poses(const PolishPosesJob& job, hipStream_t st) {
  hipLaunchKernelGGL(polish_poses_kernel, dim3(job.n_poses), dim3(QT), 0, st, job);
}

}  // namespace sc
