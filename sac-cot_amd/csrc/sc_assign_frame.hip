// sc_assign_frame.hip — correspondences of a scored frame labelled by the pose that fits best (include/saccot.h, sc_assign_poses): the
// kernel of the frame form.
//
// ONE launch, grid = ceil(n / ASSIGN_TILE), 256 threads, one tile per workgroup: no grid-stride loop, so there is no wrap that a
// frame of two tiles does not reach.  The frame's planes live in global memory; nothing of the frame is written.  Per workgroup:
//
//   poses      all K records -> dynamic LDS, 48 bytes a pose, one lane per record; an invalid pose is staged as NaN (sc_assign.hpp) and
//              its status is what workgroup 0 stores into the record.  The two tally words of a pose sit behind the poses.
//   loop       a lane owns U = ASSIGN_TILE / 256 correspondences, loaded before the loop (six coalesced loads each, all in flight
//              together); for k = 0 .. K-1 the pose comes out of LDS as three 16-byte reads of ONE address for every lane — a broadcast
//              — and serves the lane's U residual chains: 13 fused multiply-adds and two compares a pair.
//   outputs    label (and d2) stored coalesced; a labelled correspondence adds its count and score term to its pose's LDS words.
//   flush      behind a barrier: a lane per pose adds the workgroup's tally — only where it is not zero — into the record's count and
//              score with integer atomics.  The records are zero at launch (the caller's memset), so the sums do not depend on the
//              order in which the workgroups arrive.
//
// LDS or uniform loads for the poses: LDS, see DESIGN §5.6c.
#include <cstddef>

#include "sc_assign.hpp"
#include "sc_kernels.hpp"

namespace sc {

static_assert(sizeof(AssignRecord) == sizeof(sc_assign_result) && sizeof(AssignRecord) == 32, "AssignRecord is sc_assign_result, 32 bytes");
static_assert(offsetof(AssignRecord, count) == offsetof(sc_assign_result, count) && offsetof(AssignRecord, count) == 4 &&
                  offsetof(AssignRecord, score) == offsetof(sc_assign_result, score) && offsetof(AssignRecord, score) == 8,
              "the record's words: status, count, two of score, four reserved");
static_assert(ASSIGN_TILE <= 4096 && ASSIGN_TILE % ASSIGN_THREADS == 0, "a lane owns a whole number of correspondences of the tile");

namespace {

constexpr int AT = ASSIGN_THREADS;
constexpr int U = ASSIGN_TILE / AT;  // correspondences a lane owns

template <uint32_t MODE>
__global__ __launch_bounds__(AT) void assign_frame_kernel(const AssignFrameJob job) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // (no static LDS in this kernel: the base stays 16-byte aligned)
  const int K = (int)job.n_poses;
  float* const sRt = reinterpret_cast<float*>(smem);
  uint32_t* const sCnt = reinterpret_cast<uint32_t*>(sRt + (size_t)ASSIGN_POSE_FLOATS * K);
  uint32_t* const sScore = sCnt + K;
  const int tid = threadIdx.x;
  const int n = job.pts.n, ld = job.pts.ld;
  const float* __restrict__ planes = job.pts.planes;

  // ---- this lane's correspondences: on their way before the poses are looked at
  const int m0 = (int)blockIdx.x * ASSIGN_TILE + tid;
  Corr c[U];
  bool part[U];
  Assigned a[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int m = m0 + u * AT;
    c[u] = m < n ? load_corr(planes, ld, m) : Corr{};
    part[u] = m < n && assign_part(job.sel, m);
    a[u] = assign_none();
  }

  // ---- the poses and their validity, once per workgroup
  for (int k = tid; k < K; k += AT) {
    const int st = assign_stage_pose(static_cast<const char*>(job.pose) + (size_t)k * job.pose_stride, job.status != 0,
                                     sRt + ASSIGN_POSE_FLOATS * k);
    sCnt[k] = 0u; sScore[k] = 0u;
    if (blockIdx.x == 0) job.out[k].status = st;  // (count, score and reserved: the caller's memset and the flush)
  }
  __syncthreads();

  // ---- best of K
  for (int k = 0; k < K; k++) {
    const float4* const p4 = reinterpret_cast<const float4*>(sRt + ASSIGN_POSE_FLOATS * k);
    const float4 r0 = p4[0], r1 = p4[1], r2 = p4[2];
    const float M[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
#pragma unroll
    for (int u = 0; u < U; u++) assign_step<MODE>(a[u], M, c[u], part[u], job.tau2, k);
  }

  // ---- the labels, the residuals, the tallies
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int m = m0 + u * AT;
    if (m < n) {
      job.label[m] = a[u].label;
      if (job.d2) job.d2[m] = a[u].d2;
      assign_tally(sCnt, sScore, a[u], job.thr, job.score_mode);
    }
  }
  __syncthreads();
  for (int k = tid; k < K; k += AT) {
    const uint32_t cnt = sCnt[k];
    if (cnt) {  // only the poses this workgroup used
      atomicAdd(&job.out[k].count, cnt);
      atomicAdd(reinterpret_cast<unsigned long long*>(&job.out[k].score), (unsigned long long)(job.score_mode == 0 ? cnt : sScore[k]));
    }
  }
}

}  // namespace

void launch_assign_frame(const AssignFrameJob& job, hipStream_t st) {
  const dim3 grid((uint32_t)((job.pts.n + ASSIGN_TILE - 1) / ASSIGN_TILE));
  const size_t lds = assign_frame_lds_bytes(job.n_poses);
  if (job.mode == SC_ASSIGN_FIRST) hipLaunchKernelGGL(assign_frame_kernel<SC_ASSIGN_FIRST>, grid, dim3(AT), lds, st, job);
  else hipLaunchKernelGGL(assign_frame_kernel<SC_ASSIGN_BEST>, grid, dim3(AT), lds, st, job);
}

}  // namespace sc
