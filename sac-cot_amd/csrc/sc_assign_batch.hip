// sc_assign_batch.hip — correspondences of a batch's problems labelled by the pose that fits best (include/saccot.h, sc_assign_poses):
// the kernel of the batch form.
//
// One workgroup of 256 threads per problem, grid = n_problems, nothing shared between workgroups: no global atomics, no global
// scratch, no second launch, no host word.  A problem of n <= 512 correspondences lives in LDS, as in sc_info_batch.hip:
//
//   poses      the problem's K <= 64 records — motion-major: pose k of problem b is record k * n_problems + b — -> LDS, a lane per
//              record; an invalid pose is staged as NaN (sc_assign.hpp), its status kept for the record.
//   staging    either layout -> the six planes with the finiteness test on the way (sc_batch_frame.hpp).  A non-finite coordinate:
//              label -1 throughout and SC_EINVAL in every record of THIS problem.
//   loop       a lane owns two correspondences; per pose three 16-byte LDS reads of one address (a broadcast) serve both chains.
//   result     the tallies are LDS atomics on integers; behind a barrier the workgroup writes its K records itself, a dword per lane.
#include <cstddef>

#include "sc_assign.hpp"
#include "sc_batch_frame.hpp"
#include "sc_kernels.hpp"

namespace sc {

namespace {

constexpr int BT = 256;                                // threads of a workgroup
constexpr int BN = BATCH_MAX_N;                        // correspondences of a problem at most
constexpr int BU = BN / BT;                            // ... a lane owns
constexpr int BK = (int)SC_ASSIGN_BATCH_MAX_POSES;     // poses of a problem at most
constexpr int REC_WORDS = sizeof(AssignRecord) / 4;
static_assert(BN % BT == 0 && BK <= BT, "a lane per pose, a whole number of correspondences per lane");

struct alignas(16) AssignLds {
  float Rt[BK][ASSIGN_POSE_FLOATS];  // NaN: an invalid pose
  float pt[6][BN];                   // px py pz qx qy qz
  uint32_t cnt[BK], score[BK];       // a pose's tally (at most 512 x 1024: 32 bits)
  int32_t st[BK];                    // a pose's status word
  uint32_t bad;
};
static_assert(sizeof(AssignLds) < 20 * 1024, "static LDS: eight workgroups a compute unit");

template <uint32_t MODE>
__global__ __launch_bounds__(BT) void assign_batch_kernel(const AssignBatchJob job) {
  __shared__ AssignLds L;
  const int tid = threadIdx.x;
  const uint32_t b = blockIdx.x;
  const uint32_t off = job.offset[b];
  const int n = (int)(job.offset[b + 1] - off);  // 3 .. BN: the host checked
  const int K = (int)job.n_poses;                // 1 .. BK: the host checked

  // ---- the poses and the points
  if (tid == 0) L.bad = 0u;
  if (tid < K) {
    const size_t at = ((size_t)tid * job.n_problems + b) * job.pose_stride;
    L.st[tid] = assign_stage_pose(static_cast<const char*>(job.pose) + at, true, L.Rt[tid]);
    L.cnt[tid] = 0u; L.score[tid] = 0u;
  }
  __syncthreads();
  if (stage_planes<BT>(L.pt, job.src, job.tgt, job.soa, job.total, off, n)) L.bad = 1u;
  __syncthreads();
  const bool dead = L.bad != 0u;  // (uniform)

  // ---- best of K
  const float* const planes = &L.pt[0][0];
  Corr c[BU];
  Assigned a[BU];
#pragma unroll
  for (int u = 0; u < BU; u++) {
    const int m = tid + u * BT;
    c[u] = m < n ? load_corr(planes, BN, m) : Corr{};
    a[u] = assign_none();
  }
  if (!dead) {
    for (int k = 0; k < K; k++) {
      const float4* const p4 = reinterpret_cast<const float4*>(L.Rt[k]);
      const float4 r0 = p4[0], r1 = p4[1], r2 = p4[2];
      const float M[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
#pragma unroll
      for (int u = 0; u < BU; u++) assign_step<MODE>(a[u], M, c[u], tid + u * BT < n, job.tau2, k);
    }
  }
#pragma unroll
  for (int u = 0; u < BU; u++) {
    const int m = tid + u * BT;
    if (m < n) {
      job.label[(size_t)off + m] = a[u].label;
      assign_tally(L.cnt, L.score, a[u], job.thr, job.score_mode);
    }
  }
  __syncthreads();

  // ---- the records, motion-major: word w of pose k
  for (int x = tid; x < K * REC_WORDS; x += BT) {
    const int k = x / REC_WORDS, w = x % REC_WORDS;
    uint32_t v = 0u;  // (the score's high word and the reserved ones)
    if (w == 0) v = (uint32_t)(dead ? SC_EINVAL : L.st[k]);
    else if (w == 1) v = L.cnt[k];
    else if (w == 2) v = job.score_mode == 0 ? L.cnt[k] : L.score[k];
    reinterpret_cast<uint32_t*>(job.out + ((size_t)k * job.n_problems + b))[w] = v;
  }
}

}  // namespace

void launch_assign_batch(const AssignBatchJob& job, hipStream_t st) {
  if (job.mode == SC_ASSIGN_FIRST) hipLaunchKernelGGL(assign_batch_kernel<SC_ASSIGN_FIRST>, dim3(job.n_problems), dim3(BT), 0, st, job);
  else hipLaunchKernelGGL(assign_batch_kernel<SC_ASSIGN_BEST>, dim3(job.n_problems), dim3(BT), 0, st, job);
}

}  // namespace sc
