// sc_settle_batch.hip — poses relabelled and refitted until stable for a batch's problems (include/saccot.h, sc_settle_poses): the
// kernel of the batch form.
//
// One workgroup of 256 threads per problem, grid = n_problems, nothing shared between workgroups: no global atomics, no global
// scratch, no second launch, no host word.  A problem of n <= 512 correspondences lives in LDS, as in sc_polish_batch.hip and
// sc_assign_batch.hip:
//
//   poses      the problem's K <= 16 records — motion-major: pose k of problem b is record k * n_problems + b — -> LDS, a lane per
//              record; the status at byte 48 is always read; an invalid pose is staged as NaN (sc_assign.hpp).
//   staging    either layout -> the six planes with the finiteness test on the way (sc_batch_frame.hpp).  A non-finite coordinate:
//              label -1 throughout, SC_EINVAL in every record of THIS problem, rounds 0 / SC_POLISH_STOP_DECLINED.
//   rounds     settle_run (sc_settle.hpp), the function the frame form runs, on LDS storage: K x 8 chunks x 9 sums and K x 8 bit
//              words next to the planes; the barrier alone publishes them.
//   result     K records, a dword per lane; the problem's two words of d_rounds.
//
// Static LDS: 12 288 (planes) + 9 216 (sums) + 1 024 (bits) + 4 016 (SettleState<16>) + 16 = 26 560 bytes (the compiler reports 26 816):
// LDS would let six workgroups share a compute unit of 160 KiB, but the registers bind first — 112 VGPRs are 4 waves a SIMD, 16 waves,
// FOUR workgroups a compute unit.  The rounds are latency-bound (chains of up to 64 dependent fp64 operations), so several small
// workgroups share a compute unit: DESIGN §5.6d.
#include <cstddef>

#include "sc_batch_frame.hpp"
#include "sc_kernels.hpp"
#include "sc_settle.hpp"

namespace sc {

namespace {

constexpr int BT = 256;                               // threads of a workgroup
constexpr int BN = BATCH_MAX_N;                       // correspondences of a problem at most
constexpr int BCH = BN / 64;                          // chunks of the canonical summation at most
constexpr int BK = (int)SC_SETTLE_BATCH_MAX_POSES;    // poses of a problem at most

struct alignas(16) SettleBatchLds {
  SettleState<BK> state;
  float pt[6][BN];            // px py pz qx qy qz
  double sum[BK][BCH][9];     // a (pose, chunk)'s sums
  uint64_t bits[BK][BCH];     // its member word
  uint32_t bad;
};
static_assert(sizeof(SettleBatchLds) <= 26 * 1024 + 512, "static LDS: room for six workgroups a compute unit (the registers allow four)");

// settle_run's chunk storage: LDS, which the barrier alone publishes
struct BatchChunks {
  SettleBatchLds& L;
  __device__ __forceinline__ double& sum(int k, int ch, int slot) const { return L.sum[k][ch][slot]; }
  __device__ __forceinline__ uint64_t& bits(int k, int ch) const { return L.bits[k][ch]; }
  __device__ __forceinline__ void publish() const {}
};

__global__ __launch_bounds__(BT) void settle_batch_kernel(const SettleBatchJob job) {
  __shared__ SettleBatchLds L;
  const int tid = threadIdx.x;
  const uint32_t b = blockIdx.x;
  const uint32_t off = job.offset[b];
  const int n = (int)(job.offset[b + 1] - off);  // 3 .. BN: the host checked
  const int K = (int)job.n_poses;                // 1 .. BK: the host checked

  // ---- the poses and the points
  if (tid == 0) L.bad = 0u;
  if (tid < K) settle_stage_pose(L.state, tid, static_cast<const char*>(job.pose) + ((size_t)tid * job.n_problems + b) * job.pose_stride, true);
  __syncthreads();
  if (stage_planes<BT>(L.pt, job.src, job.tgt, job.soa, job.total, off, n)) L.bad = 1u;
  __syncthreads();
  const bool dead = L.bad != 0u;  // (uniform)

  // ---- the rounds
  Settled so{0u, SC_POLISH_STOP_DECLINED};
  int32_t* const label = job.label + (size_t)off;
  if (dead) {
    for (int m = tid; m < n; m += BT) label[m] = -1;
  } else {
    const SettleIn in{&L.pt[0][0], BN, n, K, nullptr, job.tau2, job.thr, job.score_mode, job.max_iter, label, nullptr};
    so = settle_run<BT>(in, L.state, BatchChunks{L});
  }

  // ---- the records, motion-major: word w of pose k
  for (int x = tid; x < K * SETTLE_REC_WORDS; x += BT) {
    const int k = x / SETTLE_REC_WORDS, w = x % SETTLE_REC_WORDS;
    reinterpret_cast<uint32_t*>(job.out + ((size_t)k * job.n_problems + b))[w] = settle_record_word(L.state, k, w, so, job.score_mode, dead);
  }
  if (job.rounds && tid < 2) job.rounds[2 * (size_t)b + tid] = tid == 0 ? so.rounds : so.stop;
}

}  // namespace

void launch_settle_batch(const SettleBatchJob& job, hipStream_t st) {
  hipLaunchKernelGGL(settle_batch_kernel, dim3(job.n_problems), dim3(BT), 0, st, job);
}

}  // namespace sc
