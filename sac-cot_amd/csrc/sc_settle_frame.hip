// sc_settle_frame.hip — poses relabelled and refitted until stable on a scored frame (include/saccot.h, sc_settle_poses): the kernel
// of the frame form.
//
// ONE launch of ONE workgroup of 1024 threads.  The rounds couple all poses — a correspondence moves from one pose's label to
// another's — so a round's labelling needs every pose of the round before, and with a workgroup per pose that is a grid barrier per
// round.  This kernel has none: one workgroup owns the frame, the K <= 64 poses and their per-pose sums live in its LDS
// (SettleState<64>, sc_settle.hpp: 16 064 bytes; the compiler reports 16 320 of static LDS), and "nothing moved" is one
// __syncthreads_or.  No workgroup waits for another.  The price is that the frame's work runs on ONE compute unit: per round the
// call costs what K grows it to, where the composed calls spread K poses over K workgroups (profiles/settle.txt).
//
//   poses      all K records -> LDS, one lane per record; an invalid pose is staged as NaN (sc_assign.hpp) and keeps its status.
//   rounds     settle_run (sc_settle.hpp): 16 waves label 16 chunks of 64 correspondences a trip, two chunks a wave side by side;
//              the refit's (pose, chunk, component) chains are dealt 1024 a trip.  The member bits and chunk sums live in global
//              scratch as polish_poses_kernel keeps them, seen pose-major (PoseChunks, sc_chunks.hpp).
//   result     K records, a dword per lane; the two words of d_rounds.
//
// DESIGN §5.6d has the resources and the measured cost.
#include <cstddef>

#include "sc_chunks.hpp"
#include "sc_kernels.hpp"
#include "sc_settle.hpp"

namespace sc {

static_assert(sizeof(PolishBatchRecord) == 4 * SETTLE_REC_WORDS, "a record is 16 dwords");

namespace {

constexpr int ST = 1024;                           // threads of the one workgroup
constexpr int SK = (int)SC_SETTLE_MAX_POSES;       // poses at most
static_assert(sizeof(SettleState<SK>) < 16 * 1024, "the poses and their sums: under 16 KB of LDS");

__global__ __launch_bounds__(ST) void settle_frame_kernel(const SettleFrameJob job) {
  __shared__ SettleState<SK> L;
  const int tid = threadIdx.x;
  const int K = (int)job.n_poses;  // 1 .. SK: the host checked
  if (tid < K) settle_stage_pose(L, tid, static_cast<const char*>(job.pose) + (size_t)tid * job.pose_stride, job.status != 0);
  __syncthreads();
  const SettleIn in{job.pts.planes, job.pts.ld, job.pts.n, K, job.sel, job.tau2, job.thr, job.score_mode, job.max_iter, job.label, job.d2};
  const Settled so = settle_run<ST>(in, L, PoseChunks<REFIT_NSUM>{job.scratch, (job.pts.n + 63) / 64});
  for (int x = tid; x < K * SETTLE_REC_WORDS; x += ST) {
    const int k = x / SETTLE_REC_WORDS, w = x % SETTLE_REC_WORDS;
    reinterpret_cast<uint32_t*>(job.out + k)[w] = settle_record_word(L, k, w, so, job.score_mode, false);
  }
  if (job.rounds && tid < 2) job.rounds[tid] = tid == 0 ? so.rounds : so.stop;
}

}  // namespace

void launch_settle_frame(const SettleFrameJob& job, hipStream_t st) {
  hipLaunchKernelGGL(settle_frame_kernel, dim3(1), dim3(ST), 0, st, job);
}

}  // namespace sc
