// sc_polish_batch.hip — iterated fp64 refits for a batch's winners (include/saccot.h, sc_polish_batch): the kernel.
//
// One workgroup of 256 threads per problem, grid = n_problems, nothing shared between workgroups: no global atomics, no global
// scratch, no second launch, no host word.  A problem of n <= 512 correspondences lives in LDS — six planes of points (12 KB), the
// chunk sums (8 chunks x 16 doubles) and the chunks' inlier words — and the iteration is refit_iterate (sc_refit.hpp), the function
// polish_kernel (sc_polish.hip) runs on global scratch: one definition of every fp64 chain, so a problem's record equals what
// sc_polish(candidates = 1) returns for the same input pose:
//
//   staging    either layout -> the planes with the finiteness test on the way (sc_batch_frame.hpp, shared with sc_batch.hip); the
//              slot form and the pairs form gather through corr while they stage.  A non-finite coordinate, or a non-finite input (R, t): SC_EINVAL
//              for THIS problem.
//   score0     the input pose's score over all n (score_term, a sum of integers).
//   iteration  refit_iterate on PolishChunks: 7 x ceil(n / 64) <= 56 and 9 x <= 72 chains, one round of the lane deal each.
//   result     the last iterate's score and mask, and the record, staged in LDS and stored one dword per lane.
//
// The iteration is latency-bound (chains of up to 64 dependent fp64 operations), so the workgroup is small and many share a
// compute unit: DESIGN §5.8a has the LDS table and the occupancy.
#include "../../include/saccot.h"
#include "sc_batch_frame.hpp"
#include "sc_block.hpp"
#include "sc_refit.hpp"
#include "sc_winner.hpp"

namespace sc {

static_assert(sizeof(PolishBatchRecord) == sizeof(sc_polish_batch_result) && sizeof(PolishBatchRecord) == 64,
              "PolishBatchRecord is sc_polish_batch_result, 64 bytes");
static_assert(offsetof(PolishBatchRecord, status) == 48 && offsetof(PolishBatchRecord, iters) == 60 && offsetof(PolishBatchRecord, stop) == 62,
              "the record's words: 12 of Rt, status, score0, score, iters | stop << 16");

namespace {

constexpr int PT = 256;           // threads of a workgroup: 4 waves ballot the 8 chunks in two rounds, 72 chains fit one round
constexpr int PN = BATCH_MAX_N;   // correspondences of a problem at most
constexpr int PCH = PN / 64;      // chunks of the canonical summation at most
constexpr int REC_WORDS = sizeof(PolishBatchRecord) / 4;

struct alignas(16) PolishLds {
  float pt[6][PN];          // px py pz qx qy qz
  double sum[PCH][16];      // a chunk's sums in [0, 9) (the stride polish_kernel's scratch has)
  uint64_t bits[PCH];       // a chunk's inlier word
  double S[8], H[9];        // the sums over the chunks
  uint64_t red[PT / 64];    // scratch of the workgroup reductions
  float Rt[12];             // the current iterate
  uint32_t go, bad;
  uint32_t rec[REC_WORDS];
};
static_assert(sizeof(PolishLds) < 16 * 1024, "static LDS: ten workgroups a compute unit");

// refit_iterate's chunk storage (sc_refit.hpp): LDS, which the barrier alone publishes
struct PolishChunks {
  PolishLds& L;
  __device__ __forceinline__ double& sum(int ch, int k) const { return L.sum[ch][k]; }
  __device__ __forceinline__ uint64_t& bits(int ch) const { return L.bits[ch]; }
  __device__ __forceinline__ void publish() const {}
};

// the record and nothing else: identity unless Rt is given
__device__ __forceinline__ void record_fill(PolishLds& L, const float* Rt, int status, uint32_t score0, uint32_t score, uint32_t iters,
                                            uint32_t stop) {
  record_pose(L.rec, Rt);
  L.rec[12] = (uint32_t)status; L.rec[13] = score0; L.rec[14] = score; L.rec[15] = iters | (stop << 16);
}

// Where a gathering form finds problem b: the first row and the rows of its points on either side (src planes of job.total, tgt
// planes of total_t), and its slot.  The slot form reads its two monotone offset arrays; the pairs form the pair's record — both
// sides come from one table, and a set may serve many pairs.
struct PolishSides { uint32_t off, rows, toff, trows, total_t, slot; };
__device__ __forceinline__ PolishSides sides_of(const PolishBatchJob& job, uint32_t b) {  // plain: the problem's correspondences
  const uint32_t off = job.offset[b];
  return PolishSides{off, job.offset[b + 1] - off, 0u, 0u, 0u, off};
}
__device__ __forceinline__ PolishSides sides_of(const PolishBatchSlotJob& a, uint32_t b) {
  const uint32_t off = a.job.offset[b], toff = a.tgt_off[b];
  return PolishSides{off, a.job.offset[b + 1] - off, toff, a.tgt_off[b + 1] - toff, a.total_t, a.slot[b]};
}
__device__ __forceinline__ PolishSides sides_of(const PolishBatchPairsJob& a, uint32_t p) {
  const uint32_t* r = a.rec + (size_t)PAIR_WORDS * p;
  return PolishSides{r[PW_SRC], r[PW_NS], r[PW_TGT], r[PW_NT], a.job.total, r[PW_SLOT]};
}

// The kernel's argument is PolishBatchJob (sc_polish_batch), PolishBatchSlotJob (sc_polish_batch_slots_device) or
// PolishBatchPairsJob (sc_polish_pairs_slots_device; sc_kernels.hpp): SLOTS — the problem is gathered through corr — is a constant of
// the instantiation, and nothing of the gathering forms is compiled into the plain one.
template <class Arg>
__global__ __launch_bounds__(PT) void polish_batch_kernel(const Arg arg) {
  constexpr bool SLOTS = sizeof(Arg) != sizeof(PolishBatchJob);
  const PolishBatchJob& job = job_of(arg);
  __shared__ PolishLds L;
  const int tid = threadIdx.x;
  const PolishSides sd = sides_of(arg, blockIdx.x);
  const uint32_t off = sd.off;
  const uint32_t rows = sd.rows;  // plain: the problem's correspondences; slots: its source points
  int n = (int)rows;              // 3 .. PN: the host checked (slots: decided on the device, checked below)
  const uint32_t at = sd.slot;    // where the problem's mask bytes start
  bool unfit = false;
  if constexpr (SLOTS) {
    const uint32_t cnt = arg.count[2 * blockIdx.x], cap = rows * arg.knn;  // (cap <= PN: the host checked)
    const bool flagged = arg.count[2 * blockIdx.x + 1] != 0u;
    unfit = flagged || cnt < 3u || cnt > cap;
    n = (flagged || cnt > cap) ? 0 : (int)cnt;
  }
  uint8_t* const mask = job.mask + at;
  const int st_in = job.in[blockIdx.x].status;
  if (st_in != SC_OK || unfit) {  // (uniform) no pose to start from: the input's status is the result's
    mask_zero<PT>(mask, n);
    if (tid == 0) record_fill(L, nullptr, st_in != SC_OK ? st_in : SC_EINVAL, 0u, 0u, 0u, SC_POLISH_STOP_DECLINED);
    record_store(L.rec, job.out);
    return;
  }

  // ---- staging: either layout -> planes; a non-finite coordinate (or input pose) ends this problem
  if (tid == 0) L.bad = 0u;
  if (tid < 12) L.Rt[tid] = job.in[blockIdx.x].Rt[tid];
  __syncthreads();
  {
    bool bad = false;
    if constexpr (SLOTS) {
      const uint32_t toff = sd.toff, trows = sd.trows;
      for (int m = tid; m < n; m += PT) {
        const uint32_t i = (uint32_t)arg.corr[2 * ((size_t)at + m)], j = (uint32_t)arg.corr[2 * ((size_t)at + m) + 1];
        if (i >= rows || j >= trows) { bad = true; continue; }  // (an index the match cannot have written: nothing is read through it)
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float p = job.src[job.soa ? (size_t)c * job.total + off + i : ((size_t)off + i) * 3 + c];
          const float q = job.tgt[job.soa ? (size_t)c * sd.total_t + toff + j : ((size_t)toff + j) * 3 + c];
          bad = bad || !(fabsf(p) < __builtin_inff()) || !(fabsf(q) < __builtin_inff());
          L.pt[c][m] = p; L.pt[3 + c][m] = q;
        }
      }
    } else {
      bad = stage_planes<PT>(L.pt, job.src, job.tgt, job.soa, job.total, off, n);
    }
    if (bad) L.bad = 1u;
  }
  __syncthreads();
  float M[12];
#pragma unroll
  for (int c = 0; c < 12; c++) M[c] = L.Rt[c];
  if (L.bad || !finite12(M)) {  // (uniform)
    mask_zero<PT>(mask, n);
    if (tid == 0) record_fill(L, nullptr, SC_EINVAL, 0u, 0u, 0u, SC_POLISH_STOP_DECLINED);
    record_store(L.rec, job.out);
    return;
  }
  const float* const planes = &L.pt[0][0];

  // ---- the input pose's score over all n
  uint32_t score0;
  {
    uint64_t s = 0;
    for (int m = tid; m < n; m += PT) {
      const Corr c = load_corr(planes, PN, m);
      s += score_term(M, c.v[0], c.v[1], c.v[2], c.v[3], c.v[4], c.v[5], job.thr, job.score_mode);
    }
    score0 = (uint32_t)block_reduce_u64(s, L.red);
  }

  // ---- the iteration
  const Refit refit = refit_iterate<PT>(planes, PN, n, job.tau2, job.max_iter, PolishChunks{L}, L.Rt, L.S, L.H, &L.go);

  // ---- the last iterate's score over all n (a sum of integers: any order), its mask, the record
#pragma unroll
  for (int c = 0; c < 12; c++) M[c] = L.Rt[c];
  const bool fin = finite12(M);
  uint64_t s = 0;
  for (int m = tid; m < n; m += PT) {
    const Corr c = load_corr(planes, PN, m);
    if (fin) s += score_term(M, c.v[0], c.v[1], c.v[2], c.v[3], c.v[4], c.v[5], job.thr, job.score_mode);
    mask[m] = (fin && within_tau(M, c, job.tau2)) ? 1 : 0;
  }
  const uint32_t score = (uint32_t)block_reduce_u64(s, L.red);
  if (tid == 0) record_fill(L, M, SC_OK, score0, score, refit.iters, refit.stop);
  record_store(L.rec, job.out);
}

}  // namespace

void launch_polish_batch(const PolishBatchJob& job, hipStream_t st) {
  hipLaunchKernelGGL(polish_batch_kernel<PolishBatchJob>, dim3(job.n_problems), dim3(PT), 0, st, job);
}

void launch_polish_batch_slots(const PolishBatchSlotJob& job, hipStream_t st) {
  hipLaunchKernelGGL(polish_batch_kernel<PolishBatchSlotJob>, dim3(job.job.n_problems), dim3(PT), 0, st, job);
}

void launch_polish_batch_pairs(const PolishBatchPairsJob& job, hipStream_t st) {
  hipLaunchKernelGGL(polish_batch_kernel<PolishBatchPairsJob>, dim3(job.job.n_problems), dim3(PT), 0, st, job);
}

}  // namespace sc
