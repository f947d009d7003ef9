// sc_info_batch.hip — the fp64 information matrix of a batch's poses (include/saccot.h, sc_pose_info_batch): the kernel.
//
// One workgroup of 256 threads per problem, grid = n_problems, nothing shared between workgroups: no global atomics, no global
// scratch, no second launch, no host word.  A problem of n <= 512 correspondences lives in LDS, as in sc_polish_batch.hip:
//
//   staging    either layout -> the six planes with the finiteness test on the way (sc_batch_frame.hpp); the slot form and the pairs
//              form gather through corr while they stage.  A non-finite coordinate, or a non-finite (R, t): SC_EINVAL for THIS problem.
//   terms      a wave's ballot per chunk of 64 — the masks' inlier test, within_tau — and, by the same lane, the correspondence's
//              x = R p + t (three doubles) and its residual term |x - q|^2, written to LDS once.
//   chains     lane = (chunk, sum): the ten sums s_r, m_rs (r <= s), sse over the chunk's set bits, sequentially in index order:
//              10 x ceil(n / 64) <= 80 chains of at most 64 dependent adds, one round of the lane deal.
//   result     ten lanes add the chunk sums in chunk order; 36 lanes assemble the matrix; the record, staged in LDS, is stored one
//              dword per lane.
//
// Every fp64 operation is a plain product or sum: the translation unit is compiled with -ffp-contract=off and no fma builtin is
// used here, so nothing fuses.  DESIGN §5.8c has the LDS table, the resources and the occupancy.
#include "../../include/saccot.h"
#include "sc_batch_frame.hpp"
#include "sc_block.hpp"
#include "sc_info.hpp"
#include "sc_winner.hpp"

namespace sc {

static_assert(sizeof(PoseInfoRecord) == sizeof(sc_pose_info_result) && sizeof(PoseInfoRecord) == 320,
              "PoseInfoRecord is sc_pose_info_result, 320 bytes");
static_assert(offsetof(PoseInfoRecord, sse) == 288 && offsetof(PoseInfoRecord, status) == 296 && offsetof(PoseInfoRecord, inliers) == 300,
              "the record's words: 72 of info, 2 of sse, status, inliers, 4 reserved");

namespace {

constexpr int IT = 256;           // threads of a workgroup: 4 waves ballot the 8 chunks in two rounds, 80 chains fit one round
constexpr int IN = BATCH_MAX_N;   // correspondences of a problem at most
constexpr int ICH = IN / 64;      // chunks of the canonical summation at most
constexpr int NSUM = INFO_NSUM;   // s0 s1 s2 | m00 m01 m02 m11 m12 m22 | sse (sc_info.hpp)
constexpr int NROW = 4;           // term rows of a chunk: x0 x1 x2, the residual term
// A chunk's row of 64 doubles is padded to 65: row (r, ch) then starts 2 (8 r + ch) dwords into the 64-dword bank row, so the lanes
// of one step of the chains — every (chunk, row) at about the same index — read 32 different banks instead of one.
constexpr int ROW_LD = 65;
constexpr int REC_WORDS = sizeof(PoseInfoRecord) / 4;

struct alignas(16) InfoLds {
  float pt[6][IN];                  // px py pz qx qy qz
  double term[NROW * ICH][ROW_LD];  // row r * ICH + ch: x_r (r < 3) or the residual term (r == 3) of chunk ch's correspondences
  double sum[ICH][NSUM];            // a chunk's ten sums
  double S[NSUM];                   // the sums over the chunks
  uint64_t bits[ICH];               // a chunk's inlier word
  float Rt[12];
  uint32_t bad;
  uint32_t rec[REC_WORDS];
};
static_assert(sizeof(InfoLds) < 32 * 1024, "static LDS: five workgroups a compute unit");

// the record and nothing else: zero but the status (and what the caller then fills)
__device__ __forceinline__ void record_zero(InfoLds& L, int status) {
#pragma unroll 1
  for (int w = 0; w < REC_WORDS; w++) L.rec[w] = 0u;
  L.rec[offsetof(PoseInfoRecord, status) / 4] = (uint32_t)status;
}
__device__ __forceinline__ void record_double(InfoLds& L, int k, double v) {  // double k of the record
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  L.rec[2 * k] = (uint32_t)u; L.rec[2 * k + 1] = (uint32_t)(u >> 32);
}

// Where a gathering form finds problem b (sc_polish_batch.hip's PolishSides, restated for this kernel's jobs: that file's
// instruction stream stays what it was).
struct InfoSides { uint32_t off, rows, toff, trows, total_t, slot; };
__device__ __forceinline__ InfoSides sides_of(const PoseInfoJob& job, uint32_t b) {  // plain: the problem's correspondences
  const uint32_t off = job.offset[b];
  return InfoSides{off, job.offset[b + 1] - off, 0u, 0u, 0u, off};
}
__device__ __forceinline__ InfoSides sides_of(const PoseInfoSlotJob& a, uint32_t b) {
  const uint32_t off = a.job.offset[b], toff = a.tgt_off[b];
  return InfoSides{off, a.job.offset[b + 1] - off, toff, a.tgt_off[b + 1] - toff, a.total_t, a.slot[b]};
}
__device__ __forceinline__ InfoSides sides_of(const PoseInfoPairsJob& a, uint32_t p) {
  const uint32_t* r = a.rec + (size_t)PAIR_WORDS * p;
  return InfoSides{r[PW_SRC], r[PW_NS], r[PW_TGT], r[PW_NT], a.job.total, r[PW_SLOT]};
}

// The kernel's argument is PoseInfoJob (sc_pose_info_batch), PoseInfoSlotJob (sc_pose_info_batch_slots_device) or PoseInfoPairsJob
// (sc_pose_info_pairs_slots_device; sc_kernels.hpp): SLOTS — the problem is gathered through corr — is a constant of the
// instantiation, and nothing of the gathering forms is compiled into the plain one.
template <class Arg>
__global__ __launch_bounds__(IT) void pose_info_kernel(const Arg arg) {
  constexpr bool SLOTS = sizeof(Arg) != sizeof(PoseInfoJob);
  const PoseInfoJob& job = job_of(arg);
  __shared__ InfoLds L;
  const int tid = threadIdx.x;
  const InfoSides sd = sides_of(arg, blockIdx.x);
  const uint32_t off = sd.off;
  const uint32_t rows = sd.rows;  // plain: the problem's correspondences; slots: its source points
  int n = (int)rows;              // 3 .. IN: the host checked (slots: decided on the device, checked below)
  const uint32_t at = sd.slot;    // where the problem's correspondences start in corr
  bool unfit = false;
  if constexpr (SLOTS) {
    const uint32_t cnt = arg.count[2 * blockIdx.x], cap = rows * arg.knn;  // (cap <= IN: the host checked)
    const bool flagged = arg.count[2 * blockIdx.x + 1] != 0u;
    unfit = flagged || cnt < 3u || cnt > cap;
    n = (flagged || cnt > cap) ? 0 : (int)cnt;
  }
  const uint32_t* const pose = reinterpret_cast<const uint32_t*>(static_cast<const char*>(job.pose) + (size_t)blockIdx.x * job.pose_stride);
  const int st_in = (int)pose[12];
  if (st_in != SC_OK || unfit) {  // (uniform) no pose: the input's status is the result's
    if (tid == 0) record_zero(L, st_in != SC_OK ? st_in : SC_EINVAL);
    record_store(L.rec, job.out);
    return;
  }

  // ---- staging: either layout -> planes; a non-finite coordinate (or pose) ends this problem
  if (tid == 0) L.bad = 0u;
  if (tid < 12) L.Rt[tid] = __uint_as_float(pose[tid]);
  __syncthreads();
  {
    bool bad = false;
    if constexpr (SLOTS) {
      const uint32_t toff = sd.toff, trows = sd.trows;
      for (int m = tid; m < n; m += IT) {
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
      bad = stage_planes<IT>(L.pt, job.src, job.tgt, job.soa, job.total, off, n);
    }
    if (bad) L.bad = 1u;
  }
  __syncthreads();
  float M[12];
#pragma unroll
  for (int c = 0; c < 12; c++) M[c] = L.Rt[c];
  if (L.bad || !finite12(M)) {  // (uniform)
    if (tid == 0) record_zero(L, SC_EINVAL);
    record_store(L.rec, job.out);
    return;
  }
  const float* const planes = &L.pt[0][0];
  const int nch = (n + 63) / 64;

  // ---- the inlier bits, one 64-bit word per chunk (a wave's ballot), and every correspondence's terms
  for (int ch = tid >> 6; ch < nch; ch += IT / 64) {
    const int j = tid & 63, m = ch * 64 + j;
    bool inl = false;
    if (m < n) {
      const Corr c = load_corr(planes, IN, m);
      inl = within_tau(M, c, job.tau2);
      const double p0 = (double)c.v[0], p1 = (double)c.v[1], p2 = (double)c.v[2];
      double e[3];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const double x = (((double)M[3 * r] * p0 + (double)M[3 * r + 1] * p1) + (double)M[3 * r + 2] * p2) + (double)M[9 + r];
        L.term[r * ICH + ch][j] = x;
        e[r] = x - (double)c.v[3 + r];
      }
      L.term[3 * ICH + ch][j] = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    }
    const unsigned long long bal = __ballot(inl);
    if (j == 0) L.bits[ch] = bal;
  }
  __syncthreads();

  // ---- the chains: lane = (chunk, sum), the chunk's inliers sequentially in index order, from 0.0
  if (tid < nch * NSUM) {
    const int ch = tid / NSUM, k = tid % NSUM;
    // the rows a sum reads: s_r: x_r; m_rs: x_r and x_s; sse: the residual term
    int ra, rb;
    if (k < 3) { ra = k; rb = k; }
    else if (k == 9) { ra = 3; rb = 3; }
    else { ra = k < 6 ? 0 : (k < 8 ? 1 : 2); rb = k < 6 ? k - 3 : (k < 8 ? k - 5 : 2); }
    const bool product = k >= 3 && k < 9;
    const double* const a = L.term[ra * ICH + ch];
    const double* const b2 = L.term[rb * ICH + ch];
    unsigned long long b = L.bits[ch];
    double c = 0.0;
    while (b) {
      const int j = __builtin_ctzll(b);
      b &= b - 1ull;
      const double va = a[j];
      c += product ? va * b2[j] : va;
    }
    L.sum[ch][k] = c;
  }
  __syncthreads();
  if (tid < NSUM) {  // the chunk sums in chunk order, one lane per sum
    double s = 0.0;
    for (int ch = 0; ch < nch; ch++) s += L.sum[ch][tid];
    L.S[tid] = s;
  }
  __syncthreads();

  // ---- the record: 36 entries of the matrix, sse, the count
  uint32_t cnt = 0;
  for (int ch = 0; ch < nch; ch++) cnt += (uint32_t)__builtin_popcountll(L.bits[ch]);
  // (no inlier: every byte of the record is zero — an exact negation of 0.0 would set a sign bit)
  constexpr int W_STATUS = offsetof(PoseInfoRecord, status) / 4, W_INLIERS = offsetof(PoseInfoRecord, inliers) / 4;
  static_assert(SC_OK == 0 && W_STATUS == 74 && W_INLIERS == 75, "doubles 0 .. 36, then status, inliers and four reserved words");
  if (tid < 36) record_double(L, tid, cnt ? info_entry(L.S, tid / 6, tid % 6, cnt) : 0.0);
  else if (tid == 36) record_double(L, 36, cnt ? L.S[9] : 0.0);
  else if (tid >= W_STATUS && tid < REC_WORDS) L.rec[tid] = tid == W_INLIERS ? cnt : 0u;
  record_store(L.rec, job.out);
}

}  // namespace

void launch_pose_info_batch(const PoseInfoJob& job, hipStream_t st) {
  hipLaunchKernelGGL(pose_info_kernel<PoseInfoJob>, dim3(job.n_problems), dim3(IT), 0, st, job);
}

void launch_pose_info_batch_slots(const PoseInfoSlotJob& job, hipStream_t st) {
  hipLaunchKernelGGL(pose_info_kernel<PoseInfoSlotJob>, dim3(job.job.n_problems), dim3(IT), 0, st, job);
}

void launch_pose_info_batch_pairs(const PoseInfoPairsJob& job, hipStream_t st) {
  hipLaunchKernelGGL(pose_info_kernel<PoseInfoPairsJob>, dim3(job.job.n_problems), dim3(IT), 0, st, job);
}

}  // namespace sc
