// sc_merge_batch.hip — duplicate poses of a batch's problems found and folded (include/saccot.h, sc_merge_poses): the kernel of the
// batch form.
//
// One workgroup of 256 threads per problem, grid = n_problems, nothing shared between workgroups: no global atomics, no global
// scratch, no second launch, no host word.  A problem of n <= 512 correspondences lives in LDS, on the batch kernels' per-problem frame
// (sc_batch_frame.hpp):
//
//   poses      the problem's K <= 64 records — motion-major — -> LDS, a lane per record; an invalid pose is staged as NaN
//              (sc_assign.hpp), its status kept for the record.
//   staging    either layout -> the six planes with the finiteness test on the way.  A non-finite coordinate: SC_EINVAL in every
//              record of THIS problem, parent -1, the count words 0, 0.
//   support    a lane owns two correspondences, a wave 64 consecutive ones: its decisions for pose k are ONE word of bit row k
//              (64 rows x 8 words in LDS); the tallies as in the frame form (sc_merge.hpp), into LDS words.
//   overlap    the 64 x 64 table in LDS, a thread per cell: eight popcounts.
//   decide     a lane per pose ranks the poses by (s_k, k); wave 0 walks the ranks in order with the kept set as ONE 64-bit word, by
//              rank: a ballot over the stronger ranks gives the pose's same-bits, the lowest set bit of (same & kept) is the strongest
//              kept pose that is the same.
//   result     wave 0 writes the K records (their positions from its kept ballot with SC_MERGE_COMPACT), the parents, the word pair.
#include <cstddef>

#include "sc_batch_frame.hpp"
#include "sc_merge.hpp"

namespace sc {

namespace {

constexpr int BT = 256;                              // threads of a workgroup
constexpr int BN = BATCH_MAX_N;                      // correspondences of a problem at most
constexpr int BU = BN / BT;                          // ... a lane owns
constexpr int BK = (int)SC_MERGE_BATCH_MAX_POSES;    // poses of a problem at most
constexpr int BW = BN / 64;                          // words of a bit row
static_assert(BN % BT == 0 && BT % 64 == 0 && BK <= 64, "a wave per word; the poses of a problem fit one wave and one 64-bit kept set");

struct alignas(16) MergeLds {
  float Rt[BK][ASSIGN_POSE_FLOATS];  // NaN: an invalid pose
  float pt[6][BN];                   // px py pz qx qy qz
  uint64_t rows[BK][BW];             // the support sets
  uint32_t table[BK][BK + 1];        // x_jk (+ 1: rows a bank apart)
  uint32_t cnt[BK], score[BK];       // c_k, s_k (at most 512 x 1024: 32 bits)
  int32_t st[BK], parent[BK];
  uint32_t order[BK];                // order[r]: the pose of rank r
  uint32_t bad;
};
static_assert(sizeof(MergeLds) < 40 * 1024, "static LDS: four workgroups a compute unit");

__global__ __launch_bounds__(BT) void merge_batch_kernel(const MergeBatchJob job) {
  __shared__ MergeLds L;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t b = blockIdx.x;
  const uint32_t off = job.offset[b];
  const int n = (int)(job.offset[b + 1] - off);  // 3 .. BN: the host checked
  const int K = (int)job.n_poses;                // 1 .. BK: the host checked
  const MergeRule rule = job.rule;

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

  if (!dead) {
    // ---- support: a word a wave
    const float* const planes = &L.pt[0][0];
    Corr c[BU];
#pragma unroll
    for (int u = 0; u < BU; u++) {
      const int m = tid + u * BT;
      c[u] = m < n ? load_corr(planes, BN, m) : Corr{};
    }
    MergeKeep<BU> keep;  // lane k of every wave keeps pose k's words and tally (K <= 64)
    keep.clear();
    for (int k = 0; k < K; k++) {
      const float4* const p4 = reinterpret_cast<const float4*>(L.Rt[k]);
      const float4 r0 = p4[0], r1 = p4[1], r2 = p4[2];
      const float M[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
#pragma unroll
      for (int u = 0; u < BU; u++) keep.take(u, lane == k, merge_support_word(M, c[u], tid + u * BT < n, job.tau2, job.thr, job.score_mode));
    }
    if (lane < K) {
#pragma unroll
      for (int u = 0; u < BU; u++) L.rows[lane][wave + u * (BT / 64)] = keep.word[u];
      keep.add_to(&L.cnt[lane], &L.score[lane]);
    }
    __syncthreads();
    // ---- overlap: a thread per cell
    for (int x = tid; x < K * K; x += BT) {
      const int j = x / K, k = x - j * K;
      L.table[j][k] = merge_overlap(L.rows[j], L.rows[k], BW);
    }
    // ---- the strength order
    if (tid < K) {
      const uint32_t sk = L.score[tid];
      int rank = 0;
      for (int j = 0; j < K; j++) rank += merge_stronger(L.score[j], j, sk, tid) ? 1 : 0;
      L.order[rank] = (uint32_t)tid;
    }
    __syncthreads();
  }

  // ---- the fold: wave 0, the kept set one word by rank
  if (wave == 0 && !dead) {
    uint64_t kept = 0ull;
    for (int r = 0; r < K; r++) {
      const int kk = (int)L.order[r];
      if (!merge_eligible(L.st[kk], L.cnt[kk], rule)) {  // invalid, or dropped
        if (lane == 0) L.parent[kk] = -1;
        continue;
      }
      bool bit = false;
      if (lane < r) {  // the stronger ranks only
        const int j = (int)L.order[lane];
        bit = merge_same(L.table[kk][j], L.cnt[j], L.cnt[kk], rule);
      }
      const uint64_t hit = __ballot(bit) & kept;
      if (hit == 0ull) kept |= 1ull << r;
      if (lane == 0) L.parent[kk] = hit == 0ull ? kk : (int32_t)L.order[__ffsll((unsigned long long)hit) - 1];
    }
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- the records, the parents, the word pair: lane k is pose k
  const int k = lane;
  const int st = k < K ? (dead ? SC_EINVAL : L.st[k]) : SC_EINVAL;
  const int parent = k < K && !dead ? L.parent[k] : -1;
  const bool is_kept = k < K && parent == k;
  const uint64_t bk = __ballot(is_kept), bv = __ballot(k < K && st == SC_OK);
  const uint32_t n_kept = (uint32_t)__popcll(bk), before = (uint32_t)__popcll(bk & ((1ull << lane) - 1ull));
  if (k < K) {
    const uint32_t pos = !rule.compact ? (uint32_t)k : (is_kept ? before : n_kept + ((uint32_t)k - before));
    const size_t at = ((size_t)k * job.n_problems + b) * job.pose_stride;
    merge_store_record(job.out + ((size_t)pos * job.n_problems + b), reinterpret_cast<const uint32_t*>(static_cast<const char*>(job.pose) + at),
                       st, parent, k, dead ? 0u : L.cnt[k], dead ? 0u : L.score[k]);
    job.parent[(size_t)k * job.n_problems + b] = parent;
  }
  if (lane == 0 && job.count) { job.count[2 * (size_t)b] = n_kept; job.count[2 * (size_t)b + 1] = (uint32_t)__popcll(bv); }
}

}  // namespace

void launch_merge_batch(const MergeBatchJob& job, hipStream_t st) {
  hipLaunchKernelGGL(merge_batch_kernel, dim3(job.n_problems), dim3(BT), 0, st, job);
}

}  // namespace sc
