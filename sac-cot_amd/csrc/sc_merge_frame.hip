// sc_merge_frame.hip — duplicate poses of a scored frame found and folded (include/saccot.h, sc_merge_poses): the three kernels of
// the frame form.  The frame's planes live in global memory; nothing of the frame is written.
//
//   support    grid = ceil(n / MERGE_TILE), 256 threads, one tile per workgroup — assign_frame_kernel's shape: all K records -> dynamic
//              LDS, 48 bytes a pose, an invalid pose staged as NaN (sc_assign.hpp), so the loop over the poses holds no branch on
//              validity.  A lane owns U = MERGE_TILE / 256 correspondences; a wave's 64 lanes own 64 CONSECUTIVE ones, so its 64
//              decisions for pose k leave as ONE word — a ballot — into bit row k: every word of every row is written by exactly one
//              wave, nothing is zeroed.  Lane i of the wave keeps the words and the tally of pose kb + i, so the wave stores and
//              adds once per 64 poses (a store an instruction per pose cost more than the residual chains: DESIGN §5.6e).  c_k and
//              s_k: the wave's popcounts and summed score terms go to the pose's LDS words; behind a barrier a lane per pose adds
//              the workgroup's tally — only where it is not zero — into the zeroed tally words.
//   overlap    a workgroup per tile of MERGE_PAIR_TILE x MERGE_PAIR_TILE pose pairs, only tiles with j-tile <= k-tile; the two tiles'
//              bit rows stream through LDS once, OVERLAP_WORDS words at a time; a thread owns 2 x 2 pairs and adds popcount(W_j & W_k);
//              the result is stored at (j, k) and mirrored to (k, j).  Integers: any order is exact.
//   decide     ONE workgroup of 1024 threads, a launch of its own (no workgroup of the launches before stays behind for it).  A thread
//              per pose ranks the poses by (s_k, k) in LDS.  Then, 64 ranks a round: the waves turn the ranks' rows of the table
//              into same-bits against the stronger ranks — the round after the one wave 0 is walking, into the other of two buffers — (a ballot a word, the table read along pose k's row, every word's cell loaded
//              before the first ballot), and wave 0 walks the 64 ranks in order — lane w holds word w of the kept set, by rank, in a
//              register, lane q the fate of the round's rank q; a pose is folded into the LOWEST set bit of (its same-bits & kept):
//              the strongest kept pose that is the same.  A step of the walk is one LDS read, two ballots and scalar work.  Last, a thread per pose writes its record, its
//              parent and — thread 0 — the count words; with SC_MERGE_COMPACT the record's position comes from the waves' kept ballots.
#include <cstddef>

#include "sc_merge.hpp"

namespace sc {

static_assert(sizeof(MergeRecord) == sizeof(sc_merge_pose) && sizeof(MergeRecord) == 64, "MergeRecord is sc_merge_pose, 64 bytes");
static_assert(offsetof(MergeRecord, status) == offsetof(sc_merge_pose, status) && offsetof(MergeRecord, status) == 48 &&
                  offsetof(MergeRecord, index) == offsetof(sc_merge_pose, index) && offsetof(MergeRecord, index) == 52 &&
                  offsetof(MergeRecord, count) == offsetof(sc_merge_pose, count) && offsetof(MergeRecord, count) == 56 &&
                  offsetof(MergeRecord, score) == offsetof(sc_merge_pose, score) && offsetof(MergeRecord, score) == 60,
              "the record's words: twelve of Rt, the status at byte 48, the index, the count, the score");
static_assert(SC_MERGE_MAX_POSES <= MERGE_DECIDE_THREADS, "the decide launch: a thread per pose");

namespace {

constexpr int MT = MERGE_THREADS;
constexpr int U = MERGE_TILE / MT;  // correspondences a lane owns
constexpr int WAVES = MT / 64;      // a wave's word of pass u: WAVES * u + wave, inside the tile's MERGE_TILE / 64

// ---- support
__global__ __launch_bounds__(MT) void merge_support_kernel(const MergeFrameJob job) {
  extern __shared__ __attribute__((aligned(16))) char smem[];  // (no static LDS in this kernel: the base stays 16-byte aligned)
  const int K = (int)job.n_poses;
  float* const sRt = reinterpret_cast<float*>(smem);
  uint32_t* const sCnt = reinterpret_cast<uint32_t*>(sRt + (size_t)ASSIGN_POSE_FLOATS * K);
  uint32_t* const sScore = sCnt + K;
  const int tid = threadIdx.x;
  const int n = job.pts.n, ld = job.pts.ld;
  const float* __restrict__ planes = job.pts.planes;
  const size_t W = merge_row_words(n);

  // ---- this lane's correspondences: on their way before the poses are looked at
  const int m0 = (int)blockIdx.x * MERGE_TILE + tid;
  Corr c[U];
  bool part[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int m = m0 + u * MT;
    c[u] = m < n ? load_corr(planes, ld, m) : Corr{};
    part[u] = m < n && assign_part(job.sel, m);
  }

  // ---- the poses and their validity, once per workgroup
  for (int k = tid; k < K; k += MT) {
    assign_stage_pose(static_cast<const char*>(job.pose) + (size_t)k * job.pose_stride, job.status != 0, sRt + ASSIGN_POSE_FLOATS * k);
    sCnt[k] = 0u; sScore[k] = 0u;
  }
  __syncthreads();

  // ---- every pose against the tile: a word a wave, kept a pose a lane and stored once per 64 poses
  const size_t word0 = (size_t)blockIdx.x * (MERGE_TILE / 64) + (size_t)(tid >> 6);
  const int lane = tid & 63;
  for (int kb = 0; kb < K; kb += 64) {
    const int ke = min(64, K - kb);
    MergeKeep<U> keep;
    keep.clear();
    for (int i = 0; i < ke; i++) {
      const float4* const p4 = reinterpret_cast<const float4*>(sRt + ASSIGN_POSE_FLOATS * (kb + i));
      const float4 r0 = p4[0], r1 = p4[1], r2 = p4[2];
      const float M[12] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
#pragma unroll
      for (int u = 0; u < U; u++) keep.take(u, lane == i, merge_support_word(M, c[u], part[u], job.tau2, job.thr, job.score_mode));
    }
    if (lane < ke) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const size_t wi = word0 + (size_t)u * WAVES;
        if (wi < W) job.rows[(size_t)(kb + lane) * W + wi] = keep.word[u];  // (a word past the row belongs to no correspondence)
      }
      keep.add_to(&sCnt[kb + lane], &sScore[kb + lane]);
    }
  }
  __syncthreads();
  for (int k = tid; k < K; k += MT) {
    const uint32_t cnt = sCnt[k];
    if (cnt) {  // only the poses this workgroup found inliers of
      atomicAdd(&job.tally[k], cnt);
      atomicAdd(&job.tally[K + k], sScore[k]);
    }
  }
}

// ---- overlap
constexpr int PT = MERGE_PAIR_TILE;
constexpr int OT = 256;            // threads: 16 x 16, a thread owns the pairs (pj + 16 a, pk + 16 b)
constexpr int OVERLAP_WORDS = 32;  // words of a row in LDS at a time
static_assert(PT == 32 && OT == (PT / 2) * (PT / 2), "a thread owns 2 x 2 pairs of the tile");

__global__ __launch_bounds__(OT) void merge_overlap_kernel(const MergeFrameJob job) {
  __shared__ uint64_t sJ[PT][OVERLAP_WORDS + 1], sK[PT][OVERLAP_WORDS + 1];  // (+ 1: rows a bank apart)
  const int K = (int)job.n_poses;
  const int W = (int)merge_row_words(job.pts.n);
  const int tid = threadIdx.x;
  // tile (tj, tk), tj <= tk, of the linear order (0,0) (0,1) (1,1) (0,2) ...
  int tk = 0, tj = (int)blockIdx.x;
  while (tj > tk) { tj -= tk + 1; tk++; }
  const int pj = tid >> 4, pk = tid & 15;
  uint32_t acc[2][2] = {{0u, 0u}, {0u, 0u}};
  for (int w0 = 0; w0 < W; w0 += OVERLAP_WORDS) {
    for (int x = tid; x < PT * OVERLAP_WORDS; x += OT) {
      const int r = x / OVERLAP_WORDS, w = x % OVERLAP_WORDS;
      const int j = tj * PT + r, k = tk * PT + r;
      const bool in = w0 + w < W;
      sJ[r][w] = in && j < K ? job.rows[(size_t)j * W + w0 + w] : 0ull;
      sK[r][w] = in && k < K ? job.rows[(size_t)k * W + w0 + w] : 0ull;
    }
    __syncthreads();
#pragma unroll 4
    for (int w = 0; w < OVERLAP_WORDS; w++) {
      const uint64_t a0 = sJ[pj][w], a1 = sJ[pj + 16][w], b0 = sK[pk][w], b1 = sK[pk + 16][w];
      acc[0][0] += (uint32_t)__popcll(a0 & b0); acc[0][1] += (uint32_t)__popcll(a0 & b1);
      acc[1][0] += (uint32_t)__popcll(a1 & b0); acc[1][1] += (uint32_t)__popcll(a1 & b1);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) {
      const int j = tj * PT + pj + 16 * a, k = tk * PT + pk + 16 * b;
      if (j < K && k < K) {
        job.overlap[(size_t)j * K + k] = acc[a][b];
        job.overlap[(size_t)k * K + j] = acc[a][b];  // mirrored (a diagonal tile writes every cell twice, with one value)
      }
    }
}

// ---- decide
constexpr int DT = MERGE_DECIDE_THREADS;
constexpr int DW = DT / 64;                     // waves; words of a rank's same-bits at most

struct DecideLds {
  uint32_t c[DT], s[DT];
  int32_t st[DT], parent[DT];
  uint16_t order[DT];      // order[r]: the pose of rank r (0: the strongest)
  uint64_t same[2][64][DW];  // two rounds' same-bits (one walked, one built): rank rb + q against the stronger ranks, by rank
  uint64_t kept[DW];       // the waves' kept ballots, by pose number
  uint32_t valid[DW];
};

__global__ __launch_bounds__(DT) void merge_decide_kernel(const MergeFrameJob job) {
  __shared__ DecideLds L;
  const int K = (int)job.n_poses;
  const int k = threadIdx.x, wave = k >> 6, lane = k & 63;
  const MergeRule rule = job.rule;
  const uint32_t* const rec = reinterpret_cast<const uint32_t*>(static_cast<const char*>(job.pose) + (size_t)k * job.pose_stride);

  // ---- a thread per pose: its validity and its tallies
  if (k < K) {
    float M[ASSIGN_POSE_FLOATS];
    L.st[k] = assign_stage_pose(rec, job.status != 0, M);
    L.c[k] = job.tally[k];
    L.s[k] = job.tally[K + k];
  }
  __syncthreads();
  // ---- the strength order
  if (k < K) {
    const uint32_t sk = L.s[k];
    int rank = 0;
    for (int j = 0; j < K; j++) rank += merge_stronger(L.s[j], j, sk, k) ? 1 : 0;
    L.order[rank] = (uint16_t)k;
  }
  __syncthreads();

  // ---- the fold, 64 ranks a round: wave 0 walks a round while the other waves build the next round's same-bits
  // same-bits of the ranks rb .. rb + 63 against the stronger ranks -> L.same[buf]; the waves first .. DW - 1 share the 64 ranks
  auto build_round = [&](int rb, int buf, int first) {
    for (int q = wave - first; q < 64; q += DW - first) {
      const int r = rb + q;
      if (r >= K) break;  // (wave-uniform)
      const int kk = L.order[r];
      const uint32_t ck = L.c[kk];
      const uint32_t* const row = job.overlap + (size_t)kk * K;
      const int nw = r / 64 + 1;
      // every word's table cell first, all loads in flight together: one trip to the table a rank, not one a word
      uint32_t x[DW], cj[DW];
#pragma unroll
      for (int w = 0; w < DW; w++) {
        const int rj = w * 64 + lane;
        x[w] = 0u; cj[w] = 0u;
        if (w < nw && rj < r) {  // the stronger ranks only
          const int j = L.order[rj];
          x[w] = row[j]; cj[w] = L.c[j];
        }
      }
#pragma unroll
      for (int w = 0; w < DW; w++) {
        if (w < nw) {  // (wave-uniform)
          const uint64_t word = __ballot(merge_same(x[w], cj[w], ck, rule));  // (x == 0: never the same)
          if (lane == 0) L.same[buf][q][w] = word;
        }
      }
    }
  };
  uint64_t kept = 0ull;  // wave 0: lane w holds the kept ranks 64 w .. 64 w + 63
  build_round(0, 0, 0);
  __syncthreads();
  for (int rb = 0, buf = 0; rb < K; rb += 64, buf ^= 1) {
    if (wave != 0) {
      if (rb + 64 < K) build_round(rb + 64, buf ^ 1, 1);
    } else {
      // lane q is rank rb + q: its pose, may it be kept or folded, and — in a register until the round is walked — its fate
      const bool there = rb + lane < K;
      const int mine = there ? (int)L.order[rb + lane] : 0;
      const uint64_t eligible = __ballot(there && merge_eligible(L.st[mine], L.c[mine], rule));
      int into = -1;  // the RANK this pose goes to (its own: kept); -1: invalid, or dropped
      for (int q = 0; q < 64; q++) {
        if (!((eligible >> q) & 1ull)) continue;  // (wave-uniform; no rank past K is eligible)
        const int r = rb + q;
        const uint64_t hit = lane <= r / 64 ? (L.same[buf][q][lane] & kept) : 0ull;
        const uint64_t any = __ballot(hit != 0ull);
        int to = r;
        if (any == 0ull) {
          if (lane == r / 64) kept |= 1ull << (r & 63);
        } else {
          const int w = __ffsll((unsigned long long)any) - 1;
          to = w * 64 + __ffsll((unsigned long long)__shfl(hit, w)) - 1;  // the lowest kept rank that is the same: the strongest
        }
        into = lane == q ? to : into;
      }
      if (there) L.parent[mine] = into < 0 ? -1 : (int32_t)L.order[into];
    }
    __syncthreads();
  }

  // ---- the records, the parents, the count words
  const bool is_kept = k < K && L.parent[k] == k, is_valid = k < K && L.st[k] == SC_OK;
  const uint64_t bk = __ballot(is_kept), bv = __ballot(is_valid);
  if (lane == 0) { L.kept[wave] = bk; L.valid[wave] = (uint32_t)__popcll(bv); }
  __syncthreads();
  uint32_t n_kept = 0, n_valid = 0, before = 0;  // before: kept poses with a lower number
  for (int w = 0; w < DW; w++) {
    const uint32_t p = (uint32_t)__popcll(L.kept[w]);
    n_kept += p; n_valid += L.valid[w];
    before += w < wave ? p : 0u;
  }
  before += (uint32_t)__popcll(bk & ((1ull << lane) - 1ull));
  if (k < K) {
    const uint32_t pos = !rule.compact ? (uint32_t)k : (is_kept ? before : n_kept + ((uint32_t)k - before));
    merge_store_record(job.out + pos, rec, L.st[k], L.parent[k], k, L.c[k], L.s[k]);
    job.parent[k] = L.parent[k];
  }
  if (k == 0 && job.count) { job.count[0] = n_kept; job.count[1] = n_valid; }
}

}  // namespace

void launch_merge_frame(const MergeFrameJob& job, hipStream_t st) {
  const uint32_t K = job.n_poses, T = (K + PT - 1) / PT;
  hipLaunchKernelGGL(merge_support_kernel, dim3((uint32_t)((job.pts.n + MERGE_TILE - 1) / MERGE_TILE)), dim3(MT), assign_frame_lds_bytes(K), st, job);
  hipLaunchKernelGGL(merge_overlap_kernel, dim3(T * (T + 1) / 2), dim3(OT), 0, st, job);
  hipLaunchKernelGGL(merge_decide_kernel, dim3(1), dim3(DT), 0, st, job);
}

}  // namespace sc
