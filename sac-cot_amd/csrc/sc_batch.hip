// sc_batch.hip — many small registrations in one launch (include/saccot.h, sc_register_batch): the kernel.
//
// One workgroup of 256 threads per problem, grid = n_problems, nothing shared between workgroups: no global atomics, no waits, no
// second launch.  A problem of n <= 512 correspondences lives in LDS — six planes of points (12 KB), the adjacency bit rows
// (ceil(n / 64) u64 per row, 32 KB at most), the degrees — and every stage of sc_register runs on it with the canonical device
// code of sc_arith.hpp and the order of sc_winner.hpp, so a problem's record equals what sc_register returns for it alone:
//
//   staging   either layout -> the planes, the finiteness test on the way (a non-finite coordinate: SC_EINVAL for THIS problem);
//             this, and how a record and a zero mask are written, is sc_batch_frame.hpp's, shared with sc_polish_batch.hip
//   stage A   a wave per (row, 64 columns): one pair test per lane (pair_weight on dist3), the wave's ballot IS the bit word; degrees
//             by popcount.  No dense S: an edge weight is recomputed from the points where a key needs it (the same bits).
//   stage B   no list.  The triangles i < j < k are ENUMERATED (TriIter: bits_i & bits_j above j), as often as a step needs them:
//             once to count; if there are more than T, four times for a radix select of the T-th largest key K* (256-bin LDS
//             histogram per 8-bit digit), and for the ties at K* — kept in ascending (i, j, k) up to T — once over all rows, once over
//             the one row the cut falls in, once over the one edge: the cut is then ONE packed triple, and "kept" is
//             key > K* || (key == K* && (i, j, k) <= cut).
//   C1 + C2   one more enumeration: a thread advances to its next kept triangle, solves it (kabsch3) and scores it over the n
//             points in LDS (score_term; every lane reads the same point: a broadcast); the winner under the frame's total order —
//             score, then key, then lowest (i, j, k) — by a lexicographic maximum of two words.
//   rank      best_rank = the kept triangles that outrank the winner: a counting enumeration.
//   C3        the winner's mask (is_inlier), and the record, staged in LDS and stored one dword per lane.
//
// Work items of an enumeration are (row, 16 columns), dealt by an LDS ticket: rows of an inlier hold most of the triangles, and a
// static deal would leave most lanes waiting for a few.  Cost: (triangles of the graph) x (passes: 3 .. 10) + (kept triangles) x n.
//
// sc_register_instances_batch is the same kernel with ROUNDS: after the frame the workgroup still holds the planes, the bit rows, K*
// and the cut, and a round of sc_peel is the C1 + C2 enumeration once more — every kept triangle scored over the correspondences no
// earlier motion claimed (a bit per correspondence in LDS; the scoring loop is a broadcast, so skipping a claimed one is a decision
// of the whole wave) —, the rank enumeration, and the winner's mask among the alive ones.  So the kernel's tail is ONE loop over
// rounds, the frame being round 0: up to max_instances passes, left at the first round that scores nothing or less than min_score.
// Without ROUNDS the loop is its first pass: the instantiations of sc_register_batch hold nothing of the rounds, and their code is
// what it was before there were any.
#include <type_traits>

#include "../../include/saccot.h"
#include "sc_arith.hpp"
#include "sc_batch_frame.hpp"
#include "sc_block.hpp"
#include "sc_winner.hpp"

namespace sc {

static_assert(sizeof(BatchRecord) == sizeof(sc_batch_result) && sizeof(BatchRecord) == 80 && BATCH_MAX_N == SC_BATCH_MAX_N,
              "BatchRecord is sc_batch_result, 80 bytes");
static_assert(INSTANCES_BATCH_MAX == SC_INSTANCES_BATCH_MAX && INSTANCES_BATCH_MAX <= 127, "a motion's index fits a label byte");

namespace {

constexpr int BT = 256;            // threads of a workgroup (block_max_u64 / block_lexmax_u64 are written for 256)
constexpr int BN = BATCH_MAX_N;    // correspondences of a problem at most
constexpr int REC_WORDS = sizeof(BatchRecord) / 4;

struct alignas(16) BatchLds {
  float pt[6][BN];                 // px py pz qx qy qz (the scoring loop reads 16 bytes of a plane at a time)
  uint64_t bits[BN * (BN / 64)];   // row i at bits + i * W, W = ceil(n / 64): the rows are packed to the problem's own width
  uint32_t deg[BN];
  uint32_t cnt[BN];                // the ties at K*: per row, then per j of one row, then per k of one edge
  uint32_t hist[256];
  uint64_t red[8];                 // scratch of the workgroup reductions
  uint32_t ticket;                 // next work item of the enumeration under way
  uint32_t bad;
  uint32_t prefix, above, eq;      // the radix select: digits fixed so far, keys above them, keys in the chosen bin
  uint32_t cut_idx, cut_rem;
  uint32_t rec[REC_WORDS];
};
static_assert(sizeof(BatchLds) < 64 * 1024, "static LDS");
// with rounds: who is still alive (bit m & 63 of word m >> 6; bits from n on are clear) and which motion claimed whom (-1: none)
struct alignas(16) RoundsLds : BatchLds {
  uint64_t alive[BN / 64];
  int8_t label[BN];
};
static_assert(3 * sizeof(RoundsLds) <= 160 * 1024, "three workgroups a compute unit, as without rounds");

__device__ __forceinline__ uint32_t pack3(int i, int j, int k) { return ((uint32_t)i << 18) | ((uint32_t)j << 9) | (uint32_t)k; }
// is the triangle with this key and packed (i, j, k) among the top T?  (kstar = 0, cut all ones: every triangle is)
__device__ __forceinline__ bool is_kept(uint32_t key, uint32_t pk, uint32_t kstar, uint32_t cut) {
  return key > kstar || (key == kstar && pk <= cut);
}

// weight of edge (a, b), a < b: S[a][b] of the dense matrix, recomputed
__device__ __forceinline__ float edge_weight(const BatchLds& L, int a, int b, const Derived& dv) {
  const float dp = dist3(L.pt[0][a], L.pt[1][a], L.pt[2][a], L.pt[0][b], L.pt[1][b], L.pt[2][b]);
  const float dq = dist3(L.pt[3][a], L.pt[4][a], L.pt[5][a], L.pt[3][b], L.pt[4][b], L.pt[5][b]);
  bool edge;
  return pair_weight(dp, dq, dv.d_thr, dv.min_len, dv.neg_inv2sig2, edge);
}

// A new enumeration: items [first, ...) are dealt from the ticket.  The barriers also close the pass before.
__device__ __forceinline__ void pass_begin(BatchLds& L, uint32_t first) {
  __syncthreads();
  if (threadIdx.x == 0) L.ticket = first;
  __syncthreads();
}

// The triangles i < j < k of the items this thread draws, one per next().  An item is (row i, columns [16 c, 16 c + 16)); items
// [.., end) of the flattened (row, c) index.  new_edge: (i, j) changed since the caller last cleared it.
struct TriIter {
  BatchLds& L;
  const int W, chunks;
  const uint32_t end;
  int i = 0, j = -1, k = 0, jbase = 0, wk = 0;
  uint32_t mj = 0;
  uint64_t mk = 0;
  bool new_edge = false;
  const uint64_t* bi = nullptr;
  const uint64_t* bj = nullptr;

  __device__ TriIter(BatchLds& lds, int n, uint32_t end_item) : L(lds), W((n + 63) >> 6), chunks((n + 15) >> 4), end(end_item) {}

  // the next item's row and its edges (i, j), j > i, of the item's 16 columns; false: none left
  __device__ __forceinline__ bool next_item() {
    const uint32_t e = atomicAdd(&L.ticket, 1u);
    if (e >= end) return false;
    i = (int)(e / (uint32_t)chunks);
    jbase = ((int)e - i * chunks) << 4;
    mj = 0;
    if (jbase + 15 > i) {
      bi = L.bits + i * W;
      mj = (uint32_t)(bi[jbase >> 6] >> (jbase & 63)) & 0xFFFFu;
      if (jbase <= i) mj &= ~((2u << (i - jbase)) - 1u);  // columns above i only
    }
    return true;
  }
  __device__ __forceinline__ bool next_edge() {  // (i, j) <- the item's next edge
    if (!mj) return false;
    j = jbase + __builtin_ctz(mj);
    mj &= mj - 1;
    bj = L.bits + j * W;
    wk = j >> 6;
    mk = bi[wk] & bj[wk] & mask_above(j & 63);
    new_edge = true;
    return true;
  }
  __device__ __forceinline__ bool next() {
    for (;;) {
      if (mk) { k = (wk << 6) + __builtin_ctzll(mk); mk &= mk - 1; return true; }
      if (j >= 0 && ++wk < W) { mk = bi[wk] & bj[wk]; continue; }
      if (next_edge()) continue;
      j = -1;
      if (!next_item()) return false;
    }
  }
};

// the ranking key of the iterator's triangle; s_ij: the caller's cache of the current edge's weight
__device__ __forceinline__ uint32_t tri_key(const BatchLds& L, TriIter& it, const Derived& dv, int rank_mode, float& s_ij) {
  if (rank_mode == SC_RANK_DEGREE) return L.deg[it.i] + L.deg[it.j] + L.deg[it.k];
  if (it.new_edge) { s_ij = edge_weight(L, it.i, it.j, dv); it.new_edge = false; }
  return tri_key_weight(s_ij, edge_weight(L, it.i, it.k, dv), edge_weight(L, it.j, it.k, dv));
}

// L.cnt holds BN counts; entry x and the remainder r with  sum(cnt[0 .. x)) < need <= sum(cnt[0 .. x]),  r = need - sum(cnt[0 .. x)).
// 1 <= need <= the sum of all.  A thread scans two consecutive entries.
__device__ __forceinline__ void find_cut(BatchLds& L, uint32_t need, uint32_t& idx, uint32_t& rem) {
  static_assert(BN == 2 * BT, "two entries per thread");
  const uint32_t v0 = L.cnt[2 * threadIdx.x], v1 = L.cnt[2 * threadIdx.x + 1];
  uint64_t total;
  const uint32_t pre = (uint32_t)block_exscan_u64((uint64_t)v0 + v1, L.red, &total);
  if (pre < need && need <= pre + v0) { L.cut_idx = 2 * threadIdx.x; L.cut_rem = need - pre; }
  else if (pre + v0 < need && need <= pre + v0 + v1) { L.cut_idx = 2 * threadIdx.x + 1; L.cut_rem = need - pre - v0; }
  __syncthreads();
  idx = L.cut_idx; rem = L.cut_rem;
}

// the record and nothing else: identity unless Rt is given
__device__ __forceinline__ void record_fill(BatchLds& L, const float* Rt, int status, uint32_t n, uint32_t edges, uint32_t kept,
                                            uint32_t total, uint32_t rank, uint32_t count) {
  record_pose(L.rec, Rt);
  L.rec[12] = (uint32_t)status; L.rec[13] = n; L.rec[14] = edges; L.rec[15] = kept;
  L.rec[16] = total; L.rec[17] = 0u;  // tri_total, u64: at most C(512, 3)
  L.rec[18] = rank; L.rec[19] = count;
}

// ---- rounds (sc_register_instances_batch)
// The score of (R, t) over the alive correspondences: the set bits of L.alive (bits from n on are clear).  Four correspondences of
// the planes at a time, as the frame's loop reads them; the planes hold BN entries, so a group of four that straddles n is read and
// not counted.  Sums of integers: no order matters.
__device__ __forceinline__ uint32_t score_alive(const RoundsLds& L, const float* M, int n, float thr, int mode) {
  uint32_t score = 0u;
  for (int w = 0; 64 * w < n; w++) {
    const uint64_t a = L.alive[w];
    for (int q = 0; q < 16 && (a >> (4 * q)) != 0ull; q++) {
      const uint32_t take = (uint32_t)(a >> (4 * q)) & 15u;
      if (!take) continue;
      float4 c6[6];
#pragma unroll
      for (int c = 0; c < 6; c++) c6[c] = *reinterpret_cast<const float4*>(&L.pt[c][64 * w + 4 * q]);
      if (take & 1u) score += score_term(M, c6[0].x, c6[1].x, c6[2].x, c6[3].x, c6[4].x, c6[5].x, thr, mode);
      if (take & 2u) score += score_term(M, c6[0].y, c6[1].y, c6[2].y, c6[3].y, c6[4].y, c6[5].y, thr, mode);
      if (take & 4u) score += score_term(M, c6[0].z, c6[1].z, c6[2].z, c6[3].z, c6[4].z, c6[5].z, thr, mode);
      if (take & 8u) score += score_term(M, c6[0].w, c6[1].w, c6[2].w, c6[3].w, c6[4].w, c6[5].w, thr, mode);
    }
  }
  return score;
}
// motion r claims the alive inliers of (R, t).  Correspondence tid + 256 u lies in word wave + 4 u: a wave's ballot is its own word.
__device__ __forceinline__ void claim(RoundsLds& L, const float* M, int n, float tau2, uint32_t r) {
  static_assert(BT % 64 == 0 && BN % BT == 0 && BN % 64 == 0, "whole waves, whole strides: a wave owns the alive word it updates");
#pragma unroll
  for (int u = 0; u < BN / BT; u++) {
    const int m = (int)threadIdx.x + BT * u;
    const bool take = m < n && ((L.alive[m >> 6] >> (m & 63)) & 1ull) && is_inlier(M, load_corr(&L.pt[0][0], BN, m), tau2);
    const uint64_t taken = __ballot(take);
    if (take) L.label[m] = (int8_t)r;
    if ((threadIdx.x & 63) == 0) L.alive[m >> 6] &= ~taken;
  }
}
// Planes [from, max_instances) of a problem: the record staged last with R = I, t = 0, no rank and no score, SC_ENOHYP unless the
// problem itself is SC_EINVAL — the counts stay plane 0's, which every record of the problem carries.
__device__ __forceinline__ void planes_empty(BatchLds& L, const BatchJob& job, uint32_t from, uint32_t max_instances) {
  __syncthreads();  // (the store of the record staged last has read it)
  if (threadIdx.x == 0) {
    record_pose(L.rec, nullptr);
    if (L.rec[12] != (uint32_t)SC_EINVAL) L.rec[12] = (uint32_t)SC_ENOHYP;
    L.rec[18] = 0u; L.rec[19] = 0u;
  }
  for (uint32_t k = from; k < max_instances; k++) record_store(L.rec, job.res + (size_t)k * job.n_problems);
}
// a problem without a motion: every label -1 (n of them; none for a flagged problem), nothing found, the further planes
__device__ __forceinline__ void rounds_none(BatchLds& L, const BatchJob& job, const BatchRounds& rd, uint32_t off, int n) {
  for (int m = threadIdx.x; m < n; m += BT) rd.label[off + m] = -1;
  if (threadIdx.x == 0) rd.nfound[blockIdx.x] = 0u;
  planes_empty(L, job, 1u, rd.max_instances);
}

// The kernel's argument is BatchJob (sc_register_batch) or BatchSlotJob (sc_register_batch_features: the problems sit in slots and
// `count` says how much of each is filled, sc_kernels.hpp), or one of the two with rounds (InstBatchJob, InstBatchSlotJob).  The
// plain instantiation is the kernel of sc_register_batch with the kernel argument it always had: COUNTED and ROUNDS are constants
// of the instantiation, and nothing of the slot form or of the rounds is compiled into it.
template <class Arg> struct ArgKind { static constexpr bool COUNTED = false, ROUNDS = false; };
template <> struct ArgKind<BatchSlotJob> { static constexpr bool COUNTED = true, ROUNDS = false; };
template <> struct ArgKind<InstBatchJob> { static constexpr bool COUNTED = false, ROUNDS = true; };
template <> struct ArgKind<InstBatchSlotJob> { static constexpr bool COUNTED = true, ROUNDS = true; };
__device__ __forceinline__ const uint32_t* count_of(const BatchJob&) { return nullptr; }
__device__ __forceinline__ const uint32_t* count_of(const BatchSlotJob& a) { return a.count; }
__device__ __forceinline__ const uint32_t* count_of(const InstBatchJob&) { return nullptr; }
__device__ __forceinline__ const uint32_t* count_of(const InstBatchSlotJob& a) { return a.count; }

template <class Arg>
__global__ __launch_bounds__(BT) void batch_register_kernel(const Arg arg) {
  constexpr bool COUNTED = ArgKind<Arg>::COUNTED, ROUNDS = ArgKind<Arg>::ROUNDS;
  const BatchJob& job = job_of(arg);
  const uint32_t* const count = count_of(arg);
  __shared__ std::conditional_t<ROUNDS, RoundsLds, BatchLds> L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t off = job.offset[blockIdx.x];
  const int n = COUNTED ? (int)count[2 * blockIdx.x] : (int)(job.offset[blockIdx.x + 1] - off);  // 3 .. BN: the host checked
  const int W = (n + 63) >> 6;
  const Derived dv = job.dv;
  uint8_t* const mask = job.mask + off;  // (with ROUNDS there is none: the labels take its place)
  if (COUNTED) {  // what the host refuses for the plain form, it cannot know here: the match decided it on the device
    const bool flagged = count[2 * blockIdx.x + 1] != 0u;
    if (flagged || n < 3 || n > BN) {  // (n > BN cannot happen: a slot's capacity is at most BN)
      if constexpr (!ROUNDS) {
        if (!flagged && n < 3) mask_zero<BT>(mask, n);
      }
      if (tid == 0) record_fill(L, nullptr, (flagged || n > BN) ? SC_EINVAL : SC_ENOHYP, flagged ? 0u : (uint32_t)n, 0u, 0u, 0u, 0u, 0u);
      record_store(L.rec, job.res);
      if constexpr (ROUNDS) rounds_none(L, job, arg.rounds, off, (!flagged && n < 3) ? n : 0);
      return;
    }
  }

  // ---- staging: either layout -> planes; a non-finite coordinate ends this problem
  if (tid == 0) L.bad = 0u;
  __syncthreads();
  if (stage_planes<BT>(L.pt, job.src, job.tgt, job.soa, job.total, off, n)) L.bad = 1u;
  __syncthreads();
  if (L.bad) {
    if constexpr (!ROUNDS) mask_zero<BT>(mask, n);
    if (tid == 0) record_fill(L, nullptr, SC_EINVAL, (uint32_t)n, 0u, 0u, 0u, 0u, 0u);
    record_store(L.rec, job.res);
    if constexpr (ROUNDS) rounds_none(L, job, arg.rounds, off, n);
    return;
  }

  // ---- stage A: a wave per (row, word); a lane per pair; the ballot is the word
  for (int e = wave; e < n * W; e += BT / 64) {
    const int i = e / W, w = e - i * W, j = (w << 6) + lane;
    bool edge = false;
    if (j < n && j != i) {
      const float dp = dist3(L.pt[0][i], L.pt[1][i], L.pt[2][i], L.pt[0][j], L.pt[1][j], L.pt[2][j]);
      const float dq = dist3(L.pt[3][i], L.pt[4][i], L.pt[5][i], L.pt[3][j], L.pt[4][j], L.pt[5][j]);
      (void)pair_weight(dp, dq, dv.d_thr, dv.min_len, dv.neg_inv2sig2, edge);
    }
    const uint64_t word = __ballot(edge);
    if (lane == 0) L.bits[e] = word;
  }
  __syncthreads();
  uint32_t edges;
  {
    uint32_t dsum = 0;
    for (int i = tid; i < n; i += BT) {
      uint32_t d = 0;
      for (int w = 0; w < W; w++) d += (uint32_t)__builtin_popcountll(L.bits[i * W + w]);
      L.deg[i] = d;
      dsum += d;
    }
    edges = (uint32_t)(block_reduce_u64(dsum, L.red) >> 1);
  }

  // ---- stage B: count
  const uint32_t items = (uint32_t)(n * ((n + 15) >> 4));
  uint32_t total;
  {
    pass_begin(L, 0u);
    TriIter it(L, n, items);
    uint32_t c = 0;
    while (it.next_item())
      while (it.next_edge()) {
        c += (uint32_t)__builtin_popcountll(it.mk);
        for (int w = it.wk + 1; w < W; w++) c += (uint32_t)__builtin_popcountll(it.bi[w] & it.bj[w]);
      }
    total = (uint32_t)block_reduce_u64(c, L.red);
  }
  const uint32_t kept_n = job.T < total ? job.T : total;
  if (total == 0u) {
    if constexpr (!ROUNDS) mask_zero<BT>(mask, n);
    if (tid == 0) record_fill(L, nullptr, SC_ENOHYP, (uint32_t)n, edges, 0u, 0u, 0u, 0u);
    record_store(L.rec, job.res);
    if constexpr (ROUNDS) rounds_none(L, job, arg.rounds, off, n);
    return;
  }

  // ---- stage B: more triangles than T — the T-th largest key K*, and the last tie that is kept
  uint32_t kstar = 0u, cut = 0xFFFFFFFFu;  // (every triangle is kept)
  if (total > job.T) {
    uint32_t prefix = 0u, above = 0u, eq = 0u;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
      const uint32_t fixed = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
      L.hist[tid] = 0u;
      pass_begin(L, 0u);
      TriIter it(L, n, items);
      float s_ij = 0.f;
      while (it.next()) {
        const uint32_t key = tri_key(L, it, dv, job.rank_mode, s_ij);
        if ((key & fixed) == prefix) atomicAdd(&L.hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (wave == 0) {  // bins in descending order, four per lane: the bin in which the count above reaches T
        uint32_t h[4], s = 0u;
#pragma unroll
        for (int u = 0; u < 4; u++) { h[u] = L.hist[255 - (4 * lane + u)]; s += h[u]; }
        const uint32_t inc = wave_inscan(s);
        const uint64_t crossed = __ballot(above + inc >= job.T);
        if (crossed != 0ull && lane == __builtin_ctzll(crossed)) {
          uint32_t a = above + inc - s;
          int u = 0;
          while (u < 3 && a + h[u] < job.T) { a += h[u]; u++; }
          L.prefix = prefix | ((uint32_t)(255 - (4 * lane + u)) << shift);
          L.above = a;
          L.eq = h[u];
        }
      }
      __syncthreads();
      prefix = L.prefix; above = L.above; eq = L.eq;
    }
    kstar = prefix;
    const uint32_t need_eq = job.T - above;  // 1 .. eq ties are kept, in ascending (i, j, k)
    if (need_eq < eq) {
      uint32_t ci, cj, ck, rem;
      {  // ties per row
        L.cnt[2 * tid] = 0u; L.cnt[2 * tid + 1] = 0u;
        pass_begin(L, 0u);
        TriIter it(L, n, items);
        float s_ij = 0.f;
        while (it.next())
          if (tri_key(L, it, dv, job.rank_mode, s_ij) == kstar) atomicAdd(&L.cnt[it.i], 1u);
        __syncthreads();
        find_cut(L, need_eq, ci, rem);
      }
      {  // ties per j of row ci
        L.cnt[2 * tid] = 0u; L.cnt[2 * tid + 1] = 0u;
        const uint32_t chunks = (uint32_t)((n + 15) >> 4);
        pass_begin(L, ci * chunks);
        TriIter it(L, n, (ci + 1u) * chunks);
        float s_ij = 0.f;
        while (it.next())
          if (tri_key(L, it, dv, job.rank_mode, s_ij) == kstar) atomicAdd(&L.cnt[it.j], 1u);
        __syncthreads();
        find_cut(L, rem, cj, rem);
      }
      {  // the ties of edge (ci, cj), a k per entry
        __syncthreads();
        const uint64_t* bi = L.bits + ci * W;
        const uint64_t* bj = L.bits + cj * W;
        const float s_ij = job.rank_mode == SC_RANK_DEGREE ? 0.f : edge_weight(L, (int)ci, (int)cj, dv);
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const int k = 2 * tid + u;
          uint32_t tie = 0u;
          if (k > (int)cj && k < n && ((bi[k >> 6] & bj[k >> 6]) >> (k & 63)) & 1ull) {
            const uint32_t key = job.rank_mode == SC_RANK_DEGREE
                                     ? L.deg[ci] + L.deg[cj] + L.deg[k]
                                     : tri_key_weight(s_ij, edge_weight(L, (int)ci, k, dv), edge_weight(L, (int)cj, k, dv));
            tie = key == kstar ? 1u : 0u;
          }
          L.cnt[k] = tie;
        }
        __syncthreads();
        find_cut(L, rem, ck, rem);
      }
      cut = pack3((int)ci, (int)cj, (int)ck);
    }
  }

  // ---- stages C1 + C2, the winner, its rank and its mask: once for the frame (round 0) and, with ROUNDS, once more per round of
  // sc_peel — the same enumerations, scored over the correspondences no earlier motion claimed.  Without ROUNDS the loop is its
  // first pass and nothing else.
  const float thr = score_thr(dv, job.score_mode);
  unsigned long long k0 = 0ull, k1 = 0ull;
  uint32_t found = 0u;  // (with ROUNDS) motions found so far
  for (uint32_t round = 0u;; round++) {
    // every kept triangle solved and scored; the winner by (score, key, lowest (i, j, k))
    {
      pass_begin(L, 0u);
      TriIter it(L, n, items);
      float s_ij = 0.f;
      for (;;) {
        bool have = false;
        uint32_t key = 0u, pk = 0u;
        while (it.next()) {  // this thread's next kept triangle
          key = tri_key(L, it, dv, job.rank_mode, s_ij);
          pk = pack3(it.i, it.j, it.k);
          if (is_kept(key, pk, kstar, cut)) { have = true; break; }
        }
        if (!have) break;
        float P[9], Q[9], M[12];
        const int v[3] = {it.i, it.j, it.k};
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
          for (int c = 0; c < 3; c++) { P[3 * m + c] = L.pt[c][v[m]]; Q[3 * m + c] = L.pt[3 + c][v[m]]; }
        kabsch3(P, Q, M);
        uint32_t score = 0u;
        if (finite12(M)) {
          bool over_all = true;
          if constexpr (ROUNDS) {
            if (round) {  // the alive ones only: the same word in every lane, so what is skipped, the whole wave skips
              over_all = false;
              score = score_alive(L, M, n, thr, job.score_mode);
            }
          }
          if (over_all) {
            int m = 0;
            for (; m + 4 <= n; m += 4) {  // (every lane reads the same 16 bytes of a plane: a broadcast)
              float4 c6[6];
#pragma unroll
              for (int c = 0; c < 6; c++) c6[c] = *reinterpret_cast<const float4*>(&L.pt[c][m]);
              score += score_term(M, c6[0].x, c6[1].x, c6[2].x, c6[3].x, c6[4].x, c6[5].x, thr, job.score_mode);
              score += score_term(M, c6[0].y, c6[1].y, c6[2].y, c6[3].y, c6[4].y, c6[5].y, thr, job.score_mode);
              score += score_term(M, c6[0].z, c6[1].z, c6[2].z, c6[3].z, c6[4].z, c6[5].z, thr, job.score_mode);
              score += score_term(M, c6[0].w, c6[1].w, c6[2].w, c6[3].w, c6[4].w, c6[5].w, thr, job.score_mode);
            }
            for (; m < n; m++)
              score += score_term(M, L.pt[0][m], L.pt[1][m], L.pt[2][m], L.pt[3][m], L.pt[4][m], L.pt[5][m], thr, job.score_mode);
          }
        }
        if (score) lexmax_take(k0, k1, ((unsigned long long)score << 32) | key, (unsigned long long)(~pk));
      }
      block_lexmax_u64(k0, k1, reinterpret_cast<unsigned long long*>(L.red));
    }
    if constexpr (ROUNDS) {
      if (round && (k0 == 0ull || (uint32_t)(k0 >> 32) < arg.rounds.min_score)) break;  // the round stops the problem
    }
    if (k0 == 0ull) {  // no hypothesis has an inlier
      if constexpr (!ROUNDS) mask_zero<BT>(mask, n);
      if (tid == 0) record_fill(L, nullptr, SC_ENOHYP, (uint32_t)n, edges, kept_n, total, 0u, 0u);
      record_store(L.rec, job.res);
      if constexpr (ROUNDS) rounds_none(L, job, arg.rounds, off, n);
      return;
    }

    // the winner: its (R, t) again (the same bits), its rank among the kept, its mask
    const uint32_t wkey = (uint32_t)k0, wpk = ~(uint32_t)k1;
    float M[12];
    {
      float P[9], Q[9];
      const int v[3] = {(int)(wpk >> 18), (int)((wpk >> 9) & 511u), (int)(wpk & 511u)};
#pragma unroll
      for (int m = 0; m < 3; m++)
#pragma unroll
        for (int c = 0; c < 3; c++) { P[3 * m + c] = L.pt[c][v[m]]; Q[3 * m + c] = L.pt[3 + c][v[m]]; }
      kabsch3(P, Q, M);
    }
    uint32_t rank;
    {
      pass_begin(L, 0u);
      TriIter it(L, n, items);
      float s_ij = 0.f;
      uint32_t r = 0u;
      while (it.next()) {
        const uint32_t key = tri_key(L, it, dv, job.rank_mode, s_ij), pk = pack3(it.i, it.j, it.k);
        if (is_kept(key, pk, kstar, cut) && outranks(key, pk, wkey, wpk)) r++;
      }
      rank = (uint32_t)block_reduce_u64(r, L.red);
    }
    if constexpr (!ROUNDS) {
      for (int m = tid; m < n; m += BT) mask[m] = is_inlier(M, load_corr(&L.pt[0][0], BN, m), dv.tau2) ? 1 : 0;
      if (tid == 0) record_fill(L, M, SC_OK, (uint32_t)n, edges, kept_n, total, rank, (uint32_t)(k0 >> 32));
      record_store(L.rec, job.res);
      break;
    } else {
      const BatchRounds& rd = arg.rounds;
      if (round == 0u) {  // everyone is alive; motion 0 is the frame's winner if it scores min_score
        for (int m = tid; m < BN; m += BT) L.label[m] = -1;
        if (tid < BN / 64) L.alive[tid] = 64 * tid + 64 <= n ? ~0ull : (64 * tid < n ? (1ull << (n & 63)) - 1ull : 0ull);
        __syncthreads();
      }
      if (tid == 0) record_fill(L, M, SC_OK, (uint32_t)n, edges, kept_n, total, rank, (uint32_t)(k0 >> 32));
      record_store(L.rec, job.res + (size_t)round * job.n_problems);
      if ((uint32_t)(k0 >> 32) < rd.min_score) break;  // (round 0 only: plane 0 is written whatever min_score is)
      claim(L, M, n, dv.tau2, round);  // (the next pass's first barrier publishes it)
      found = round + 1u;
      if (found == rd.max_instances) break;
      k0 = 0ull; k1 = 0ull;
    }
  }
  if constexpr (ROUNDS) {  // the labels, the count, and the planes without a motion
    const BatchRounds& rd = arg.rounds;
    __syncthreads();
    for (int m = tid; m < n; m += BT) rd.label[off + m] = L.label[m];
    if (tid == 0) rd.nfound[blockIdx.x] = found;
    planes_empty(L, job, found ? found : 1u, rd.max_instances);
  }
}

}  // namespace

void launch_batch_register(const BatchJob& job, hipStream_t st) {
  hipLaunchKernelGGL(batch_register_kernel<BatchJob>, dim3(job.n_problems), dim3(BT), 0, st, job);
}

void launch_batch_register_slots(const BatchSlotJob& job, hipStream_t st) {
  hipLaunchKernelGGL(batch_register_kernel<BatchSlotJob>, dim3(job.job.n_problems), dim3(BT), 0, st, job);
}

void launch_instances_batch(const InstBatchJob& job, hipStream_t st) {
  hipLaunchKernelGGL(batch_register_kernel<InstBatchJob>, dim3(job.job.n_problems), dim3(BT), 0, st, job);
}

void launch_instances_batch_slots(const InstBatchSlotJob& job, hipStream_t st) {
  hipLaunchKernelGGL(batch_register_kernel<InstBatchSlotJob>, dim3(job.job.n_problems), dim3(BT), 0, st, job);
}

}  // namespace sc
