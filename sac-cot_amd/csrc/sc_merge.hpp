// sc_merge.hpp — what the kernels of sc_merge_poses share (include/saccot.h; sc_merge_frame.hip, sc_merge_batch.hip), once each: a
// wave's 64 inlier decisions for one pose as ONE word with their tallies, the overlap of two bit rows, the strength order, same(j, k),
// a pose's fate and its record.  The pose records, their validity and the selection are sc_assign.hpp's: an invalid pose is staged as
// twelve NaNs, so its bit row is zero and it overlaps nothing — "an invalid pose claims nothing" stays a property of the arithmetic.
#pragma once
#include "sc_assign.hpp"
#include "sc_kernels.hpp"

namespace sc {

constexpr int MERGE_TILE = ASSIGN_TILE;        // correspondences of one workgroup of the support launch: eight words of every bit row
constexpr int MERGE_THREADS = ASSIGN_THREADS;  // its threads: four waves, a lane owns MERGE_TILE / MERGE_THREADS correspondences
constexpr int MERGE_PAIR_TILE = 32;            // poses a side of one workgroup of the overlap launch
constexpr int MERGE_DECIDE_THREADS = 1024;     // the decide launch: ONE workgroup, a thread per pose
static_assert(MERGE_TILE % 64 == 0 && MERGE_THREADS % 64 == 0, "a wave's 64 lanes own 64 consecutive correspondences: one word");

__device__ __forceinline__ uint32_t merge_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Pose k (M: its twelve floats, NaN if invalid) against this lane's correspondence: the wave's 64 decisions cand(k, m) as one word —
// bit l is lane l's — with the wave's count and its summed score terms (0 for an empty word), the same in every lane.  Called by
// whole waves, uniformly.
struct MergeWord {
  uint64_t word;
  uint32_t members, terms;
};
__device__ __forceinline__ MergeWord merge_support_word(const float* M, const Corr& c, bool part, float tau2, float thr, int score_mode) {
  const float d2 = resid2(M, c.v[0], c.v[1], c.v[2], c.v[3], c.v[4], c.v[5]);
  const bool cand = part && d2 < tau2;
  MergeWord w;
  w.word = __ballot(cand);
  w.members = (uint32_t)__popcll(w.word);
  w.terms = w.members;
  if (score_mode != 0 && w.word != 0) w.terms = merge_wave_sum(cand ? assign_score(d2, thr, score_mode) : 0u);  // (wave-uniform)
  return w;
}
// What a wave found for 64 consecutive poses, a pose a lane: lane i keeps pose kb + i's words (one per correspondence the lane owns)
// and tally, so that the wave stores and adds ONCE per 64 poses — a store and two LDS atomics with 64 addresses — and not per pose.
template <int U>
struct MergeKeep {
  uint64_t word[U];
  uint32_t members, terms;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int u = 0; u < U; u++) word[u] = 0ull;
    members = terms = 0u;
  }
  __device__ __forceinline__ void take(int u, bool mine, const MergeWord& w) {  // mine: this lane is the pose's
    word[u] = mine ? w.word : word[u];
    members += mine ? w.members : 0u;
    terms += mine ? w.terms : 0u;
  }
  // (a workgroup holds at most MERGE_TILE correspondences of at most 1024 units: 32 bits)
  __device__ __forceinline__ void add_to(uint32_t* cnt, uint32_t* score) const {
    if (members) { atomicAdd(cnt, members); atomicAdd(score, terms); }
  }
};

// x_jk over `words` words of two bit rows
__device__ __forceinline__ uint32_t merge_overlap(const uint64_t* a, const uint64_t* b, int words) {
  uint32_t x = 0;
  for (int w = 0; w < words; w++) x += (uint32_t)__popcll(a[w] & b[w]);
  return x;
}

// strength: larger score first, ties to the lower pose number
__device__ __forceinline__ bool merge_stronger(uint32_t sj, int j, uint32_t sk, int k) { return sj > sk || (sj == sk && j < k); }

// same(j, k): integers only
__device__ __forceinline__ bool merge_same(uint32_t x, uint32_t cj, uint32_t ck, const MergeRule& r) {
  const uint64_t base = r.measure == SC_MERGE_OVER_UNION ? (uint64_t)cj + ck - x : (uint64_t)min(cj, ck);
  return x >= 1u && (uint64_t)x * r.den >= (uint64_t)r.num * base;
}

// may pose k be kept, or be folded?  (else its parent is -1: invalid, or dropped)
__device__ __forceinline__ bool merge_eligible(int status, uint32_t count, const MergeRule& r) { return status == SC_OK && count >= r.min_count; }

// Pose k's record from its fate.  status: the staged pose's (assign_stage_pose); parent: k kept, another pose folded, -1 dropped or
// invalid; rt: the input record's twelve words (read only for a kept pose).  Dword stores: the caller's array is 4-byte aligned.
__device__ __forceinline__ void merge_store_record(MergeRecord* out, const uint32_t* rt, int status, int parent, int k, uint32_t count,
                                                   uint32_t score) {
  uint32_t* const w = reinterpret_cast<uint32_t*>(out);
  const bool kept = parent == k;
  const bool valid = status == SC_OK;
#pragma unroll
  for (int c = 0; c < 12; c++) w[c] = kept ? rt[c] : __float_as_uint((c == 0 || c == 4 || c == 8) ? 1.f : 0.f);
  w[12] = (uint32_t)(kept ? SC_OK : (valid ? SC_ENOHYP : status));
  w[13] = (uint32_t)parent;
  w[14] = valid ? count : 0u;
  w[15] = valid ? score : 0u;
}

}  // namespace sc
