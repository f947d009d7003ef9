// sc_tri_prune.hip — stage B, the pruning: the samples, the bound and the strong graph they give; sharded, the cut by its work
// (sc_tri.hpp: the pipeline).
#include <cstring>

#include "sc_tri.hpp"

namespace sc {

// ------------------------------------------------------------------------------------------------
// 3b. certified pruning (weight ranking only)
//
// Claim: let LB be any value such that at least T triangles have key >= LB.  Then the top-T list of the full graph
// equals the top-T list of the subgraph of "strong" edges, s >= smin := LB - 2 - 1e-6.
// Proof: w = fl(fl(a+b)+c) with a,b,c in (0,1] satisfies w <= a+b+c + 5*2^-24, so a triangle with w >= LB has every
// edge >= LB - 2 - 3e-7 > smin: all triangles with key >= LB live in the strong subgraph, there are >= T of them, and
// every triangle outside it has key < LB, i.e. strictly below at least T others — it cannot enter the top-T, ties
// included.  Ordinals keep their relative order (same CSR edge order, same ascending k), so the tie-break is unchanged.
// LB comes from a SAMPLE: the triangles of every R-th edge are enumerated once, their keys go into a 256-bin
// histogram over [klo, khi]; walking it from the top to the first bin where the count reaches T gives a bin whose
// lower edge is a valid LB (>= T genuine triangles lie at or above it).  Bin 0 collects everything below klo, so a
// crossing in bin 0 certifies nothing and disables the pruning (smin = -1).
// ------------------------------------------------------------------------------------------------

// Flush of a workgroup's LDS histogram, COPIES rotated copies laid out [bin][copy], into one of PR_HCOPIES global copies
// (by block): a thousand blocks adding into the SAME 256 words serialise at the memory side (~12 ns per add and address);
// the copies are summed by the reader.  Every thread of a 256-thread block calls it; it starts with the barrier that
// ends the counting.
template <int COPIES>
__device__ __forceinline__ void hist_flush(const uint32_t* lh, uint32_t* __restrict__ hist) {
  __syncthreads();
  uint32_t* __restrict__ myh = hist + (size_t)(blockIdx.x & (PR_HCOPIES - 1)) * PR_BINS;
  for (int b = threadIdx.x; b < PR_BINS; b += 256) {
    uint32_t v = 0;
#pragma unroll
    for (int c = 0; c < COPIES; c++) v += lh[b * COPIES + ((c + threadIdx.x) & (COPIES - 1))];
    if (v) atomicAdd(&myh[b], v);
  }
}

__device__ __forceinline__ uint32_t prune_bin(uint32_t key, uint32_t klo, uint32_t shift) {
  if (key <= klo) return 0u;
  const uint32_t b = (key - klo) >> shift;
  return b < (uint32_t)PR_BINS ? b : (uint32_t)(PR_BINS - 1);
}

// The ESTIMATING sample (3c) bins by d = 3.0 - key instead — exact in fp32 for keys in [2, 3] — LOGARITHMICALLY, 16 bins per
// octave of d over [2^-17, 2^-1): the top-T keys crowd against 3.0 (three weights near 1), where linear bins of 0.002
// cannot tell the key of rank T from the key of rank 5 T; a bin 4.4 % wide in d is ~13 % wide in rank.  Bin 0: d >= 0.5
// (nothing can be said), bin 255: d < 2^-17 (1 + 1/16).  Selected by shift == PR_LOGBINS.
constexpr uint32_t PR_LOGBINS = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t est_bin(uint32_t key) {
  const float d = 3.0f - __uint_as_float(key);
  if (!(d > 0.0f)) return (uint32_t)(PR_BINS - 1);
  const uint32_t u = __float_as_uint(d) >> 19;  // exponent and four mantissa bits
  return u >= 2016u ? 0u : (u <= 1761u ? (uint32_t)(PR_BINS - 1) : 2016u - u);
}
// a value every key of bin b (>= 1) lies strictly ABOVE: 3.0 - (upper edge of the bin's d interval), exact in fp32
__device__ __forceinline__ float est_bin_floor(uint32_t b) { return 3.0f - __uint_as_float((2017u - b) << 19); }

// Which edges are sampled.  Any subset of genuine triangles certifies a bound; the question is which subset certifies
// a TIGHT one for the fewest key evaluations.
//   TOP = false: every stride-th edge (round 1).  The T-th largest sampled key is then about the (stride x T)-th key
//     of the graph: with ~32 k sampled edges on C2 the certified subgraph still holds 1.47 M triangles for T = 50 k.
//   TOP = true: the `target` HEAVIEST edges (weight at or above the lower edge of the bin of a 256-bin weight histogram
//     where the count from the top reaches target; es_hist_kernel).  A top triangle has three heavy edges, so its first
//     edge is far more likely to be in this set than in a uniform sample of the same size.  A block takes a contiguous
//     chunk of the edge list, compacts the qualifying edges into LDS (coalesced read of es, ballot prefix) and deals
//     them to its groups.
constexpr int SM_CHUNK = 256;  // edges per block and chunk in the TOP form (small: a chunk inside an inlier row is all heavy edges)

template <int TG, bool TOP>
__global__ __launch_bounds__(256) void tri_sample_hist_kernel(const uint64_t* __restrict__ bits, int W,
                                                              const uint32_t* __restrict__ wpre,
                                                              const uint32_t* __restrict__ ebi,
                                                              const uint32_t* __restrict__ ebj,
                                                              const uint32_t* __restrict__ ei,
                                                              const uint32_t* __restrict__ ej,
                                                              const float* __restrict__ es, uint64_t E,
                                                              uint32_t stride, uint32_t part, uint32_t parts,
                                                              uint32_t klo, uint32_t shift,
                                                              uint32_t* __restrict__ hist,
                                                              const uint32_t* __restrict__ es_hist, uint64_t target,
                                                              uint32_t wlo, uint32_t wshift,
                                                              const uint64_t* __restrict__ E_dev) {
  // Launched before the host knew the count (E: what the arrays hold).  More edges than that: the CSR indices this kernel
  // derives from the bit rows would point beyond the edge arrays — nothing may run (the host repeats the call: sc_capi.hip).
  if (E_dev && *E_dev > E) return;
  if (E_dev) E = *E_dev;
  __shared__ uint32_t lh[PR_BINS * PR_COPIES];  // [bin][copy]
  __shared__ uint32_t l_e[TOP ? SM_CHUNK : 1];  // TOP: the qualifying edges of the current chunk
  __shared__ uint32_t s_theta, s_cnt, s_wtot[4];
  __shared__ uint64_t plds[8];
  for (int b = threadIdx.x; b < PR_BINS * PR_COPIES; b += 256) lh[b] = 0;
  if (TOP) {  // the weight bin at which the count from the top reaches `target` (no such bin: every edge qualifies)
    static_assert(PR_BINS == 256, "one bin per thread, walked from the top");
    const uint32_t bin = PR_BINS - 1 - threadIdx.x;
    uint64_t mine = 0;
    for (int c = 0; c < PR_HCOPIES; c++) mine += es_hist[c * PR_BINS + bin];
    if (threadIdx.x == 0) s_theta = 0u;
    uint64_t tot;
    const uint64_t before = block_exscan_u64(mine, plds, &tot);  // (its barriers also order the s_theta default)
    if (before < target && target <= before + mine) s_theta = bin;
  }
  __syncthreads();
  const int gl = threadIdx.x & (TG - 1);
  const uint64_t n_s = (E + stride - 1) / stride;  // sampled edges: e = g * stride, g = 0 .. n_s - 1
  // this launch takes the sampled edges g = part, part + parts, ... (one process per GPU: every rank samples its share
  // and the histograms are summed by an all-reduce — distinct edges give distinct triangles, so the sum certifies)
  const uint64_t n_loc = n_s > part ? (n_s - part + parts - 1) / parts : 0;
  const uint64_t groups = TOP ? (256 / TG) : (uint64_t)gridDim.x * (256 / TG);
  const uint32_t theta = TOP ? s_theta : 0u;
  // a chunk is SM_CHUNK x parts consecutive edges, of which this rank considers every parts-th: the same number of
  // candidates per block whatever the number of ranks sharing the sample (per-block fixed costs stay amortised)
  const uint64_t chunk_edges = (uint64_t)SM_CHUNK * parts;
  const uint64_t n_chunks = TOP ? (E + chunk_edges - 1) / chunk_edges : 1;
  for (uint64_t ch = TOP ? blockIdx.x : 0; ch < n_chunks; ch += TOP ? gridDim.x : 1) {
  uint64_t q_end = n_loc;
  if (TOP) {
    // compaction of the chunk's qualifying edges, in edge order: four rounds of 256 edges (ballot prefix per wave,
    // wave totals through LDS); part / parts: this rank takes the qualifying edges with e % parts == part
    if (threadIdx.x == 0) s_cnt = 0u;
    __syncthreads();
    for (uint32_t r = 0; r < (SM_CHUNK / 256) * parts; r++) {
      // thread t of round r looks at edge (chunk base + r * 256 + t) only if it is this rank's (e % parts == part):
      // the edges are dealt so that consecutive threads of a round see consecutive edges of THIS rank
      const uint64_t e = ch * chunk_edges + ((uint64_t)r * 256 + threadIdx.x);
      const bool ok = e < E && (e % parts) == part && weight_bin(__float_as_uint(es[e]), wlo, wshift) >= theta;
      const uint64_t bal = __ballot(ok);
      const int wave = threadIdx.x >> 6;
      if ((threadIdx.x & 63) == 0) s_wtot[wave] = (uint32_t)__popcll(bal);
      __syncthreads();
      uint32_t pos = s_cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
      for (int w = 0; w < wave; w++) pos += s_wtot[w];
      if (ok) l_e[pos] = (uint32_t)e;
      __syncthreads();
      if (threadIdx.x == 0) s_cnt += s_wtot[0] + s_wtot[1] + s_wtot[2] + s_wtot[3];
      __syncthreads();
    }
    q_end = s_cnt;
  }
  for (uint64_t q = TOP ? (threadIdx.x / TG) : (uint64_t)blockIdx.x * (256 / TG) + (threadIdx.x / TG); q < q_end; q += groups) {
    const uint64_t e = TOP ? (uint64_t)l_e[q] : (q * parts + part) * stride;
    const uint32_t i = ei[e], j = ej[e];
    const uint32_t rowi = i * (uint32_t)W, rowj = j * (uint32_t)W;
    const int w0 = j >> 6;
    const float s_ij = es[e];
    const uint32_t bi = ebi[e], bj = ebj[e];  // the CSR bases travel with the edge: same memory level as ei / ej
    // No cross-lane step: every lane owns its words.  The loads of RB rounds are issued together, level by level (row
    // words -> prefix words -> weights).  Measured on C2: 33 us either way — the time is not the per-round latency chain
    // but gather / LDS-atomic throughput: most sampled edges join two inliers (the inlier clique holds ~60 % of all
    // edges) with ~250 common neighbours above j each, i.e. ~8 M key evaluations per call.
    constexpr int RB = 4;
    for (int wb = w0 + gl; wb < W; wb += TG * RB) {
      uint64_t ai[RB], aj[RB], m[RB];
#pragma unroll
      for (int r = 0; r < RB; r++) {  // level 1: row words
        const int w = wb + r * TG;
        const bool live = w < W;
        ai[r] = bits[rowi + (live ? w : w0)];
        aj[r] = bits[rowj + (live ? w : w0)];
        m[r] = live ? (ai[r] & aj[r]) : 0ull;
        if (w == w0) m[r] &= mask_above(j & 63);
      }
      uint32_t pi[RB], pj[RB];
#pragma unroll
      for (int r = 0; r < RB; r++) {  // level 2: prefix words (idle slots re-read the row's first one)
        const int w = wb + r * TG;
        pi[r] = bi + wpre[rowi + (m[r] ? w : w0)];
        pj[r] = bj + wpre[rowj + (m[r] ? w : w0)];
      }
#pragma unroll
      for (int r = 0; r < RB; r++) {  // level 3: weights of the common neighbours, four at a time
        uint64_t mr = m[r];
        while (mr) {
          int b[4];
          const int nbits = pop4(mr, b);
          float s_ik[4], s_jk[4];
          tri_weights4(es, b, nbits, {pi[r], ai[r]}, {pj[r], aj[r]}, s_ik, s_jk);
#pragma unroll
          for (int q = 0; q < 4; q++)
            if (q < nbits)
              atomicAdd(&lh[prune_bin(tri_key_weight(s_ij, s_ik[q], s_jk[q]), klo, shift) * PR_COPIES +
                            (threadIdx.x & (PR_COPIES - 1))], 1u);
        }
      }
    }
  }
  if (TOP) __syncthreads();  // l_e is rewritten by the next chunk
  }  // chunks
  hist_flush<PR_COPIES>(lh, hist);
}

// ------------------------------------------------------------------------------------------------
// 3c. pruning by an ESTIMATED bound (r04)
//
// The certifying samples above pay for their certificate: to exhibit T genuine triangles above the bound they evaluate
// 4 - 8 M keys at C2 (25 us, the largest launch of stage B), and the bound they can certify sits well below the T-th
// key, so the pruned graph still holds 10 T triangles.  But the bound need not be certified BEFORE it is used: it can be
// verified AFTERWARDS, for free.  Take ANY value LB, prune with smin = LB - 2 - 1e-6, enumerate, select.  If the strong
// subgraph turns out to hold >= T triangles with key >= LB, the proof of 3b applies word for word (it only needs "at least
// T triangles have key >= LB") and the selection is the full graph's top-T, ties included; if not, nothing is known and the
// call is repeated with a certifying sample.  The select's first round already counts the keys in [LB, 3.0] — the check
// is one comparison where that round is resolved (select_resolve, SelectState::want_req).
// So LB only has to be a good GUESS of a key of rank ~2 T: the lower edge of the histogram bin where
// rate x (sampled count from the top) reaches margin x T, from a uniform 1-in-rate sample of ALL the graph's triangles.
// The sample: a triangle (i, j, k), i < j < k, is found from its edge (i, j) in the 64-column word k / 64 of the row pair;
// edge e looks at the words w >= j / 64 with w = hash(e) (mod rate) only — every (edge, word) pair, hence every triangle,
// with probability exactly 1 / rate, independently across edges and words, so the sample is not dominated by a few edges
// (an inlier-inlier edge has hundreds of triangles; a sampled word holds a handful).  One lane per edge: an edge record,
// two gathered row words and — where they meet — the two prefix words and two weights per triangle: 0.36 M key
// evaluations at C2 instead of 4 M, no block-level step at all.
// With margin = 2 the estimate fails when the sample overstates the density of the top keys twofold: at >= 1000 expected
// samples above the bound that is > 10 sigma even with word-sized clusters.  Failing costs a repeated call, never a wrong
// result; a context that has seen one failure stops estimating (sc_capi.hip).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t edge_hash(uint32_t e) {
  e ^= e >> 16; e *= 0x7FEB352Du; e ^= e >> 15; e *= 0x846CA68Bu; e ^= e >> 16;  // (lowbias32)
  return e;
}

constexpr uint32_t SAMPLE_CAND_BLOCKS = 256;  // workgroups of the estimating sample that leave a candidate triangle behind
__global__ __launch_bounds__(256) void tri_sample_words_kernel(const uint64_t* __restrict__ bits, int W,
                                                               const uint32_t* __restrict__ wpre,
                                                               const uint32_t* __restrict__ ebi,
                                                               const uint32_t* __restrict__ ebj,
                                                               const uint32_t* __restrict__ ei,
                                                               const uint32_t* __restrict__ ej,
                                                               const float* __restrict__ es, uint64_t E, uint32_t rmask,
                                                               uint32_t* __restrict__ hist,
                                                               const uint64_t* __restrict__ E_dev,
                                                               const uint32_t* __restrict__ ebase, uint4* __restrict__ cand,
                                                               unsigned long long* __restrict__ cand_slot) {
  // ebase (with ebi == ebj == nullptr): the per-row CSR bases are looked up (after launch_edge_build)
  // cand (optional): the best-keyed triangle this workgroup sampled, {key bits, i, j, k} (key 0: none) — the voters of stage
  // C2's reference frame (sc_gramref.hpp)
  if (E_dev && *E_dev > E) return;  // (launched before the host knew the count: see tri_sample_hist_kernel)
  if (E_dev) E = *E_dev;
  // a host-free call's grid covers more edges than there are: the workgroups beyond them leave before they clear 16 KiB of LDS
  // (one that would have left a candidate says "none": cand is not cleared between calls)
  if ((uint64_t)blockIdx.x * 256 >= E) {
    if (cand != nullptr && blockIdx.x < SAMPLE_CAND_BLOCKS && threadIdx.x == 0) cand[blockIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  uint32_t best_key = 0u, best_e = 0u, best_k = 0u;  // (E < 2^32)
  // only the first SAMPLE_CAND_BLOCKS workgroups keep their best triangle (tracking it in every one cost the launch 3.6 us at C2;
  // 64 voters want 64 good triangles, and the best of these workgroups' ~50 000 sampled keys per voter is that)
  const bool track = cand != nullptr && blockIdx.x < SAMPLE_CAND_BLOCKS;
  __shared__ uint32_t lh[PR_BINS * EST_COPIES];
  for (int b = threadIdx.x; b < PR_BINS * EST_COPIES; b += 256) lh[b] = 0;
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += stride) {
    const uint32_t j = ej[e], i = ei[e];
    const int w0 = (int)(j >> 6);
    // the first word >= w0 in this edge's residue class (hashed by its END POINTS: the sample does not depend on the edge numbering)
    int w = w0 + (int)((edge_hash(i * 0x9E3779B1u + j) - (uint32_t)w0) & rmask);
    if (w >= W) continue;
    const uint32_t rowi = i * (uint32_t)W, rowj = j * (uint32_t)W;
    for (; w < W; w += (int)rmask + 1) {
      const uint64_t ai = bits[rowi + w], aj = bits[rowj + w];
      uint64_t m = ai & aj;
      if (w == w0) m &= mask_above((int)(j & 63));
      if (m == 0) continue;
      // only the lanes that found a triangle pay for the edge's weight and CSR bases (one memory level, beside the prefix words)
      const float s_ij = es[e];
      const uint32_t bi = ebi ? ebi[e] : ebase[i], bj = ebj ? ebj[e] : ebase[j];
      const uint32_t pi = bi + wpre[rowi + w], pj = bj + wpre[rowj + w];
      while (m) {
        int b[4];
        const int nbits = pop4(m, b);
        float s_ik[4], s_jk[4];
        tri_weights4(es, b, nbits, {pi, ai}, {pj, aj}, s_ik, s_jk);
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (q < nbits) {
            const uint32_t kb = tri_key_weight(s_ij, s_ik[q], s_jk[q]);
            atomicAdd(&lh[est_bin(kb) * EST_COPIES + (threadIdx.x & (EST_COPIES - 1))], 1u);
            if (track && kb > best_key) { best_key = kb; best_e = (uint32_t)e; best_k = (uint32_t)(64 * w + b[q]); }
          }
      }
    }
  }
  hist_flush<EST_COPIES>(lh, hist);
  if (track) {  // (workgroup-uniform) the workgroup's best: by key, then by lowest thread — the sample is deterministic, so is this
    __shared__ uint32_t s_best[4], s_who[4];
    uint32_t bk = best_key;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bk = max(bk, (uint32_t)__shfl_xor((int)bk, o));
    const uint64_t holders = __ballot(best_key == bk);
    if ((threadIdx.x & 63) == 0) { s_best[threadIdx.x >> 6] = bk; s_who[threadIdx.x >> 6] = (threadIdx.x & ~63u) + (uint32_t)(__ffsll((unsigned long long)holders) - 1); }
    __syncthreads();
    uint32_t wk = s_best[0], wt = s_who[0];
#pragma unroll
    for (int v = 1; v < 4; v++)
      if (s_best[v] > wk) { wk = s_best[v]; wt = s_who[v]; }  // (waves in order: equal keys keep the lower thread)
    if (threadIdx.x == wt) {
      cand[blockIdx.x] = wk ? make_uint4(best_key, ei[best_e], ej[best_e], best_k) : make_uint4(0u, 0u, 0u, 0u);
      // voter v of the frame = the best candidate among the workgroups = v (mod 64): one 64-bit max per workgroup (ControlBlock::ref_slot, zeroed per call)
      if (wk) atomicMax(&cand_slot[blockIdx.x & 63u], ((unsigned long long)wk << 32) | (unsigned long long)blockIdx.x);
    }
  }
}

// sum of the copies -> one 256-bin histogram (the form the ranks exchange)
__global__ __launch_bounds__(256) void hist_reduce_kernel(const uint32_t* __restrict__ copies, uint32_t* __restrict__ out) {
  uint32_t v = 0;
#pragma unroll
  for (int c = 0; c < PR_HCOPIES; c++) v += copies[c * PR_BINS + threadIdx.x];
  out[threadIdx.x] = v;
}
void launch_hist_reduce(const uint32_t* copies, uint32_t* out, hipStream_t st) {
  hipLaunchKernelGGL(hist_reduce_kernel, dim3(1), dim3(256), 0, st, copies, out);
}

// every block derives smin from the histogram (256 bins: cheap) and sets the strong bits of its edges in `mbits`
// (zeroed beforehand; only upper-triangle entries are needed: bit j of row i for i < j).  Block 0 publishes smin.
__global__ __launch_bounds__(256) void prune_bits_kernel(const uint32_t* __restrict__ hist, int copies, uint64_t want,
                                                         uint32_t klo, uint32_t shift,
                                                         const uint32_t* __restrict__ ei,
                                                         const uint32_t* __restrict__ ej,
                                                         const float* __restrict__ es, uint64_t E, int W,
                                                         unsigned long long* __restrict__ mbits,
                                                         float* __restrict__ smin_out,
                                                         uint32_t* __restrict__ klb_out, StrongList sl,
                                                         uint32_t* __restrict__ tcnt,
                                                         const uint64_t* __restrict__ own,
                                                         const uint64_t* __restrict__ E_dev, int trimmed) {
  // E: what the grid and the arrays cover; Ea: the edges there really are (E_dev: launched before the host knew).  More than
  // the arrays hold: nothing may run — no strong edge is listed, so the counting and key kernels that follow find no work
  // (the host repeats the call)
  if (E_dev && *E_dev > E) return;
  const uint64_t Ea = E_dev ? *E_dev : E;
  // a host-free call's grid covers more edges than there are: the workgroups beyond them have nothing to list, and their tcnt
  // entries are never read (the scan of a host-free call skips the tiles beyond ControlBlock::live_edges and treats what lies
  // beyond the count as zero) — they leave before the histogram walk
  if (trimmed && E_dev && sl.region_blocks == 0 && (uint64_t)blockIdx.x * (sl.cnt ? ORD_BLOCK_EDGES : 256u) >= Ea) return;
  __shared__ uint64_t lds[8];
  __shared__ float s_smin;
  __shared__ uint32_t s_klb, s_base, s_wcnt[4], s_rcnt[4][4];
  static_assert(PR_BINS == 256, "one bin per thread, walked from the top");
  const uint32_t bin = PR_BINS - 1 - threadIdx.x;
  uint64_t mine = 0;
  if (copies == PR_HCOPIES) {  // (the sample's own copies: four loads in flight — a loop of `copies` trips is four round trips to hipcc)
    static_assert(PR_HCOPIES == 4, "four copies");
    const uint32_t h0 = hist[bin], h1 = hist[PR_BINS + bin], h2 = hist[2 * PR_BINS + bin], h3 = hist[3 * PR_BINS + bin];
    mine = (uint64_t)h0 + h1 + h2 + h3;
  } else {
    for (int c = 0; c < copies; c++) mine += hist[c * PR_BINS + bin];  // (1: summed by the caller)
  }
  if (threadIdx.x == 0) { s_smin = -1.0f; s_klb = 0u; }  // default: no certified bound -> every edge is strong
  uint64_t tot;
  const uint64_t before = block_exscan_u64(mine, lds, &tot);
  if (before < want && want <= before + mine && bin > 0) {
    const float lb = shift == PR_LOGBINS ? est_bin_floor(bin) : __uint_as_float(klo + (bin << shift));  // lower edge of the crossing bin
    s_smin = (lb - 2.0f) - 1e-6f;
    s_klb = __float_as_uint(lb);  // >= want triangles have a key >= this one: the select may ignore anything below
  }
  __syncthreads();
  const float smin = s_smin;
  if (blockIdx.x == 0 && threadIdx.x == 0) { *smin_out = smin; *klb_out = s_klb; }
  if (sl.cnt) {
    // the ORDERED form (2c; one rank, region_blocks == 0): the block takes ORD_BLOCK_EDGES consecutive edges — four runs of 256, a
    // quarter of the histogram walks above — and writes the strong ones in ascending order into its own slot, their number into
    // cnt[blockIdx]: no atomic, one barrier, and no tcnt entry is zeroed (nothing scans the counts; an overflow's fall-back
    // zeroes the weak ones)
    static_assert(ORD_BLOCK_EDGES == 4 * 256, "four runs of 256");
    const int wave = threadIdx.x >> 6;
    bool st[4]; uint64_t bal[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint64_t e = (uint64_t)blockIdx.x * ORD_BLOCK_EDGES + q * 256 + threadIdx.x;
      st[q] = e < Ea && es[e] >= smin;
      if (st[q]) {
        const uint32_t i = ei[e], j = ej[e];
        atomicOr(&mbits[(size_t)i * W + (j >> 6)], 1ull << (j & 63));
      }
      bal[q] = __ballot(st[q]);
      if ((threadIdx.x & 63) == 0) s_rcnt[q][wave] = (uint32_t)__popcll(bal[q]);
    }
    __syncthreads();
    uint32_t run = 0;  // strong edges of the runs and waves before (q, w)
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
      for (int w = 0; w < 4; w++) {
        if (w == wave && st[q])
          sl.list[(uint64_t)blockIdx.x * ORD_BLOCK_EDGES + run + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[q] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[q], 0u))] =
              (uint32_t)((uint64_t)blockIdx.x * ORD_BLOCK_EDGES + q * 256 + threadIdx.x);
        run += s_rcnt[q][w];
      }
    }
    if (threadIdx.x == 0) sl.cnt[blockIdx.x] = run;
    return;
  }
  // region = blockIdx % ST_SHARDS in both forms (blocks that run side by side add to different counters: with consecutive
  // blocks on one counter this kernel took 61 us instead of 33 at C3); with contiguous regions the block's 256 EDGES are what
  // moves: block b takes chunk (b % ST_SHARDS) * region_blocks + b / ST_SHARDS
  const uint32_t region = blockIdx.x & (ST_SHARDS - 1);
  const uint64_t chunk = sl.region_blocks ? (uint64_t)region * sl.region_blocks + blockIdx.x / ST_SHARDS : (uint64_t)blockIdx.x;
  const uint64_t e = (sl.region_blocks && blockIdx.x / ST_SHARDS >= sl.region_blocks) ? E : chunk * 256 + threadIdx.x;
  bool strong = e < Ea && es[e] >= smin;
  if (strong) {  // the strong bit matrix is whole on every rank: membership of ANY vertex pair is looked up in it
    const uint32_t i = ei[e], j = ej[e];
    atomicOr(&mbits[(size_t)i * W + (j >> 6)], 1ull << (j & 63));
  }
  // sharded stage B: only this rank's edge range [own[0], own[1]) enters the list of edges to enumerate
  if (own) strong = strong && e >= own[0] && e < own[1];
  if (sl.list) {
    // the strong edges, compacted (any order: everything downstream is indexed by the edge id): one atomic per block
    // on one of ST_SHARDS counters; region r receives the blocks with blockIdx % ST_SHARDS == r (or, StrongList::region_blocks,
    // a run of consecutive blocks: ceil(blocks / ST_SHARDS) of them), so sl.cap = ceil(blocks / ST_SHARDS) * 256 entries can
    // never overflow.  Weak edges carry no triangle: count 0.
    if (e < E && (!strong || sl.region_blocks)) tcnt[e] = 0u;
    const uint64_t bal = __ballot(strong);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_wcnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) {  // ONE atomic per block (returning atomics on a shared address cost ~170 ns each here)
      const uint32_t tot = s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
      s_base = tot ? atomicAdd(&sl.fill[region], tot) : 0u;
    }
    __syncthreads();
    if (strong) {
      uint32_t pos = s_base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
      for (int w = 0; w < wave; w++) pos += s_wcnt[w];
      sl.list[(uint64_t)region * sl.cap + pos] = (uint32_t)e;
    }
  }
}

uint32_t strong_list_cap(uint64_t E) {
  const uint64_t blocks = (E + 255) / 256;
  return (uint32_t)(((blocks + ST_SHARDS - 1) / ST_SHARDS) * 256);
}
size_t strong_list_bytes(uint64_t E) { return (size_t)strong_list_cap(E) * ST_SHARDS * sizeof(uint32_t); }


// histogram window in key space: [bits(key_floor), bits(3.0f)], monotone in the value; (khi - klo) >> shift < 256
static void prune_window(float key_floor, uint32_t* klo_out, uint32_t* shift_out) {
  const uint32_t khi = 0x40400000u;  // 3.0f
  uint32_t klo;
  memcpy(&klo, &key_floor, 4);
  if (!(key_floor > 0.f) || klo >= khi) klo = 0x3F800000u;  // 1.0f
  const uint32_t range = khi - klo;
  const int bitsn = 32 - __builtin_clz(range);
  *klo_out = klo;
  *shift_out = bitsn > 8 ? (uint32_t)(bitsn - 8) : 0u;
}

void launch_sample_hist(const Graph& g, const EdgeList& el, uint64_t want, float key_floor, uint32_t part, uint32_t parts,
                        uint32_t* hist, uint32_t* es_hist, const Tuning& tn, hipStream_t st) {
  uint32_t klo, shift;
  prune_window(key_floor, &klo, &shift);
  const uint64_t E = el.E, Ed = el.E_hint;  // Ed: the count the host-side choices are made with
  // Which form (r02 sweeps, profiles/r02_ab_heaviest_edge_sample.txt and r02_ab_sample_size.txt): the heaviest edges
  // certify a much tighter bound per sampled edge, but each of them is a costly one (an edge between two inliers has
  // hundreds of common neighbours).  That pays when T is a small part of the graph's triangles — C3 (N = 20 000, T = 200 k):
  // stage B 962 -> 551 us, 10.6 M -> 2.1 M enumerated — is a wash on C2 (167 vs 165 us) and loses where T is most of
  // what there is (C4, T = 500 k of 8.8 M triangles: the uniform sample at stride 1 already certifies 2 T: 211 vs 248 us).
  // C1 (N = 2000, T = 10 k) loses too: 94 vs 82 us; C2, a wash with every stage bracketed, gains on the hot path (stage B
  // 154.5 -> 138.5 us: fewer keys also means the speculative launches finish sooner).  What separates them is how small T
  // is against the triangles the graph holds, for which E^2 / N is a proxy known before any is counted: C3 2550 T, C2
  // 890 T, C1 320 T, C4 90 T.
  // sample_mode: 0 = by this rule (E^2 / N >= 600 T), 1 = every stride-th edge, 2 = the heaviest edges.
  const bool top = tn.sample_mode == 2 ||
                   (tn.sample_mode == 0 && (double)Ed * (double)Ed / (double)(g.n > 0 ? g.n : 1) >= 600.0 * (double)want);
  if (top && es_hist) {
    // the heaviest edges (TOP form): weight histogram, then the sample itself
    uint32_t wlo, wshift;
    {
      const float wfloor = key_floor / 3.0f;
      uint32_t lo; memcpy(&lo, &wfloor, 4);
      const uint32_t hi = 0x3F800000u;  // 1.0f
      if (!(wfloor > 0.f) || lo >= hi) lo = 0x3F000000u;  // 0.5f
      const int bitsn = 32 - __builtin_clz(hi - lo);
      wlo = lo; wshift = bitsn > 8 ? (uint32_t)(bitsn - 8) : 0u;
    }
    uint64_t target = tn.sample_edges ? tn.sample_edges : (want / 3 < 16384 ? 16384 : want / 3);
    const int tg = tn.tg_sample ? tn.tg_sample : (g.W > 256 ? 32 : 16);  // C3 (W = 313): 134 (16) vs 107 us (32); C2: 24.4 vs 25.9
    uint64_t nb = (E + (uint64_t)SM_CHUNK * parts - 1) / ((uint64_t)SM_CHUNK * parts);
    if (nb > 8192) nb = 8192;
    if (tn.sample_blocks) nb = tn.sample_blocks;
    with_lanes<16, 4, 8, 32, 64>(tg, [&](auto lanes) {
      hipLaunchKernelGGL((tri_sample_hist_kernel<decltype(lanes)::value, true>), dim3((unsigned)nb), dim3(256), 0, st, g.bits, g.W, g.wpre,
                         el.ebi, el.ebj, el.ei, el.ej, el.es, E, 1u, part, parts, klo, shift, hist, es_hist, target, wlo, wshift, el.E_dev);
    });
    return;
  }
  // every R-th edge.  The sample must grow with T: the bound is the T-th largest SAMPLED key, so a small sample of a
  // large T certifies little.  ~5T/8 sampled edges (>= 32k) is the sweet spot on C2 for T = 50k ... 400k (swept again
  // at the end of round 1); Tuning::sample_edges overrides.
  uint64_t target = want * 5 / 8;
  if (target < 32768) target = 32768;
  if (tn.sample_edges) target = tn.sample_edges;
  uint64_t stride = Ed / (target ? target : 1);
  if (stride < 1) stride = 1;
  if (stride > 64) stride = 64;
  const uint64_t n_s = (E + stride - 1) / stride;
  const uint64_t n_loc = n_s > part ? (n_s - part + parts - 1) / parts : 0;
  if (n_loc == 0) return;
  // lanes per sampled edge (r02 sweep, profiles/r02_ab_lanes_per_edge.txt): 16 while the sample is small enough for
  // about one edge per group (C2 26.9 -> 19.8 us, C3 129 -> 112), 8 once groups take several trips (C4: 74 vs 81)
  const int tg = tn.tg_sample ? tn.tg_sample : ((n_loc <= 131072 || g.W > 256) ? 16 : 8);
  uint64_t nb = (n_loc + (256 / tg) - 1) / (256 / tg);
  // about one sampled edge per group (measured: 256 blocks 70 us, 1024+ blocks 35 us on C2)
  if (nb > 4096) nb = 4096;
  with_lanes<16, 4, 8, 32, 64>(tg, [&](auto lanes) {
    hipLaunchKernelGGL((tri_sample_hist_kernel<decltype(lanes)::value, false>), dim3((unsigned)nb), dim3(256), 0, st, g.bits, g.W, g.wpre,
                       el.ebi, el.ebj, el.ei, el.ej, el.es, E, (uint32_t)stride, part, parts, klo, shift, hist, (const uint32_t*)nullptr,
                       (uint64_t)0, 0u, 0u, el.E_dev);
  });
}

SamplePlan sample_plan(uint64_t want, bool allow_estimate, const Tuning& tn, uint64_t E, int W) {
  SamplePlan sp{false, 1u, want};
  if (!allow_estimate || tn.no_estimate || tn.sample_mode != 0 || want == 0) return sp;
  // rate: 64 while 2 T still leaves >= 1024 expected samples above the bound, halved below that, never under 8 (a whole-graph
  // enumeration is what the pruning is there to avoid)
  uint32_t rate = 64;
  while (rate > 8 && 2 * want / rate < 1024) rate >>= 1;
  // ... and beyond 64 on big graphs: the sample looks at E x (row words) / rate word pairs — 16 M random 8-byte gathers at C3
  // (N = 20 000, rate 64: 156 us) for 6000 samples above the bound where 1500 do (rate 256: 45 us)
  while (rate < 512 && 2 * want / (2 * rate) >= 1024 && (double)E * (double)(W > 0 ? W : 1) / 2.0 / rate > 2.0e6) rate <<= 1;  // (an edge has ~W / 2 words beyond its higher end)
  // the rank the bound aims at, in % of T: T plus FIVE standard deviations of the sampled count at rank T — a sampled word
  // brings its triangles together, ~8 at a time — within [115, 200] (C2 151, C3 151 at its rate of 256, C4 116).  Eight until r05
  // (C2 181): over 30 000 frames of 256 distinct C2 scenes no estimate failed at 130 % nor at 115 %, 17 did at 105 % — and the bound is
  // the lower edge of the histogram bin that holds the aimed rank (256 log bins: ~0.4 T keys per bin up there), which adds to
  // the margin more often than not.  A failed estimate costs a repeated call, never a result.  C2: 186 k -> 151 k triangles
  // enumerated, - 1.9 us per frame.
  uint64_t margin = tn.est_margin_pct;
  if (!margin) {
    const double at_T = (double)want / rate;
    double m = 1.0 + 5.0 * __builtin_sqrt(8.0 / (at_T > 1.0 ? at_T : 1.0));
    m = m < 1.15 ? 1.15 : (m > 2.0 ? 2.0 : m);
    margin = (uint64_t)(m * 100.0 + 0.5);
  }
  const uint64_t aim = (want * margin + 99) / 100;
  uint64_t hw = (aim + rate - 1) / rate;
  if (hw < 128 && !tn.est_margin_pct) hw = 128;
  if (hw < 1) hw = 1;
  sp.estimate = true; sp.rate = rate; sp.hist_want = hw;
  return sp;
}

uint32_t sample_estimate_blocks(uint64_t E, const Tuning& tn) {
  uint64_t nb = (E + 255) / 256;
  if (nb > 4096) nb = 4096;
  if (tn.sample_blocks) nb = tn.sample_blocks;
  return (uint32_t)nb;
}
uint32_t sample_candidate_blocks(uint64_t E, const Tuning& tn) {  // how many of them write a candidate (launch_sample_estimate, cand)
  const uint32_t nb = sample_estimate_blocks(E, tn);
  return nb < SAMPLE_CAND_BLOCKS ? nb : SAMPLE_CAND_BLOCKS;
}

void launch_sample_estimate(const Graph& g, const EdgeList& el, uint32_t rate, uint32_t* hist, const SampleCands& cands, const Tuning& tn,
                            hipStream_t st) {
  if (el.E == 0) return;  // (the logarithmic bins need no window)
  const uint32_t nb = sample_estimate_blocks(el.E, tn);
  hipLaunchKernelGGL(tri_sample_words_kernel, dim3(nb), dim3(256), 0, st, g.bits, g.W, g.wpre, el.ebi, el.ebj, el.ei, el.ej, el.es, el.E,
                     rate - 1u, hist, el.E_dev, el.ebase, cands.slot ? cands.cand : nullptr, cands.slot);
}

void launch_prune_bits(const Graph& g, const uint32_t* hist, bool hist_is_copies, const EdgeList& el, uint64_t want, float key_floor,
                       const Pruned& pr, const EdgeCounts& ec, const PruneOpts& o, hipStream_t st) {
  uint32_t klo, shift;
  prune_window(key_floor, &klo, &shift);
  if (o.logbins) shift = PR_LOGBINS;  // the histogram of launch_sample_estimate
  const StrongList& sl = pr.sl;
  const uint64_t E = el.E;
  const uint64_t blocks = sl.cnt ? (E + ORD_BLOCK_EDGES - 1) / ORD_BLOCK_EDGES : sl.region_blocks ? (uint64_t)sl.region_blocks * ST_SHARDS : (E + 255) / 256;
  hipLaunchKernelGGL(prune_bits_kernel, dim3((unsigned)blocks), dim3(256), 0, st, hist, hist_is_copies ? PR_HCOPIES : 1, want, klo, shift,
                     el.ei, el.ej, el.es, E, g.W, reinterpret_cast<unsigned long long*>(pr.mbits), pr.smin, pr.klb, sl, ec.tcnt, ec.own,
                     el.E_dev, o.trimmed ? 1 : 0);
}

// Sharded stage B, after the certificate: what enumerating row i of the PRUNED graph costs — 32 x the triangles of a
// SAMPLE of its strong edges (every edge (i, j) with (i + j) % 32 == 0: AND + popcount of the two strong rows above j,
// exactly what the counting pass does, for one edge in 32) plus one per strong edge (the counting pass spends
// about a triangle's worth of time on an edge without any).  One wave per row: the sampled edges are taken one after the
// other (wave-uniform), the 64 lanes AND the row words in parallel.  Saturated to u32.  The prefix of these costs cuts the
// rows into the ranks' ranges: a correspondence list in keypoint order puts the inliers — and nearly all the triangles of
// the pruned graph — into a few rows, which the a-priori estimate of row_stats_kernel (every edge of the FULL graph weighs
// the same) cannot see.  (A proxy from the strong degrees alone left 1.4 x between the ranks on such a scene: outlier rows
// have strong edges but hardly a triangle.)
__global__ __launch_bounds__(256) void strong_rowcost_kernel(const uint64_t* __restrict__ mbits, int n, int W,
                                                             uint32_t* __restrict__ rowcost) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const uint64_t* __restrict__ ri = mbits + (size_t)i * W;
  const uint64_t pattern = 0x0000000100000001ull << ((32 - (i & 31)) & 31);  // bits b of any word with (i + 64 w + b) % 32 == 0
  uint64_t tri = 0, sdeg = 0;
  for (int wb = i >> 6; wb < W; wb += 64) {
    const int w = wb + lane;
    const uint64_t v = w < W ? ri[w] : 0ull;  // (only bits above i are ever set: the strong matrix is upper-triangular)
    sdeg += (uint64_t)__popcll(v);
    const uint64_t sm = v & pattern;
    uint64_t bal = __ballot(sm != 0);
    while (bal) {  // wave-uniform: one lane's word after the other
      const int L = __builtin_ctzll(bal);
      bal &= bal - 1;
      const int wL = wb + L;
      uint64_t mL = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(sm >> 32), L) << 32) |
                    (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)sm, L);
      while (mL) {
        const int bpos = __builtin_ctzll(mL);
        mL &= mL - 1;
        const uint64_t* __restrict__ rj = mbits + (size_t)(wL * 64 + bpos) * W;
        for (int w2 = wL + lane; w2 < W; w2 += 64) {
          uint64_t m = ri[w2] & rj[w2];
          if (w2 == wL) m &= mask_above(bpos);
          tri += (uint64_t)__popcll(m);
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { tri += __shfl_xor(tri, o); sdeg += __shfl_xor(sdeg, o); }
  const uint64_t cost = 32ull * tri + sdeg;
  if (lane == 0) rowcost[i] = cost > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cost;
}

// prefix of the row costs AND this rank's range in one single-block launch (n values: 80 KB at N = 20 000): rows [lo, hi)
// with lo = the first row whose cost prefix reaches rank / world of the total (the rule of shard_split_kernel).
// Wave w of 16 takes the w-th sixteenth of the rows, 256 rows per step (a lane loads four consecutive rows with one 16-byte
// load: a quarter of the dependent trips the 4-byte form made — at N = 20 000 this launch took 20 us, nearly all of it load
// latency); the wave whose segment holds a boundary walks it a second time.  rowcost holds roundup(n, 4) + 1024 entries.
__device__ __forceinline__ uint4 cost4(const uint32_t* __restrict__ rowcost, int r, int r1) {  // rows r .. r + 3, zero from r1 on
  uint4 v = *reinterpret_cast<const uint4*>(rowcost + r);
  if (r + 0 >= r1) v.x = 0u;
  if (r + 1 >= r1) v.y = 0u;
  if (r + 2 >= r1) v.z = 0u;
  if (r + 3 >= r1) v.w = 0u;
  return v;
}
__global__ __launch_bounds__(1024) void cost_split_kernel(const uint32_t* __restrict__ rowcost,
                                                          const uint64_t* __restrict__ edge_off, int n, uint32_t rank,
                                                          uint32_t world, uint32_t* __restrict__ own_row,
                                                          uint64_t* __restrict__ own_edge) {
  __shared__ uint64_t s_tot[16];
  __shared__ uint32_t s_row[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = ((n + 15) / 16 + 255) / 256 * 256, r0 = min(n, wave * seg), r1 = min(n, r0 + seg);
  uint64_t mine = 0;
#pragma unroll 4
  for (int rb = r0; rb < r1; rb += 256) {
    const uint4 v = cost4(rowcost, rb + 4 * lane, r1);
    mine += (uint64_t)v.x + v.y + v.z + v.w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if (lane == 0) s_tot[wave] = mine;
  if (threadIdx.x < 2) s_row[threadIdx.x] = (uint32_t)n;
  __syncthreads();
  uint64_t pre = 0, total = 0;
  for (int w = 0; w < 16; w++) { if (w < wave) pre += s_tot[w]; total += s_tot[w]; }
  for (int which = 0; which < 2; which++) {
    const uint32_t l = rank + (uint32_t)which;
    if (l == 0 || l >= world) continue;
    const uint64_t target = (uint64_t)(((unsigned __int128)total * l) / world);
    // the first row r with (sum of the costs before r) >= target lies in this wave's segment iff pre < target <= pre + mine,
    // or it is the segment's first row (pre >= target and the wave before did not reach it: handled by the min below)
    if (pre + mine < target && wave != 15) continue;       // (wave-uniform) beyond this segment
    if (pre >= target) { if (lane == 0) atomicMin(&s_row[which], (uint32_t)min(r0, n)); continue; }
    uint64_t run = pre;
    for (int rb = r0; rb < r1; rb += 256) {
      const int r = rb + 4 * lane;
      const uint4 v = cost4(rowcost, r, r1);
      const uint64_t lane_sum = (uint64_t)v.x + v.y + v.z + v.w;
      const uint64_t inc = wave_inscan(lane_sum);
      const uint64_t b0 = run + inc - lane_sum;              // sum of the costs before row r
      const uint64_t b1 = b0 + v.x, b2 = b1 + v.y, b3 = b2 + v.z;
      // the first of this lane's four rows whose "before" reaches the target (4: none)
      const int k = (r < r1 && b0 >= target) ? 0 : ((r + 1 < r1 && b1 >= target) ? 1 : ((r + 2 < r1 && b2 >= target) ? 2 : ((r + 3 < r1 && b3 >= target) ? 3 : 4)));
      const uint64_t hit = __ballot(k < 4);
      if (hit) {
        const int L = __builtin_ctzll(hit);  // "before" grows with the row: the lowest lane that hit holds the first such row
        const int kk = __shfl(k, L);
        if (lane == 0) atomicMin(&s_row[which], (uint32_t)(rb + 4 * L + kk));
        break;
      }
      run += __shfl(inc, 63);
    }
    // (no row of the segment reached it: the boundary is the first row of the next segment, or n — its wave reports r0)
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const uint32_t l = rank + threadIdx.x;
    const uint32_t row = l == 0 ? 0u : (l >= world ? (uint32_t)n : s_row[threadIdx.x]);
    own_row[threadIdx.x] = row;
    own_edge[threadIdx.x] = edge_off[row];
  }
}
void launch_cost_split(const RowOffsets& ro, const ShardCut& cut, const uint32_t* rowcost, int n, hipStream_t st) {
  hipLaunchKernelGGL(cost_split_kernel, dim3(1), dim3(1024), 0, st, rowcost, (const uint64_t*)ro.edge_off, n, cut.rank, cut.world,
                     cut.own_row, cut.own_edge);
}
void launch_strong_rowcost(const Graph& g, const Pruned& pr, uint32_t* rowcost, hipStream_t st) {
  hipLaunchKernelGGL(strong_rowcost_kernel, dim3((unsigned)((g.n + 3) / 4)), dim3(256), 0, st, pr.mbits, g.n, g.W, rowcost);
}

}  // namespace sc
