// sc_polish.hip — refits iterated to a fixed point on a scored frame (include/saccot.h, sc_polish): the kernels of  select -> polish -> winner / mask.
//
// A frame leaves its T hypotheses (c->rt), their ranking keys (c->sel_key), their scores over all n correspondences (c->cnt) and the
// staged planes in the context.  Three launches of a dependent chain, whatever the number of refits:
//
//   polish_select_kernel  one workgroup.  The first K <= 64 hypotheses of the frame's total order — score, then ranking key, then
//                         lowest (i, j, k) — by a radix select over the 96-bit key (score, key, ~position): one byte per pass, most
//                         significant first from the top byte of the largest score, and it stops as soon as the bucket that holds the K-th key holds nothing but keys that
//                         are taken (typically after the score's bytes and one or two of the key's).  The K are then ordered among
//                         themselves, and their ranks in the ranked list counted the way the finalize kernel counts its winner's.
//   polish_kernel         one workgroup per candidate, EVERY iteration inside the launch: refit_iterate (sc_refit.hpp, which says
//                         what an iteration is; sc_polish_batch.hip runs the same function on LDS), here with a chunk's sums and
//                         its inlier word — in the spare slot of the sums: no n-sized mask — in global scratch.  Then the last
//                         iterate's score over all n.
//   polish_winner_kernel  the candidate with the largest polished score, its mask, the records for the caller, the host words.
#include <cstddef>

#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_chunks.hpp"
#include "sc_kernels.hpp"
#include "sc_refit.hpp"
#include "sc_winner.hpp"

namespace sc {

namespace {

constexpr int POLISH_THREADS = 1024;

// ---- select ------------------------------------------------------------------------------------------------------------------
// The 96-bit key of hypothesis g as three words, most significant first: w[0] = score, w[1] = ranking key, w[2] = ~g.
struct Key96 { uint32_t w[3]; };
__device__ __forceinline__ bool key_above(const Key96& a, const Key96& b) {  // a > b
  if (a.w[0] != b.w[0]) return a.w[0] > b.w[0];
  if (a.w[1] != b.w[1]) return a.w[1] > b.w[1];
  return a.w[2] > b.w[2];
}

__global__ __launch_bounds__(POLISH_THREADS) void polish_select_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ sel_key,
                                                                       uint32_t T, const float* __restrict__ RtSoA, uint32_t ld_local,
                                                                       uint32_t want, PolishCand* __restrict__ cand,
                                                                       uint32_t* __restrict__ n_cand) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_digit, s_above, s_match, s_total, s_count;
  __shared__ Key96 s_sel[POLISH_MAX_CAND];
  __shared__ uint32_t s_pos[POLISH_MAX_CAND], s_rank[POLISH_MAX_CAND];
  const uint32_t tid = threadIdx.x;
  if (want > POLISH_MAX_CAND) want = POLISH_MAX_CAND;
  // the prefix fixed so far (value and mask per word), and how many keys are still wanted among those that match it
  Key96 pre{{0u, 0u, 0u}}, msk{{0u, 0u, 0u}};
  uint32_t need = want;
  bool done = false, none = false;
  // the largest score: the select starts at its highest non-zero byte (an inlier count has two bytes of zeros on top)
  uint32_t top;
  {
    uint32_t mx = 0u;
#pragma unroll 8
    for (uint64_t g = tid; g < T; g += POLISH_THREADS) mx = max(mx, cnt[g]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, o));
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    if ((tid & 63u) == 0u) atomicMax(&hist[0], mx);
    __syncthreads();
    top = hist[0];
    __syncthreads();
  }
  const int d0 = top >> 24 ? 11 : (top >> 16 ? 10 : (top >> 8 ? 9 : 8));
#pragma unroll 1
  for (int d = d0; d >= 0 && !done; d--) {
    const int word = 2 - (d >> 2), shift = (d & 3) * 8;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    uint32_t cur = 0u, run = 0u;
#pragma unroll 8
    for (uint64_t g = tid; g < T; g += POLISH_THREADS) {  // (both loads unconditional: eight iterations' loads are in flight together)
      const Key96 k{{cnt[g], sel_key[g], ~(uint32_t)g}};
      // a hypothesis that explains nothing is no candidate
      if (k.w[0] != 0u && (k.w[0] & msk.w[0]) == pre.w[0] && (k.w[1] & msk.w[1]) == pre.w[1] && (k.w[2] & msk.w[2]) == pre.w[2]) {
        // runs of one bucket are counted in a register: in the score's upper bytes nearly every key falls into bucket 0, and
        // 50 000 atomics on one LDS word cost 20 us a pass
        const uint32_t b = ((word == 0 ? k.w[0] : (word == 1 ? k.w[1] : k.w[2])) >> shift) & 255u;
        if (b != cur) {
          if (run) atomicAdd(&hist[cur], run);
          cur = b; run = 0u;
        }
        run++;
      }
    }
    if (run) atomicAdd(&hist[cur], run);
    __syncthreads();
    if (tid < 64) {  // wave 0: the bucket that holds the need-th largest matching key; lane l owns buckets 255 - 4 l .. 252 - 4 l
      const int hi = 255 - 4 * (int)tid;
      const uint32_t h0 = hist[hi], h1 = hist[hi - 1], h2 = hist[hi - 2], h3 = hist[hi - 3];
      const uint32_t own = h0 + h1 + h2 + h3;
      const uint32_t inc = wave_inscan(own);
      const uint32_t total = __shfl(inc, 63);
      const uint32_t nd = need < total ? need : total;  // (first pass only: fewer candidates than asked for)
      if (tid == 0) s_total = total;
      const uint32_t exc = inc - own;
      if (nd != 0u && exc < nd && nd <= inc) {  // exactly one lane
        uint32_t run = exc; int b = hi; uint32_t h = h0;
        if (run + h < nd) { run += h; b = hi - 1; h = h1; }
        if (b == hi - 1 && run + h < nd) { run += h; b = hi - 2; h = h2; }
        if (b == hi - 2 && run + h < nd) { run += h; b = hi - 3; h = h3; }
        s_digit = (uint32_t)b; s_above = run; s_match = h;
      }
    }
    __syncthreads();
    if (s_total == 0u) { none = true; break; }  // (uniform) every score is 0
    if (need > s_total) need = s_total;
#pragma unroll
    for (int w = 0; w < 3; w++)  // (no run-time index into the two keys: they stay in registers)
      if (w == word) { pre.w[w] |= s_digit << shift; msk.w[w] |= 255u << shift; }
    need -= s_above;
    done = s_match == need;  // the bucket holds only keys that are taken: everything at or above the prefix is the selection
    __syncthreads();         // (hist and the s_ words are rewritten by the next pass)
  }
  if (tid == 0) s_count = 0u;
  if (tid < POLISH_MAX_CAND) s_rank[tid] = 0u;
  __syncthreads();
  if (!none) {
#pragma unroll 8
    for (uint64_t g = tid; g < T; g += POLISH_THREADS) {
      const Key96 k{{cnt[g], sel_key[g], ~(uint32_t)g}};
      const Key96 km{{k.w[0] & msk.w[0], k.w[1] & msk.w[1], k.w[2] & msk.w[2]}};
      if (k.w[0] != 0u && !key_above(pre, km)) {
        const uint32_t slot = atomicAdd(&s_count, 1u);
        if (slot < POLISH_MAX_CAND) s_sel[slot] = k;  // (never more than `want` of them)
      }
    }
  }
  __syncthreads();
  const uint32_t K = s_count < want ? s_count : want;
  // order among the K: a key's place is the number of keys above it (they are distinct)
  if (tid < K) {
    uint32_t above = 0;
    for (uint32_t j = 0; j < K; j++) above += key_above(s_sel[j], s_sel[tid]) ? 1u : 0u;
    s_pos[above] = tid;
  }
  // rank in the ranked list: the keys that outrank one's own (sc_winner.hpp: what finalize_kernel counts for its winner), eight
  // candidates per walk over the keys
  __syncthreads();
#pragma unroll 1
  for (uint32_t c0 = 0; c0 < K; c0 += 8) {
    uint32_t r[8], ck[8], cg[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const bool live = c0 + j < K;  // (past K: a key nothing outranks)
      r[j] = 0u; ck[j] = live ? s_sel[c0 + j].w[1] : 0xFFFFFFFFu; cg[j] = live ? ~s_sel[c0 + j].w[2] : 0u;
    }
#pragma unroll 8
    for (uint64_t g = tid; g < T; g += POLISH_THREADS) {
      const uint32_t k = sel_key[g];
#pragma unroll
      for (int j = 0; j < 8; j++) r[j] += outranks(k, (uint32_t)g, ck[j], cg[j]) ? 1u : 0u;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      uint32_t v = r[j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if ((tid & 63u) == 0u && v != 0u && c0 + j < K) atomicAdd(&s_rank[c0 + j], v);
    }
  }
  __syncthreads();
  if (tid < want) {
    PolishCand out;
    if (tid < K) {
      const uint32_t j = s_pos[tid];
      const uint32_t g = ~s_sel[j].w[2];
#pragma unroll
      for (int c = 0; c < 12; c++) out.Rt[c] = RtSoA[(size_t)c * ld_local + g];
      out.rank = s_rank[j]; out.score0 = s_sel[j].w[0];
    } else {
#pragma unroll
      for (int c = 0; c < 12; c++) out.Rt[c] = 0.f;
      out.rank = 0u; out.score0 = 0u;
    }
    out.score = 0u; out.iters = 0; out.reserved = 0;
    cand[tid] = out;
  }
  if (tid == 0) *n_cand = K;
}

// ---- polish ------------------------------------------------------------------------------------------------------------------
// (refit_iterate's chunk storage: ChunkScratch, sc_chunks.hpp — global scratch, the candidate's block)
__global__ __launch_bounds__(POLISH_THREADS) void polish_kernel(const float* __restrict__ planes, int n, int ld, PolishCand* __restrict__ cand,
                                                                const uint32_t* __restrict__ n_cand, uint32_t max_iter, float tau2,
                                                                float thr, int score_mode, double* __restrict__ scratch_all) {
  __shared__ float sRt[12];
  __shared__ double sS[8], sH[9];
  __shared__ uint32_t s_go;
  __shared__ uint64_t s_red[POLISH_THREADS / 64];
  if (blockIdx.x >= *n_cand) return;  // (uniform)
  const uint32_t tid = threadIdx.x;
  const auto ck = ChunkScratch<REFIT_NSUM>::of_pose(scratch_all, blockIdx.x, n);
  PolishCand* me = cand + blockIdx.x;
  if (tid < 12) sRt[tid] = me->Rt[tid];
  __syncthreads();
  const uint32_t iters = refit_iterate<POLISH_THREADS>(planes, ld, n, tau2, max_iter, ck, sRt, sS, sH, &s_go).iters;
  // the last iterate's score over all n, in the frame's score mode (a sum of integers: any order)
  float M[12];
#pragma unroll
  for (int c = 0; c < 12; c++) M[c] = sRt[c];
  uint64_t s = 0;
  if (finite12(M))
    for (int m = (int)tid; m < n; m += POLISH_THREADS) {
      const Corr c = load_corr(planes, ld, m);
      s += score_term(M, c.v[0], c.v[1], c.v[2], c.v[3], c.v[4], c.v[5], thr, score_mode);
    }
  s = block_reduce_u64(s, s_red);
  if (tid < 12) me->Rt[tid] = M[tid];
  if (tid == 0) { me->score = (uint32_t)s; me->iters = (uint16_t)iters; }
}

// ---- winner / mask -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void polish_winner_kernel(const float* __restrict__ planes, int n, int ld,
                                                            const PolishCand* __restrict__ cand, const uint32_t* __restrict__ n_cand,
                                                            uint32_t want, float tau2, float* __restrict__ Rt12, uint8_t* __restrict__ mask,
                                                            PolishCand* __restrict__ out_cand, uint32_t* __restrict__ out_n,
                                                            unsigned long long* __restrict__ host_out) {
  __shared__ float sRt[12];
  __shared__ uint32_t s_win;
  const uint32_t K = *n_cand;
  if (threadIdx.x < 64) {  // largest score, ties to the earlier candidate
    unsigned long long k = threadIdx.x < K ? (((unsigned long long)cand[threadIdx.x].score << 32) | (0xFFFFFFFFu - threadIdx.x)) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(k, o);
      k = other > k ? other : k;
    }
    if (threadIdx.x == 0) s_win = K ? 0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull) : 0u;
  }
  __syncthreads();
  const uint32_t win = s_win;
  winner_rt_to_lds(cand[win].Rt, 1, K != 0u, sRt, Rt12);  // (a record's twelve floats are consecutive)
  __syncthreads();
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m < n) mask[m] = winner_inlier(sRt, K != 0u, load_corr(planes, ld, m), tau2) ? 1 : 0;
  if (blockIdx.x != 0) return;
  if (out_cand) {  // the records, 16 words each (entries past K are zero already)
    const uint32_t* from = reinterpret_cast<const uint32_t*>(cand);
    uint32_t* to = reinterpret_cast<uint32_t*>(out_cand);
    for (uint32_t w = threadIdx.x; w < want * 16u; w += 256u) to[w] = from[w];
  }
  if (threadIdx.x == 0) {
    if (out_n) *out_n = K;
    const unsigned long long rs = K ? (((unsigned long long)cand[win].rank << 32) | (unsigned long long)cand[win].score) : 0ull;
    __hip_atomic_store(&host_out[1], rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_host(reinterpret_cast<uint64_t*>(host_out), ((uint64_t)win << 32) | (uint64_t)K);  // [0] last: the host polls it
  }
}

}  // namespace

void launch_polish_select(const PolishSet& ps, const uint32_t* cnt, const uint32_t* sel_key, uint32_t T, const float* RtSoA, uint32_t ld_local,
                          hipStream_t st) {
  hipLaunchKernelGGL(polish_select_kernel, dim3(1), dim3(POLISH_THREADS), 0, st, cnt, sel_key, T, RtSoA, ld_local, ps.want, ps.cand, ps.n_cand);
}

void launch_polish(const Points& pts, const PolishSet& ps, uint32_t max_iter, float tau2, float thr, int score_mode, double* scratch,
                   hipStream_t st) {
  hipLaunchKernelGGL(polish_kernel, dim3(ps.want), dim3(POLISH_THREADS), 0, st, pts.planes, pts.n, pts.ld, ps.cand, (const uint32_t*)ps.n_cand,
                     max_iter, tau2, thr, score_mode, scratch);
}

void launch_polish_winner(const Points& pts, const PolishSet& ps, const WinnerOut& out, PolishCand* out_cand, uint32_t* out_n, float tau2,
                          hipStream_t st) {
  hipLaunchKernelGGL(polish_winner_kernel, dim3((pts.n + 255) / 256), dim3(256), 0, st, pts.planes, pts.n, pts.ld, (const PolishCand*)ps.cand,
                     (const uint32_t*)ps.n_cand, ps.want, tau2, out.Rt12, out.mask, out_cand, out_n,
                     reinterpret_cast<unsigned long long*>(out.host_out));
}

}  // namespace sc
