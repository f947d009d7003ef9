// sc_peel.hip — rounds on a scored frame (include/saccot.h, sc_peel): the kernels of  claim -> compact -> [score -> arg-max] -> winner / mask.
//
// A frame leaves its T hypotheses (c->rt), their ranking keys (c->sel_key) and the staged planes in the context.  A round scores
// those hypotheses over the correspondences no earlier winner has claimed.  The scores are sums of integers over the alive
// correspondences, so a round may score a COMPACTED copy of them with the frame's own C2 kernel (launch_score) and arg-max
// (launch_argmax): what is new here is the compaction in front and the winner kernel behind, which works on the ORIGINAL planes.
//
//   peel_compact_kernel   one launch.  Every thread owns one correspondence: it folds the previous winner's mask into the claimed
//                         bytes (recomputed from that winner's fp32 (R, t) with the canonical chain: the very bits the round
//                         before returned, so the library never reads an output buffer again), takes its slot among the alive
//                         ones of its wave from a ballot (v_mbcnt), of its workgroup from the four wave counts, of the launch by
//                         decoupled look-back over the tiles (sc_block.hpp), and writes its six coordinates there.  Order
//                         preserved: a round is then reproducible down to the order in which its scoring kernel meets the points.
//   peel_winner_kernel    finalize_kernel's work for one shard — reduce the arg-max launch's pairs, load the winner's (R, t), count
//                         its rank index among the keys, mask — with mask[m] = !claimed[m] && inlier.
//   peel_label_kernel     label[m] = r where mask[m] (sc_register_instances).
#include <cstddef>

#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_kernels.hpp"

namespace sc {

namespace {

constexpr int PEEL_THREADS = 256;  // one correspondence per thread: a tile is 256 of them (C2: 20 tiles; 2^24: 65 536, look-back 64 per step)

__device__ __forceinline__ unsigned long long peel_block_max_u64(unsigned long long k, unsigned long long* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(k, o);
    k = other > k ? other : k;
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = k;
  __syncthreads();
  unsigned long long b = lds[0];
  for (int w = 1; w < 4; w++) b = lds[w] > b ? lds[w] : b;
  return b;
}

__global__ __launch_bounds__(PEEL_THREADS) void peel_compact_kernel(const float* __restrict__ planes, int n, int ld,
                                                                    const float* __restrict__ RtSoA, uint32_t ld_local,
                                                                    uint32_t prev_pos, float tau2, int fresh,
                                                                    uint8_t* __restrict__ claimed, float* __restrict__ alive,
                                                                    PeelWords* __restrict__ words, LbArgs lb,
                                                                    uint64_t* __restrict__ host_alive) {
  __shared__ uint32_t s_tile;
  __shared__ uint32_t s_wave[4];
  __shared__ uint64_t s_prefix;
  if (threadIdx.x == 0) s_tile = __hip_atomic_fetch_add(lb.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const uint32_t tile = s_tile;
  if (tile >= gridDim.x) return;  // (a ticket that was not zero at launch: never index memory with it)
  const int m = (int)(tile * PEEL_THREADS + threadIdx.x);
  const bool in = m < n;
  float cp[6];
#pragma unroll
  for (int c = 0; c < 6; c++) cp[c] = in ? planes[(size_t)c * ld + m] : 0.f;
  bool taken = in && !fresh && claimed[m] != 0;
  if (prev_pos != 0xFFFFFFFFu) {  // the winner before this round: its mask, recomputed (uniform branch)
    float M[12];
#pragma unroll
    for (int c = 0; c < 12; c++) M[c] = RtSoA[(size_t)c * ld_local + prev_pos];
    const float d2 = resid2(M, cp[0], cp[1], cp[2], cp[3], cp[4], cp[5]);
    taken = taken || (finite12(M) && d2 < tau2);
  }
  if (in) claimed[m] = taken ? 1 : 0;
  const bool keep = in && !taken;
  // slot inside the wave: the alive lanes below this one; inside the workgroup: the waves before it
  const unsigned long long bal = __ballot(keep);
  const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = (uint32_t)__builtin_popcountll(bal);
  __syncthreads();
  uint32_t wave_base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const uint32_t x = s_wave[w];
    if (w < wave) wave_base += x;
    tot += x;
  }
  // across the tiles: decoupled look-back (wave 0)
  if (threadIdx.x < 64) {
    uint64_t* const desc[1] = {lb.desc};
    const uint64_t own[1] = {tot};
    uint64_t pre[1];
    lb_lookback<1>(desc, tile, lb.epoch, own, pre, lb.err);
    if (threadIdx.x == 0) s_prefix = pre[0];
  }
  __syncthreads();
  const uint64_t pre = s_prefix;
  if (keep) {
    const size_t slot = (size_t)(pre + wave_base + below);  // < n: one slot per alive correspondence
    if (slot < (size_t)n) {
#pragma unroll
      for (int c = 0; c < 6; c++) alive[(size_t)c * ld + slot] = cp[c];
    }
  }
  if (tile == gridDim.x - 1 && threadIdx.x == 0) {
    words->n_alive = (uint32_t)(pre + tot);
    if (host_alive) publish_host(host_alive, pre + tot);
    __hip_atomic_store(lb.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // every tile has taken its ticket
  }
}

__global__ __launch_bounds__(256) void peel_winner_kernel(const float* __restrict__ planes, int n, int ld,
                                                          const uint8_t* __restrict__ claimed,
                                                          const float* __restrict__ RtSoA, uint32_t ld_local,
                                                          const uint32_t* __restrict__ sel_key, uint32_t T,
                                                          const unsigned long long* __restrict__ pairs, int npairs, float tau2,
                                                          float* __restrict__ Rt12, uint8_t* __restrict__ mask,
                                                          PeelWords* __restrict__ words,
                                                          unsigned long long* __restrict__ host_out) {
  __shared__ uint64_t lds[8];
  __shared__ float sRt[12];
  __shared__ uint32_t s_last;
  const int m = blockIdx.x * 256 + threadIdx.x;
  float cp[6];
#pragma unroll
  for (int c = 0; c < 6; c++) cp[c] = m < n ? planes[(size_t)c * ld + m] : 0.f;
  const bool free_m = m < n && claimed[m] == 0;
  const uint32_t T4 = T >> 2;  // 16-byte loads, grid-strided
  const uint4* __restrict__ k4 = reinterpret_cast<const uint4*>(sel_key);
  // the arg-max launch's per-workgroup pairs -> (best key, lowest position attaining it): a lexicographic max
  unsigned long long k0 = 0, k1 = 0;
  for (int w = threadIdx.x; w < npairs; w += 256) {
    const unsigned long long a = pairs[2 * w], b = pairs[2 * w + 1];
    if (a > k0 || (a == k0 && b > k1)) { k0 = a; k1 = b; }
  }
  {
    unsigned long long* l4 = reinterpret_cast<unsigned long long*>(lds);
    const unsigned long long K = peel_block_max_u64(k0, l4);
    __syncthreads();
    const unsigned long long P = peel_block_max_u64(k0 == K ? k1 : 0ull, l4);
    __syncthreads();
    k0 = K; k1 = P;
  }
  uint32_t g = 0;
  if (k0 != 0) g = 0xFFFFFFFFu - (uint32_t)(k1 & 0xFFFFFFFFull);
  if (k0 != 0 && g >= T) { k0 = 0; k1 = 0; g = 0; }  // (cannot happen with pairs of this context's own arg-max: never index with it)
  if (blockIdx.x == 0 && threadIdx.x == 0) { words->key2[0] = k0; words->key2[1] = k0 ? k1 : 0ull; }
  if (threadIdx.x < 12) {
    const float ident = (threadIdx.x == 0 || threadIdx.x == 4 || threadIdx.x == 8) ? 1.f : 0.f;
    const float v = k0 != 0 ? RtSoA[(size_t)threadIdx.x * ld_local + g] : ident;
    sRt[threadIdx.x] = v;
    if (blockIdx.x == 0) Rt12[threadIdx.x] = v;
  }
  // the winner's rank index: keys above its own, and equal keys at lower positions
  uint32_t r = 0;
  if (k0 != 0) {
    const uint32_t wk = (uint32_t)(k0 & 0xFFFFFFFFull);  // = sel_key[g]
    const uint32_t qs = gridDim.x * 256;
    for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < T4; q += qs) {
      const uint4 v = k4[q];
      const uint32_t t = q << 2;
      r += (v.x > wk) || (v.x == wk && t < g);
      r += (v.y > wk) || (v.y == wk && t + 1 < g);
      r += (v.z > wk) || (v.z == wk && t + 2 < g);
      r += (v.w > wk) || (v.w == wk && t + 3 < g);
    }
    if (blockIdx.x == 0) {
      const uint32_t t = (T4 << 2) + threadIdx.x;  // the last T % 4 keys
      if (t < T) { const uint32_t kt = sel_key[t]; r += (kt > wk) || (kt == wk && t < g); }
    }
  }
  const uint64_t rb = block_reduce_u64(r, lds);  // also the barrier that publishes sRt to the block
  if (m < n) {
    float M[12];
#pragma unroll
    for (int c = 0; c < 12; c++) M[c] = sRt[c];
    const bool live = k0 != 0ull && finite12(M);
    const float d2 = resid2(M, cp[0], cp[1], cp[2], cp[3], cp[4], cp[5]);
    mask[m] = (free_m && live && d2 < tau2) ? 1 : 0;
  }
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const unsigned long long was = __hip_atomic_fetch_add(&words->fin_word, (1ull << 32) | (unsigned long long)(uint32_t)rb,
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = ((uint32_t)(was >> 32) == gridDim.x - 1) ? 1u : 0u;
    if (s_last) {
      const uint32_t rank = (uint32_t)was + (uint32_t)rb;
      __hip_atomic_store(&words->fin_word, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next round
      __hip_atomic_store(&host_out[1], k0 ? (((unsigned long long)rank << 32) | (unsigned long long)g) : 0ull, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
      publish_host(reinterpret_cast<uint64_t*>(host_out), k0);  // [0] last: the host polls it (release orders the others before it)
    }
  }
}

__global__ __launch_bounds__(256) void peel_label_kernel(const uint8_t* __restrict__ mask, int n, int32_t value,
                                                         int32_t* __restrict__ label) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m < n && mask[m]) label[m] = value;
}

}  // namespace

uint32_t peel_compact_tiles(int n) { return (uint32_t)((n + PEEL_THREADS - 1) / PEEL_THREADS); }

void launch_peel_compact(const Points& pts, const float* RtSoA, uint32_t ld_local, uint32_t prev_pos, float tau2, bool fresh,
                         uint8_t* claimed, float* alive, PeelWords* words, LbArgs lb, uint64_t* host_alive, hipStream_t st) {
  hipLaunchKernelGGL(peel_compact_kernel, dim3(peel_compact_tiles(pts.n)), dim3(PEEL_THREADS), 0, st, pts.planes, pts.n, pts.ld,
                     RtSoA, ld_local, prev_pos, tau2, fresh ? 1 : 0, claimed, alive, words, lb, host_alive);
}

void launch_peel_winner(const Points& pts, const uint8_t* claimed, const float* RtSoA, uint32_t ld_local, const uint32_t* sel_key,
                        uint32_t T, const uint64_t* pairs, int npairs, float tau2, float* Rt12, uint8_t* mask, PeelWords* words,
                        uint64_t* host_out, hipStream_t st) {
  uint32_t blocks = (uint32_t)((pts.n + 255) / 256);  // the mask needs these; more only if the key list is long (launch_finalize)
  const uint32_t for_keys = (T / 4 + 1023) / 1024;
  if (for_keys > blocks) blocks = for_keys < 1024u ? for_keys : 1024u;
  hipLaunchKernelGGL(peel_winner_kernel, dim3(blocks), dim3(256), 0, st, pts.planes, pts.n, pts.ld, claimed, RtSoA, ld_local,
                     sel_key, T, reinterpret_cast<const unsigned long long*>(pairs), npairs, tau2, Rt12, mask, words,
                     reinterpret_cast<unsigned long long*>(host_out));
}

void launch_peel_label(const uint8_t* mask, int n, int32_t value, int32_t* label, hipStream_t st) {
  hipLaunchKernelGGL(peel_label_kernel, dim3((n + 255) / 256), dim3(256), 0, st, mask, n, value, label);
}

}  // namespace sc
