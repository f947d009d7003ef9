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
//                         its rank index among the keys, mask — with mask[m] = !claimed[m] && inlier: both compose sc_winner.hpp's steps.
//   peel_label_kernel     label[m] = r where mask[m] (sc_register_instances).
#include <cstddef>

#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_kernels.hpp"
#include "sc_winner.hpp"

namespace sc {

namespace {

constexpr int PEEL_THREADS = 256;  // one correspondence per thread: a tile is 256 of them (C2: 20 tiles; 2^24: 65 536, look-back 64 per step)

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
  const Corr cp = in ? load_corr(planes, ld, m) : Corr{};
  bool taken = in && !fresh && claimed[m] != 0;
  if (prev_pos != 0xFFFFFFFFu) {  // the winner before this round: its mask, recomputed (uniform branch)
    float M[12];
#pragma unroll
    for (int c = 0; c < 12; c++) M[c] = RtSoA[(size_t)c * ld_local + prev_pos];
    taken = taken || is_inlier(M, cp, tau2);
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
      for (int c = 0; c < 6; c++) alive[(size_t)c * ld + slot] = cp.v[c];
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
  const int m = blockIdx.x * 256 + threadIdx.x;
  const Corr cp = m < n ? load_corr(planes, ld, m) : Corr{};
  const bool free_m = m < n && claimed[m] == 0;
  const uint4 v_first = rank_prefetch(sel_key, T);
  // the arg-max launch's per-workgroup pairs -> (best key, lowest position attaining it)
  unsigned long long k0, k1;
  reduce_pairs(pairs, npairs, reinterpret_cast<unsigned long long*>(lds), k0, k1);
  const Winner w = winner_decode(k0, k1, true, T);
  winner_key_store(words->key2, w);
  winner_rt_to_lds(RtSoA + w.g, ld_local, w.k0 != 0, sRt, Rt12);
  uint32_t r = 0;  // (the key's low half is sel_key[g])
  if (w.k0 != 0) r = rank_count(sel_key, T, v_first, (uint32_t)(w.k0 & 0xFFFFFFFFull), w.g);
  const uint64_t rb = block_reduce_u64(r, lds);  // also the barrier that publishes sRt to the block
  if (m < n) mask[m] = (free_m && winner_inlier(sRt, w.k0 != 0ull, cp, tau2)) ? 1 : 0;
  uint32_t rank;
  if (threadIdx.x == 0 && last_workgroup_sum(&words->fin_word, (uint32_t)rb, &rank)) {
    __hip_atomic_store(&host_out[1], w.k0 ? (((unsigned long long)rank << 32) | (unsigned long long)w.g) : 0ull, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
    publish_host(reinterpret_cast<uint64_t*>(host_out), w.k0);  // [0] last: the host polls it (release orders the others before it)
  }
}

__global__ __launch_bounds__(256) void peel_label_kernel(const uint8_t* __restrict__ mask, int n, int32_t value,
                                                         int32_t* __restrict__ label) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m < n && mask[m]) label[m] = value;
}

}  // namespace

uint32_t peel_compact_tiles(int n) { return (uint32_t)((n + PEEL_THREADS - 1) / PEEL_THREADS); }

void launch_peel_compact(const Points& pts, const Hyps& h, const PeelSets& ps, uint32_t prev_pos, float tau2, bool fresh,
                         PeelWords* words, LbArgs lb, hipStream_t st) {
  hipLaunchKernelGGL(peel_compact_kernel, dim3(peel_compact_tiles(pts.n)), dim3(PEEL_THREADS), 0, st, pts.planes, pts.n, pts.ld,
                     h.soa, h.sh.ld_local, prev_pos, tau2, fresh ? 1 : 0, ps.claimed, ps.alive, words, lb, ps.host_alive);
}

void launch_peel_winner(const Points& pts, const Hyps& h, const WinnerIn& in, const WinnerOut& out, const uint8_t* claimed, float tau2,
                        PeelWords* words, hipStream_t st) {
  hipLaunchKernelGGL(peel_winner_kernel, dim3(winner_blocks(pts.n, in.T)), dim3(256), 0, st, pts.planes, pts.n, pts.ld, claimed,
                     h.soa, h.sh.ld_local, in.sel_key, in.T, reinterpret_cast<const unsigned long long*>(in.keys),
                     in.npairs, tau2, out.Rt12, out.mask, words, reinterpret_cast<unsigned long long*>(out.host_out));
}

void launch_peel_label(const uint8_t* mask, int n, int32_t value, int32_t* label, hipStream_t st) {
  hipLaunchKernelGGL(peel_label_kernel, dim3((n + 255) / 256), dim3(256), 0, st, mask, n, value, label);
}

}  // namespace sc
