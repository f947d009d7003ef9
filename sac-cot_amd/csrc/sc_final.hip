// sc_final.hip — stage C3: the winner of a scored frame, its rank index and its mask in one launch (finalize_kernel), the mask of an
// explicit hypothesis (mask_kernel), and the optional fp64 refit over the mask (refine_kernel).  SURVEY.md §8a row C3, §8f-2.
// What finalize_kernel shares with the winner kernels of sc_peel.hip and sc_polish.hip is in sc_winner.hpp.
#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_kernels.hpp"
#include "sc_refine.hpp"
#include "sc_gramref.hpp"
#include "sc_winner.hpp"

namespace sc {

// ------------------------------------------------------------------------------------------------
// C3
// ------------------------------------------------------------------------------------------------
// C3 in ONE launch: every block re-solves the winner (thread 0; deterministic, so all blocks hold the same R,t) while
// its other threads count their slice of the winner's rank index (#keys above the winner's + #equal keys at lower
// positions — the number the ranked list would have given it), then masks its 256 correspondences.  The slice counts
// meet in a control-block counter; the block that takes the last ticket publishes (key, position, rank) to the host.
// (A single-block rank count cost 42 us at T = 400 k; a separate mask launch another ~4.5 us floor.)
__global__ __launch_bounds__(256) void finalize_kernel(const float* __restrict__ planes, int n, int ld,
                                                       TriSource ts, Shard sh, const float* __restrict__ RtSoA,
                                                       const uint32_t* __restrict__ sel_key, uint32_t T,
                                                       const unsigned long long* __restrict__ key2, int npairs,
                                                       unsigned long long* __restrict__ key_out, float tau2,
                                                       float* __restrict__ Rt12, uint8_t* __restrict__ mask,
                                                       unsigned long long* __restrict__ fin_word,
                                                       unsigned long long* __restrict__ host_out, DeferredPub dp) {
  __shared__ uint64_t lds[8];
  __shared__ float sRt[12];
  // (what does not depend on the winner is on its way before the pairs are looked at: this thread's correspondence, its first
  // keys of the rank count — the kernel is a chain of dependent loads, ~1 us each)
  const int m = blockIdx.x * 256 + threadIdx.x;
  const Corr cp = m < n ? load_corr(planes, ld, m) : Corr{};
  const uint4 v_first = rank_prefetch(sel_key, T);
  // key2: npairs winner key pairs (one per rank, all-gathered; npairs = 1: an already reduced pair).  The reduction of
  // include/saccot.h — K0 = max pair[0], K1 = max pair[1] among the pairs attaining K0 — is a lexicographic max.
  unsigned long long k0 = 0, k1 = 0;
  if (npairs <= 8) {
    for (int w = 0; w < npairs; w++) lexmax_take(k0, k1, key2[2 * w], key2[2 * w + 1]);  // wave-uniform addresses: scalar loads
  } else {
    reduce_pairs(key2, npairs, reinterpret_cast<unsigned long long*>(lds), k0, k1);
  }
  // The pairs come from the caller (an all-gather): one that decodes to nothing of the selection is reported — host_out[1] = all
  // ones makes the host return SC_EINVAL.
  const bool two_stage = sel_key != nullptr;
  const Winner w = winner_decode(k0, k1, two_stage, T);
  if (key_out) winner_key_store(key_out, w);
  // The winner's (R,t): if THIS rank scored it, phase 1 left it in RtSoA (kabsch3 is deterministic, so these are the
  // very bits a re-solve gives) — 12 parallel loads; otherwise thread 0 re-solves it from the replicated selection.
  const uint32_t gb = sh.block ? w.g / sh.block : 0u;
  const bool local = RtSoA != nullptr && w.k0 != 0 && w.g < sh.T_eff && (gb % sh.world) == sh.rank;
  if (local) {
    const uint32_t l = (gb / sh.world) * sh.block + (w.g % sh.block);
    winner_rt_to_lds(RtSoA + l, sh.ld_local, true, sRt, Rt12);
  } else if (threadIdx.x == 0) {
    float Rt[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    uint32_t v[3];
    if (w.k0 != 0 && tri_lookup(ts, w.g, v)) {
      float P[9], Q[9];
      load_triangle(planes, ld, v, P, Q);
      kabsch3(P, Q, Rt);
    }
#pragma unroll
    for (int c = 0; c < 12; c++) sRt[c] = Rt[c];
    if (blockIdx.x == 0) {
#pragma unroll
      for (int c = 0; c < 12; c++) Rt12[c] = Rt[c];
    }
  }
  uint32_t r = 0;  // (the key's low half is sel_key[g]: score_argmax_kernel)
  if (two_stage && w.k0 != 0) r = rank_count(sel_key, T, v_first, (uint32_t)(w.k0 & 0xFFFFFFFFull), w.g);
  const uint64_t rb = block_reduce_u64(r, lds);  // also the barrier that publishes sRt to the block
  if (m < n) mask[m] = winner_inlier(sRt, w.k0 != 0ull, cp, tau2) ? 1 : 0;
  uint32_t rank;
  if (threadIdx.x == 0 && last_workgroup_sum(fin_word, (uint32_t)rb, &rank)) {
    if (host_out && dp.host) {
      // a host-free call: the words its earlier kernels would have published one by one go to the host HERE, with the winner
      // (relaxed system-scope stores: the release store of the key below orders them before it).  Every such store costs the
      // kernel that makes it ~0.5 us (seven of them cost the staging kernel 1.7 us; nine here cost this kernel 5:
      // profiles/r05_ab_deferred_publish.txt), so stage B's two counts travel in ONE word — edges in the low half, triangles in
      // the high half, all ones where one of them does not fit (the host then repeats the call) — and the staging kernel's
      // coordinate statistics only every 64th host-free call of a context (dp.with_stats): a host-free call picks stage C2's
      // kernel by the statistics of an earlier frame anyway, and any pick gives the same counts.
      auto put = [&](int idx, unsigned long long v) { __hip_atomic_store(&dp.host[idx], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
      const unsigned long long e = *dp.dev_edges, m = *dp.dev_triangles;
      put(HW_EDGES, (e < (1ull << 32) && m < (1ull << 32)) ? (e | (m << 32)) : ~0ull);
      if (dp.with_stats) {
        for (int k = 0; k < 6; k++) put(HW_BOX + k, ((unsigned long long)dp.coord_max[8 + k] << 32) | dp.coord_max[2 + k]);
        put(HW_COORD_MAX, ((unsigned long long)dp.coord_max[1] << 32) | dp.coord_max[0]);
      }
    }
    if (host_out) {  // [0] last: the host polls it (release orders the others before it)
      // ONE word beside the key (a system-scope store costs ~0.5 us: see DeferredPub): the winner's rank index in the high half,
      // its position in the low half — or all ones: a key pair that decodes to nothing of the selection (the host: SC_EINVAL)
      const unsigned long long rk = w.k0 ? (two_stage ? (unsigned long long)rank : (unsigned long long)w.g) : 0ull;
      __hip_atomic_store(&host_out[1], w.bad ? ~0ull : ((rk << 32) | (unsigned long long)w.g), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      publish_host(reinterpret_cast<uint64_t*>(host_out), w.k0);
    }
  }
}

__global__ __launch_bounds__(256) void mask_kernel(const float* __restrict__ planes, int n, int ld,
                                                   const float* __restrict__ Rt12,
                                                   const unsigned long long* __restrict__ key, float tau2,
                                                   uint8_t* __restrict__ mask) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= n) return;
  mask[m] = winner_inlier(Rt12, key == nullptr || *key != 0ull, load_corr(planes, ld, m), tau2) ? 1 : 0;
}

void launch_finalize(const Points& pts, const TriSource& ts, const Hyps& h, const WinnerIn& in, const WinnerOut& out, float tau2,
                     uint64_t* key_out, unsigned long long* fin_word, const DeferredPub* dp, hipStream_t st) {
  hipLaunchKernelGGL(finalize_kernel, dim3(winner_blocks(pts.n, in.T)), dim3(256), 0, st, pts.planes, pts.n, pts.ld, ts, h.sh,
                     h.soa, in.sel_key, in.T, reinterpret_cast<const unsigned long long*>(in.keys), in.npairs,
                     reinterpret_cast<unsigned long long*>(key_out), tau2, out.Rt12, out.mask, fin_word,
                     reinterpret_cast<unsigned long long*>(out.host_out), dp ? *dp : DeferredPub{nullptr, nullptr, nullptr, nullptr, 0});
}

// ------------------------------------------------------------------------------------------------
// Winner refinement (optional — SC_FLAG_REFINE): fp64 least-squares rigid refit over the inlier mask.
// Canonical order shared with oracle/saccot_oracle.c::so_refine: chunks of 64 consecutive points are summed
// sequentially in index order (one thread per chunk), chunk sums are added sequentially in chunk order (thread 0);
// pass 1 gives count and centroids, pass 2 H = sum (p - pc)(q - qc)^T by fma, then the two-dominant-pairs +
// cross-product construction of kabsch3 in double with 10 Jacobi sweeps.  One workgroup: N is a few thousand.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void refine_kernel(const float* __restrict__ planes, int n, int ld,
                                                      const uint8_t* __restrict__ mask,
                                                      const unsigned long long* __restrict__ key2,
                                                      double* __restrict__ scratch, float* __restrict__ Rt12) {
  __shared__ double cen[8];
  if (key2[0] == 0ull) return;  // no hypothesis: nothing to refine (uniform)
  const int nch = (n + 63) / 64;
  // pass 1: per-chunk count / sum p / sum q
  for (int ch = threadIdx.x; ch < nch; ch += 1024) {
    double c[7] = {0, 0, 0, 0, 0, 0, 0};
    const int m1 = min(n, ch * 64 + 64);
    for (int m = ch * 64; m < m1; m++) {
      if (!mask[m]) continue;
      c[0] += 1.0;
#pragma unroll
      for (int k = 0; k < 3; k++) { c[1 + k] += (double)planes[(size_t)k * ld + m]; c[4 + k] += (double)planes[(size_t)(3 + k) * ld + m]; }
    }
#pragma unroll
    for (int k = 0; k < 7; k++) scratch[(size_t)ch * 16 + k] = c[k];
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    double S[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int ch = 0; ch < nch; ch++)
#pragma unroll
      for (int k = 0; k < 7; k++) S[k] += scratch[(size_t)ch * 16 + k];
    cen[0] = S[0];
#pragma unroll
    for (int k = 0; k < 3; k++) { cen[1 + k] = S[1 + k] / S[0]; cen[4 + k] = S[4 + k] / S[0]; }
  }
  __syncthreads();
  if (cen[0] < 3.0) return;  // uniform
  const double pc[3] = {cen[1], cen[2], cen[3]}, qc[3] = {cen[4], cen[5], cen[6]};
  // pass 2: per-chunk covariance
  for (int ch = threadIdx.x; ch < nch; ch += 1024) {
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int m1 = min(n, ch * 64 + 64);
    for (int m = ch * 64; m < m1; m++) {
      if (!mask[m]) continue;
      double a[3], b[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        a[k] = (double)planes[(size_t)k * ld + m] - pc[k];
        b[k] = (double)planes[(size_t)(3 + k) * ld + m] - qc[k];
      }
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) h[3 * r + c] = __builtin_fma(a[r], b[c], h[3 * r + c]);
    }
#pragma unroll
    for (int k = 0; k < 9; k++) scratch[(size_t)ch * 16 + k] = h[k];
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x != 0) return;
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int ch = 0; ch < nch; ch++)
#pragma unroll
    for (int k = 0; k < 9; k++) H[k] += scratch[(size_t)ch * 16 + k];
  refine_solve(H, pc, qc, Rt12);  // (a non-finite result leaves Rt12 untouched)
}

size_t refine_scratch_bytes(int n) { return (size_t)((n + 63) / 64) * 16 * sizeof(double); }

void launch_refine(const Points& pts, const uint8_t* mask, const uint64_t* key2, double* scratch, float* Rt12,
                   hipStream_t st) {
  hipLaunchKernelGGL(refine_kernel, dim3(1), dim3(1024), 0, st, pts.planes, pts.n, pts.ld, mask,
                     reinterpret_cast<const unsigned long long*>(key2), scratch, Rt12);
}

void launch_mask(const Points& pts, const float* Rt12, float tau2, uint8_t* mask, hipStream_t st) {
  hipLaunchKernelGGL(mask_kernel, dim3((pts.n + 255) / 256), dim3(256), 0, st, pts.planes, pts.n, pts.ld, Rt12,
                     (const unsigned long long*)nullptr, tau2, mask);
}

}  // namespace sc
