// sc_score.hip — stage C2's plain kernel: hypothesis x correspondence inlier counting (every score mode) with its arg-max.
// SURVEY.md §8a row C2.  (C1 — the per-triangle rigid transform — is sc_kabsch.hip; C3 — the winner, its mask, the refit — sc_final.hip.)
//
// Stage C is four translation units over sc_score.hpp.  The library is built without relocatable device code, so a __device__ function
// is callable only from the file that defines it — and that pins exactly one group together: kabsch_shard_kernel calls filter_tile_block
// and gram_coef_block (the Kabsch launch carries C2's fp16 tile and the Gram coefficient rows), so C1, the tile and the coefficients
// are sc_kabsch.hip.  Nothing else calls across: this file holds the plain C2 kernel and the arg-max, sc_filter.hip the linear filter,
// the exact pass and the Gram filter (gram_geom is shared by those two kernels), sc_gram_guard.hip the probe of the matrix pipe.
//
// C2 is the arithmetic-heavy kernel of the path (T*N tests, 27 flop each) and moves almost no HBM bytes
// (48 B per hypothesis in, 4 B out), so it is bounded by the fp32 vector rate, not by HBM.  Mapping:
//   lane          = one hypothesis: its 12 coefficients live in VGPRs for the whole kernel, its inlier
//                   count is a private register — no cross-lane reduction, no atomics on the hot loop;
//   workgroup     = 256 hypotheses x one chunk of <= 1024 correspondences staged once into LDS;
//   inner loop    = every lane reads the SAME point (one ds_read_b128 + one ds_read_b64, LDS broadcast,
//                   conflict-free), then 12 FMA-class ops for the residual, 3 for its square norm, one
//                   compare and one add-with-carry: 17 VALU instructions per test;
//   grid          = ceil(T/256) x chunks, so a 50k x 5k problem is ~1000 workgroups (~4 waves per SIMD);
//   partial counts are stored coalesced ([chunk][hypothesis]) and summed by the arg-max kernel.
#include <cstddef>

#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_score.hpp"
#include "sc_gramref.hpp"  // shard_global_index

namespace sc {

// ------------------------------------------------------------------------------------------------
// sharding of the ranked list: blocks of `block` triangles dealt round-robin to ranks
// ------------------------------------------------------------------------------------------------

uint32_t shard_local_count(uint32_t T_eff, uint32_t block, uint32_t rank, uint32_t world) {
  uint64_t n = 0;
  for (uint64_t gb = rank; gb * block < T_eff; gb += world) {
    const uint64_t lo = gb * block, hi = (gb + 1) * (uint64_t)block;
    n += (hi < T_eff ? hi : T_eff) - lo;
  }
  return (uint32_t)n;
}

// ------------------------------------------------------------------------------------------------
// C2
// ------------------------------------------------------------------------------------------------
constexpr int SCORE_THREADS = 256;
constexpr int SCORE_PC = 512;  // correspondences per chunk (LDS: 12 KiB per workgroup, 8 workgroups per CU)

// Point chunking of C2: workgroups = (hypothesis groups of 256) x chunks.  Chunks are as long as LDS allows (512) for
// big problems, shorter for small ones so that the launch still has ~2048 workgroups (8 per CU) to fill the chip.
void score_plan(int n, uint32_t ld_local, uint32_t* chunks, int* chunk_pts) {
  const uint32_t groups = ld_local / SCORE_THREADS ? ld_local / SCORE_THREADS : 1u;
  uint32_t want = 2048 / groups;                                      // at most one resident generation (8 per CU)
  const uint32_t min_chunks = (uint32_t)((n + SCORE_PC - 1) / SCORE_PC);  // LDS capacity
  const uint32_t max_chunks = (uint32_t)((n + 63) / 64);                  // at least 64 points per chunk
  if (want < min_chunks) want = min_chunks;
  if (want > max_chunks) want = max_chunks;
  if (want < 1) want = 1;
  int per = (int)((n + want - 1) / want);
  per = (per + 3) & ~3;                                               // multiple of 4, <= SCORE_PC
  if (per > SCORE_PC) per = SCORE_PC;
  *chunk_pts = per;
  *chunks = (uint32_t)((n + per - 1) / per);
}
// (r02 also had a lane = correspondence mapping with the hypothesis in scalar registers: bit-exact, 114.8 us against 93.9 at C2
// — VALU instructions with a scalar-register operand issue at 4.4 cycles on this part against 3.04 — removed in r05;
// profiles/r02_* keep its numbers.)
uint32_t score_chunks(int n, uint32_t ld_local) {
  uint32_t c; int p;
  score_plan(n, ld_local, &c, &p);
  return c;
}

// One inlier test, written so that hipcc keeps 17 single-issue VALU ops (build.py passes -fno-slp-vectorize:
// SLP packing turns the chain into v_pk_* plus ~5 v_mov per test, which is slower on gfx950).
// MODE 0: 1 if inlier.  MODE 1 / 2 (include/saccot.h, SC_SCORE_MSE / _MAE): floor(1024 max(0, 1 - d2 / tau^2)) resp.
// floor(1024 max(0, 1 - d / tau)) — integers, so the sum over the correspondences is exact in any order.  `thr` is
// tau^2, 1 / tau^2 or 1 / tau.  (d2 = +inf -> fma = -inf -> 0; the float -> u32 conversion truncates.)
template <int MODE>
__device__ __forceinline__ uint32_t inlier_bit(const float (&M)[12], const float4 a, const float2 b, float thr) {
  const float d2 = resid2(M, a.x, a.y, a.z, a.w, b.x, b.y);
  if (MODE == 0) return d2 < thr ? 1u : 0u;
  const float x = MODE == 1 ? d2 : sqrt_rn(d2);
  return (uint32_t)(fmaxf(fma_(-x, thr, 1.0f), 0.0f) * 1024.0f);
}

// VALU body: lane = hypothesis.  bx = workgroup index along the hypotheses (256 per workgroup), hyp_base = first one.
template <int MODE>
__device__ __forceinline__ void score_valu_body(float4* __restrict__ smem, uint32_t hyp_base, int chunk,
                                                const float* __restrict__ planes, int n, int ld,
                                                const float* __restrict__ RtSoA, uint32_t ld_local, float tau2,
                                                int chunk_pts, uint32_t* __restrict__ partial) {
  float4* pA = smem;                                          // px py pz qx
  float2* pB = reinterpret_cast<float2*>(smem + SCORE_PC);    // qy qz
  const int m0 = chunk * chunk_pts;
  const int cnt_pts = min(chunk_pts, n - m0);
  const int padded = (cnt_pts + 3) & ~3;  // <= chunk_pts <= SCORE_PC (chunk_pts is a multiple of 4)
  for (int t = threadIdx.x; t < padded; t += SCORE_THREADS) {
    const int m = m0 + t;
    if (t < cnt_pts) {
      pA[t] = make_float4(planes[m], planes[(size_t)ld + m], planes[2 * (size_t)ld + m], planes[3 * (size_t)ld + m]);
      pB[t] = make_float2(planes[4 * (size_t)ld + m], planes[5 * (size_t)ld + m]);
    } else {  // sentinel: p = 0, q = 1e30 -> residual ~1e30, squared = +inf: never < tau2, score 0, never NaN
      pA[t] = make_float4(0.f, 0.f, 0.f, 1e30f);
      pB[t] = make_float2(1e30f, 1e30f);
    }
  }
  const uint32_t l = hyp_base + threadIdx.x;
  float M[12];
#pragma unroll
  for (int c = 0; c < 12; c++) M[c] = RtSoA[(size_t)c * ld_local + l];
  const bool ok = finite12(M);
  __syncthreads();
  uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (int t = 0; t < padded; t += 4) {
    const float4 a0 = pA[t], a1 = pA[t + 1], a2 = pA[t + 2], a3 = pA[t + 3];
    const float2 b0 = pB[t], b1 = pB[t + 1], b2 = pB[t + 2], b3 = pB[t + 3];
    c0 += inlier_bit<MODE>(M, a0, b0, tau2);
    c1 += inlier_bit<MODE>(M, a1, b1, tau2);
    c2 += inlier_bit<MODE>(M, a2, b2, tau2);
    c3 += inlier_bit<MODE>(M, a3, b3, tau2);
  }
  partial[(size_t)chunk * ld_local + l] = ok ? (c0 + c1) + (c2 + c3) : 0u;
}

// ------------------------------------------------------------------------------------------------
// C2 on the matrix pipe.  v_mfma_f32_16x16x4_f32 computes D = A(16x4) B(4x16) + C as a k-ordered fp32 fma chain
// (one rounding per product, bit-for-bit fmaf: cdna guide §3 "FP32-input MFMA"), which is exactly the canonical
// residual  e_c = fma(t_c,1, fma(r_c2,pz, fma(r_c1,py, fma(r_c0,px, -q_c))))  when
//   A[row = 4 hq + c][k] = (r_c0, r_c1, r_c2, t_c)[k]      4 hypotheses hq x 3 components c (row 4hq+3 is zero)
//   B[k][col]            = (px, py, pz, 1)[k] of point col   16 correspondences
//   C[row][col]          = -q_c of point col
// so one instruction yields the residuals of 4 x 16 tests.  Lane l receives D rows 4 (l>>4) + {0,1,2} of column
// l & 15: the three components of ONE test, so the squared norm, the compare and the count stay lane-local (5 VALU
// instructions per 64 tests instead of 17.5), and 4 shuffles per hypothesis at the very end sum the 16 columns.
// ------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int MF_QUADS = 8;                 // hypothesis quads per wave: 32 hypotheses
constexpr int MF_HYPS_PER_BLOCK = 4 * 4 * MF_QUADS;  // 4 waves

// MFMA body: hyp_base = first hypothesis of the workgroup (MF_HYPS_PER_BLOCK per workgroup).
__device__ __forceinline__ void score_mfma_body(float4* __restrict__ smem, uint32_t hyp_base, int chunk,
                                                const float* __restrict__ planes, int n, int ld,
                                                const float* __restrict__ RtSoA, uint32_t ld_local, float tau2,
                                                int chunk_pts, uint32_t* __restrict__ partial) {
  float4* P4 = smem;             // px py pz 1
  float4* Qn = smem + SCORE_PC;  // -qx -qy -qz 0
  const int m0 = chunk * chunk_pts;
  const int cnt_pts = min(chunk_pts, n - m0);
  const int padded = (cnt_pts + 15) & ~15;  // whole 16-point groups; chunk_pts <= SCORE_PC and SCORE_PC % 16 == 0
  for (int t = threadIdx.x; t < padded; t += 256) {
    const int m = m0 + t;
    if (t < cnt_pts) {
      P4[t] = make_float4(planes[m], planes[(size_t)ld + m], planes[2 * (size_t)ld + m], 1.0f);
      Qn[t] = make_float4(-planes[3 * (size_t)ld + m], -planes[4 * (size_t)ld + m], -planes[5 * (size_t)ld + m], 0.f);
    } else {  // sentinel: residual ~ -1e30, squared = +inf, never < tau2, never NaN
      P4[t] = make_float4(0.f, 0.f, 0.f, 1.0f);
      Qn[t] = make_float4(-1e30f, -1e30f, -1e30f, 0.f);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t hyp0 = hyp_base + wave * (4 * MF_QUADS);  // first hypothesis of this wave
  // A operands: lane l feeds row (l & 15) = 4 hq + c, k = l >> 4
  const int a_hq = (lane & 15) >> 2, a_c = lane & 3, a_k = lane >> 4;
  float a[MF_QUADS];
  uint64_t badmask[MF_QUADS];
#pragma unroll
  for (int q = 0; q < MF_QUADS; q++) {
    const uint32_t h = hyp0 + 4 * q + a_hq;  // < ld_local: ld_local is a multiple of 256 >= MF_HYPS_PER_BLOCK blocks
    float v = 0.0f;
    if (a_c < 3) v = RtSoA[(size_t)(a_k < 3 ? 3 * a_c + a_k : 9 + a_c) * ld_local + h];
    a[q] = v;
    badmask[q] = __ballot(!(fabsf(v) < __builtin_inff()));  // lanes holding a non-finite coefficient
  }
  __syncthreads();
  uint32_t cnt[MF_QUADS];
#pragma unroll
  for (int q = 0; q < MF_QUADS; q++) cnt[q] = 0;
  const float* P4f = reinterpret_cast<const float*>(P4);
  const int col = lane & 15, kb = lane >> 4;
  for (int g = 0; g < padded; g += 16) {
    const float b = P4f[(g + col) * 4 + kb];
    const float4 cq = Qn[g + col];
    const f32x4 c = {cq.x, cq.y, cq.z, cq.w};
    // all MF_QUADS products first, into distinct result tiles (independent: they pipeline at the 32-cycle issue rate),
    // then the lane-local epilogues — a single reused tile would serialise on the 40-cycle result latency
    f32x4 d[MF_QUADS];
#pragma unroll
    for (int q = 0; q < MF_QUADS; q++) d[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b, c, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < MF_QUADS; q++) {
      const float d2 = fma_(d[q][2], d[q][2], fma_(d[q][1], d[q][1], d[q][0] * d[q][0]));
      cnt[q] += (d2 < tau2) ? 1u : 0u;
    }
  }
  // lane l counted hypothesis (quad q, member l >> 4) over the columns l & 15: sum the 16 columns
#pragma unroll
  for (int q = 0; q < MF_QUADS; q++) {
    uint32_t c = cnt[q];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) c += __shfl_xor(c, o, 16);
    // coefficient lanes of member hq' = l >> 4 are {16 k + 4 hq' + c}: any non-finite one zeroes the hypothesis
    const uint64_t mine = 0x000F000F000F000Full << (4 * (lane >> 4));
    if (badmask[q] & mine) c = 0;
    const uint32_t h = hyp0 + 4 * q + (lane >> 4);
    if (col == 0) partial[(size_t)chunk * ld_local + h] = c;
  }
}

// One launch, two kinds of workgroup.  Hypotheses [0, hv) go to VALU workgroups (256 each), [hv, ld_local) to MFMA
// workgroups (128 each); the two kinds are interleaved along blockIdx.x so that every CU holds both and its vector
// and matrix pipes work at the same time (cdna guide: "MFMA and VALU pipes are separate").
// __launch_bounds__(256, 8): <= 64 VGPRs, 8 waves per SIMD — plain v_fma_f32 needs that occupancy on gfx950
// (measured 45 / 80 / 99 / 117 TFLOP/s at 1 / 2 / 4 / 8 waves per SIMD, tools/ubench_valu.hip).
template <int MODE>
__global__ __launch_bounds__(SCORE_THREADS, 8) void score_kernel(const float* __restrict__ planes, int n, int ld,
                                                                 const float* __restrict__ RtSoA, uint32_t ld_local,
                                                                 float tau2, int chunk_pts,
                                                                 uint32_t* __restrict__ partial, uint32_t nv,
                                                                 uint32_t nm) {
  __shared__ float4 smem[2 * SCORE_PC];  // 16 KiB: both bodies carve their point images out of it
  const uint32_t bx = blockIdx.x, tot = nv + nm;
  // Bresenham spread of the nm MFMA workgroups among the nv VALU ones
  const uint32_t m_before = (uint32_t)(((uint64_t)bx * nm) / tot), m_after = (uint32_t)(((uint64_t)(bx + 1) * nm) / tot);
  if (MODE == 0 && m_after != m_before)  // the matrix-pipe body counts inliers only
    score_mfma_body(smem, nv * SCORE_THREADS + m_before * MF_HYPS_PER_BLOCK, blockIdx.y, planes, n, ld, RtSoA, ld_local,
                    tau2, chunk_pts, partial);
  else
    score_valu_body<MODE>(smem, (bx - m_before) * SCORE_THREADS, blockIdx.y, planes, n, ld, RtSoA, ld_local, tau2, chunk_pts,
                    partial);
}

// Per-hypothesis count (sum of the chunk partials) and the winner key pair, in ONE launch and without atomics on
// the keys: every block reduces its hypotheses to (best key, lowest position attaining it) and stores the pair; the
// block that takes the last ticket reduces the pairs and writes key2[0..1] (so key2 needs no zeroing).
//   key = (count << 32) | second, second = sel_key[g] or, without sel_key, 0xFFFFFFFF - g;  position = 0xFFFFFFFF - g.
// (r04 let the workgroup that takes the last ticket go on with the winner's own work — mask, rank index, (R, t) — instead of
// finalize_kernel's launch: bit-exact, and the arg-max launch went from 8.6 to 33 us at C2 against 6.4 us for that kernel's grid
// (one workgroup walks 5000 correspondences and 50 000 keys in ~70 dependent load rounds); removed in r05.)
__global__ __launch_bounds__(256) void score_argmax_kernel(const uint32_t* __restrict__ partial, uint32_t n_chunks,
                                                           Shard sh, const uint32_t* __restrict__ sel_key,
                                                           uint32_t* __restrict__ cnt_out,
                                                           unsigned long long* __restrict__ pairs,
                                                           uint32_t* __restrict__ ticket,
                                                           unsigned long long* __restrict__ key2) {
  __shared__ unsigned long long lds[4];
  __shared__ uint32_t s_last;
  // grid-stride over the hypotheses: at most 256 workgroups take a ticket (2000 same-address atomics cost ~20 us: C4)
  unsigned long long k = 0, pos = 0;
  for (uint32_t l = blockIdx.x * 256 + threadIdx.x; l < sh.n_local; l += gridDim.x * 256) {
    uint32_t c = 0;
    {  // (four rows in flight: a loop of n_chunks trips is n_chunks dependent round trips to hipcc — five at C2)
      uint32_t ch = 0;
      for (; ch + 4 <= n_chunks; ch += 4) {
        const uint32_t p0 = partial[(size_t)ch * sh.ld_local + l], p1 = partial[(size_t)(ch + 1) * sh.ld_local + l],
                       p2 = partial[(size_t)(ch + 2) * sh.ld_local + l], p3 = partial[(size_t)(ch + 3) * sh.ld_local + l];
        c += (p0 + p1) + (p2 + p3);
      }
      uint32_t pr[3];
#pragma unroll
      for (uint32_t u = 0; u < 3; u++) pr[u] = ch + u < n_chunks ? partial[(size_t)(ch + u) * sh.ld_local + l] : 0u;
      c += pr[0] + pr[1] + pr[2];
    }
    cnt_out[l] = c;
    const uint32_t g = shard_global_index(l, sh.block, sh.rank, sh.world);
    const uint32_t second = sel_key ? sel_key[g] : 0xFFFFFFFFu - g;
    if (c) {
      const unsigned long long kk = ((unsigned long long)c << 32) | (unsigned long long)second;
      const unsigned long long pp = (unsigned long long)(0xFFFFFFFFu - g);
      lexmax_take(k, pos, kk, pp);
    }
  }
  block_lexmax_u64(k, pos, lds);
  if (threadIdx.x == 0) {
    __hip_atomic_store(&pairs[2 * blockIdx.x], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&pairs[2 * blockIdx.x + 1], pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // key2 == nullptr: the pairs go to this context's own finalize_kernel, whose workgroups each reduce them themselves (r05: the
  // release, the ticket and the last workgroup's pass over the pairs were ~2.5 us of this launch's 8.6 at C2)
  if (!key2) return;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == gridDim.x - 1) ? 1u : 0u;
    if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (!s_last) return;
  unsigned long long gk = 0, gp = 0;
  for (uint32_t b = threadIdx.x; b < gridDim.x; b += 256) {
    const unsigned long long a = __hip_atomic_load(&pairs[2 * b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long q = __hip_atomic_load(&pairs[2 * b + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lexmax_take(gk, gp, a, q);
  }
  block_lexmax_u64(gk, gp, lds);  // (lds: the barrier behind the ticket lies between the two reductions)
  if (threadIdx.x == 0) {
    key2[0] = gk;
    key2[1] = (gk != 0 && sel_key) ? gp : 0ull;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
  }
}

// Tuning::score_split: share of the hypotheses (in 256ths) scored on the matrix pipe (default 0; experiments)
void launch_score(const Points& pts, const Hyps& h, const Partial& out, const Stamps& ev, const Derived& dv, int score_mode,
                  const Tuning& tn, hipStream_t st) {
  const Shard& sh = h.sh;
  if (sh.n_local == 0) return;
  uint32_t chunks;
  int chunk_pts;
  score_plan(pts.n, sh.ld_local, &chunks, &chunk_pts);
  const uint32_t groups = sh.ld_local / SCORE_THREADS;            // 256-hypothesis groups
  const uint32_t split = score_mode == 0 ? (tn.score_split <= 256 ? tn.score_split : 256u) : 0u;
  const uint32_t gm = (uint32_t)(((uint64_t)groups * split + 128) / 256);  // groups on the matrix pipe
  const uint32_t nv = groups - gm, nm = gm * (SCORE_THREADS / MF_HYPS_PER_BLOCK);
  const dim3 grid(nv + nm, chunks);
  if (score_mode == 1)
    SC_LAUNCH_EV(score_kernel<1>, grid, dim3(SCORE_THREADS), st, ev.first, ev.last, pts.planes, pts.n, pts.ld, h.soa,
                          sh.ld_local, dv.inv_tau2, chunk_pts, out.counts, nv, nm);
  else if (score_mode == 2)
    SC_LAUNCH_EV(score_kernel<2>, grid, dim3(SCORE_THREADS), st, ev.first, ev.last, pts.planes, pts.n, pts.ld, h.soa,
                          sh.ld_local, dv.inv_tau, chunk_pts, out.counts, nv, nm);
  else
    SC_LAUNCH_EV(score_kernel<0>, grid, dim3(SCORE_THREADS), st, ev.first, ev.last, pts.planes, pts.n, pts.ld, h.soa,
                          sh.ld_local, dv.tau2, chunk_pts, out.counts, nv, nm);
}

uint32_t argmax_blocks(uint32_t ld_local) { return ld_local / 256 < 256 ? ld_local / 256 : 256; }
size_t argmax_scratch_bytes(uint32_t ld_local) { return (size_t)(ld_local / 256 + 1) * 2 * sizeof(uint64_t); }

void launch_argmax(const Shard& sh, const Partial& in, const ArgmaxOut& out, hipStream_t st) {
  if (sh.n_local == 0) {  // nothing scored: the pair is (0, 0)
    (void)hipMemsetAsync(out.key2, 0, 2 * sizeof(uint64_t), st);
    return;
  }
  const uint32_t blocks = argmax_blocks(sh.ld_local);
  hipLaunchKernelGGL(score_argmax_kernel, dim3(blocks), dim3(256), 0, st, in.counts, in.rows, sh, out.sel_key, out.cnt,
                     reinterpret_cast<unsigned long long*>(out.pairs), out.ticket, reinterpret_cast<unsigned long long*>(out.key2));
}


}  // namespace sc
