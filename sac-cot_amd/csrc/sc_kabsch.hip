// sc_kabsch.hip — stage C1, the per-triangle rigid transform, and what its launch carries for C2's filters: the fp16 tile of the
// correspondences (extra workgroups), the Gram filter's coefficient rows (the Kabsch threads themselves) — with the reference-frame
// vote that both are made in, and the host-side jobs and views of those buffers.  SURVEY.md §8a row C1.  kabsch_shard_kernel calls
// filter_tile_block and gram_coef_block, and the library is built without relocatable device code: the three stay one file.
// (The Gram filter these feed, and the derivation of its bound, are sc_filter.hip's.)
#include <cstddef>

#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_score.hpp"
#include "sc_gramref.hpp"

namespace sc {

__device__ __forceinline__ void split2(double x, _Float16& hi, _Float16& lo) {
  hi = (_Float16)(float)x;
  lo = (_Float16)(float)(x - (double)(float)hi);
}

// the vote in a launch of its own (stage hook, sharded stage C, certified paths: wherever the counting pass did not carry it)
__global__ __launch_bounds__(4 * GX_VOTE) void gram_ref_kernel(GramRefJob job) {
  __shared__ float lds[GX_REF_LDS_WORDS];
  gram_ref_block(job, lds);
}

// exclusive rank of this thread among the threads of its 256-thread workgroup for which `flag` holds, and their number
// (two barriers; every thread of the workgroup must call it)
__device__ __forceinline__ uint32_t block_rank256(bool flag, uint32_t* __restrict__ s_w /* 4 words of LDS */, uint32_t* total) {
  const uint64_t b = __ballot(flag);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; w++) { const uint32_t v = s_w[w]; pre += w < wave ? v : 0u; tot += v; }
  __syncthreads();
  *total = tot;
  return pre + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// tile: per group of 32 rows 4 x 32 uint4 — for block k (0: hi halves, 1: lo halves): the 32 first halves (slots 0..7), then the 32
// second halves (slots 8..15), so that lane l reads uint4 number 64 k + l of the group (linear, conflict-free).
//   slots   0..8 Q'_i P'_j (index 3 i + j)   9 norm piece   10..12 256 P'_j   13..15 256 V'_i
//   MFMA 1: coefficient hi x block 0 (norm hi);   MFMA 2: coefficient hi x block 1 (norm lo);   MFMA 3: coefficient lo x block 0
// Row of correspondence m: NEAR ones from the front in the order their workgroups' atomics arrive, FAR ones from row n - 1 down;
// rows [n, rows) are sentinels.  pperm[row] = m.
// one read of the frame per workgroup (all threads call; one barrier)
__device__ __forceinline__ void load_frame(const GramFrame* __restrict__ fr, GramFrameRO* __restrict__ s_fr) {
  static_assert(sizeof(GramFrameRO) == 176 && offsetof(GramFrame, pmax_o) == 168, "GramFrameRO is the head of GramFrame");
  if (threadIdx.x < sizeof(GramFrameRO) / 8) reinterpret_cast<double*>(s_fr)[threadIdx.x] = reinterpret_cast<const double*>(fr)[threadIdx.x];
  __syncthreads();
}

__device__ void gram_tile_block(const float* __restrict__ planes, int n, int ld, const FilterTileJob& job, uint32_t block,
                                uint32_t blocks) {
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_base[2];
  __shared__ GramFrameRO s_fr;
  const uint32_t m = block * 256 + threadIdx.x;
  for (uint32_t z = m; z < job.zero_words; z += blocks * 256) job.zero[z] = 0u;
  GramFrame* __restrict__ fr = job.coef.frame;
  load_frame(fr, &s_fr);
  const bool real = m < (uint32_t)n;
  double P[3] = {0.0, 0.0, 0.0}, Q[3] = {0.0, 0.0, 0.0}, V[3] = {0.0, 0.0, 0.0}, vv = 0.0;
  if (real) {
    const double s = s_fr.s;
    double dq[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      P[c] = s * ((double)planes[(size_t)c * ld + m] - s_fr.c[c]);
      dq[c] = (double)planes[(size_t)(3 + c) * ld + m] - s_fr.t0[c];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
      Q[i] = s * ((s_fr.R0[i] * dq[0] + s_fr.R0[3 + i] * dq[1] + s_fr.R0[6 + i] * dq[2]) - s_fr.c[i]);  // (R0^T dq)_i
      V[i] = Q[i] - P[i];
      vv += V[i] * V[i];
    }
  }
  const bool near = real && vv <= s_fr.th_v * s_fr.th_v;
  uint32_t tot_near;
  const uint32_t r_near = block_rank256(near, s_w, &tot_near);
  // (the real correspondences of a workgroup are its first threads: rank among the FAR ones = thread - rank among the NEAR ones)
  const uint32_t n_real = (uint32_t)n > block * 256 ? min(256u, (uint32_t)n - block * 256) : 0u, tot_far = n_real - tot_near;
  const uint32_t r_far = threadIdx.x - r_near;
  if (threadIdx.x == 0) {  // ONE atomic per workgroup: both counts in one 64-bit word
    const unsigned long long was = n_real ? atomicAdd(&fr->pts, (unsigned long long)tot_near | ((unsigned long long)tot_far << 32)) : 0ull;
    s_base[0] = (uint32_t)was; s_base[1] = (uint32_t)(was >> 32);
  }
  _Float16 h[16], l[16], n2[2];  // (made while thread 0's atomic is on its way)
  if (real) {
    double F[16];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) F[3 * i + j] = Q[i] * P[j];
    const double N = 0.5 * vv;
#pragma unroll
    for (int c = 0; c < 3; c++) { F[10 + c] = 256.0 * P[c]; F[13 + c] = 256.0 * V[c]; }
    F[9] = 0.0;
#pragma unroll
    for (int k = 0; k < 16; k++) split2(F[k], h[k], l[k]);
    n2[0] = (_Float16)(float)N;
    n2[1] = (_Float16)(float)(N - (double)(float)n2[0]);  // what is left: < 2^-22 N (GX_NORM)
  } else {  // sentinel: far away under every hypothesis (D~ = 2 x 60000 + ...), never undecided
#pragma unroll
    for (int k = 0; k < 16; k++) { h[k] = (_Float16)0.f; l[k] = (_Float16)0.f; }
    n2[0] = (_Float16)60000.f; n2[1] = (_Float16)0.f;
  }
  __syncthreads();
  if (m >= job.rows) return;
  const uint32_t row = near ? s_base[0] + r_near : (real ? (uint32_t)n - 1u - (s_base[1] + r_far) : m);
  if (real) job.coef.pperm[row] = m;
  uint4* tile = static_cast<uint4*>(job.tile) + (size_t)(row >> 5) * (32 * GX_TILE_Q) + (row & 31u);
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const _Float16* v = k == 1 ? l : h;
    half8 f0 = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
    half8 f1 = {v[8], n2[k], v[10], v[11], v[12], v[13], v[14], v[15]};
    tile[64 * k] = *reinterpret_cast<uint4*>(&f0);
    tile[64 * k + 32] = *reinterpret_cast<uint4*>(&f1);
  }
}

// The fp16 image of the correspondences, 32 bytes each, in the K order of the B operand:
//   [Pxh Pxl Pxh  Pyh Pyl Pyh  Pzh Pzl | Pzh  Qxh Qxl  Qyh Qyl  Qzh Qzl  0];  rows [n, rows) are sentinels (far away).
// The two 16-byte halves of a correspondence are NOT adjacent: see the group layout at the end of filter_tile_block.
// mx_cur: max |p| and max |q| of the call (bit patterns; stage_points_kernel's atomicMax).  Also clears the filter's
// counters and bitmap for this call, so nothing needs a memset.
__device__ void filter_tile_block(const float* __restrict__ planes, int n, int ld, const FilterTileJob& job, uint32_t block,
                                  uint32_t blocks) {
  if (job.mode == 2) { gram_tile_block(planes, n, ld, job, block, blocks); return; }
  const uint32_t m = block * 256 + threadIdx.x;
  for (uint32_t z = m; z < job.zero_words; z += blocks * 256) job.zero[z] = 0u;
  const float Pmax = __uint_as_float(job.mx_cur[0]), Qmax = __uint_as_float(job.mx_cur[1]), mxv = fmaxf(Pmax, Qmax);
  const int e = (int)((__float_as_uint(mxv) >> 23) & 255u) - 127;  // mxv in [2^e, 2^(e+1))
  int k = 8 - e;
  k = k > 100 ? 100 : (k < -100 ? -100 : k);
  const float s = __uint_as_float((uint32_t)(k + 127) << 23);
  if (m == 0) *static_cast<FilterInfo*>(job.info) = FilterInfo{s, Pmax, Qmax, 0.f};
  if (m >= job.rows) return;
  _Float16 hi[6], lo[6];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const float X = m < (uint32_t)n ? planes[(size_t)c * ld + m] * s : (c < 3 ? 0.f : 32768.f);
    hi[c] = (_Float16)X;
    lo[c] = (_Float16)(X - (float)hi[c]);
  }
  half8 f0 = {hi[0], lo[0], hi[0], hi[1], lo[1], hi[1], hi[2], lo[2]};
  half8 f1 = {hi[2], hi[3], lo[3], hi[4], lo[4], hi[5], lo[5], (_Float16)0.f};
  // per group of 32 correspondences (one MFMA step): the 32 first halves (k0..7), then the 32 second halves (k8..15) —
  // lane l of a wave then reads the 16 bytes at 16 l of the group's 1 KiB: a linear, bank-conflict-free ds_read_b128
  // (with the two halves of a correspondence side by side the lanes of a half stride 32 bytes: 2-way conflicts, +4
  // cycles on each 8-cycle read by SQ_LDS_BANK_CONFLICT)
  uint4* tile = static_cast<uint4*>(job.tile);
  const size_t slot = (size_t)(m >> 5) * 64 + (m & 31u);
  tile[slot] = *reinterpret_cast<uint4*>(&f0);
  tile[slot + 32] = *reinterpret_cast<uint4*>(&f1);
}
__global__ __launch_bounds__(256) void filter_tile_kernel(const float* __restrict__ planes, int n, int ld, FilterTileJob job) {
  filter_tile_block(planes, n, ld, job, blockIdx.x, gridDim.x);
}

// Per-hypothesis coefficients of the Gram filter, made ONCE per call (by the Kabsch launch's own threads, or by
// gram_coef_kernel for the stage hook): thread = hypothesis l of this rank's shard, a whole 256-thread workgroup calls it.
// The row a hypothesis gets: NEAR ones from the front, everything else from row ldl - 1 down (one atomic per workgroup and
// class); hperm[row] = l.
//   coef.A      64 bytes per row: [hi halves of the 16 coefficients | lo halves] (NOT yet scaled by the row's alpha)
//   coef.C      RS (|tau'|^2 - LO_h), or +huge for a row that is switched off
//   coef.W      RS (HI_h - LO_h), 0 for a row that is not filtered
//   coef.flag   bit 0 normal (filtered), bit 1 recount (its group of 8 rows goes to the exact pass), bits 8.. log2 of the largest
//               alpha the row's coefficients can take without leaving fp16's range
__device__ void gram_coef_block(const GramCoef& coef, const float v[12], uint32_t l, uint32_t ldl, uint32_t n_local, float tau2) {
  __shared__ uint32_t s_w[4];
  __shared__ uint32_t s_base[2];
  __shared__ GramFrameRO s_fr;
  GramFrame* __restrict__ fr = coef.frame;
  load_frame(fr, &s_fr);
  const double s = s_fr.s, st = s_fr.st, Pn = s_fr.Pn, Qn = s_fr.Qn, Vn = Pn + Qn;
  double R[9], dM[9], G[9], Tp[3];
#pragma unroll
  for (int c = 0; c < 9; c++) R[c] = (double)v[c];
  double F2 = 0.0, mm = 0.0, gdef = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      // (fp64 products of this block are fused by hand: the build runs -ffp-contract=off for the canonical fp32 chains, and an
      // unfused a b + c is two half-rate instructions here — C4's 500 000 hypotheses make this launch 12 % of its step)
      const double Mij = __builtin_fma(s_fr.R0[i], R[j], __builtin_fma(s_fr.R0[3 + i], R[3 + j], s_fr.R0[6 + i] * R[6 + j]));  // (R0^T R)_ij
      const double d = Mij - (i == j ? 1.0 : 0.0);
      dM[3 * i + j] = d;
      F2 = __builtin_fma(d, d, F2);
      mm = fmax(mm, fabs(d));
    }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = i; j < 3; j++) {  // (R^T R - I)_ij, symmetric
      const double g = __builtin_fma(R[i], R[j], __builtin_fma(R[3 + i], R[3 + j], __builtin_fma(R[6 + i], R[6 + j], i == j ? -1.0 : 0.0)));
      G[3 * i + j] = g; G[3 * j + i] = g;
      gdef = fmax(gdef, fabs(g));
    }
  {
    const double d0 = (double)v[9] - s_fr.t0[0], d1 = (double)v[10] - s_fr.t0[1], d2 = (double)v[11] - s_fr.t0[2];
#pragma unroll
    for (int i = 0; i < 3; i++)
      Tp[i] = s * __builtin_fma(s_fr.R0[i], d0, __builtin_fma(s_fr.R0[3 + i], d1, __builtin_fma(s_fr.R0[6 + i], d2,
                   __builtin_fma(dM[3 * i], s_fr.c[0], __builtin_fma(dM[3 * i + 1], s_fr.c[1], dM[3 * i + 2] * s_fr.c[2])))));
  }
  float nanp = 0.f;
#pragma unroll
  for (int c = 0; c < 12; c++) nanp += v[c] * 0.f;
  // |dM|_F and |tau'|: fp32 square roots, pushed up / down by more than their rounding — every bound below is monotone in them
  const double T2 = __builtin_fma(Tp[0], Tp[0], __builtin_fma(Tp[1], Tp[1], Tp[2] * Tp[2]));
  const double Fn = (double)sqrt_rn((float)F2) * (1.0 + 4e-7) + 1e-30, Tr = (double)sqrt_rn((float)T2);
  const double Tn = Tr * (1.0 + 4e-7) + 1e-30, Tn_lo = Tr * (1.0 - 4e-7);
  const double tmax_o = fmax(fabs((double)v[9]), fmax(fabs((double)v[10]), fabs((double)v[11])));
  const double dE = GX_CANON * s * ((double)s_fr.qmax_o + 1.75 * (double)s_fr.pmax_o + tmax_o);
  const bool finite = nanp == 0.f;
  const bool pad = l >= n_local;
  const bool rot = finite && gdef <= 1e-3 && T2 < 1e12;
  const bool far = rot && (Tn_lo - Fn * Pn - Vn >= 1.05 * st + dE + 1e-3);
  // The hypothesis' own cut: a correspondence with |V'| > vb_h = reach_h + 1.05 st + dE_h is an outlier of h (triangle inequality),
  // so the shell only has to hold for |V'| <= vb_h — PROVIDED the filter cannot call such a correspondence an inlier either: with
  // U(v) the sum form of the bound, D~ >= (v - reach_h)^2 - U(v), which grows with v from vb_h on (its slope there is
  // 2.1 st - U' > 0 for st >= 0.2), so U(vb_h) <= 0.1 st^2 < (1.05^2 - 1) st^2 keeps D~ above st^2 >= LO_h.  Otherwise the shell is made
  // for every correspondence of the call (vb = Vn).
  const double reach = Fn * Pn + Tn;
  double vb = reach + 1.05 * st + dE + 1e-3, Qb = fmin(Qn, Pn + vb);
  const bool own = rot && vb < Vn && st >= 0.2 && gram_eps_sum(Fn, mm, Tn, gdef, Pn, Qb, vb, st) <= 0.1 * st * st;
  if (!own) { vb = Vn; Qb = Qn; }
  const double eps = gram_eps(Fn, mm, Tn, gdef, Pn, Qb, vb, st);
  // NEAR the reference: its workgroup of the filter looks only at the NEAR correspondences (|V'| <= th_v = th_h + 1.05 st + 1e-3)
  const bool close = own && !far && !pad && (reach + dE <= s_fr.th_h);
  // coefficients (A operand), scaled by GX_RS; the P' / V' features are stored x 256
  double a16[16], cmax = 0.0;
#pragma unroll
  for (int k = 0; k < 9; k++) a16[k] = (double)GX_RS * __builtin_fma(-2.0, dM[k], G[k]);
  a16[9] = 2.0 * (double)GX_RS;
#pragma unroll
  for (int j = 0; j < 3; j++) a16[10 + j] = 2.0 * (double)GX_RS / 256.0 * __builtin_fma(dM[j], Tp[0], __builtin_fma(dM[3 + j], Tp[1], dM[6 + j] * Tp[2]));
#pragma unroll
  for (int i = 0; i < 3; i++) a16[13 + i] = -2.0 * (double)GX_RS / 256.0 * Tp[i];
#pragma unroll
  for (int k = 0; k < 16; k++) cmax = fmax(cmax, fabs(a16[k]));
  uint32_t lg = 4;  // alpha <= 16
  while (lg > 0 && cmax * (double)(1u << lg) > 30000.0) lg--;
  // (st <= 32: the sentinel correspondences' 2 x 60000 must stay far above every threshold)
  const bool normal = rot && !far && !pad && (eps <= 0.25 * st * st) && (dE <= 0.1 * st) && (st <= 32.0) && (cmax <= 30000.0);
  const bool recount = !pad && !far && !normal;
  const bool good = close && normal;
  const double LOh = (st - dE) * (st - dE) * (1.0 - 1e-5) - eps, HIh = (st + dE) * (st + dE) * (1.0 + 1e-5) + eps;
  uint32_t n_good;
  const uint32_t r_good = block_rank256(good, s_w, &n_good), r_bad = threadIdx.x - r_good, n_bad = 256u - n_good;
  // this workgroup's segment of the coefficient rows (sc_gramref.hpp): NEAR hypotheses from its front, the others from its back
  const uint32_t groups = ldl / 256u, S = gram_segments(groups), wg = l / 256u, sg = wg % S, seg_rows = 256u * ((groups - sg + S - 1u) / S);
  if (threadIdx.x == 0) {  // ONE atomic per workgroup: both counts in one 64-bit word
    const unsigned long long was = atomicAdd(&fr->seg[sg].cnt, (unsigned long long)n_good | ((unsigned long long)n_bad << 32));
    s_base[0] = (uint32_t)was; s_base[1] = (uint32_t)(was >> 32);
  }
  // (the fp16 halves are made while thread 0's atomic is on its way: ~1.5 us of latency every workgroup used to sit out)
  _Float16 ah[16], al[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    split2(a16[k], ah[k], al[k]);
    if (!normal) { ah[k] = (_Float16)0.f; al[k] = (_Float16)0.f; }
  }
  al[9] = (_Float16)0.f;  // (2 RS is a power of two: no low half)
  const float c_row = normal ? (float)((double)GX_RS * (T2 - LOh)) : 1e30f;
  const float w_row = normal ? (float)((double)GX_RS * (HIh - LOh) * (1.0 + 1e-6)) : 0.0f;
  __syncthreads();
  if (l >= ldl) return;
  const uint32_t row = gram_seg_row(good ? s_base[0] + r_good : seg_rows - 1u - (s_base[1] + r_bad), sg, S);
  coef.hperm[row] = l;
  coef.C[row] = c_row;
  coef.W[row] = w_row;
  coef.flag[row] = (normal ? 1u : 0u) | (recount ? 2u : 0u) | (lg << 8);
  uint4* __restrict__ out = reinterpret_cast<uint4*>(coef.A) + (size_t)row * 4;
  half8 q0 = {ah[0], ah[1], ah[2], ah[3], ah[4], ah[5], ah[6], ah[7]}, q1 = {ah[8], ah[9], ah[10], ah[11], ah[12], ah[13], ah[14], ah[15]};
  half8 q2 = {al[0], al[1], al[2], al[3], al[4], al[5], al[6], al[7]}, q3 = {al[8], al[9], al[10], al[11], al[12], al[13], al[14], al[15]};
  out[0] = *reinterpret_cast<uint4*>(&q0); out[1] = *reinterpret_cast<uint4*>(&q1);
  out[2] = *reinterpret_cast<uint4*>(&q2); out[3] = *reinterpret_cast<uint4*>(&q3);
}

__global__ __launch_bounds__(256) void gram_coef_kernel(const float* __restrict__ RtSoA, uint32_t ldl, uint32_t n_local, float tau2,
                                                        GramCoef coef) {
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;
  float v[12];
#pragma unroll
  for (int c = 0; c < 12; c++) v[c] = l < ldl ? RtSoA[(size_t)c * ldl + l] : 0.f;
  gram_coef_block(coef, v, l, ldl, n_local, tau2);
}

// ------------------------------------------------------------------------------------------------
// C1
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kabsch_shard_kernel(const float* __restrict__ planes, int n, int ld, TriSource ts,
                                                           Shard sh, float* __restrict__ RtSoA,
                                                           float* __restrict__ RtAoS, FilterTileJob job,
                                                           uint32_t kabsch_blocks,
                                                           const uint64_t* __restrict__ t_eff_dev) {
  if (blockIdx.x >= kabsch_blocks) {  // the extra workgroups: C2's fp16 tile of the correspondences (see filter_tile_block)
    filter_tile_block(planes, n, ld, job, blockIdx.x - kabsch_blocks, gridDim.x - kabsch_blocks);
    return;
  }
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;  // < ld_local: a multiple of 256, kabsch_blocks = ld_local / 256
  float Rt[12];
  // t_eff_dev: the launch was sized for sh.T_eff = the requested T before the host knew how many triangles there are; a
  // position beyond the real selection holds nothing that may be dereferenced (the host repeats such a call: sc_capi.hip)
  const uint32_t g = l < sh.n_local ? shard_global_index(l, sh.block, sh.rank, sh.world) : 0u;
  uint32_t v[3];
  if (l < sh.n_local && (!t_eff_dev || (uint64_t)g < *t_eff_dev) && tri_lookup(ts, g, v)) {
    float P[9], Q[9];
    load_triangle(planes, ld, v, P, Q);
    kabsch3(P, Q, Rt);
  } else {
#pragma unroll
    for (int c = 0; c < 12; c++) Rt[c] = 0.0f;
  }
#pragma unroll
  for (int c = 0; c < 12; c++) RtSoA[(size_t)c * sh.ld_local + l] = Rt[c];
  if (RtAoS) {  // 12 consecutive floats per hypothesis: what the lane = correspondence scoring kernel loads as scalars
    float4* o = reinterpret_cast<float4*>(RtAoS + 12 * (size_t)l);
    o[0] = make_float4(Rt[0], Rt[1], Rt[2], Rt[3]);
    o[1] = make_float4(Rt[4], Rt[5], Rt[6], Rt[7]);
    o[2] = make_float4(Rt[8], Rt[9], Rt[10], Rt[11]);
  }
  // the Gram filter's coefficients of this hypothesis (whole workgroups get here: ld_local is a multiple of 256)
  if (job.mode == 2) gram_coef_block(job.coef, Rt, l, sh.ld_local, sh.n_local, job.tau2);
}

void launch_kabsch(const Points& pts, const TriSource& ts, const Hyps& h, const FilterTileJob* tile_job, hipStream_t st) {
  if (h.sh.ld_local == 0) return;
  const uint32_t kb = h.sh.ld_local / 256, tb = tile_job ? (tile_job->rows + 255) / 256 : 0u;
  hipLaunchKernelGGL(kabsch_shard_kernel, dim3(kb + tb), dim3(256), 0, st, pts.planes, pts.n, pts.ld, ts, h.sh, h.soa, h.aos,
                     tile_job ? *tile_job : FilterTileJob{}, kb, h.t_eff_dev);
}

__global__ __launch_bounds__(256) void kabsch_aos_kernel(const float* __restrict__ planes, int ld,
                                                         const uint32_t* __restrict__ tri, uint32_t T,
                                                         float* __restrict__ Rt_out) {
  const uint32_t h = blockIdx.x * 256 + threadIdx.x;
  if (h >= T) return;
  float P[9], Q[9], Rt[12];
  load_triangle(planes, ld, tri + 3 * (size_t)h, P, Q);
  kabsch3(P, Q, Rt);
#pragma unroll
  for (int c = 0; c < 12; c++) Rt_out[12 * (size_t)h + c] = Rt[c];
}

void launch_kabsch_aos(const Points& pts, const uint32_t* tri, uint32_t T, float* Rt, hipStream_t st) {
  if (T == 0) return;
  hipLaunchKernelGGL(kabsch_aos_kernel, dim3((T + 255) / 256), dim3(256), 0, st, pts.planes, pts.ld, tri, T, Rt);
}

__global__ __launch_bounds__(256) void rt_to_soa_kernel(const float* __restrict__ Rt, uint32_t T, uint32_t ld_local,
                                                        float* __restrict__ RtSoA) {
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;
  if (l >= ld_local) return;
#pragma unroll
  for (int c = 0; c < 12; c++) RtSoA[(size_t)c * ld_local + l] = (l < T) ? Rt[12 * (size_t)l + c] : 0.0f;
}

void launch_rt_to_soa(const float* Rt, uint32_t T, uint32_t ld_local, float* RtSoA, hipStream_t st) {
  if (ld_local == 0) return;
  hipLaunchKernelGGL(rt_to_soa_kernel, dim3(ld_local / 256), dim3(256), 0, st, Rt, T, ld_local, RtSoA);
}

GramCoef gram_coef_view(void* buf, uint32_t ld_local, void* frame) {
  GramCoef g;
  unsigned char* p = static_cast<unsigned char*>(buf);
  g.A = p; p += (size_t)ld_local * 64;
  g.C = reinterpret_cast<float*>(p); p += (size_t)ld_local * 4;
  g.W = reinterpret_cast<float*>(p); p += (size_t)ld_local * 4;
  g.flag = reinterpret_cast<uint32_t*>(p); p += (size_t)ld_local * 4;
  g.hperm = reinterpret_cast<uint32_t*>(p); p += (size_t)ld_local * 4;
  g.pperm = reinterpret_cast<uint32_t*>(p);
  g.frame = static_cast<GramFrame*>(frame);
  return g;
}

FilterTileJob filter_tile_job(const FilterBufs& fb, uint32_t ld_local, float tau2) {
  const FilterPlan& fp = fb.plan;
  const FilterState f = filter_state(fb.state, fp);
  FilterTileJob j{fp.rows, fb.mx, nullptr, fb.tile, f.info, f.qcount, f.zero_words, fp.mode,
                  GramCoef{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, tau2};
  if (fp.mode == 2) j.coef = gram_coef_view(fb.coef, ld_local, fb.frame);
  return j;
}

size_t gram_frame_bytes() { return sizeof(GramFrame); }  // (the class counters sit on 128-byte lines of their own)

GramRefJob gram_ref_job(const Points& pts, const FilterBufs& fb, float tau2, const Tuning& tn) {
  GramRefJob j{};
  j.planes = pts.planes; j.n = pts.n; j.ld = pts.ld;
  j.mx = fb.mx; j.tau2 = tau2;
  j.kappa = tn.gram_kappa_q4 ? (float)tn.gram_kappa_q4 / 16.0f : (float)GX_KAPPA;
  j.out = static_cast<GramFrame*>(fb.frame);
  return j;
}

// the frame of this call's Gram filter in a launch of its own: before the tile / the coefficients are made (it also clears their
// counters).  ts == nullptr: the hypotheses exist already (stage hook), in h.soa; else they are solved from the selection `*ts`.
void launch_gram_ref(const Points& pts, const TriSource* ts, const Hyps& h, const FilterBufs& fb, float tau2, const Tuning& tn, hipStream_t st) {
  if (h.sh.n_local == 0) return;
  GramRefJob j = gram_ref_job(pts, fb, tau2, tn);
  j.src.RtSoA = ts ? nullptr : h.soa; j.src.ts = ts ? *ts : TriSource{}; j.src.sh = h.sh; j.src.t_eff_dev = h.t_eff_dev;
  hipLaunchKernelGGL(gram_ref_kernel, dim3(1), dim3(4 * GX_VOTE), 0, st, j);
}

void launch_gram_coef(const Hyps& h, float tau2, const GramCoef& coef, hipStream_t st) {
  if (h.sh.ld_local == 0) return;
  hipLaunchKernelGGL(gram_coef_kernel, dim3(h.sh.ld_local / 256), dim3(256), 0, st, h.soa, h.sh.ld_local, h.sh.n_local, tau2, coef);
}

void launch_filter_tile(const Points& pts, const FilterTileJob& job, hipStream_t st) {
  hipLaunchKernelGGL(filter_tile_kernel, dim3((job.rows + 255) / 256), dim3(256), 0, st, pts.planes, pts.n, pts.ld, job);
}

}  // namespace sc
