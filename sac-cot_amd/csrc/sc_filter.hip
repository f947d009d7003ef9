// sc_filter.hip — stage C2's inlier count by matrix-pipe filter + exact fix-up: which calls take which filter and with what plan,
// the linear filter, the exact pass, the Gram filter (with the derivation of its bound) and their launcher.  SURVEY.md §8a row C2.
// The tile, the coefficients and the reference frame these kernels read are made in the Kabsch launch (sc_kabsch.hip); the plain
// fp32 kernel and the arg-max are sc_score.hip's.
#include <cstddef>
#include <vector>

#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_score.hpp"
#include "sc_gramref.hpp"

namespace sc {

// ------------------------------------------------------------------------------------------------
// C2, inlier count, the default since r02: a matrix-pipe FILTER decides almost every test, an EXACT pass settles the rest.
//
// The count of hypothesis h is  #{m : d2(h, m) < tau^2}  with d2 the canonical fp32 chain (resid2, above).  Two kernels:
//
//   F  score_filter_kernel   evaluates  E' = 1024 s (R p + t - q)  for 8 hypotheses x 32 correspondences per
//      v_mfma_f32_32x32x16_f16: rows = (hypothesis, component) — three per hypothesis, the fourth idle — columns =
//      correspondences, K = 16 slots:
//          k0..8   (rh, rh, rl) x (Ph, Pl, Ph) for x, y, z     r = 1024 R and P = s p, each split in two fp16 halves
//          k9..14  -1024 x (Qh, Ql) of the row's own component  Q = s q
//          C       1024 s t (fp32)
//      (s: the power of two that puts the largest |coordinate| of the call into [256, 512).)  A lane then holds the three
//      components of ONE test; x = |E'|^2 - LO costs three fmas, its sign bit is shifted into a register (v_alignbit) and
//      counted once per 32 tests.  4.6 vector instructions per test instead of 17.
//      What F computes is NOT the canonical chain, so it only decides tests that are clear:
//          |E'| < 1024 (s tau - eta)  inlier        |E'| >= 1024 (s tau + eta)  outlier         else  UNDECIDED
//      eta bounds the distance between the two evaluations (below).  Undecided tests (about 1 in 10^4) go to a queue.
//   X  score_exact_kernel    evaluates the queued tests with the canonical chain and adds them to the counts (integer
//      atomics: order-free).  It also recounts, exactly, every (wave, split) F gave up on: a hypothesis outside the
//      filter's range (non-finite, |R_ij| > 1.5, huge t), tau too small or too large against the coordinate scale, a
//      queue that overflowed.  F never guesses; whatever it cannot bound it hands over.
//
// eta.  With |P|, |Q| <= Pmax, Qmax < 512, |t| s <= Tmax and sum_k |R_ck| <= 4.5, per component and in units of E'/1024:
//   fp16 splits   x = hi + lo + rem, |rem| <= 2^-22 |x| (or 2^-25 absolute below the fp16 normal range; inputs flushed
//                 to zero there would add < 1e-4): dropped rl Pl plus the two remainders <= 3.01 * 2^-22 sum|R| Pmax,
//                 and 2^-22 Qmax for q; the products themselves (11 x 11 bits) and C are exact in fp32;
//   accumulation  <= 17 additions, each off by <= 2^-23 of S = sum|R| Pmax + Qmax + Tmax (truncation allowed for);
//   the canonical chain itself: 4 roundings, <= 4 * 2^-24 S.
//   Sum <= 12.5 * 2^-22 S per component, sqrt(3) of it for the vector: < 2^-17.5 S.   eta = 2^-16 (2.6 Pmax + Qmax +
//   Tmax) >= 2^-16 S / 1.73 leaves a factor 1.7; LO and HI carry another 4e-6 for the roundings of the squares, of
//   sqrt(tau^2) and of d2 itself.  The parity suite compares every count with the canonical kernel's.
// ------------------------------------------------------------------------------------------------
// Which kernel.  The filters pay a tile kernel, an exact pass and a few microseconds of set-up per workgroup: below ~1.3e8
// tests the plain kernel is as fast or faster (C1, 2e7 tests: 9 us plain, 20 us filtered).  Big calls take the Gram filter
// wherever even a hypothesis FAR from the call's reference frame keeps its shell inside tau'^2 (all four BASELINE scenes since
// r04b; until then tau had to be > ~2 % of the clouds' extent, which left C3 to the linear filter), else the linear one.
int score_filter_mode(int score_mode, const Tuning& tn, int n, uint32_t ld_local, uint64_t host_max, const uint64_t* host_box,
                      float tau2) {
  if (score_mode != 0 || tn.score_filter == 1 || tn.score_split != 0) return 0;
  if (ld_local == 0 || ld_local / 8 >= (1u << 27)) return 0;
  // beyond 2^36 tests the queue of undecided tests (sized T n / 512 entries: ~20x what the BASELINE scenes need) would
  // pass 1 GB: such calls keep the plain kernel rather than a queue that may overflow into wholesale recounts
  const uint64_t tests = (uint64_t)ld_local * (uint64_t)n;
  if (tests > (1ull << 36)) return 0;
  const bool big = tests >= (1ull << 27);
  if (tn.score_filter == 2) return 1;
  const bool gram_fits = ld_local <= (1u << 20) && n <= (1 << 24);  // (the queue entry carries wave << 17)
  if (tn.score_filter == 3) return gram_fits ? 2 : 1;
  if (!big) return 0;
  if (host_max == ~0ull) return 1;  // statistics not known: the linear filter sorts itself out (it recounts what it cannot bound)
  if (gram_fits && host_box) {
    // Gram: even a hypothesis FAR from the call's reference frame (dM of size 1, tau' a quarter of the clouds, every
    // correspondence looked at) must keep its shell well inside tau'^2 — the NEAR ones are two orders of magnitude better off.
    // The frame itself is voted on the device later; here it is taken to map one box's centre onto the other's.
    double hP2 = 0.0, hQ2 = 0.0, hmax = 0.0;
    for (int c = 0; c < 6; c++) {
      const float mx = float_unkey((uint32_t)host_box[c]), mn = -float_unkey((uint32_t)(host_box[c] >> 32));
      const float ctr = 0.5f * mx + 0.5f * mn;
      const double a = (double)mx - (double)ctr, b = (double)ctr - (double)mn, h = a > b ? a : b;
      (c < 3 ? hP2 : hQ2) += h * h;
      if (c < 3 && h > hmax) hmax = h;
    }
    const double hQn = sqrt(hQ2);
    hmax = hQn > hmax ? hQn : hmax;
    union { uint32_t u; float f; } pa, qa;
    pa.u = (uint32_t)host_max; qa.u = (uint32_t)(host_max >> 32);
    if (hmax > 0.0 && hmax < 1e30) {
      int e = 0;
      (void)frexp(hmax, &e);  // hmax in [2^(e-1), 2^e)
      const double s = ldexp(1.0, 6 - e), Pn = s * sqrt(hP2), Qn = s * hQn, st = s * sqrt((double)tau2);
      const double eps = gram_eps(2.0, 1.0, 0.25 * (Pn + Qn), 3e-7, Pn, Qn, Pn + Qn, st);
      const double dE = GX_CANON * s * ((double)qa.f + 1.75 * (double)pa.f + (double)qa.f);
      if (eps <= 0.2 * st * st && dE <= 0.02 * st && st <= 32.0 && st >= 0.2) return 2;
    }
  }
  return filter_in_range(host_max, tau2) ? 1 : 0;
}

bool filter_in_range(uint64_t host_max, float tau2) {
  if (host_max == ~0ull) return true;
  union { uint32_t u; float f; } a, b, m;
  a.u = (uint32_t)host_max; b.u = (uint32_t)(host_max >> 32);
  const float pmax = a.f, qmax = b.f;
  m.f = pmax > qmax ? pmax : qmax;
  const uint32_t mb = m.u;
  int k = 8 - ((int)((mb >> 23) & 255u) - 127);
  k = k > 100 ? 100 : (k < -100 ? -100 : k);
  const float s = ldexpf(1.0f, k), st = s * sqrtf(tau2);
  const float eta = (2.6f * (pmax * s) + qmax * s) * (1.0f / 65536.0f);  // a wave adds its own |t| s to this
  return (eta <= 0.25f * st) && (st <= 4096.f) && (pmax * s < 512.f) && (qmax * s < 512.f);  // false on NaN
}

FilterPlan filter_plan(int n, uint32_t ld_local, const Tuning& tn, uint32_t mode) {
  FilterPlan fp;
  fp.mode = mode;
  fp.windows = (uint32_t)((n + FX_WIN - 1) / FX_WIN);
  fp.n_waves = ld_local / 8;  // recount units: 8 hypotheses (a wave of the linear filter, a quarter of a Gram wave)
  // grid.y: the windows are split so that the launch has several generations of workgroups and the last one is well filled
  // (linear: 32 hypotheses per workgroup, 6 resident per CU; Gram: 256 hypotheses, 2 resident)
  const uint32_t groups = mode == 2 ? (ld_local + 32 * GX_WAVES - 1) / (32 * GX_WAVES) : ld_local / (8 * FX_WAVES);
  const uint32_t slots = mode == 2 ? 256 * 2 : 256 * 6;
  uint32_t best = 1; double best_eff = 0.0;
  const uint32_t smax = fp.windows < 8 ? fp.windows : 8;
  for (uint32_t sp = 1; sp <= smax; sp++) {
    const uint32_t per = (fp.windows + sp - 1) / sp, used = (fp.windows + per - 1) / per;  // splits that get windows
    if (used != sp) continue;
    const double blocks = (double)groups * sp, gens = (double)((uint64_t)(blocks + slots - 1) / slots);
    // every workgroup pays its set-up once: ~6 % per extra split (C2: 71 / 61 / 61 / 66 us at 1 / 2 / 3 / 5 splits,
    // C4: 476 / 492 / 514 / 555)
    const double eff = blocks / (gens * slots) * (1.0 - 0.06 * (sp - 1));
    if (eff > best_eff + 1e-9) { best_eff = eff; best = sp; }
  }
  fp.splits = tn.filter_splits && tn.filter_splits <= fp.windows ? tn.filter_splits : best;
  {  // a forced value must still give every split at least one window
    const uint32_t per = (fp.windows + fp.splits - 1) / fp.splits;
    fp.splits = (fp.windows + per - 1) / per;
  }
  if (mode == 2) {
    // The Gram filter cuts in UNITS (gram_geom), and only its rows FAR from the call's frame — a tenth of them on the BASELINE
    // scenes — walk every unit.  Their workgroups must not outlast everything else (C3 at 3 splits of 27 units: 113 of the
    // kernel's 120 us were those workgroups' own length), but every split is another workgroup per group of rows with its own
    // set-up (C4: 112 / 127 / 138 / 150 us at 1 / 3 / 5 / 8 splits).  So: the fewest splits that keep a far workgroup's walk —
    // ~4.2 us per unit — under half of what the whole launch should take if 15 % of the rows are far and a fifth of the
    // correspondences near (0.32 units' worth per group and unit, over 512 resident workgroups), and never below 4 units.
    // C2 5 splits (4 units), C3 4 (20), C4 1 (20).  (Empty workgroups cost nothing: tools/ubench/dispatch_rate.hip, 0.25 ns apiece.)
    const uint32_t units = fp.windows * (uint32_t)(FX_WIN / GX_UNIT);
    // r04c: + 2.5 units' worth of set-up per workgroup in the launch's length, and 0.6 of it instead of half — C4 (1954 row blocks of
    // 20 units) is a launch of ~34 units, most of it the near workgroups' fixed cost; its far workgroups' 20 units fit in it whole:
    // 1 split 98 us, 2 splits 108, 3 108, 4 112, 8 131 (C3: 1 167, 3 149, 4 133, 5 131, 8 130 — it takes 4 now; C2 unchanged: 5)
    const double launch_units = 0.6 * (double)groups * (2.5 + 0.32 * (double)units) / 512.0;  // 0.6 of the launch, in units of one workgroup's walk
    const uint32_t walk = launch_units < 4.0 ? 4u : (uint32_t)launch_units;
    uint32_t sp = tn.filter_splits ? tn.filter_splits : (units + walk - 1) / walk;
    sp = sp < 1u ? 1u : (sp > 8u ? 8u : sp);
    if (sp > units) sp = units;
    const uint32_t pu = (units + sp - 1) / sp;
    fp.splits = (units + pu - 1) / pu;  // every split gets at least one unit
  }
  fp.rows = fp.windows * FX_WIN + (mode == 2 ? GX_UNIT : FX_UNIT);
  uint64_t cap = (uint64_t)ld_local * (uint64_t)n / 512;  // ~20x what the BASELINE scenes queue
  if (cap < (1u << 16)) cap = 1u << 16;
  if (cap > (1u << 27)) cap = 1u << 27;
  if (tn.filter_queue_cap) cap = tn.filter_queue_cap;
  fp.queue_cap = (uint32_t)(cap / FX_NQ * FX_NQ);
  if (fp.queue_cap < FX_NQ) fp.queue_cap = FX_NQ;
  fp.tile_bytes = (size_t)fp.rows * (mode == 2 ? GX_TILE_B : 32);
  const size_t bm_words = ((size_t)fp.splits * fp.n_waves + 31) / 32;
  fp.state_bytes = FX_INFO_BYTES + (size_t)FX_NQ * 128 + (bm_words * 4 + 127) / 128 * 128 + (size_t)fp.queue_cap * 8;
  // Gram: per coefficient row 64 bytes of fp16 halves + C, W, flag, hperm; per tile row pperm
  fp.coef_bytes = mode == 2 ? (size_t)ld_local * (64 + 16) + (size_t)fp.rows * 4 : 0;
  return fp;
}

// F.  Workgroup = FX_WAVES waves; wave w of workgroup b owns hypotheses 8 (FX_WAVES b + w) .. + 7 and never talks to
// the others except through the B tile: a unit of 256 correspondences (8 KiB) is brought into LDS by LDS-DMA while
// the previous one is being used (two buffers, one barrier per unit).  blockIdx.y = split of the windows.
// 80 VGPRs: six waves per SIMD cover the MFMA and LDS latencies, so nothing is double-buffered inside a wave.
// VAR (Tuning::filter_variant): 0 = one MFMA, then its epilogue (the wave idles through the MFMA's latency; the other
// waves of the SIMD fill it); bit 0 = the NEXT step's MFMA is issued before this step's epilogue (two accumulator sets,
// 96 VGPRs, 5 waves per SIMD): vector and matrix work of ONE wave overlap; bit 1 = s_setprio 1 around the MFMA issue;
// 16 / 32: timing-only ablations (no MFMA / no epilogue: wrong counts) for tools/ab_stage.py.
template <int WAVES, int VAR>
__global__ __launch_bounds__(64 * WAVES, (VAR & 128) ? 8 : ((VAR & 1) ? 5 : 6)) void score_filter_kernel(const float* __restrict__ Rt, uint32_t ldl, float tau2,
                                                                     const uint4* __restrict__ tile,
                                                                     const FilterInfo* __restrict__ info, uint32_t windows,
                                                                     uint32_t splits, uint32_t n_waves,
                                                                     uint32_t* __restrict__ cnt_out, uint2* __restrict__ gq,
                                                                     uint32_t cap_sq, uint32_t* __restrict__ qcount,
                                                                     uint32_t* __restrict__ redo_bits, uint32_t ql) {
  __shared__ uint4 Bt[2][FX_UNIT * 2];
  __shared__ float4 Ttab[WAVES][8];
  constexpr int QL = (VAR & 128) ? FX_QL / 2 : FX_QL;  // (128: 8 workgroups per CU — their LDS must fit 160 KiB)
  __shared__ uint32_t queue[WAVES][QL];
  if (ql > (uint32_t)QL) ql = QL;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, hf = lane >> 5;
  const uint32_t per = (windows + splits - 1) / splits, w0 = blockIdx.y * per, w1 = min(windows, w0 + per);
  const uint32_t wid = blockIdx.x * WAVES + wave, h0 = wid * 8;
  const uint32_t u0 = w0 * (FX_WIN / FX_UNIT), u1 = w1 * (FX_WIN / FX_UNIT);  // staging units of this workgroup
  // The DMA is issued through asm so that hipcc does not count it: with the builtin the compiler waits vmcnt(0) before
  // the NEXT ds_read (it cannot tell the two buffers apart), which exposes the whole DMA latency in every unit.  Our own
  // wait sits before the barrier that publishes the buffer.  (Uncounted loads only make the compiler's own vmcnt(N)
  // waits stronger: the counter retires in order.)
  auto stage = [&](uint32_t u, int buf) {
#pragma unroll
    for (int i = 0; i < 8 / WAVES; i++) {
      const uint4* gsrc = tile + (size_t)u * (FX_UNIT * 2) + 64 * WAVES * i + tid;
      const uint32_t lds_dst = __builtin_amdgcn_readfirstlane(
          (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(&Bt[buf][64 * WAVES * i + wave * 64]));
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
    }
  };
  if (u0 < u1) stage(u0, 0);
  const FilterInfo fi = *info;
  // A fragment: row r = (hypothesis r >> 2, component r & 3); lane half 0 holds k0..7, half 1 k8..15
  half8 A;
  {
    const int r = lane & 31, hy = r >> 2, c = r & 3;
    float x[3];
#pragma unroll
    for (int kk = 0; kk < 3; kk++) x[kk] = Rt[(size_t)(3 * (c < 3 ? c : 0) + kk) * ldl + h0 + hy];  // unconditional: one round trip
    _Float16 rh[3], rl[3];
#pragma unroll
    for (int kk = 0; kk < 3; kk++) {
      const float v = c < 3 ? x[kk] * FX_RS : 0.f;
      rh[kk] = (_Float16)v;
      rl[kk] = (_Float16)(v - (float)rh[kk]);
    }
    const _Float16 z = (_Float16)0.f, mone = (_Float16)(-FX_RS);
    const half8 a0 = {rh[0], rh[0], rl[0], rh[1], rh[1], rl[1], rh[2], rh[2]};
    const half8 a1 = {rl[2], c == 0 ? mone : z, c == 0 ? mone : z, c == 1 ? mone : z, c == 1 ? mone : z, c == 2 ? mone : z, c == 2 ? mone : z, z};
    A = hf ? a1 : a0;
  }
  float tmax = 0.f;
  bool wild = false;
  if (lane < 8) {
    const uint32_t h = h0 + lane;
    float v[12];
#pragma unroll
    for (int c = 0; c < 12; c++) v[c] = Rt[(size_t)c * ldl + h];  // all twelve in flight together
    float rmax = 0.f, nanp = 0.f;
#pragma unroll
    for (int c = 0; c < 9; c++) rmax = fmaxf(rmax, fabsf(v[c]));
    tmax = fmaxf(fabsf(v[9]), fmaxf(fabsf(v[10]), fabsf(v[11])));
#pragma unroll
    for (int c = 0; c < 12; c++) nanp += v[c] * 0.f;  // NaN or infinity anywhere poisons the sum (fmaxf drops NaNs)
    wild = !(rmax <= 1.5f) || !(tmax < 1e30f) || !(nanp == 0.f);
    Ttab[wave][lane] = make_float4(v[9] * FX_RS * fi.s, v[10] * FX_RS * fi.s, v[11] * FX_RS * fi.s, 0.f);
  }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, o));
  tmax = __shfl(tmax, 0);
  const bool any_wild = __ballot(wild) != 0;
  const float s = fi.s, st = s * sqrt_rn(tau2);
  const float Sb = 2.6f * (fi.pmax * s) + fi.qmax * s + tmax * s;
  const float eta = Sb * (1.0f / 65536.0f);
  // the filter's range (every comparison is false on a NaN): the shell must stay thin against tau, the scaled
  // quantities inside what the error bound assumes
  const bool fast = !any_wild && (eta <= 0.25f * st) && (st <= 4096.f) && (tmax * s <= 2048.f) && (fi.pmax * s < 512.f) &&
                    (fi.qmax * s < 512.f);
  const float lo_e = FX_RS * (st - eta), hi_e = FX_RS * (st + eta);
  const float LO = lo_e * lo_e * (1.0f - 4e-6f), HI = hi_e * hi_e * (1.0f + 4e-6f);
  const uint32_t W2b = fast ? __float_as_uint(HI - LO) : 0u;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // Ttab: written and read by this wave only
  f32x16 C;
#pragma unroll
  for (int jj = 0; jj < 4; jj++) {
    const float4 T = Ttab[wave][2 * jj + hf];
    C[4 * jj] = T.x; C[4 * jj + 1] = T.y; C[4 * jj + 2] = T.z; C[4 * jj + 3] = 0.f;
  }
  uint32_t total[4] = {0, 0, 0, 0};
  uint32_t sr[4] = {0, 0, 0, 0};
  uint32_t qn = 0;
  bool redo = !fast;
  uint32_t* q = queue[wave];
  auto flush = [&]() {  // the wave's queue -> its global sub-queue (one ticket)
    const uint32_t sq = wid % FX_NQ;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&qcount[sq * 32], qn);
    base = __shfl(base, 0);
    // a ticket that does not fit leaves no hole: the part of it inside the sub-queue is filled with empty entries (the
    // exact pass reads min(count, capacity) of them), and the wave asks for a recount
    const bool fits = base + qn <= cap_sq;
    for (uint32_t i = lane; i < qn && base + i < cap_sq; i += 64)
      gq[(size_t)sq * cap_sq + base + i] = fits ? make_uint2(q[i] >> 5, (wid << 5) | (q[i] & 31u)) : make_uint2(0u, 0u);
    if (!fits) redo = true;
    qn = 0;
  };
  for (uint32_t u = u0; u < u1; u++) {
    const int buf = (int)((u - u0) & 1u);
    if constexpr ((VAR & 256) == 0) {                    // (256: timing-only ablation, no barrier)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's part of unit u has landed
      __syncthreads();                                   // ... everybody's has, and the other buffer is free
    }
    if (u + 1 < u1) stage(u + 1, buf ^ 1);
    if (!redo) {
      const half8* Bc = reinterpret_cast<const half8*>(Bt[buf]) + lane;  // (tile layout: filter_tile_block)
      auto mfma = [&](const half8& b) -> f32x16 {
        if constexpr ((VAR & 16) != 0) {  // ablation: no matrix instruction (the operand stays live)
          f32x16 D = C;
          asm volatile("" ::"v"(b));
#pragma unroll
          for (int i = 0; i < 16; i++) asm volatile("" : "+v"(D[i]));  // opaque: nothing of the epilogue can be hoisted
          return D;
        } else {
          if constexpr ((VAR & 2) != 0) __builtin_amdgcn_s_setprio(1);
          const f32x16 D = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, b, C, 0, 0, 0);
          if constexpr ((VAR & 2) != 0) __builtin_amdgcn_s_setprio(0);
          return D;
        }
      };
      // the vector work of one step: x = |E'|^2 - LO per test, sign bit into the shift register, shell test, queue
      auto epilogue = [&](const f32x16& D, int g) {
        if constexpr ((VAR & 32) != 0) {  // ablation: no epilogue
          sr[0] ^= __float_as_uint(D[0]) ^ __float_as_uint(D[5]) ^ __float_as_uint(D[10]) ^ __float_as_uint(D[14]);
          return;
        }
        float x[4];
        uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
          const float v = fma_(D[4 * jj + 2], D[4 * jj + 2], fma_(D[4 * jj + 1], D[4 * jj + 1], fma_(D[4 * jj], D[4 * jj], -LO)));
          x[jj] = v;
          sr[jj] = __builtin_amdgcn_alignbit(sr[jj], __float_as_uint(v), 31);  // sign bit: |E'|^2 < LO, a certain inlier
          mn = min(mn, __float_as_uint(v));
        }
        if constexpr ((VAR & 512) != 0) { sr[0] ^= mn; return; }  // (512: timing-only ablation, no shell test)
        const uint64_t hm = __ballot(mn < W2b);  // as unsigned integers: 0 <= x < HI - LO, the undecided shell
        if (__builtin_expect(hm != 0, 0)) {
          const uint32_t k2 = (uint32_t)__popcll(hm);
          if (qn + k2 <= ql) {
            uint32_t bits = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) bits |= (__float_as_uint(x[t]) < W2b) ? (1u << t) : 0u;
            if (mn < W2b) q[qn + __popcll(hm & ((1ull << lane) - 1ull))] = ((u * FX_UNIT + 32 * g + col) << 5) | ((uint32_t)hf << 4) | bits;
            qn += k2;
          } else {
            redo = true;  // more undecided tests than the queue holds: the exact pass takes the whole (wave, split)
          }
        }
        // The idle fourth rows of D stay "in use" up to here: otherwise the register allocator parks this epilogue's
        // temporaries in the idle rows of the OTHER accumulator set — whose MFMA is still in flight — and has to pad the
        // write-after-write hazard with s_nop until that MFMA has finished, which is the overlap this variant is after.
        if constexpr ((VAR & 1) != 0) asm volatile("" ::"v"(D[3]), "v"(D[7]), "v"(D[11]), "v"(D[15]));
      };
      if constexpr ((VAR & 1) != 0) {
        // software pipeline inside the unit: step g + 1's MFMA is in the matrix pipe while step g's epilogue issues
        constexpr int G = FX_UNIT / 32;
        half8 b0 = Bc[0], b1 = Bc[64];
        f32x16 D0 = mfma(b0), D1;
#pragma unroll 1
        for (int g = 0; g < G; g += 2) {
          D1 = mfma(b1);                                   // step g + 1
          if (g + 2 < G) b0 = Bc[64 * (g + 2)];
          epilogue(D0, g);
          if (g + 2 < G) {
            D0 = mfma(b0);                                 // step g + 2
            b1 = Bc[64 * (g + 3)];
          }
          epilogue(D1, g + 1);
        }
      } else {
        half8 b = Bc[0];
#pragma unroll 2  // (by 4: no gain; fully unrolled: 144 bytes of spills inside the loop, 64 -> 118 us on C2)
        for (int g = 0; g < FX_UNIT / 32; g++) {
          const f32x16 D = mfma(b);
          if constexpr ((VAR & 64) == 0) {  // (64: ablation, the operand is not re-read)
            if (g + 1 < FX_UNIT / 32) b = Bc[64 * (g + 1)];
          }
          epilogue(D, g);
        }
      }
      if ((u + 1) % (FX_WIN / FX_UNIT) == 0) {  // window boundary: 32 tests per register
#pragma unroll
        for (int t = 0; t < 4; t++) { total[t] += (uint32_t)__popc(sr[t]); sr[t] = 0; }
      }
      if (qn > ql / 2) flush();
    }
  }
  if (qn && !redo) flush();
  if (redo && lane == 0) {
    const size_t bit = (size_t)blockIdx.y * n_waves + wid;
    atomicOr(&redo_bits[bit >> 5], 1u << (bit & 31));
  }
#pragma unroll
  for (int t = 0; t < 4; t++) {
    uint32_t c = total[t];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 32);
    if (col == 0) cnt_out[(size_t)blockIdx.y * ldl + h0 + 2 * t + hf] = redo ? 0u : c;
  }
}

// How the Gram filter's launch cuts the tile's units (256 correspondences) into the `splits` workgroups of a group of 256 rows —
// shared by the filter and the exact pass (which must find the split a queued test belongs to).
//   rows not all near the frame: split y walks units [y pu_far, (y + 1) pu_far) of ALL the units;
//   rows all near the frame:     only `ns` splits work — split y walks [y pu_near, (y + 1) pu_near) of the NEAR units —, and ns grows
//                                beyond 1 only while the launch has fewer workgroups than the chip has slots (C2: 196 groups).
struct GramGeom { uint32_t units, near_units, pu_far, ns, pu_near; };
__device__ __forceinline__ GramGeom gram_geom(uint32_t windows, uint32_t splits, uint32_t groups, const GramFrame* __restrict__ fr) {
  GramGeom g;
  g.units = windows * (uint32_t)(FX_WIN / GX_UNIT);
  g.near_units = min(g.units, ((uint32_t)fr->pts + GX_UNIT - 1) / GX_UNIT);
  g.pu_far = (g.units + splits - 1) / splits;
  const uint32_t room = 512u / max(groups, 1u);
  g.ns = max(1u, min(min(splits, max(g.near_units, 1u)), room));
  g.pu_near = (max(g.near_units, 1u) + g.ns - 1) / g.ns;
  return g;
}
__device__ __forceinline__ bool gram_near_block(uint32_t bx, uint32_t S, const GramFrame* __restrict__ fr) {
  return (bx / S + 1u) * (32u * GX_WAVES) <= (uint32_t)fr->seg[bx % S].cnt;  // all 256 rows are hypotheses near the frame
}

// X.  First the queued tests (one per thread; workgroup b serves sub-queue b % FX_NQ), then the (wave, split) pairs F
// gave up on (one per workgroup at a time).  Everything here is the canonical chain; the counts are integers.
__device__ __forceinline__ void load_rt_aos(const float4* __restrict__ RtAoS, uint32_t h, float (&M)[12]) {
  const float4 a = RtAoS[3 * (size_t)h], b = RtAoS[3 * (size_t)h + 1], c = RtAoS[3 * (size_t)h + 2];
  M[0] = a.x; M[1] = a.y; M[2] = a.z; M[3] = a.w; M[4] = b.x; M[5] = b.y; M[6] = b.z; M[7] = b.w;
  M[8] = c.x; M[9] = c.y; M[10] = c.z; M[11] = c.w;
}
__global__ __launch_bounds__(256) void score_exact_kernel(const float* __restrict__ planes, int n, int ld,
                                                          const float4* __restrict__ RtAoS, uint32_t ldl, float tau2,
                                                          uint32_t windows, uint32_t splits, uint32_t n_waves,
                                                          const uint2* __restrict__ gq, uint32_t cap_sq,
                                                          const uint32_t* __restrict__ qcount,
                                                          const uint32_t* __restrict__ redo_bits,
                                                          uint32_t* __restrict__ cnt_out,
                                                          const uint32_t* __restrict__ hperm,
                                                          const uint32_t* __restrict__ pperm,
                                                          const GramFrame* __restrict__ fr) {
  // hperm / pperm (the Gram filter; null for the linear one): its rows are PERMUTED — coefficient row -> hypothesis, tile row ->
  // correspondence.  Queue entries and recount bits speak of rows; the counts and the canonical chain of hypotheses and correspondences.
  const bool gram = hperm != nullptr;
  const uint32_t per = (windows + splits - 1) / splits;
  // the Gram filter's splits are cut in units, differently for rows near the frame and the others (gram_geom)
  const uint32_t groups = ldl / (32u * GX_WAVES), S = gram_segments(groups);
  GramGeom gg{};
  if (gram) gg = gram_geom(windows, splits, groups, fr);
  const float4* __restrict__ aos4 = reinterpret_cast<const float4*>(planes + 6 * (size_t)ld);  // 8 floats per correspondence
  const uint32_t sq = blockIdx.x % FX_NQ, nq = min(qcount[sq * 32], cap_sq);
  for (uint32_t i = (blockIdx.x / FX_NQ) * 256 + threadIdx.x; i < nq; i += (gridDim.x / FX_NQ) * 256) {
    const uint2 e = gq[(size_t)sq * cap_sq + i];
    if (gram) {  // {tile row, wave of 32 rows << 17 | lane half << 16 | one bit per accumulator register}
      const uint32_t mr = e.x, w32 = e.y >> 17, ehf = (e.y >> 16) & 1u;
      const uint32_t sp = (mr / (uint32_t)GX_UNIT) / (gram_near_block(w32 / GX_WAVES, S, fr) ? gg.pu_near : gg.pu_far);
      const uint32_t m = pperm[mr];
      const float4 pa = aos4[2 * (size_t)m], pb = aos4[2 * (size_t)m + 1];
      for (uint32_t bits = e.y & 0xFFFFu; bits; bits &= bits - 1) {
        const uint32_t i16 = (uint32_t)(__ffs(bits) - 1), row = 8 * (i16 >> 2) + 4 * ehf + (i16 & 3u), hr = w32 * 32 + row;
        const size_t bit = (size_t)sp * n_waves + (hr >> 3);
        if ((redo_bits[bit >> 5] >> (bit & 31)) & 1u) continue;  // recounted as a whole below
        const uint32_t h = hperm[hr];
        float M[12];
        load_rt_aos(RtAoS, h, M);
        const float d2 = resid2(M, pa.x, pa.y, pa.z, pa.w, pb.x, pb.y);
        if (finite12(M) && d2 < tau2) atomicAdd(&cnt_out[(size_t)sp * ldl + h], 1u);
      }
      continue;
    }
    const uint32_t m = e.x, wid = e.y >> 5, ehf = (e.y >> 4) & 1u, sp = (m / FX_WIN) / per;
    const size_t bit = (size_t)sp * n_waves + wid;
    if ((redo_bits[bit >> 5] >> (bit & 31)) & 1u) continue;  // recounted as a whole below
    const float4 pa = aos4[2 * (size_t)m], pb = aos4[2 * (size_t)m + 1];  // the correspondence in two 16-byte loads
    for (uint32_t bits = e.y & 0xFu; bits; bits &= bits - 1) {
      const uint32_t h = wid * 8 + 2 * (uint32_t)(__ffs(bits) - 1) + ehf;
      float M[12];
      load_rt_aos(RtAoS, h, M);
      const float d2 = resid2(M, pa.x, pa.y, pa.z, pa.w, pb.x, pb.y);
      if (finite12(M) && d2 < tau2) atomicAdd(&cnt_out[(size_t)sp * ldl + h], 1u);
    }
  }
  const size_t nbits = (size_t)splits * n_waves;
  for (size_t w = blockIdx.x; w < (nbits + 31) / 32; w += gridDim.x) {
    uint32_t word = redo_bits[w];
    while (word) {
      const size_t bit = w * 32 + (size_t)(__ffs(word) - 1);
      word &= word - 1;
      const uint32_t sp = (uint32_t)(bit / n_waves), wid = (uint32_t)(bit % n_waves);
      const uint32_t hr = wid * 8 + (threadIdx.x & 7), h = gram ? hperm[hr] : hr;
      float M[12];
      load_rt_aos(RtAoS, h, M);
      const bool ok = finite12(M);
      uint32_t m0 = sp * per * FX_WIN, m1 = min((uint32_t)n, min(windows, (sp + 1) * per) * FX_WIN);
      if (gram) {  // the units its filter workgroup walked (rows near the frame: of the near units only — the rest cannot hold an inlier)
        const bool nb = gram_near_block(wid / 32u, S, fr);
        const uint32_t pu = nb ? gg.pu_near : gg.pu_far, ue = nb ? gg.near_units : gg.units;
        m0 = sp * pu * (uint32_t)GX_UNIT;
        m1 = min((uint32_t)n, min(ue, (sp + 1) * pu) * (uint32_t)GX_UNIT);
      }
      uint32_t cnt = 0;
      for (uint32_t mr = m0 + (threadIdx.x >> 3); mr < m1; mr += 32) {
        const uint32_t m = gram ? pperm[mr] : mr;
        const float4 pa = aos4[2 * (size_t)m], pb = aos4[2 * (size_t)m + 1];
        const float d2 = resid2(M, pa.x, pa.y, pa.z, pa.w, pb.x, pb.y);
        cnt += (ok && d2 < tau2) ? 1u : 0u;
      }
      cnt += __shfl_xor(cnt, 8);
      cnt += __shfl_xor(cnt, 16);
      cnt += __shfl_xor(cnt, 32);
      if ((threadIdx.x & 63) < 8 && cnt) atomicAdd(&cnt_out[(size_t)sp * ldl + h], cnt);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// C2, inlier count, the GRAM filter (r03): the matrix pipe evaluates the squared residual itself — since r04b in the FRAME OF A
// REFERENCE HYPOTHESIS, which (a) makes the cancelling terms small exactly where precision is needed and (b) lets most tests be
// skipped with a proof instead of being evaluated.
//
// The frame.  gram_ref_kernel lets GX_VOTE hypotheses spread over the ranked list vote for the one most of them agree with
// (R0, t0; R0 rebuilt orthogonal in fp64 — ANY rotation is a valid frame, a good one is only faster).  With c the centre of the
// source cloud's box and s a power of two,
//     P' = s (p - c),   Q' = s (R0^T (q - t0) - c),   V' = Q' - P'          (per correspondence; every |coordinate| < 64)
//     M  = R0^T R_h,    dM = M - I,    tau' = s (R0^T (t_h - t0) + dM c)     (per hypothesis; fp64)
// and because R0 is orthogonal, in exact arithmetic
//     s^2 |R_h p + t_h - q|^2 = |dM P' + tau' - V'|^2
//         = sum_ij (-2 dM_ij + G_ij) Q'_i P'_j + |V'|^2 + |tau'|^2 + 2 (dM^T tau') . P' - 2 tau' . V'  -  V'^T G P' ,
// G = R_h^T R_h - I the hypothesis' own defect (~1e-7 for a Kabsch result; the last term, <= 3 g |V'| |P'|, goes into the bound).
// That is a DOT PRODUCT of 16 features of the correspondence
//     Q'_i P'_j (9), |V'|^2 / 2, 256 P'_j (3), 256 V'_i (3)                         (tile workgroups of the Kabsch launch, fp64)
// with 16 coefficients of the hypothesis  -2 dM_ij + G_ij, 2, 2 (dM^T tau')_j / 256, -2 tau'_i / 256  plus the constant |tau'|^2
// (the Kabsch launch's own threads, fp64).  For a hypothesis NEAR the reference dM is small (C2: 0.02 - 0.05) and so is every
// term: the nine products that cancelled at the size of the CLOUDS in r03's form (|P'|^2 + |Q'|^2 against tau'^2) now cancel at
// dM times that, and a true correspondence has a small V' besides.  Features and coefficients are split into two fp16 halves; hi x hi,
// hi x lo and lo x hi products are kept: 48 slots = three chained v_mfma_f32_32x32x16_f16, rows = 32 hypotheses, columns = 32
// correspondences, accumulator initialised to |tau'|^2 - LO: a lane then holds x = D~ - LO for 16 hypotheses of one
// correspondence — sign bit into a shift register (1 instruction), shell test 0 <= x < HI - LO as an unsigned min over
// the 16 (0.5), nothing else: 1.6 vector instructions per test against the linear filter's 4.75.
//
// The cut.  reach_h = |dM|_F Pn + |tau'| bounds |dM P' + tau'| over the whole cloud, so a correspondence with
// |V'| > reach_h + tau' + dE_h + margin is an outlier of h by the triangle inequality — whatever the canonical chain's roundings
// (dE_h, below).  Correspondences are dealt into NEAR (|V'| <= th_v: first tile rows) and FAR (last rows), hypotheses into NEAR
// (reach_h + dE_h <= th_h = GX_KAPPA tau': first coefficient rows) and the rest (last rows) — both by one atomic per workgroup inside
// the Kabsch launch; th_v = th_h + 1.05 tau' + 1e-3.  A filter workgroup whose 256 rows are all NEAR hypotheses walks the NEAR
// units only.  On the BASELINE scenes ~90 % of the ranked hypotheses are near the voted reference and 11 - 20 % of the
// correspondences are near (the inliers and what lies around them): three quarters of the tests are never made.  The order inside
// each class is whatever the atomics give — the counts are integers, every permutation gives the same ones; hperm / pperm lead back.
//
// What the squared form costs is precision.  How the matrix
// pipe adds the 16 products and C is not in the ISA text.  tools/ubench/mfma_numerics.hip probes it (profiles/
// r03_ubench_mfma_numerics.txt): the final rounding is to nearest-even; fp16 sub-normals are NOT flushed; terms far below the
// largest one lose their low bits before the sum (a product 1.5 beside 2^24 arrives as 1; beside a C of 2^24 it arrives
// whole) — consistent with aligning all 17 terms to the largest exponent, products counted one binade up, and cutting them at
// a 2^-25 fraction of it, which reproduces two thirds of 3000 random cancelling dot products bit for bit; and over 15 000
// such dot products |hardware - exact| never passed 3.75 x 2^-24 of the LARGEST term (17 cuts of < 2^-24 of it each would
// allow 17).  The bound takes 18.5 x 2^-24 of the largest term per MFMA — the cut model's worst case, five times the worst
// seen.  This is a MEASURED model of gfx950's matrix pipe, not an ISA guarantee: every context probes its own pipe before the
// first call that would use this filter (gram_guard_kernel), and the parity suite compares EVERY count with the canonical
// kernel's at the BASELINE shapes, on adversarial scenes and on random degenerate clouds.  With F = |dM|_F, m = max |dM_ij|,
// Tn = |tau'|, g = max |G_ab|, and the correspondences a row is tested against bounded by |V'| <= vb, |Q'| <= Qb (NEAR rows:
// vb = th_v, Qb = Pn + th_v; the others: vb = Pn + Qn, Qb = Qn), u = 2^-24, D* the exact value:
//     terms        2 (m + g/2) Qb Pn | vb^2 | 2 F Tn Pn | 2 Tn vb | Tn^2 + 1.5 tau'^2 (the constant):  Mh = 1.05 x the largest
//     MFMA 1       18.5 u Mh                                                                    (GX_ACC)
//     MFMAs 2, 3   their terms are <= 2^-10 of MFMA 1's; their C is the running value: 18.5 u (|x| + 3e-3 S) each — the part
//                  proportional to x (2.2e-6) is carried by the factors (1 -+ 1e-5) of LO / HI, the rest is the 1e-8 S term
//     splits       x = hi + lo + rem, |rem| <= 2^-22 |x|;  w F - (wh Fh + wh Fl + wl Fh) = wl Fl + ... <= 3.01 x 2^-22 |w F|:
//                  7.2e-7 Sl, Sl = (2 F + 3 g) Qb Pn + 2 F Tn Pn + 2 Tn vb  (exact arithmetic, no model)          (GX_Q)
//     norm         the norm feature's coefficient 2 RS alpha has no low half, so of its three products only hi x hi and
//                  hi x lo exist: its two pieces leave 2^-22 of it, 2.4e-7 vb^2                                   (GX_NORM)
//     accumulator  initial value RS (|tau'|^2 - LO_h) rounded to fp32: u Mh (inside GX_ACC's margin)
//     defect       - V'^T G P': <= 3 g vb Pn  (beyond g = 1e-3: not a rotation, the hypothesis is recounted exactly)
//     frame        R0^T R0 = I to 3e-16, P' / Q' / dM / tau' evaluated in fp64: < 1e-9 in these units (inside the 1e-4)
//   sum: eps_h = 1.1e-6 Mh + 7.5e-7 Sl + 2.5e-7 vb^2 + 1e-8 S + 3 g vb Pn + 1e-4                                  (gram_eps)
// The canonical fp32 chain itself deviates from exact arithmetic: its residual VECTOR by <= dE = sqrt(3) 4 u s (qmax + 1.75 pmax
// + |t|max) (original, uncentred magnitudes), its square by 3 more roundings.  So, with st = s sqrt(tau2):
//     D~ <  LO_h = (st - dE)^2 (1 - 1e-5) - eps_h   =>  canonical inlier;     D~ >= HI_h = (st + dE)^2 (1 + 1e-5) + eps_h  =>  outlier;
// Every hypothesis keeps its OWN shell: the filter wave scales row h by alpha_h = the largest power of two <= min(16, widest shell
// of its 32 rows / the row's own width) — exact in fp16 / fp32 — so that "0 <= x < W" with one W per wave tests alpha_h RS (D~ - LO_h)
// against at least alpha_h RS (HI_h - LO_h).  Hypotheses fall into four classes, decided with the coefficients:
//     normal   eps_h <= 0.25 st^2: filtered;        far      |tau'| - F Pn - Vn >= 1.05 st + dE: no correspondence can be an inlier,
//     padding  beyond n_local: count 0;              recount  everything else (non-finite, not a rotation, shell too wide): its
//                                                             group of 8 rows goes to the exact pass wholesale.
// ------------------------------------------------------------------------------------------------
// sum of `v` over each aligned group of 32 lanes, valid in the group's upper 16 lanes (DPP: quad swaps, half mirror, mirror,
// then lane 15 of the lower row broadcast into the upper row)
__device__ __forceinline__ uint32_t dpp_sum32_upper(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);  // row_mirror: every lane holds its row's sum
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast15 into rows 1 and 3
  return v;
}

template <int VAR>  // (timing-only ablations for tools/ab_stage.py: 512 = no shell test, 256 = no barrier, 32 = no epilogue)
__global__ __launch_bounds__(64 * GX_WAVES, 2) void score_gram_kernel(GramCoef coef, uint32_t ldl,
                                                                     const uint4* __restrict__ tile, uint32_t windows,
                                                                     uint32_t splits, uint32_t n_waves8,
                                                                     uint32_t* __restrict__ cnt_out, uint2* __restrict__ gq,
                                                                     uint32_t cap_sq, uint32_t* __restrict__ qcount,
                                                                     uint32_t* __restrict__ redo_bits, uint32_t ql, uint32_t group_major) {
  __shared__ uint4 Bt[3][GX_UNIT * GX_TILE_Q];   // ring of three 16 KiB units: one being read, one landing, one being issued
  __shared__ uint2 queue[GX_WAVES][GX_QL];
  constexpr int PIECES = GX_UNIT * GX_TILE_Q / (64 * GX_WAVES);  // LDS-DMA instructions per wave and unit
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, hf = lane >> 5;
#ifdef SC_ABLATIONS  // lab build: where a workgroup's life goes (tools/r4/gramtick.py; ql == 127 switches the printing on)
  long long tk[5];
  tk[0] = wall_clock64();
#define SC_GRAM_TICK(i) tk[i] = wall_clock64()
#else
#define SC_GRAM_TICK(i)
#endif
  // The grid is one-dimensional, groups x splits workgroups, and the LONG ones go first: the row blocks that hold
  // a hypothesis not near the reference are the LAST ones of their segment (sc_gramref.hpp: segment = row block % S) — the highest
  // row blocks — and walk every correspondence, the others a few near units (dispatched in row order, the last workgroups to
  // start were the longest: a tail as long as the kernel's useful part).
  const GramFrame* __restrict__ fr = coef.frame;
  const uint32_t groups = gridDim.x / splits, S = gram_segments(groups);
  // GROUP-major, highest row blocks first (r04c): EVERY split of a far row block is dispatched before the first near one.  Split-
  // major (r04b) started split k's far workgroups — the longest of the launch — only after the splits before it had been
  // dispatched, near workgroups, empty ones and all (C4: the second split's 267 far workgroups of 10 units began ~45 us into the
  // launch).  Within a row block the splits are rotated by r(block): workgroup b runs on XCD b % 8, and with by = b % splits the
  // WORKING workgroups of the near rows (by < ns) would sit on 8 / gcd(splits, 8) of the eight XCDs (by = b % 8 at 8 splits put
  // them all on one: C3 508 us instead of 150); r advances once per 8 / gcd blocks, which deals them to all eight evenly.
  // Only for launches of about two resident generations (launch_score_filter: C2's 980 workgroups, 22.6 -> 20.2 us): at C4's 3908
  // the same order measured 147 us against 109 — two far workgroups sharing a CU run at half speed each, and far-first pairs them
  // all; split-major pairs most of them with short near ones.  There: split-major, the highest row blocks first within a split.
  uint32_t bx, by;
  if (group_major) {
    const uint32_t gidx = blockIdx.x / splits, sidx = blockIdx.x - gidx * splits;
    const uint32_t dg = min(splits & (0u - splits), 8u);            // gcd(splits, 8): splits <= 8
    bx = groups - 1u - gidx; by = (sidx + ((gidx * dg) >> 3) % dg) % splits;
  } else {
    bx = groups - 1u - blockIdx.x % groups; by = blockIdx.x / groups;
  }
  const uint32_t wid = bx * GX_WAVES + wave;  // wave of 32 hypotheses
  // The cut: a workgroup whose 256 rows are all hypotheses NEAR the reference walks the NEAR correspondences only — the tile's
  // first rows; every other correspondence is an outlier of every one of them by the triangle inequality (see the header).
  const GramGeom gg = gram_geom(windows, splits, groups, fr);
  const bool near_block = gram_near_block(bx, S, fr);
  if (near_block && by >= gg.ns) return;  // (its rows of these splits are cleared by split 0, below)
  const uint32_t u0 = by * (near_block ? gg.pu_near : gg.pu_far);
  const uint32_t u1 = near_block ? min(u0 + gg.pu_near, gg.near_units) : min(u0 + gg.pu_far, gg.units);
  // ---- every global read of the prologue is ISSUED here, before anything waits: the coefficients of this lane's row, the
  // per-row words of the wave's 16 accumulator rows.  (Written where they are used, each group of four rows became a load ->
  // wait -> branch chain of its own, and the epilogue sixteen load -> wait -> store round trips: by the lab build's timestamps
  // a workgroup of C2 spent 4 - 5.7 us before its first step and 3.1 - 4.1 us after its last one, as long as in the 4.6 - 7.9 us
  // of steps between them.)  Behind the early exit, not before it: issued first of all — under the frame's own two dependent
  // reads — the workgroups with nothing to do, most of C2's grid, read ~230 bytes per thread for nothing: 24.1 -> 26.2 us.
  const uint32_t row = (uint32_t)col, h = wid * 32 + row;  // (< ldl: a multiple of 256, the grid has ldl / 256 workgroups)
  const uint4* __restrict__ ca = reinterpret_cast<const uint4*>(coef.A) + (size_t)h * 4;
  typedef float f32q __attribute__((ext_vector_type(4)));
  typedef uint32_t u32q __attribute__((ext_vector_type(4)));
  const u32q a0 = *reinterpret_cast<const u32q*>(ca + hf), a2 = *reinterpret_cast<const u32q*>(ca + 2 + hf);
  const float wrow = coef.W[h];
  const uint32_t frow = coef.flag[h], hrow = coef.hperm[h];
  f32q c4[4], w4[4];
  u32q f4[4];
#pragma unroll
  for (int jj = 0; jj < 4; jj++) {
    const size_t base = (size_t)wid * 32 + 8 * jj + 4 * hf;
    c4[jj] = *reinterpret_cast<const f32q*>(coef.C + base);
    w4[jj] = *reinterpret_cast<const f32q*>(coef.W + base);
    f4[jj] = *reinterpret_cast<const u32q*>(coef.flag + base);
  }
  // the places in the ranked list of this lane's 16 accumulator rows (read at the end, 16 registers the step loop has no room for)
  auto ranked_rows = [&](uint32_t* hp) {
    u32q hp4[4];
#pragma unroll
    for (int jj = 0; jj < 4; jj++) hp4[jj] = *reinterpret_cast<const u32q*>(coef.hperm + (size_t)wid * 32 + 8 * jj + 4 * hf);
    asm volatile("" ::"v"(hp4[0]), "v"(hp4[1]), "v"(hp4[2]), "v"(hp4[3]));  // (four loads, ONE wait)
#pragma unroll
    for (int jj = 0; jj < 4; jj++) { hp[4 * jj] = hp4[jj].x; hp[4 * jj + 1] = hp4[jj].y; hp[4 * jj + 2] = hp4[jj].z; hp[4 * jj + 3] = hp4[jj].w; }
  };
  auto stage = [&](uint32_t u, int buf) {  // (asm: see score_filter_kernel)
#pragma unroll
    for (int i = 0; i < PIECES; i++) {
      const uint4* gsrc = tile + (size_t)u * (GX_UNIT * GX_TILE_Q) + 64 * GX_WAVES * i + tid;
      const uint32_t lds_dst = __builtin_amdgcn_readfirstlane(
          (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)(&Bt[buf][64 * GX_WAVES * i + wave * 64]));
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
    }
  };
  if (u0 < u1) stage(u0, 0);
  if (u0 + 1 < u1) stage(u0 + 1, 1);
  // (the asm pins the loads above the branches below: nothing is sunk into the block that uses it)
  asm volatile("" ::"v"(a0), "v"(a2), "v"(wrow), "v"(frow), "v"(c4[0]), "v"(c4[1]), "v"(c4[2]), "v"(c4[3]), "v"(w4[0]), "v"(w4[1]),
               "v"(w4[2]), "v"(w4[3]));
  asm volatile("" ::"v"(f4[0]), "v"(f4[1]), "v"(f4[2]), "v"(f4[3]), "v"(hrow));
  if (near_block && by == 0 && hf == 0 && h < ldl)  // the splits no workgroup of these rows works in count nothing
    for (uint32_t y = gg.ns; y < splits; y++) cnt_out[(size_t)y * ldl + hrow] = 0u;
  if (u0 >= u1) {  // (workgroup-uniform) nothing to look at in this split
    if (hf == 0 && h < ldl) cnt_out[(size_t)by * ldl + hrow] = 0u;
    return;
  }
  // ---- prologue: the coefficients were made once per call by gram_coef_block (lane (row, hf) takes the halves of its row).  What
  // belongs to the WAVE — the widest shell of its 32 rows, every row's alpha, the groups of 8 rows the exact pass recounts — is
  // made here: the rows of a wave come from all over the ranked list (NEAR hypotheses first), only this kernel sees them together.
  half8 A0 = *reinterpret_cast<const half8*>(&a0), A2 = *reinterpret_cast<const half8*>(&a2);
  float wmax = wrow;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o, 32));  // (both lane halves hold the same 32 rows)
  const uint32_t normal_rows = (uint32_t)__ballot((frow & 1u) != 0u), rc = (uint32_t)__ballot((frow & 2u) != 0u);
  uint32_t redo4 = 0, live_rows = normal_rows;
#pragma unroll
  for (int jj = 0; jj < 4; jj++)
    if ((rc >> (8 * jj)) & 0xFFu) { redo4 |= 1u << jj; live_rows &= ~(0xFFu << (8 * jj)); }  // rows of a group that is recounted anyway are switched off
  const bool any_normal = live_rows != 0u;
  // alpha: the largest power of two <= min(what the row's fp16 coefficients allow, widest shell / own shell) — scaling by it is exact
  auto alpha_of = [&](float w, uint32_t fl) -> float {  // (no division: w 2^k is exact, the comparisons decide; 17 correctly rounded divides per lane cost the prologue ~350 instructions)
    const int cap = (int)((fl >> 8) & 7u);
    float a = 1.0f;
#pragma unroll
    for (int k = 1; k <= 4; k++) a = (k <= cap && w * (float)(1 << k) <= wmax) ? (float)(1 << k) : a;
    return a;
  };
  {
    const bool live = (live_rows >> row) & 1u;
    const _Float16 am = (_Float16)(live ? alpha_of(wrow, frow) : 0.0f);
    A0 = A0 * am; A2 = A2 * am;
  }
  const half8 A1 = A0;  // hi x lo: the tile's second block holds the low halves of the features
  // alpha_h x own width <= wmax: one W for the wave (a hair above wmax)
  const uint32_t W2b = ((VAR & 512) || !any_normal) ? 0u : __float_as_uint(wmax * (1.0f + 4e-7f));
  f32x16 C;
#pragma unroll
  for (int jj = 0; jj < 4; jj++) {
    const float cc[4] = {c4[jj].x, c4[jj].y, c4[jj].z, c4[jj].w}, ww[4] = {w4[jj].x, w4[jj].y, w4[jj].z, w4[jj].w};
    const uint32_t ff[4] = {f4[jj].x, f4[jj].y, f4[jj].z, f4[jj].w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const bool live = (live_rows >> (8 * jj + 4 * hf + i)) & 1u;
      C[4 * jj + i] = live ? cc[i] * alpha_of(ww[i], ff[i]) : 1e30f;
    }
  }
  // The coefficients are USED here, so that the compiler's wait for these global loads sits here and not at their first real
  // use — the first MFMA of the step loop, where an s_waitcnt vmcnt(0) in every trip also waited for the LDS-DMA of the units
  // ahead (the compiler cannot see into the asm that issues them): until r03c every unit's first step stood still until the
  // NEXT unit had landed, i.e. nothing was prefetched at all.
  asm volatile("" ::"v"(A0), "v"(A2), "v"(C), "s"(W2b), "s"(redo4));
  SC_GRAM_TICK(1);
  uint32_t total[16], sr[16];
#pragma unroll
  for (int i = 0; i < 16; i++) { total[i] = 0; sr[i] = 0; }
  const int my_step = __builtin_amdgcn_readfirstlane(wave) & (GX_UNIT / 32 - 1);  // the step at which this wave issues its LDS-DMA
  uint32_t qn = 0;  // entries in this wave's queue: wave-uniform, lives in a scalar register
  uint2* q = queue[wave];
  bool flushed = false;  // a flush's global stores are younger than the LDS-DMA pieces in flight: the next wait is a full one
  auto flush_queue = [&]() {  // the wave's queue -> its global sub-queue (one ticket); see score_filter_kernel
    const uint32_t sq = wid % FX_NQ;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&qcount[sq * 32], qn);
    base = __shfl(base, 0);
    const bool fits = base + qn <= cap_sq;
    for (uint32_t i = lane; i < qn && base + i < cap_sq; i += 64)
      gq[(size_t)sq * cap_sq + base + i] = fits ? make_uint2(q[i].x, (wid << 17) | q[i].y) : make_uint2(0u, 0u);
    if (!fits) redo4 = 0xFu;
    qn = 0;
    flushed = true;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the entries were read before the queue is written again
  };
  for (uint32_t u = u0; u < u1; u++) {
    const int buf = (int)((u - u0) % 3u);
    if constexpr ((VAR & 256) == 0) {
      // this wave's part of unit u has landed: everything it issued except the youngest unit's pieces (loads return in order)
      if (u + 1 < u1 && !flushed) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      flushed = false;
      __syncthreads();  // ... everybody's has, and nobody reads unit u - 1's buffer any more (it takes unit u + 2)
    }
#ifdef SC_ABLATIONS
    if (u == u0) tk[2] = wall_clock64();
#endif
    // Unit u + 2 is issued right behind the barrier, TWO units ahead: with two buffers the pieces of unit u + 1 were issued here
    // and — see the note on the coefficients above — waited for at once.  (VAR bit 0: each wave issues at a step of its own
    // inside the step loop instead, so that the eight waves' LDS-DMA instructions, ~125 cycles apiece, do not queue up behind
    // each other — tools/ubench/gram_loop.hip loses 20 % to that; here it measured 2 % SLOWER, C4 319 vs 313 us.)
    const bool stage_ahead = (VAR & 64) == 0 && u + 2 < u1;
    const int nbuf = buf == 0 ? 2 : buf - 1;
    if constexpr ((VAR & 1) == 0) {
      if (stage_ahead) stage(u + 2, nbuf);
    }
    if (any_normal && redo4 != 0xFu) {
      const half8* Bc = reinterpret_cast<const half8*>(Bt[buf]) + lane;
      // the vector work of one step.  sign bit: D~ < LO_h, a certain inlier.  Shell test 0 <= x < W as an unsigned minimum,
      // kept per group of four registers: with 1024 tests per step a step has an undecided test one time in four, so the
      // path that queues them must be short — it looks at the four group minima first and only at a group that hit.
      auto epilogue = [&](const f32x16& D, int g) {
        if constexpr ((VAR & 32) != 0) { sr[0] ^= __float_as_uint(D[0]) ^ __float_as_uint(D[5]) ^ __float_as_uint(D[10]) ^ __float_as_uint(D[15]); return; }
        uint32_t gm[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
          for (int i = 4 * j; i < 4 * j + 4; i++) sr[i] = __builtin_amdgcn_alignbit(sr[i], __float_as_uint(D[i]), 31);
          gm[j] = min(min(min(__float_as_uint(D[4 * j]), __float_as_uint(D[4 * j + 1])), __float_as_uint(D[4 * j + 2])), __float_as_uint(D[4 * j + 3]));  // v_min3 + v_min
        }
        const uint32_t mn = min(min(min(gm[0], gm[1]), gm[2]), gm[3]);
        if (__builtin_expect(__ballot(mn < W2b) != 0, 0)) {
          // A step has an undecided test one time in three, and a wave that dawdles here holds up the seven others at the next
          // barrier: nothing on this path waits for anything.  Groups of four registers that no lane hit are skipped (wave-
          // uniform branch); in a group that hit, the lanes take consecutive slots of the wave's LDS queue by the ballot mask
          // (v_mbcnt) above a fill count that lives in a scalar register — the LDS atomic with its returned value and the
          // s_waitcnt behind it that did this before cost a third of the kernel (C4: 341 us, 228 without this path).
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const uint64_t hit = __ballot(gm[j] < W2b);
            if (hit == 0) continue;
            const uint32_t slot = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(hit >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hit, 0u));
            if (gm[j] < W2b) {
              uint32_t bits = 0;
#pragma unroll
              for (int i = 0; i < 4; i++) bits |= (__float_as_uint(D[4 * j + i]) < W2b) ? (1u << (4 * j + i)) : 0u;
              if (slot < ql) q[slot] = make_uint2(u * GX_UNIT + 32 * g + col, ((uint32_t)hf << 16) | bits);
            }
            qn += (uint32_t)__popcll(hit);
          }
        }
      };
      // One step after the other: issuing step g + 1's chain before step g's vector work (a software pipeline with two
      // accumulator sets) was built and measured — hipcc rotates the loop into THREE sets with 16 moves per trip and
      // spills in the queueing path: C4 335 -> 403 us, C2 52 -> 57.  The waves of a SIMD overlap each other instead.
      half8 b0 = Bc[0], b1 = Bc[64];
#pragma unroll 1
      for (int g = 0; g < GX_UNIT / 32; g++) {
        f32x16 D = __builtin_amdgcn_mfma_f32_32x32x16_f16(A0, b0, C, 0, 0, 0);
        D = __builtin_amdgcn_mfma_f32_32x32x16_f16(A1, b1, D, 0, 0, 0);
        D = __builtin_amdgcn_mfma_f32_32x32x16_f16(A2, b0, D, 0, 0, 0);  // lo x hi: the hi halves of the features again
        // the next step's operands: two 16-byte LDS reads, in flight under this step's vector work
        if (g + 1 < GX_UNIT / 32) { b0 = Bc[32 * GX_TILE_Q * (g + 1)]; b1 = Bc[32 * GX_TILE_Q * (g + 1) + 64]; }
        if constexpr ((VAR & 1) != 0) {
          if (stage_ahead && g == my_step) stage(u + 2, nbuf);
        }
        epilogue(D, g);
      }
      // beyond ql entries were dropped — the exact pass takes the whole (wave, split)
      if (qn > ql) { redo4 = 0xFu; qn = 0; }
      if (((u - u0 + 1) & 3u) == 0) {  // every fourth unit: 32 tests per register
#pragma unroll
        for (int i = 0; i < 16; i++) { total[i] += (uint32_t)__popc(sr[i]); sr[i] = 0; }
      }
      if (qn > ql / 2) flush_queue();
    } else if ((VAR & 1) != 0 && stage_ahead) {
      stage(u + 2, nbuf);  // (a wave with nothing to filter still brings its share of the tile)
    }
  }
  SC_GRAM_TICK(3);
  if (qn && redo4 != 0xFu) flush_queue();
  uint32_t hp[16];
  ranked_rows(hp);
  if (lane == 0) {
#pragma unroll
    for (int jj = 0; jj < 4; jj++)
      if (((redo4 >> jj) & 1u) && (wid * 4 + jj) < n_waves8) {
        const size_t bit = (size_t)by * n_waves8 + wid * 4 + jj;
        atomicOr(&redo_bits[bit >> 5], 1u << (bit & 31));
      }
  }
  // the 32 columns of a lane half are two DPP rows: five v_add_dpp per register instead of five dependent ds_bpermute round
  // trips (80 of them in a row were ~2.5 us at the end of every wave — a fifth of a wave's life at C2's 32 steps)
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const uint32_t c = dpp_sum32_upper(total[i] + (uint32_t)__popc(sr[i]));  // (+ what a NEAR range that ends inside a window left in the shift register)
    const uint32_t r = 8 * (i >> 2) + 4 * hf + (i & 3), hh = wid * 32 + r;
    if (col == 31 && hh < ldl) cnt_out[(size_t)by * ldl + hp[i]] = ((redo4 >> (i >> 2)) & 1u) ? 0u : c;
  }
#ifdef SC_ABLATIONS
  SC_GRAM_TICK(4);
  if (ql == 127 && tid == 0 && blockIdx.x % 97 == 0)  // (wall_clock64: 100 MHz)
    printf("gram wg %u near %d units %u: prologue %lld, first unit %lld, steps %lld, tail %lld (x 10 ns)\n", blockIdx.x, (int)near_block,
           u1 - u0, tk[1] - tk[0], tk[2] - tk[1], tk[3] - tk[2], tk[4] - tk[3]);
#endif
#undef SC_GRAM_TICK
}

// (A persistent one-generation form of this kernel — contiguous runs of (hypothesis group, unit) items per workgroup, counts by
// atomics, recounts per unit: what VERDICT r03 #4 proposed — was built in round 4, bit-exact, and measured 3 - 4 % SLOWER at C2 and
// C4: profiles/r04_ab_gram_persistent.txt, DESIGN.md 5.0.  Its code left the tree when the reference-frame form below arrived.)

void launch_score_filter(const Points& pts, const Hyps& h, const FilterBufs& fb, const Partial& out, const Stamps& ev, const Derived& dv,
                         const Tuning& tn, hipStream_t st) {
  const Shard& sh = h.sh;
  if (sh.n_local == 0) return;
  const FilterPlan& fp = fb.plan;
  const FilterState f = filter_state(fb.state, fp);
  // exact pass: one thread per queue entry, grid-stride — a chain of dependent loads per entry, so big calls want more
  // threads in flight: workgroups per sub-queue by the number of tests (C4, 2.5e9 tests, 0.9 M entries: 36 -> 28 us at 8;
  // C2's 0.15 M entries are served by 2, more only adds launch tail)
  const uint64_t tests = (uint64_t)pts.n * sh.ld_local;
  const uint32_t exact_mult = tests >= (1ull << 31) ? 8u : (tests >= (1ull << 29) ? 4u : 2u);
  // hperm / pperm / frame: the Gram filter's permutations and frame (all null after the linear filter)
  auto launch_exact = [&](const uint32_t* hperm, const uint32_t* pperm, const GramFrame* gframe) {
    SC_LAUNCH_EV(score_exact_kernel, dim3(FX_NQ * exact_mult), dim3(256), st, (hipEvent_t) nullptr, ev.last, pts.planes, pts.n, pts.ld,
                          reinterpret_cast<const float4*>(h.aos), sh.ld_local, dv.tau2, fp.windows, fp.splits, fp.n_waves,
                          static_cast<const uint2*>(f.queue), f.cap_sq, static_cast<const uint32_t*>(f.qcount),
                          static_cast<const uint32_t*>(f.redo), out.counts, hperm, pperm, gframe);
  };
  // entries of the filter's LDS queue: the kernel's own size unless tuned smaller; one step can add 64 entries
  const uint32_t ql_max = fp.mode == 2 ? (uint32_t)GX_QL : (uint32_t)FX_QL;
  uint32_t ql = tn.filter_lds_queue ? tn.filter_lds_queue : ql_max;
  if (ql > ql_max) ql = ql_max;
  if (ql < 64) ql = 64;
  if (fp.mode == 2) {
    const GramCoef gc = gram_coef_view(fb.coef, sh.ld_local, fb.frame);
    const uint32_t group_major = (uint64_t)((sh.ld_local + 32 * GX_WAVES - 1) / (32 * GX_WAVES)) * fp.splits <= 1024u ? 1u : 0u;  // (see the kernel)
#define SC_GRAM_LAUNCH(V)                                                                                                         \
    SC_LAUNCH_EV(score_gram_kernel<V>, dim3((sh.ld_local + 32 * GX_WAVES - 1) / (32 * GX_WAVES) * fp.splits), dim3(64 * GX_WAVES), \
                          st, ev.first, ev.mid, gc, sh.ld_local, static_cast<const uint4*>(fb.tile), fp.windows, fp.splits, fp.n_waves, out.counts, \
                          f.queue, f.cap_sq, f.qcount, f.redo, ql, group_major)
    // The shipped library holds variant 0 only.  -DSC_ABLATIONS (sac-cot_amd/build.py --ablations; tools/pmc_gram_variants.sh)
    // also instantiates the bit-identical scheduling variant 1 and the TIMING-ONLY bodies (no shell test / no barrier / no
    // epilogue: wrong counts by design), which sc_set_debug refuses without it.
    switch (tn.filter_variant) {
#ifdef SC_ABLATIONS
      case 512: SC_GRAM_LAUNCH(512); break;
      case 256: SC_GRAM_LAUNCH(256); break;
      case 768: SC_GRAM_LAUNCH(768); break;
      case 32: SC_GRAM_LAUNCH(32); break;
      case 288: SC_GRAM_LAUNCH(288); break;
      case 352: SC_GRAM_LAUNCH(352); break;
      case 320: SC_GRAM_LAUNCH(320); break;
      case 1: SC_GRAM_LAUNCH(1); break;
#endif
      default: SC_GRAM_LAUNCH(0); break;
    }
#undef SC_GRAM_LAUNCH
    launch_exact(gc.hperm, gc.pperm, gc.frame);
    return;
  }
  const dim3 grid(sh.ld_local / (8 * FX_WAVES), fp.splits), block(64 * FX_WAVES);
#define SC_FILTER_LAUNCH(V)                                                                                                  \
  SC_LAUNCH_EV((score_filter_kernel<FX_WAVES, V>), grid, block, st, ev.first, ev.mid, h.soa, sh.ld_local, dv.tau2, \
                     static_cast<const uint4*>(fb.tile), f.info, fp.windows, fp.splits, fp.n_waves, out.counts, f.queue, f.cap_sq, \
                     f.qcount, f.redo, ql)
  switch (tn.filter_variant) {
#ifdef SC_ABLATIONS
    case 1: SC_FILTER_LAUNCH(1); break;
    case 2: SC_FILTER_LAUNCH(2); break;
    case 3: SC_FILTER_LAUNCH(3); break;
    case 16: SC_FILTER_LAUNCH(16); break;
    case 32: SC_FILTER_LAUNCH(32); break;
    case 17: SC_FILTER_LAUNCH(17); break;
    case 33: SC_FILTER_LAUNCH(33); break;
    case 64: SC_FILTER_LAUNCH(64); break;
    case 96: SC_FILTER_LAUNCH(96); break;
    case 80: SC_FILTER_LAUNCH(80); break;
    case 128: SC_FILTER_LAUNCH(128); break;
    case 256: SC_FILTER_LAUNCH(256); break;
    case 512: SC_FILTER_LAUNCH(512); break;
    case 768: SC_FILTER_LAUNCH(768); break;
    case 288: SC_FILTER_LAUNCH(288); break;
    case 272: SC_FILTER_LAUNCH(272); break;
#endif
    default: SC_FILTER_LAUNCH(0); break;
  }
#undef SC_FILTER_LAUNCH
  launch_exact(nullptr, nullptr, nullptr);
}

hipError_t filter_read_counters(const void* state, const FilterPlan& fp, hipStream_t st, uint64_t* undecided, uint64_t* recounts) {
  const FilterState f = filter_state(const_cast<void*>(state), fp);
  const size_t bm_words = ((size_t)fp.splits * fp.n_waves + 31) / 32;
  std::vector<uint32_t> h((size_t)FX_NQ * 32 + bm_words);
  hipError_t e = hipMemcpyAsync(h.data(), f.qcount, h.size() * 4, hipMemcpyDeviceToHost, st);  // counters, then the bitmap
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  uint64_t u = 0, r = 0;
  for (int q = 0; q < FX_NQ; q++) u += h[(size_t)q * 32];  // entries asked for (an overflowing sub-queue counts what was asked)
  for (size_t w = 0; w < bm_words; w++) r += (uint64_t)__builtin_popcount(h[(size_t)FX_NQ * 32 + w]);
  *undecided = u; *recounts = r;
  return hipSuccess;
}

hipError_t filter_read_frame(const void* frame, hipStream_t st, uint32_t out[5]) {
  std::vector<unsigned char> buf(sizeof(GramFrame));  // (8.5 KiB)
  GramFrame& f = *reinterpret_cast<GramFrame*>(buf.data());
  hipError_t e = hipMemcpyAsync(&f, frame, sizeof(GramFrame), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  uint32_t good = 0, all = 0;
  for (int v = 0; v < 64; v++) { good += (uint32_t)f.seg[v].cnt; all += (uint32_t)f.seg[v].cnt + (uint32_t)(f.seg[v].cnt >> 32); }
  out[0] = (uint32_t)f.pts; out[1] = good; out[2] = all; out[3] = f.ref_index; out[4] = f.ref_votes_q8;
  return hipSuccess;
}

bool filter_ablations_built() {
#ifdef SC_ABLATIONS
  return true;
#else
  return false;
#endif
}

}  // namespace sc
