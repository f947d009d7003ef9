// sc_score.hpp — what the translation units of stage C1 / C2 share: sc_score.hip (plain C2 kernel, arg-max), sc_kabsch.hip (C1 and what
// its launch carries: the filters' tile, the Gram coefficients, the reference-frame vote), sc_filter.hip (linear filter, exact pass,
// Gram filter) and sc_gram_guard.hip (the matrix-pipe probe).  Constants and layouts both sides of a buffer must agree on: the tile
// and queue geometry (FX_* / GX_*), the Gram bound (gram_eps, also evaluated by tests/test_gram_bound.py's host twin), the
// filter's state buffer.
#pragma once
#include <cstddef>
#include <hip/hip_ext.h>

#include "sc_kernels.hpp"

namespace sc {

// ---- Gram filter: constants shared by host and device -------------------------------------------------------------
constexpr int GX_UNIT = 256;     // correspondences per staging unit (8 MFMA steps of 32): 16 KiB; LDS holds three
constexpr int GX_TILE_B = 64;    // bytes of the tile per correspondence: hi halves and lo halves of its 16 features
constexpr int GX_TILE_Q = GX_TILE_B / 16;  // ... in 16-byte pieces
constexpr int GX_WAVES = 8;      // waves per workgroup, 32 hypotheses each: eight waves share a tile, so each of them issues three 1 KiB
                                 // LDS-DMA pieces per eight steps (with 4 waves and 128-correspondence units the DMA issue alone cost a quarter of the kernel)
constexpr int GX_QL = 128;       // LDS queue entries per wave (8 bytes each)
constexpr float GX_RS = 256.0f;  // scale of the A operand (keeps the low halves of the coefficients out of fp16's sub-normal range)
constexpr double GX_ACC = 1.1e-6;    // 18.5 x 2^-24: error of one MFMA per unit of its LARGEST term (five times the largest seen: score_gram_kernel)
constexpr double GX_Q = 7.5e-7;      // 3.01 x 2^-22 (+ margin): the dropped lo x lo products and split remainders per unit of sum |w F|
constexpr double GX_NORM = 2.5e-7;   // 2^-22 (+ margin): what the norm feature's two fp16 pieces leave, per unit of max |V'|^2
constexpr double GX_CANON = 4.2e-7;  // sqrt(3) * 4 * 2^-24: deviation of the canonical fp32 residual VECTOR per unit of magnitude
// shell half-width of a hypothesis, in units of the scaled squared residual.  F = |dM|_F, m = max |dM_ij|, Tn = |tau'|, g = the defect of
// R^T R; the correspondences it is tested against have |V'| <= vb and |Q'| <= Qb.  Mh: the largest single term of the 48-term
// dot product; Sl: the sum of the absolute values of the 15 split terms; S: the sum of all |terms|.  (Derivation: score_gram_kernel.)
__host__ __device__ inline double gram_eps(double F, double m, double Tn, double g, double Pn, double Qb, double vb, double st) {
  const double t1 = 2.0 * (m + 1.5 * g) * Qb * Pn, t2 = vb * vb, t3 = 2.0 * F * Tn * Pn, t4 = 2.0 * Tn * vb, t5 = Tn * Tn + 1.5 * st * st;
  double Mh = t1;
  Mh = t2 > Mh ? t2 : Mh; Mh = t3 > Mh ? t3 : Mh; Mh = t4 > Mh ? t4 : Mh; Mh = t5 > Mh ? t5 : Mh;
  Mh *= 1.05;
  const double Sl = 2.0 * (F + 4.5 * g) * Qb * Pn + t3 + t4, S = Sl + t2 + t5;
  return GX_ACC * Mh + GX_Q * Sl + GX_NORM * t2 + 1e-8 * S + 3.0 * g * vb * Pn + 1e-4;
}
// the same with the SUM of the terms in place of their maximum: an upper bound of gram_eps that is a quadratic in vb with positive
// coefficients (gram_coef_block: a shell made for |V'| <= vb_h is safe beyond vb_h if this stays under 0.1 tau'^2)
__host__ __device__ inline double gram_eps_sum(double F, double m, double Tn, double g, double Pn, double Qb, double vb, double st) {
  const double t1 = 2.0 * (m + 1.5 * g) * Qb * Pn, t2 = vb * vb, t3 = 2.0 * F * Tn * Pn, t4 = 2.0 * Tn * vb, t5 = Tn * Tn + 1.5 * st * st;
  const double Sl = 2.0 * (F + 4.5 * g) * Qb * Pn + t3 + t4, S = Sl + t2 + t5;
  return GX_ACC * 1.05 * (t1 + t2 + t3 + t4 + t5) + GX_Q * Sl + GX_NORM * t2 + 1e-8 * S + 3.0 * g * vb * Pn + 1e-4;
}

// a launch that takes its dispatch packet's own start / stop timestamps only when asked to (SC_FLAG_TIMING_HOT): without events it is
// a plain launch
#define SC_LAUNCH_EV(kernel, grid, block, st, e0, e1, ...)                                              \
  do {                                                                                                  \
    if ((e0) != nullptr || (e1) != nullptr) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, e0, e1, 0, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);                                   \
  } while (0)
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr float FX_RS = 1024.0f;
constexpr int FX_UNIT = 256;    // correspondences per staging unit (8 MFMA steps); LDS holds two
constexpr int FX_WIN = 1024;    // correspondences per window: 32 steps, one 32-bit shift register per test
constexpr int FX_NQ = 256;      // global sub-queues (one ticket counter for ~6000 waves costs ~50 us of same-address atomics)
constexpr int FX_QL = 256;      // LDS queue entries per wave
constexpr int FX_WAVES = 4;     // waves per workgroup, 8 hypotheses each
struct FilterInfo { float s, pmax, qmax, pad; };
constexpr size_t FX_INFO_BYTES = 512;

struct FilterState {  // device view of the state buffer (filter_plan().state_bytes)
  FilterInfo* info;   // written by the tile kernel
  uint32_t* qcount;   // FX_NQ ticket counters, one per 128-byte line
  uint32_t* redo;     // bit (split * n_waves + wave): X recounts the wave's 8 hypotheses over the split exactly
  uint2* queue;       // FX_NQ sub-queues of cap_sq entries {correspondence, wave << 5 | lane half << 4 | tests}
  uint32_t cap_sq;
  uint32_t zero_words;  // counters + bitmap, cleared by the tile kernel
};
inline FilterState filter_state(void* state, const FilterPlan& fp) {
  FilterState f;
  unsigned char* p = static_cast<unsigned char*>(state);
  f.info = reinterpret_cast<FilterInfo*>(p); p += FX_INFO_BYTES;
  f.qcount = reinterpret_cast<uint32_t*>(p); p += (size_t)FX_NQ * 128;
  f.redo = reinterpret_cast<uint32_t*>(p);
  const size_t bm_words = ((size_t)fp.splits * fp.n_waves + 31) / 32;
  p += (bm_words * 4 + 127) / 128 * 128;
  f.queue = reinterpret_cast<uint2*>(p);
  f.cap_sq = fp.queue_cap / FX_NQ;
  f.zero_words = (uint32_t)(FX_NQ * 32 + bm_words);
  return f;
}

}  // namespace sc
