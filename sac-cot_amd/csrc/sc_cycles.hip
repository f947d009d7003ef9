// sc_cycles.hip — the kernels of sc_pairs_cycles (include/saccot.h): loop consistency of a pair list's poses, and the pruning of
// the list to a fixed point.  max_rounds + 2 launches on data the host staged once (sc_cycles_check.hpp: a record per pair, every
// set's neighbour entries sorted by (neighbour, pair)):
//
//   prepare   a thread per pair: the prologue every pair-list entry shares (sc_pose64.hpp: the record's validity, its status, the
//             pose widened ONCE into two oriented fp64 transforms), alive_0, and the head of the pair's output record.
//   round k   a WAVE per pair that is in alive_{k-1}.  The pair sits on {lo, hi}; a loop of three closes through every set z that
//             is a neighbour of both.  The lanes take the entries of the SHORTER of the two lists, one each, and look the entry's
//             set up in the longer list by binary search: a list longer than a workgroup (a hub) costs its pairs a logarithm, not a
//             sweep, and nothing is tiled through LDS.  A run of equal neighbours in the longer list is the repeated pairs: the lane
//             walks it, so every combination is a triangle of its own.  Each hit whose two other pairs are in alive_{k-1} is
//             composed in the header's order — nothing fused: the library is built with -ffp-contract=off and this file says so
//             again — and tested.  The tallies are integers and the extrema are taken in a total order, so the wave's reduction is
//             order-free.  The triangle is recomputed by each of its three pairs and in every round: the workspace stays O(pairs).
//             Round 1 is also the pass over alive_0 that leaves cycles, ok, min_trace and max_e2.
//             The stop is the device's: dropped[k] counts what round k dropped, and the launch of round k + 1 returns at once when
//             that word is 0 — as does every launch behind it, which then finds its own predecessor's word still 0.
//   finish    one thread: K, stable and the counts into the summary.
//
// The alive bytes are double-buffered (buffer k & 1 holds alive_k): a round reads one and writes every byte of the other.
#include <cstddef>

#include "sc_arith.hpp"
#include "sc_cycles_check.hpp"
#include "sc_kernels.hpp"
#include "sc_pose64.hpp"

#pragma clang fp contract(off)

namespace sc {

static_assert(sizeof(CycleRecord) == sizeof(sc_cycle_result) && sizeof(CycleRecord) == 48, "CycleRecord is sc_cycle_result, 48 bytes");
static_assert(offsetof(CycleRecord, status) == offsetof(sc_cycle_result, status) && offsetof(CycleRecord, cycles) == offsetof(sc_cycle_result, cycles) &&
              offsetof(CycleRecord, ok) == offsetof(sc_cycle_result, ok) && offsetof(CycleRecord, ok_alive) == offsetof(sc_cycle_result, ok_alive) &&
              offsetof(CycleRecord, alive) == offsetof(sc_cycle_result, alive) && offsetof(CycleRecord, dropped_round) == offsetof(sc_cycle_result, dropped_round) &&
              offsetof(CycleRecord, min_trace) == offsetof(sc_cycle_result, min_trace) && offsetof(CycleRecord, min_trace) == 24 &&
              offsetof(CycleRecord, max_e2) == offsetof(sc_cycle_result, max_e2) && offsetof(CycleRecord, max_e2) == 32 &&
              offsetof(CycleRecord, reserved) == offsetof(sc_cycle_result, reserved), "CycleRecord's fields sit where sc_cycle_result's do");
static_assert(sizeof(CycleSummary) == sizeof(sc_cycle_summary) && sizeof(CycleSummary) == 32 &&
              offsetof(CycleSummary, triangles) == offsetof(sc_cycle_summary, triangles) && offsetof(CycleSummary, consistent) == offsetof(sc_cycle_summary, consistent),
              "CycleSummary is sc_cycle_summary, 32 bytes");
static_assert(sizeof(CyclesCtl) <= CYCLES_CTL_BYTES && CYCLES_ROUNDS_MAX == 64, "the round words fit their area: dropped[1 .. 64]");
static_assert(CYCLES_POSE_BYTES == 2 * 12 * sizeof(double), "two transforms of 12 doubles a pair");

namespace {

constexpr int CT = 256;           // threads of a workgroup of either launch: four waves, a pair each in a round
constexpr int CYCLES_BLOCKS = 2048;  // a round's grid at most: eight workgroups a CU, the pairs dealt round-robin to the waves

// tr and e2 of E = C o M: the diagonal of E.R and E.t are all a test reads, and each is the full composition's entry
__device__ __forceinline__ void loop_error(const T64& C, const T64& M, double* tr, double* e2) {
  double d[3], t[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    d[i] = ((C.R[3 * i] * M.R[i] + C.R[3 * i + 1] * M.R[3 + i]) + C.R[3 * i + 2] * M.R[6 + i]);
    t[i] = ((C.R[3 * i] * M.t[0] + C.R[3 * i + 1] * M.t[1]) + C.R[3 * i + 2] * M.t[2]) + C.t[i];
  }
  *tr = (d[0] + d[1]) + d[2];
  *e2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
}

// A double as a key whose unsigned order is the numbers' order, -0 below +0: the extrema of a wave do not depend on who met whom.
__device__ __forceinline__ uint64_t order_key(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double order_value(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}
constexpr uint64_t KEY_MAX = ~0ull;  // above every double's key: "no triangle yet" of a minimum
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint64_t u = __shfl_xor(v, o); v = u < v ? u : v; }
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint64_t u = __shfl_xor(v, o); v = u > v ? u : v; }
  return v;
}

__global__ __launch_bounds__(CT) void cycles_prepare_kernel(const CyclesJob job) {
  const uint32_t p = blockIdx.x * CT + threadIdx.x;
  bool edge = false;
  if (p < job.n_pairs) {
    const int status = pair_prologue(job.pose, job.pose_stride, job.status, job.rec, job.wide, p, &edge);
    job.alive[p] = edge ? 1 : 0;  // alive_0 (buffer 1 is written whole by round 1)
    CycleRecord out{};
    out.status = status;
    out.alive = edge ? 1u : 0u;
    out.min_trace = 3.0;
    job.res[p] = out;
  }
  const uint32_t n_edges = (uint32_t)__popcll(__ballot(edge));
  if ((threadIdx.x & 63) == 0 && n_edges) atomicAdd(&job.ctl->edges, n_edges);
}

__global__ __launch_bounds__(CT) void cycles_round_kernel(const CyclesJob job, const uint32_t round) {
  if (round > 1 && job.ctl->dropped[round - 1] == 0) return;  // the list was stable a round ago
  const uint32_t n = job.n_pairs;
  const uint8_t* const __restrict__ prev = job.alive + (size_t)((round - 1) & 1) * n;
  uint8_t* const __restrict__ cur = job.alive + (size_t)(round & 1) * n;
  const uint64_t* const __restrict__ ent = job.entries;
  const int lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (CT / 64);
  for (uint32_t p = __builtin_amdgcn_readfirstlane(blockIdx.x * (CT / 64) + (threadIdx.x >> 6)); p < n; p += waves) {
    if (!prev[p]) {  // dead, or never an edge: it stays out, and what it closed a round ago no longer counts
      if (lane == 0) { cur[p] = 0; job.res[p].ok_alive = 0; }
      continue;
    }
    const uint32_t* const r = job.rec + (size_t)CYCLES_REC_WORDS * p;
    const uint32_t lo = r[CW_LO], hi = r[CW_HI];
    const uint32_t lo_n = r[CW_LO_END] - r[CW_LO_BEGIN], hi_n = r[CW_HI_END] - r[CW_HI_BEGIN];
    const bool lo_short = lo_n <= hi_n;  // the lanes take the shorter list
    const uint32_t s_begin = lo_short ? r[CW_LO_BEGIN] : r[CW_HI_BEGIN], s_n = lo_short ? lo_n : hi_n;
    const uint32_t l_begin = lo_short ? r[CW_HI_BEGIN] : r[CW_LO_BEGIN], l_end = l_begin + (lo_short ? hi_n : lo_n);
    uint32_t cnt = 0, okc = 0, tri = 0, tri_ok = 0;
    uint64_t kmin = KEY_MAX, kmax = order_key(0.0);
    for (uint32_t i = lane; i < s_n; i += 64) {
      const uint64_t es = ent[s_begin + i];
      const uint32_t z = cycles_entry_set(es);
      if (!prev[cycles_entry_pair(es)]) continue;
      // the first entry of the longer list whose set is not below z (the other end of the pair itself is in neither list's run)
      uint32_t a = l_begin, b = l_end;
      while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (cycles_entry_set(ent[m]) < z) a = m + 1; else b = m;
      }
      for (; a < l_end; a++) {
        const uint64_t el = ent[a];
        if (cycles_entry_set(el) != z) break;
        if (!prev[cycles_entry_pair(el)]) continue;
        // e1: the pair on {lo, z}; e2: the pair on {hi, z}.  Each pair's transforms: lower -> higher at 0, higher -> lower at 12.
        const double* const w1 = job.wide + (size_t)24 * cycles_entry_pair(lo_short ? es : el);
        const double* const w2 = job.wide + (size_t)24 * cycles_entry_pair(lo_short ? el : es);
        const double* const wp = job.wide + (size_t)24 * p;
        const double *P, *Q, *C;  // E = C o (Q o P) over the three sets in ascending order
        if (z < lo)      { P = w1; Q = wp; C = w2 + 12; }  // z < lo < hi: z -> lo, lo -> hi, hi -> z
        else if (z < hi) { P = w1; Q = w2; C = wp + 12; }  // lo < z < hi: lo -> z, z -> hi, hi -> lo
        else             { P = wp; Q = w2; C = w1 + 12; }  // lo < hi < z: lo -> hi, hi -> z, z -> lo
        double tr, e2;
        loop_error(load_t64(C), compose_t64(load_t64(Q), load_t64(P)), &tr, &e2);
        const bool good = tr >= job.tr_min && e2 <= job.e2_max;
        cnt++; okc += good ? 1u : 0u;
        if (z > hi) { tri++; tri_ok += good ? 1u : 0u; }  // the summary counts a triangle where its pair on the two lowest sets meets it
        const uint64_t kt = order_key(tr), ke = order_key(e2);
        kmin = kt < kmin ? kt : kmin;
        kmax = ke > kmax ? ke : kmax;
      }
    }
    cnt = wave_sum_u32(cnt); okc = wave_sum_u32(okc);
    if (round == 1) {
      tri = wave_sum_u32(tri); tri_ok = wave_sum_u32(tri_ok);
      kmin = wave_min_u64(kmin); kmax = wave_max_u64(kmax);
    }
    if (lane == 0) {
      CycleRecord* const out = job.res + p;
      const bool stays = okc >= job.min_ok || (job.keep && job.keep[p] != 0);
      cur[p] = stays ? 1 : 0;
      out->ok_alive = okc;
      if (round == 1) {
        out->cycles = cnt; out->ok = okc;
        out->min_trace = cnt ? order_value(kmin) : 3.0;
        out->max_e2 = order_value(kmax);
        if (tri) atomicAdd(reinterpret_cast<unsigned long long*>(&job.ctl->triangles), (unsigned long long)tri);
        if (tri_ok) atomicAdd(reinterpret_cast<unsigned long long*>(&job.ctl->consistent), (unsigned long long)tri_ok);
      }
      if (!stays) {
        out->alive = 0; out->dropped_round = round;
        atomicAdd(&job.ctl->dropped[round], 1u);
      }
    }
  }
}

__global__ void cycles_finish_kernel(const CyclesJob job) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const CyclesCtl* const ctl = job.ctl;
  uint32_t K = job.max_rounds, stable = 0, gone = 0;
  for (uint32_t k = 1; k <= job.max_rounds; k++) {
    if (ctl->dropped[k] == 0) { K = k; stable = 1; break; }
    gone += ctl->dropped[k];
  }
  CycleSummary s;
  s.rounds = K; s.stable = stable; s.alive = ctl->edges - gone; s.edges = ctl->edges;
  s.triangles = ctl->triangles; s.consistent = ctl->consistent;
  *job.sum = s;
}

}  // namespace

void launch_pairs_cycles(const CyclesJob& job, hipStream_t st) {
  const uint32_t n = job.n_pairs;
  hipLaunchKernelGGL(cycles_prepare_kernel, dim3((n + CT - 1) / CT), dim3(CT), 0, st, job);
  const uint32_t per = CT / 64, want = (n + per - 1) / per, blocks = want < (uint32_t)CYCLES_BLOCKS ? want : (uint32_t)CYCLES_BLOCKS;
  for (uint32_t k = 1; k <= job.max_rounds; k++) hipLaunchKernelGGL(cycles_round_kernel, dim3(blocks), dim3(CT), 0, st, job, k);
  hipLaunchKernelGGL(cycles_finish_kernel, dim3(1), dim3(64), 0, st, job);
}

}  // namespace sc
