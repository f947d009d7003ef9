// sc_sync.hip — the kernels of sc_pairs_sync (include/saccot.h): the absolute poses of a pair list's sets by anchored Jacobi
// averaging.  max_rounds + 2 launches on data the host staged once (sc_cycles_check.hpp's image: the records, the sorted
// neighbour entries, and the list starts behind them):
//
//   prepare   a thread per pair: the prologue every pair-list entry shares (sc_pose64.hpp: the record's validity, its status, the
//             pose widened ONCE into the two oriented fp64 transforms), use and weight — one double a pair, 0.0 where the pair is
//             not usable;
//             a thread per set: X_0 and known_0 in buffer 0, and the set's tallies cleared.
//   round k   a WAVE per set.  The header's sum has 64 slots and entry i adds into slot i mod 64: a lane IS a slot, and takes
//             entries lane, lane + 64, ... of the set's sorted list in that order.  For a live entry it loads the neighbour's state
//             and the oriented pose, composes them and adds.  The fold "slot[j] += slot[j + h], h = 32 .. 1" is a butterfly of
//             xor shuffles: lane j adds lane j ^ h's value, which for j < h is the header's sum and for the others the same two
//             numbers the other way round — a rounded sum does not depend on the order of its two operands —, so every lane ends
//             with slot 0 and rot(M) runs wave-uniform, no broadcast and no LDS.  Nothing is fused: the library is built with
//             -ffp-contract=off and this file says so again.  The state is double-buffered (buffer k & 1 holds X_k): a round reads
//             one and writes every set of the other.
//             The stop is the device's: changed[k] counts what round k changed, and the launch of round k + 1 returns at once when
//             that word is 0 — as does every launch behind it, which then finds its own predecessor's word still 0.
//   finish    K from the round words; a thread per set: its record; a thread per pair: its residual; the workgroup that finishes
//             last: the summary.
#include <cstddef>

#include "sc_arith.hpp"
#include "sc_kernels.hpp"
#include "sc_pose64.hpp"
#include "sc_rot.hpp"
#include "sc_sync_check.hpp"

#pragma clang fp contract(off)

namespace sc {

static_assert(sizeof(SyncSetRecord) == sizeof(sc_sync_set) && sizeof(SyncSetRecord) == 160 && offsetof(SyncSetRecord, status) == offsetof(sc_sync_set, status) &&
              offsetof(SyncSetRecord, status) == 48 && offsetof(SyncSetRecord, known_round) == offsetof(sc_sync_set, known_round) &&
              offsetof(SyncSetRecord, used) == offsetof(sc_sync_set, used) && offsetof(SyncSetRecord, degenerate) == offsetof(sc_sync_set, degenerate) &&
              offsetof(SyncSetRecord, X) == offsetof(sc_sync_set, X) && offsetof(SyncSetRecord, X) == 64, "SyncSetRecord is sc_sync_set, 160 bytes");
static_assert(sizeof(SyncPairRecord) == sizeof(sc_sync_pair) && sizeof(SyncPairRecord) == 32 && offsetof(SyncPairRecord, used) == offsetof(sc_sync_pair, used) &&
              offsetof(SyncPairRecord, r2) == offsetof(sc_sync_pair, r2) && offsetof(SyncPairRecord, r2) == 8 &&
              offsetof(SyncPairRecord, e2) == offsetof(sc_sync_pair, e2) && offsetof(SyncPairRecord, reserved) == offsetof(sc_sync_pair, reserved),
              "SyncPairRecord is sc_sync_pair, 32 bytes");
static_assert(sizeof(SyncSummary) == sizeof(sc_sync_summary) && sizeof(SyncSummary) == 32 && offsetof(SyncSummary, changed_last) == offsetof(sc_sync_summary, changed_last),
              "SyncSummary is sc_sync_summary, 32 bytes");
static_assert(sizeof(SyncCtl) <= SYNC_CTL_BYTES && SYNC_ROUNDS_MAX == 256, "the round words fit their area: changed[1 .. 256]");
static_assert(sizeof(SyncState) == SYNC_STATE_BYTES && sizeof(SyncInfo) == SYNC_INFO_BYTES, "a set's state is 104 bytes, its tallies 16");

namespace {

constexpr int ST = 256;            // threads of a workgroup of every launch: four waves, a set each in a round
constexpr int SYNC_BLOCKS = 2048;  // a round's grid at most: 8192 waves, the sets dealt round-robin to them

__global__ __launch_bounds__(ST) void sync_prepare_kernel(const SyncJob job) {
  const uint32_t i = blockIdx.x * ST + threadIdx.x;
  if (i < job.n_pairs) {
    const uint32_t p = i;
    bool edge;
    const int status = pair_prologue(job.pose, job.pose_stride, job.status, job.rec, job.wide, p, &edge);
    const bool use = pair_use(job.use, job.use_stride, p);
    const double wt = job.weight ? (double)job.weight[p] : 1.0;
    job.wt[p] = (edge && use && wt > 0.0 && wt < __builtin_inf()) ? wt : 0.0;  // (a NaN is neither)
    job.pair[p].status = status;  // (the rest of the record is finish's)
  }
  if (i < job.n_sets) {
    const bool anchor = i == job.anchor;
    SyncState s{};
    if (anchor) { s.X[0] = 1.0; s.X[4] = 1.0; s.X[8] = 1.0; s.known = 1; }
    job.state[i] = s;  // X_0, known_0 (buffer 1 is written whole by round 1)
    job.info[i] = SyncInfo{};
  }
}

__global__ __launch_bounds__(ST) void sync_round_kernel(const SyncJob job, const uint32_t round) {
  if (round > 1 && job.ctl->changed[round - 1] == 0) return;  // no set changed a round ago
  const uint32_t n = job.n_sets;
  const SyncState* const __restrict__ prev = job.state + (size_t)((round - 1) & 1) * n;
  SyncState* const __restrict__ cur = job.state + (size_t)(round & 1) * n;
  const uint64_t* const __restrict__ ent = job.entries;
  const int lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (ST / 64);
  for (uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * (ST / 64) + (threadIdx.x >> 6)); s < n; s += waves) {
    const SyncState mine = prev[s];
    if (s == job.anchor) {  // never recomputed
      if (lane == 0) cur[s] = mine;
      continue;
    }
    const uint32_t begin = job.off[s], end = job.off[s + 1];
    double acc[12], accW = 0.0;
#pragma unroll
    for (int c = 0; c < 12; c++) acc[c] = 0.0;
    uint32_t live = 0;
    for (uint32_t i = begin + lane; i < end; i += 64) {  // slot `lane`: entries lane, lane + 64, ... in this order
      const uint64_t e = ent[i];
      const uint32_t nb = cycles_entry_set(e), p = cycles_entry_pair(e);
      const double w = job.wt[p];
      if (!(w > 0.0) || !prev[nb].known) continue;
      // T_p(s -> nb): lower -> higher at 0, higher -> lower at 12
      const T64 P = compose_t64(load_t64(prev[nb].X), load_t64(job.wide + (size_t)24 * p + (s < nb ? 0 : 12)));
#pragma unroll
      for (int c = 0; c < 9; c++) acc[c] = acc[c] + w * P.R[c];
#pragma unroll
      for (int c = 0; c < 3; c++) acc[9 + c] = acc[9 + c] + w * P.t[c];
      accW = accW + w;
      live++;
    }
    live = wave_sum_u32(live);
    bool fin = false, fresh = false, moved = false;
    double X[12];
    if (live) {  // (wave-uniform)
#pragma unroll
      for (int h = 32; h > 0; h >>= 1) {
#pragma unroll
        for (int c = 0; c < 12; c++) acc[c] = acc[c] + __shfl_xor(acc[c], h);
        accW = accW + __shfl_xor(accW, h);
      }
      double M[9], R[9];
#pragma unroll
      for (int c = 0; c < 9; c++) M[c] = acc[c];
      rot_plain(M, R);
      fin = true;
#pragma unroll
      for (int c = 0; c < 9; c++) { X[c] = R[c]; fin = fin && finite64(R[c]); }
#pragma unroll
      for (int c = 0; c < 3; c++) { X[9 + c] = acc[9 + c] / accW; fin = fin && finite64(X[9 + c]); }
      if (fin) {
        double dR2 = 0.0, dt2 = 0.0;
#pragma unroll
        for (int c = 0; c < 9; c++) { const double d = X[c] - mine.X[c]; dR2 = c ? dR2 + d * d : d * d; }
#pragma unroll
        for (int c = 0; c < 3; c++) { const double d = X[9 + c] - mine.X[9 + c]; dt2 = c ? dt2 + d * d : d * d; }
        fresh = !mine.known;
        moved = fresh || dR2 > job.r2_max || dt2 > job.e2_max;
      }
    }
    if (lane == 0) {
      SyncState out = mine;  // no live entry, or no finite pose: unchanged
      if (fin) {
#pragma unroll
        for (int c = 0; c < 12; c++) out.X[c] = X[c];
        out.known = 1;
      }
      cur[s] = out;
      SyncInfo* const info = job.info + s;
      info->used = live;
      if (live && !fin) info->degenerate = info->degenerate + 1;
      if (fresh) info->known_round = round;
      if (moved) atomicAdd(&job.ctl->changed[round], 1u);
    }
  }
}

__global__ __launch_bounds__(ST) void sync_finish_kernel(const SyncJob job) {
  __shared__ uint32_t sh_K, sh_known, sh_used;
  if (threadIdx.x == 0) {
    uint32_t K = job.max_rounds;
    for (uint32_t k = 1; k <= job.max_rounds; k++)
      if (job.ctl->changed[k] == 0) { K = k; break; }
    sh_K = K; sh_known = 0; sh_used = 0;
  }
  __syncthreads();
  const uint32_t K = sh_K;
  const SyncState* const __restrict__ fin = job.state + (size_t)(K & 1) * job.n_sets;
  const uint32_t i = blockIdx.x * ST + threadIdx.x;
  bool known = false, used = false;
  if (i < job.n_sets) {
    const SyncState s = fin[i];  // (a set never reached still holds X_0: zeros)
    const SyncInfo info = job.info[i];
    known = s.known != 0;
    SyncSetRecord out;
#pragma unroll
    for (int c = 0; c < 12; c++) { out.Rt[c] = (float)s.X[c]; out.X[c] = s.X[c]; }
    out.status = known ? SC_OK : SC_ENOHYP;
    out.known_round = info.known_round; out.used = i == job.anchor ? 0u : info.used; out.degenerate = info.degenerate;
    job.set[i] = out;
  }
  if (i < job.n_pairs) {
    const uint32_t* const r = job.rec + (size_t)CYCLES_REC_WORDS * i;
    const StoredPair sp = stored_pair(r);
    double r2 = 0.0, e2 = 0.0;
    used = job.wt[i] > 0.0 && fin[sp.a].known && fin[sp.b].known;
    if (used) {
      const T64 A = load_t64(fin[sp.a].X);
      const T64 Q = compose_t64(load_t64(fin[sp.b].X), load_t64(job.wide + (size_t)24 * i + (sp.fwd ? 0 : 12)));  // the record itself
#pragma unroll
      for (int c = 0; c < 9; c++) { const double d = A.R[c] - Q.R[c]; r2 = c ? r2 + d * d : d * d; }
#pragma unroll
      for (int c = 0; c < 3; c++) { const double d = A.t[c] - Q.t[c]; e2 = c ? e2 + d * d : d * d; }
    }
    SyncPairRecord* const out = job.pair + i;  // (status: prepare's)
    out->used = used ? 1u : 0u; out->r2 = r2; out->e2 = e2; out->reserved[0] = 0; out->reserved[1] = 0;
  }
  // the tallies: a word per wave into the workgroup's, a word per workgroup into the call's, and the last workgroup to hand its
  // in writes the summary (every access to the three words is a device-scope atomic: nothing depends on where a workgroup runs)
  const uint32_t n_known = (uint32_t)__popcll(__ballot(known)), n_used = (uint32_t)__popcll(__ballot(used));
  if ((threadIdx.x & 63) == 0) {
    if (n_known) atomicAdd(&sh_known, n_known);
    if (n_used) atomicAdd(&sh_used, n_used);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    SyncCtl* const ctl = job.ctl;
    if (sh_known) atomicAdd(&ctl->known, sh_known);
    if (sh_used) atomicAdd(&ctl->used, sh_used);
    __threadfence();
    if (atomicAdd(&ctl->done, 1u) == gridDim.x - 1) {
      __threadfence();
      SyncSummary s{};
      s.rounds = K; s.changed_last = ctl->changed[K]; s.converged = s.changed_last == 0 ? 1u : 0u;
      s.known = atomicAdd(&ctl->known, 0u); s.used = atomicAdd(&ctl->used, 0u);
      *job.sum = s;
    }
  }
}

}  // namespace

void launch_pairs_sync(const SyncJob& job, hipStream_t st) {
  const uint32_t most = job.n_pairs > job.n_sets ? job.n_pairs : job.n_sets, flat = (most + ST - 1) / ST;
  hipLaunchKernelGGL(sync_prepare_kernel, dim3(flat), dim3(ST), 0, st, job);
  const uint32_t per = ST / 64, want = (job.n_sets + per - 1) / per, blocks = want < (uint32_t)SYNC_BLOCKS ? want : (uint32_t)SYNC_BLOCKS;
  for (uint32_t k = 1; k <= job.max_rounds; k++) hipLaunchKernelGGL(sync_round_kernel, dim3(blocks), dim3(ST), 0, st, job, k);
  hipLaunchKernelGGL(sync_finish_kernel, dim3(flat), dim3(ST), 0, st, job);
}

}  // namespace sc
