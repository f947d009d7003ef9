// sc_tri.hip — stage B, the enumeration: per-edge triangle counts and per-triangle keys, by rows or by the event list; then
// selection and hand-over: radix select, compaction, the sharded candidate exchange, decode, ranked order (sc_tri.hpp: the pipeline).
#include "sc_tri.hpp"
#include "sc_gramref.hpp"

namespace sc {

// ------------------------------------------------------------------------------------------------
// 2. tri_count: 16 lanes per edge
// ------------------------------------------------------------------------------------------------
// lanes per edge: Tuning::tg_count / tg_keys / tg_sample (4|8|16|32|64); 8 measured best on C2

constexpr int TK_MAX_BLOCKS = 4096;  // bounds the per-block min/max arrays

// mbits: the bit matrix that decides MEMBERSHIP (the full adjacency, or the pruned "strong" upper-triangle matrix);
// smin != nullptr: edges with es[e] < *smin are outside the pruned graph and count 0 without touching any row.
// EB edges per group are processed together: every dependent memory level (edge record -> rows -> ...) is then paid
// once per batch instead of once per edge.  These kernels are latency-bound (PMC: > 60 % of wave cycles waiting), so
// the batch is worth ~EB in time until the L2 request queues fill.
constexpr int EB = 4;

template <int TG>
__global__ __launch_bounds__(256) void tri_count_kernel(const uint64_t* __restrict__ mbits, int W,
                                                        const uint32_t* __restrict__ ei,
                                                        const uint32_t* __restrict__ ej,
                                                        const float* __restrict__ es,
                                                        const float* __restrict__ smin, uint64_t E,
                                                        uint32_t* __restrict__ tcnt,
                                                        const uint64_t* __restrict__ own) {
  // own (optional): [lo, hi) of the edges this rank enumerates (sharded stage B); the others count 0
  const int gl = threadIdx.x & (TG - 1);
  const float s_floor = smin ? *smin : -1.0f;
  const uint64_t own_lo = own ? own[0] : 0ull, own_hi = own ? own[1] : E;
  const uint64_t groups = (uint64_t)gridDim.x * (256 / TG);
  const uint64_t g0 = (uint64_t)blockIdx.x * (256 / TG) + (threadIdx.x / TG);
  for (uint64_t e0 = g0 * EB; e0 < E; e0 += groups * EB) {  // a group owns EB consecutive edges per trip
    uint32_t rowi[EB], rowj[EB], c[EB];
    int w0[EB], jb[EB];
    bool on[EB];
#pragma unroll
    for (int q = 0; q < EB; q++) {  // level 1: the edge records of the whole batch
      const uint64_t e = e0 + q;
      on[q] = e < E;
      const uint64_t ec = on[q] ? e : 0;
      const float s = es[ec];
      const uint32_t i = ei[ec], j = ej[ec];
      on[q] = on[q] && (s >= s_floor) && e >= own_lo && e < own_hi;
      rowi[q] = i * (uint32_t)W; rowj[q] = j * (uint32_t)W;
      w0[q] = (int)(j >> 6); jb[q] = (int)(j & 63);
      c[q] = 0;
    }
    int wmin = W;
#pragma unroll
    for (int q = 0; q < EB; q++) wmin = on[q] ? min(wmin, w0[q]) : wmin;
    for (int wb = wmin; wb < W; wb += TG) {  // level 2..: one round of words for all EB edges at a time
      const int w = wb + gl;
      uint64_t a[EB], bq[EB];
#pragma unroll
      for (int q = 0; q < EB; q++) {
        const bool live = on[q] && w >= w0[q] && w < W;
        a[q] = live ? mbits[rowi[q] + w] : 0ull;
        bq[q] = live ? mbits[rowj[q] + w] : 0ull;
      }
#pragma unroll
      for (int q = 0; q < EB; q++) {
        uint64_t m = a[q] & bq[q];
        if (w == w0[q]) m &= mask_above(jb[q]);
        c[q] += (uint32_t)__popcll(m);
      }
    }
#pragma unroll
    for (int q = 0; q < EB; q++) {
#pragma unroll
      for (int o = TG / 2; o > 0; o >>= 1) c[q] += __shfl_xor(c[q], o, TG);
      if (gl == 0 && e0 + q < E) tcnt[e0 + q] = c[q];
    }
  }
}

void launch_tri_count(const Graph& g, const Pruned& pr, const EdgeList& el, const EdgeCounts& ec, const Tuning& tn, hipStream_t st) {
  if (el.E == 0) return;
  const int tg = tn.tg_count;
  const uint64_t per = (uint64_t)(256 / tg) * EB;
  uint64_t nb = (el.E + per - 1) / per;
  if (nb > 4096) nb = 4096;
  with_lanes<16, 4, 8, 32>(tg, [&](auto lanes) {  // (no 64-lane form)
    hipLaunchKernelGGL(tri_count_kernel<decltype(lanes)::value>, dim3((unsigned)nb), dim3(256), 0, st, member_bits(g, pr), g.W,
                       el.ei, el.ej, el.es, pr.smin, el.E, ec.tcnt, ec.own);
  });
}

// ------------------------------------------------------------------------------------------------
// 3. tri_keys
// ------------------------------------------------------------------------------------------------

// bits / wpre / ebase: full adjacency + its word-prefix popcounts + per-row CSR bases: the index of edge (v,k) in the
// edge arrays is ebase[v] + wpre[v][k/64] + popc(bits[v][k/64] & below k) — an O(1) lookup, no running prefix.
// mbits: membership matrix (== bits when nothing is pruned); smin: strong-edge threshold or nullptr.
// Per round only the member words are ANDed; the one remaining group scan (triangle rank inside the edge, for the
// ordinal) is skipped when the whole group found nothing — the common case in the pruned graph.
template <int TG>
__global__ __launch_bounds__(256) void tri_keys_kernel(const uint64_t* __restrict__ bits,
                                                       const uint64_t* __restrict__ mbits,
                                                       const float* __restrict__ smin, int W,
                                                       const uint32_t* __restrict__ deg,
                                                       const uint32_t* __restrict__ wpre,
                                                       const uint32_t* __restrict__ ebase,
                                                       const uint32_t* __restrict__ ei,
                                                       const uint32_t* __restrict__ ej,
                                                       const float* __restrict__ es,
                                                       const uint64_t* __restrict__ toff, uint64_t E,
                                                       int rank_mode, uint32_t* __restrict__ wkey,
                                                       uint2* __restrict__ kcol,
                                                       uint32_t* __restrict__ blk_min,
                                                       uint32_t* __restrict__ blk_max,
                                                       const uint64_t* __restrict__ own) {
  const int gl = threadIdx.x & (TG - 1);
  const uint64_t own_lo = own ? own[0] : 0ull, own_hi = own ? own[1] : E;
  const uint64_t gmask = (TG == 64) ? ~0ull : (((1ull << TG) - 1ull) << ((threadIdx.x & 63) & ~(TG - 1)));
  uint32_t kmin = 0xFFFFFFFFu, kmax = 0;
  const uint64_t groups = (uint64_t)gridDim.x * (256 / TG);
  const bool pruned = (mbits != bits);
  const float s_floor = smin ? *smin : -1.0f;
  for (uint64_t e = (uint64_t)blockIdx.x * (256 / TG) + (threadIdx.x / TG); e < E; e += groups) {
    const float s_ij = es[e];
    if (s_ij < s_floor || e < own_lo || e >= own_hi) continue;  // group-uniform: outside the pruned graph / not this rank's
    const uint32_t i = ei[e], j = ej[e];
    const uint32_t rowi = i * (uint32_t)W, rowj = j * (uint32_t)W;  // word offsets: n * W < 2^32
    const int w0 = j >> 6;
    const uint32_t dsum_ij = (rank_mode == 0) ? 0u : deg[i] + deg[j];
    const uint32_t ebi = ebase[i], ebj = ebase[j];
    uint32_t out = (uint32_t)0;  // triangle rank inside the edge
    const uint64_t out0 = toff[e];
    const int rounds = (W - w0 + TG - 1) / TG;
    for (int it = 0; it < rounds; it++) {
      const int w = w0 + it * TG + gl;
      uint64_t m = 0;
      if (w < W) {
        m = mbits[rowi + w] & mbits[rowj + w];
        if (w == w0) m &= mask_above(j & 63);
      }
      const uint64_t any = __ballot(m != 0) & gmask;
      if (any == 0) continue;  // group-uniform
      uint32_t tm;
      uint32_t pm = out + group_exscan<TG>((uint32_t)__popcll(m), &tm);
      out += tm;
      if (m) {
        // full-row words and prefixes only where a triangle was found
        const uint64_t ai = pruned ? bits[rowi + w] : 0ull, aj = pruned ? bits[rowj + w] : 0ull;
        const uint64_t fi = pruned ? ai : mbits[rowi + w], fj = pruned ? aj : mbits[rowj + w];
        const uint32_t pi = ebi + wpre[rowi + w], pj = ebj + wpre[rowj + w];
        while (m) {
          int b[4];
          const int nbits = pop4(m, b);
          uint32_t key[4];
          if (rank_mode == 0) {
            float s_ik[4], s_jk[4];
            tri_weights4(es, b, nbits, {pi, fi}, {pj, fj}, s_ik, s_jk);
#pragma unroll
            for (int q = 0; q < 4; q++) key[q] = tri_key_weight(s_ij, s_ik[q], s_jk[q]);
          } else {
#pragma unroll
            for (int q = 0; q < 4; q++) key[q] = dsum_ij + deg[w * 64 + b[q]];
          }
#pragma unroll
          for (int q = 0; q < 4; q++) {
            if (q < nbits) {
              kcol[out0 + pm] = make_uint2((uint32_t)(w * 64 + b[q]), (uint32_t)e);  // third vertex + edge: tri_decode
              wkey[out0 + pm++] = key[q];
              kmin = min(kmin, key[q]);
              kmax = max(kmax, key[q]);
            }
          }
        }
      }
    }
  }
  block_minmax_store(kmin, kmax, blk_min, blk_max);
}

__global__ __launch_bounds__(1024) void key_range_kernel(const uint32_t* __restrict__ blk_min,
                                                         const uint32_t* __restrict__ blk_max, int nb,
                                                         SelectState* __restrict__ sel, uint64_t want) {
  __shared__ uint32_t lmin[16], lmax[16];
  uint32_t kmin = 0xFFFFFFFFu, kmax = 0;
  for (int b = threadIdx.x; b < nb; b += 1024) { kmin = min(kmin, blk_min[b]); kmax = max(kmax, blk_max[b]); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (uint32_t)__shfl_xor(kmin, o));
    kmax = max(kmax, (uint32_t)__shfl_xor(kmax, o));
  }
  if ((threadIdx.x & 63) == 0) { lmin[threadIdx.x >> 6] = kmin; lmax[threadIdx.x >> 6] = kmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; w++) { kmin = min(kmin, lmin[w]); kmax = max(kmax, lmax[w]); }
    sel->kmin = kmin; sel->kmax = kmax;
    sel->st[0] = SelSnap{0u, 0u, 0u, 0u, want, 0ull, 0ull, 0ull};  // (a speculative key pass may have preset a window)
    sel->want_req = 0;
  }
}

size_t tri_keys_blocks(uint64_t E, int tg) {
  const uint64_t per = 256 / tg;
  const uint64_t nb = (E + per - 1) / per;
  return (size_t)(nb < (uint64_t)TK_MAX_BLOCKS ? nb : (uint64_t)TK_MAX_BLOCKS);
}

void launch_tri_keys(const Graph& g, const Pruned& pr, const EdgeList& el, const EdgeCounts& ec, int rank_mode, const KeyArrays& ka,
                     uint64_t want, const Tuning& tn, hipStream_t st) {
  if (el.E == 0) return;
  const int tg = tn.tg_keys;
  const int nb = (int)tri_keys_blocks(el.E, tg);
  with_lanes<16, 4, 8, 32, 64>(tg, [&](auto lanes) {
    hipLaunchKernelGGL(tri_keys_kernel<decltype(lanes)::value>, dim3(nb), dim3(256), 0, st, g.bits, member_bits(g, pr), pr.smin, g.W, g.deg,
                       g.wpre, el.ebase, el.ei, el.ej, el.es, ec.toff, el.E, rank_mode, ka.wkey, ka.kcol, ka.blk_minmax,
                       ka.blk_minmax + TK_MAX_BLOCKS, ec.own);
  });
  hipLaunchKernelGGL(key_range_kernel, dim3(1), dim3(1024), 0, st, ka.blk_minmax, ka.blk_minmax + TK_MAX_BLOCKS, nb, ka.sel, want);
}

// ------------------------------------------------------------------------------------------------
// 2b/3'. event list: count and keys without enumerating twice
//
// tri_count and tri_keys used to AND the same pairs of bit rows, and tri_keys paid three dependent memory levels per
// wave-round (rows -> prefix words -> edge weights).  Now the counting pass also records every non-zero member word
// as an EVENT {member word m, word offsets of both rows, CSR bases of both ends, edge, rank of its first triangle
// inside the edge}.  Events are staged per WAVE in LDS and appended to one of EV_SHARDS global regions with a single
// atomic per flush (one counter per region: same-address RETURNING atomics serialise at ~170 ns each).  After the scan
// of the per-edge counts, tri_keys_events_kernel runs one lane per event: all its gathers are independent, and a
// triangle's key lands at its ordinal toff[e] + rank.  Event order is arbitrary; the result is not.
// If a region overflows, a flag reaches the host with the triangle count and the call falls back to the row-walking
// tri_keys_kernel (and doubles the event capacity for the next call).
// ------------------------------------------------------------------------------------------------
constexpr int EV_SHARDS = 1024;  // ~26 k flushes per call on C2: with 256 counters the returning atomics serialise (7.7 us)

// Staging is per WAVE (EVW records of LDS each).  The rounds loop is wave-uniform: it runs to the largest round count
// among the wave's groups and idle groups contribute empty words, so (a) events are appended with __ballot / mbcnt —
// no atomics, (b) the flush decision is taken by the whole wave after any round — a round adds at most 64 records, so
// the segment can never overflow, whatever the row width, and (c) no workgroup barrier is needed.  One global atomic
// per flush, on one of EV_SHARDS counters.
// Shapes measured and rejected (C2 unless noted): workgroup staging with two barriers per trip (48 us, and it overflows
// into per-event global atomics at W = 313: 4.7 ms on C3), per-wave staging with a global-atomic overflow path
// (235 us), per-group staging (118 us), a one-round-per-iteration state machine with software prefetch (98 us).
//
// 2c. ORD — ordinals from an ORDERED strong list, without the scan of the per-edge counts.  A triangle's ordinal is (triangles of the
// earlier edges, in edge order) + (its rank inside its edge), and only strong edges carry triangles.  The pruning kernel's block b
// (ORD_BLOCK_EDGES consecutive edges) leaves its strong edges in ascending order in its own slot and their number in cnt[b] (StrongList::cnt), so the flat list — the
// slots' runs one after the other — is in edge order.  A workgroup takes 256 / TG consecutive positions of it per trip: chunk
// bid + trip * nblk.  At the end of a trip it scans its groups' counts (wave shuffles, four LDS words, one barrier; the rounds loop
// stays barrier-free) and stores tloc[x], the triangles of the chunk's earlier edges, and ctot[chunk]; an event carries x.  Every
// workgroup of the key kernel then makes the exclusive prefix over the chunk totals in its prologue (as select_resolve does with a
// histogram) and a key lands at cpre[x / chunk] + tloc[x] + rank.  The same numbers as toff[e] + rank: same edge order, same rank.
// Every entry of cnt / tloc / ctot that is read was written by this call (reads are bounded by the live blocks and by S): nothing
// to clear.  tcnt[e] is still written for the strong edges: the fall-back of an overflow scans it (launch_zero_weak_counts first).
template <int TG, bool ORD>
__global__ __launch_bounds__(256) void tri_count_events_kernel(const uint64_t* __restrict__ mbits, int W,
                                                               const uint32_t* __restrict__ deg,
                                                               const uint32_t* __restrict__ ebi,
                                                               const uint32_t* __restrict__ ebj,
                                                               const uint32_t* __restrict__ ei,
                                                               const uint32_t* __restrict__ ej,
                                                               StrongList sl, int rank_mode,
                                                               uint32_t* __restrict__ tcnt, EventList ev,
                                                               const uint64_t* __restrict__ own,
                                                               const uint32_t* __restrict__ ebase, GramRefJob ref,
                                                               OrdList ord) {
  // ref (ref.out != null): workgroup 0 is a RIDER — it does none of this kernel's work but votes for the reference frame of
  // stage C2's Gram filter among the candidate triangles the estimating sample left behind (sc_gramref.hpp): ~10 us of one
  // workgroup's latency that would otherwise stand between the selection and the Kabsch launch, hidden under this launch
  const uint32_t rider = ref.out ? 1u : 0u;
  const uint32_t bid = blockIdx.x - rider, nblk = gridDim.x - rider;
  // ebase (with ebi == ebj == nullptr): the per-row CSR bases are looked up (edge_build_kernel does not write them per edge)
  // own (optional, sharded stage B): [lo, hi) of the edges this rank enumerates; the strong list holds every rank's, the
  // others count 0 here (their tcnt entry is written too: the scan that follows reads zeros outside the range)
  constexpr int EVW = 192;  // records per wave segment: flush above 128, a round adds <= 64
  __shared__ uint64_t l_m[4 * EVW];
  __shared__ uint32_t l_wi[4 * EVW], l_wj[4 * EVW], l_a[4 * EVW], l_b[4 * EVW], l_e[4 * EVW], l_rb[4 * EVW];
  __shared__ uint32_t l_pre[ORD ? ORD_MAX_BLOCKS + 1 : ST_SHARDS + 1];  // exclusive prefix of the strong-list region fills (ORD: of the pruning kernel's block counts)
  __shared__ uint32_t l_x[ORD ? 4 * EVW : 1];                // ORD: the events' list positions
  __shared__ uint32_t l_wtot[2][4];                          // ORD: the waves' triangle counts of a trip (double-buffered: one barrier per trip)
  static_assert(sizeof(l_m) >= GX_REF_LDS_WORDS * sizeof(float), "the rider borrows the event staging area");
  if (rider && blockIdx.x == 0) { gram_ref_block(ref, reinterpret_cast<float*>(l_m)); return; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = threadIdx.x & (TG - 1);
  static_assert(ST_SHARDS == 256, "one region per thread");
  if constexpr (ORD) {
    // the blocks of the pruning kernel that hold a live edge (a host-free call's grid covers more, and what lies beyond was not
    // written by this call; a graph that outgrew the cover: nothing was listed at all)
    static_assert(ORD_MAX_BLOCKS == 4 * 256, "four blocks per thread");
    __shared__ uint64_t plds[8];
    const uint64_t Ea = ord.E_dev ? (*ord.E_dev > ord.E ? 0ull : *ord.E_dev) : ord.E;
    const uint32_t nlive = (uint32_t)min((Ea + ORD_BLOCK_EDGES - 1) / ORD_BLOCK_EDGES, (uint64_t)ORD_MAX_BLOCKS);
    const uint4 t4 = reinterpret_cast<const uint4*>(ord.cnt)[threadIdx.x];
    const uint32_t b0 = threadIdx.x * 4;
    const uint32_t v0 = b0 < nlive ? t4.x : 0u, v1 = b0 + 1 < nlive ? t4.y : 0u, v2 = b0 + 2 < nlive ? t4.z : 0u, v3 = b0 + 3 < nlive ? t4.w : 0u;
    uint64_t tot;
    const uint32_t run = (uint32_t)block_exscan_u64((uint64_t)v0 + v1 + v2 + v3, plds, &tot);
    l_pre[b0] = run; l_pre[b0 + 1] = run + v0; l_pre[b0 + 2] = run + v0 + v1; l_pre[b0 + 3] = run + v0 + v1 + v2;
    if (threadIdx.x == 0) {
      l_pre[ORD_MAX_BLOCKS] = (uint32_t)tot;
      if (bid == 0) {
        *ord.n_strong = (uint32_t)tot;
        // more chunks than a workgroup of the key kernel holds: as if an event region were full (the host walks the rows again);
        // the word's high half says why, so that the context keeps the scan form from then on instead of growing its event buffer
        if ((tot + (256 / TG) - 1) / (256 / TG) > ord.chunk_max) { ev.overflow[0] = 1u; ev.overflow[1] = 1u; }
      }
    }
  } else {
    __shared__ uint64_t plds[8];
    const uint64_t v = sl.fill[threadIdx.x];
    uint64_t tot;
    l_pre[threadIdx.x] = (uint32_t)block_exscan_u64(v, plds, &tot);
    if (threadIdx.x == 0) l_pre[ST_SHARDS] = (uint32_t)tot;
  }
  __syncthreads();
  const uint64_t S = l_pre[ORD ? ORD_MAX_BLOCKS : ST_SHARDS];  // strong edges (only they can carry a triangle of the pruned graph)
  // the part of the flat list this rank walks: everything, or — regions being contiguous edge ranges — the regions its own
  // edge range touches (the others' tcnt entries were zeroed by the pruning kernel)
  uint64_t x0 = 0, x1 = S;
  if (own && sl.region_blocks) {
    const uint64_t per_region = (uint64_t)sl.region_blocks * 256;
    if (own[1] > own[0]) {
      const uint64_t r_lo = min(own[0] / per_region, (uint64_t)(ST_SHARDS - 1));
      const uint64_t r_hi = min((own[1] - 1) / per_region, (uint64_t)(ST_SHARDS - 1));
      x0 = l_pre[r_lo]; x1 = l_pre[r_hi + 1];
    } else {
      x1 = 0;
    }
  }
  const uint64_t groups = (uint64_t)nblk * (256 / TG);
  const uint64_t g0 = (uint64_t)bid * (256 / TG) + (threadIdx.x / TG);
  // region of this wave's NEXT ticket: it moves on by one with every ticket, so a wave with many events spreads them over
  // the regions (r03: every wave kept one region and a region overflowed in one C4 call in three at 2.2 records of capacity
  // per event — the call then fell back to the row-walking key kernel)
  uint32_t shard = (bid * 4 + wave) & (EV_SHARDS - 1);
  const uint64_t trips = (x1 - x0 + groups - 1) / groups;  // the same for every lane of the wave
  const int wbase = wave * EVW;
  uint32_t scnt = 0;  // records staged by this wave (wave-uniform)
  auto flush = [&]() {  // wave-uniform
    // A ticket that does not fit whole leaves no hole: the part inside the region is written (the key kernel reads
    // min(fill, capacity) records of a region), the rest moves on to the next region.  So the list overflows only when the
    // regions are full TOGETHER — a single region filling early (the strong list keeps the edges of a row together, so a run
    // of waves inside the inlier clique stages several times the mean) costs a second ticket, not the whole call's event path.
    uint32_t start = 0;  // records [start, scnt) are still to be placed
    for (int tries = 0; tries < EV_SHARDS && start < scnt; tries++) {
      const uint32_t cnt = scnt - start;
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&ev.fill[shard], cnt);
      base = __builtin_amdgcn_readfirstlane(base);
      const uint32_t fit = (uint64_t)base >= ev.shard_cap ? 0u : (uint32_t)min((uint64_t)cnt, ev.shard_cap - (uint64_t)base);
      for (uint32_t k = lane; k < fit; k += 64) {
        const uint64_t o = (uint64_t)shard * ev.shard_cap + (uint64_t)base + k;
        const int q = wbase + (int)(start + k);
        ev.m[o] = l_m[q]; ev.wi[o] = l_wi[q]; ev.wj[o] = l_wj[q]; ev.a[o] = l_a[q]; ev.b[o] = l_b[q];
        ev.e[o] = l_e[q]; ev.rb[o] = l_rb[q];
        if constexpr (ORD) ev.x[o] = l_x[q];
      }
      start += fit;
      shard = (shard + 1u) & (EV_SHARDS - 1);
    }
    if (start < scnt && lane == 0) *ev.overflow = 1u;
    scnt = 0;
  };
  for (uint64_t trip = 0; trip < trips; trip++) {
    const uint64_t x = x0 + g0 + trip * groups;  // position in the flat strong list
    const bool on = x < x1;                      // group-uniform
    uint32_t e = 0, rowi = 0, rowj = 0, fa = 0, fb = 0, c = 0;
    int w0 = 0, jbit = 0, rounds = 0;
    if (on) {
      int r = 0;  // region of x: the largest r with l_pre[r] <= x (ORD: the pruning kernel's block; empty ones are skipped)
#pragma unroll
      for (int step = (ORD ? ORD_MAX_BLOCKS : ST_SHARDS) / 2; step > 0; step >>= 1) r += (l_pre[r + step] <= (uint32_t)x) ? step : 0;
      e = sl.list[(uint64_t)r * (ORD ? ORD_BLOCK_EDGES : sl.cap) + ((uint32_t)x - l_pre[r])];
      if (!own || ((uint64_t)e >= own[0] && (uint64_t)e < own[1])) {
        const uint32_t i = ei[e], j = ej[e];
        rowi = i * (uint32_t)W; rowj = j * (uint32_t)W;
        fa = (rank_mode == 0) ? (ebi ? ebi[e] : ebase[i]) : deg[i] + deg[j];  // weight mode: CSR bases; degree mode: the degree sum
        fb = (rank_mode == 0) ? (ebj ? ebj[e] : ebase[j]) : 0u;
        w0 = (int)(j >> 6); jbit = (int)(j & 63);
        rounds = (W - w0 + TG - 1) / TG;
      }
    }
    int wave_rounds = rounds;  // max over the wave: the loop below is wave-uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wave_rounds = max(wave_rounds, __shfl_xor(wave_rounds, o));
    auto take = [&](uint64_t m, int w) {  // one round's words: count, stage the non-zero ones (wave-uniform control flow)
      const uint64_t bal = __ballot(m != 0);
      if (bal != 0) {
        uint32_t tm;
        const uint32_t rb = c + group_exscan<TG>((uint32_t)__popcll(m), &tm);
        c += tm;
        if (m) {
          const int q = wbase + (int)scnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
          l_m[q] = m; l_wi[q] = rowi + w; l_wj[q] = rowj + w; l_a[q] = fa; l_b[q] = fb; l_e[q] = e; l_rb[q] = rb;
          if constexpr (ORD) l_x[q] = (uint32_t)x;
        }
        scnt += (uint32_t)__popcll(bal);
        if (scnt > (uint32_t)(EVW - 64)) flush();
      }
    };
    // SEVERAL rounds' row words are loaded before the first is looked at (r05, by time stamps inside the workgroups: a round is one
    // L2 round trip, ~0.45 us, and an edge's 6 - 19 rounds were most of a workgroup's 9 - 14 us)
    constexpr int RU = 2;  // rounds whose words are in flight together (4: no better at C2 and C4, + 6 us at C3)
    for (int it = 0; it < wave_rounds; it += RU) {
      uint64_t mi[RU], mj[RU];
#pragma unroll
      for (int u = 0; u < RU; u++) {
        const int w = w0 + (it + u) * TG + gl;
        const bool in = it + u < rounds && w < W;
        mi[u] = in ? mbits[rowi + w] : 0ull;
        mj[u] = in ? mbits[rowj + w] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < RU; u++) {
        if (it + u >= wave_rounds) break;  // (wave-uniform)
        const int w = w0 + (it + u) * TG + gl;
        uint64_t m = mi[u] & mj[u];
        if (w == w0) m &= mask_above(jbit);
        take(m, w);
      }
    }
    if (gl == 0 && on) tcnt[e] = c;  // weak edges were zeroed by prune_bits_kernel (ORD: by nobody — only an overflow's fall-back reads tcnt)
    if constexpr (ORD) {  // the chunk's exclusive prefix over its groups' counts, and its total (trips is the same in every wave)
      const uint32_t inc = wave_inscan<uint32_t>(gl == 0 ? c : 0u);  // (c is 0 in an idle group)
      if (lane == 63) l_wtot[trip & 1][wave] = inc;
      __syncthreads();
      uint32_t base = 0, tot = 0;
#pragma unroll
      for (int w = 0; w < 4; w++) { const uint32_t t = l_wtot[trip & 1][w]; base += w < wave ? t : 0u; tot += t; }
      if (gl == 0 && on) ord.tloc[x] = base + inc - c;
      const uint64_t chunk = (x0 + (uint64_t)bid * (256 / TG) + trip * groups) / (256 / TG);  // = bid + trip * nblk
      if (threadIdx.x == 0 && chunk * (256 / TG) < x1) ord.ctot[chunk] = tot;
    }
  }
  if (scnt) flush();
}

// one lane per event.  ORD (2c): the ordinals come from the ordered strong list — cpre[x / chunk] + tloc[x] + rank, cpre made here —
// and workgroup 0 leaves the triangle count where the scan would (ord.total = toff[E]; host_total: the word a waited call polls)
template <bool ORD>
__global__ __launch_bounds__(256) void tri_keys_events_kernel(const uint64_t* __restrict__ bits,
                                                              const uint32_t* __restrict__ wpre,
                                                              const uint32_t* __restrict__ deg,
                                                              const float* __restrict__ es,
                                                              const uint64_t* __restrict__ toff, int rank_mode,
                                                              EventList ev, uint32_t* __restrict__ wkey,
                                                              uint2* __restrict__ kcol,
                                                              uint32_t* __restrict__ blk_min,
                                                              uint32_t* __restrict__ blk_max,
                                                              SelectState* __restrict__ preset,
                                                              const uint32_t* __restrict__ klb, uint64_t want,
                                                              uint64_t E, uint64_t cap, int check_bound, OrdList ord,
                                                              int chunk_shift, uint64_t* __restrict__ host_total) {
  // cap: entries wkey / kcol hold.  The host may launch this kernel BEFORE it knows the triangle count (into the
  // arrays of the previous call, while it polls for the count): writes beyond cap are dropped and the host re-runs.
  // For the same reason `want` is clipped here to the count the scan left in toff[E].
  // (ORD: 32-bit — the event buffer holds at most 2^28 records — so that four workgroups' LDS still fit a CU beside cpre)
  using pre_t = typename std::conditional<ORD, uint32_t, uint64_t>::type;
  __shared__ pre_t pre[EV_SHARDS + 1];
  __shared__ uint32_t cpre[ORD ? ORD_CHUNK_MAX : 1];  // ORD: exclusive prefix of the chunk totals
  uint64_t triangles = 0;  // what the scan leaves in toff[E]
  if constexpr (ORD) {
    // wave w scans the chunk totals [w per, (w + 1) per), 64 at a time — coalesced loads, four in flight, conflict-free LDS stores —
    // and then adds the sum of the waves before it.  More chunks than cpre holds: the counting pass has raised the overflow flag —
    // the ordinals below are void (in bounds: writes beyond cap are dropped) and workgroup 0 adds the rest to the count in a loop
    static_assert(ORD_CHUNK_MAX == 4 * 2048, "four waves, at most 2048 chunks each");
    __shared__ uint64_t plds[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t S = *ord.n_strong;
    const uint32_t nch = (uint32_t)(((uint64_t)S + (1u << chunk_shift) - 1) >> chunk_shift);
    const uint32_t lim = min(ord.chunk_max, ORD_CHUNK_MAX), nchc = min(nch, lim);
    const uint32_t per = (nchc + 255) / 256 * 64, lo = min((uint32_t)wave * per, nchc), hi = min(lo + per, nchc);
    uint64_t carry = 0;
    for (uint32_t i0 = lo; i0 < hi; i0 += 256) {
      uint32_t v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { const uint32_t i = i0 + 64 * u + lane; v[u] = i < hi ? ord.ctot[i] : 0u; }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t i = i0 + 64 * u + lane;
        const uint32_t inc = wave_inscan<uint32_t>(v[u]);
        if (i < hi) cpre[i] = (uint32_t)carry + inc - v[u];
        carry += (uint32_t)__shfl(inc, 63);
      }
    }
    if (lane == 0) plds[wave] = carry;
    __syncthreads();
    uint64_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) { const uint64_t t = plds[w]; base += w < wave ? t : 0ull; tot += t; }
    if (wave) for (uint32_t i = lo + lane; i < hi; i += 64) cpre[i] += (uint32_t)base;
    if (blockIdx.x == 0 && nch > nchc) {  // (an overflow: the count is still exact; uniform over the workgroup)
      uint64_t rest = 0;
      for (uint32_t k = nchc + threadIdx.x; k < nch; k += 256) rest += ord.ctot[k];
      __syncthreads();
      tot += block_reduce_u64(rest, plds);
    }
    triangles = tot;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      *ord.total = tot;
      if (host_total) publish_host(host_total, tot);
    }
  }
  // Weight keys of a graph whose edges all weigh >= 2/3 live in one binade, [2.0, 3.0]: the select window is known
  // before a single key exists — [certified bound (or 2.0), 3.0] — so no key-range pass, and two 12-bit rounds
  // always resolve it.  (Keys below a certified bound cannot be among the `want` largest: sc_tri_prune.hip 3b.)
  if (preset && blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t lo = *klb ? *klb : 0x40000000u, hi = 0x40400000u;  // 2.0f, 3.0f
    const uint32_t range_m1 = hi - lo;
    preset->kmin = lo; preset->kmax = hi;
    preset->st[0] = SelSnap{lo, range_m1 == 0 ? 0u : (uint32_t)(32 - __builtin_clz(range_m1)), 1u, 0u, min(want, ORD ? triangles : (uint64_t)toff[E]), 0ull, 0ull, 0ull};
    // a pruning bound promises `want` keys at or above it — a certified one by construction, an ESTIMATED one (3c) unless
    // it was set too high: whoever resolves the select's first round compares (the UNclipped want: a pruned graph with fewer triangles than
    // that proves nothing about the full one)
    preset->want_req = (check_bound && *klb) ? want : 0ull;
  }  // exclusive prefix of the region fills: one flat index space over all events
  {
    constexpr int PT = EV_SHARDS / 256;  // regions per thread
    __shared__ uint64_t plds[8];
    uint64_t f[PT], mine = 0;
#pragma unroll
    for (int k = 0; k < PT; k++) { f[k] = min((uint64_t)ev.fill[threadIdx.x * PT + k], ev.shard_cap); mine += f[k]; }
    uint64_t tot;
    uint64_t run = block_exscan_u64(mine, plds, &tot);
#pragma unroll
    for (int k = 0; k < PT; k++) { pre[threadIdx.x * PT + k] = (pre_t)run; run += f[k]; }
    if (threadIdx.x == 0) pre[EV_SHARDS] = (pre_t)tot;
    __syncthreads();
  }
  uint32_t kmin = 0xFFFFFFFFu, kmax = 0;
  const uint64_t nthreads = (uint64_t)gridDim.x * 256, total = pre[EV_SHARDS];
  {
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < total; x += nthreads) {
      int sh = 0;  // largest sh with pre[sh] <= x
#pragma unroll
      for (int step = EV_SHARDS / 2; step > 0; step >>= 1) sh += (pre[sh + step] <= x) ? step : 0;
      const uint64_t o = (uint64_t)sh * ev.shard_cap + (x - pre[sh]);
      uint64_t m = ev.m[o];
      const uint32_t wi = ev.wi[o], wj = ev.wj[o], fa = ev.a[o], e = ev.e[o];
      uint64_t out;
      if constexpr (ORD) {
        const uint32_t xs = ev.x[o];
        out = (uint64_t)cpre[min(xs >> chunk_shift, ORD_CHUNK_MAX - 1)] + ord.tloc[xs] + ev.rb[o];
      } else {
        out = toff[e] + ev.rb[o];
      }
      const uint32_t kbase = (uint32_t)(wi % (uint32_t)ev.W) * 64u;  // column index of bit 0 of this word
      if (rank_mode == 0) {
        const uint32_t fb = ev.b[o];
        const uint64_t fi = bits[wi], fj = bits[wj];  // full-graph words: ranks in the CSR edge arrays
        const uint32_t pi = fa + wpre[wi], pj = fb + wpre[wj];
        const float s_ij = es[e];
        while (m) {
          int b[4];
          const int nbits = pop4(m, b);
          float s_ik[4], s_jk[4];
          tri_weights4(es, b, nbits, {pi, fi}, {pj, fj}, s_ik, s_jk);
#pragma unroll
          for (int q = 0; q < 4; q++) {
            if (q < nbits) {
              const uint32_t key = tri_key_weight(s_ij, s_ik[q], s_jk[q]);
              if (out < cap) { kcol[out] = make_uint2(kbase + (uint32_t)b[q], e); wkey[out] = key; }
              out++;
              kmin = min(kmin, key);
              kmax = max(kmax, key);
            }
          }
        }
      } else {
        while (m) {
          const int b = __builtin_ctzll(m);
          m &= m - 1;
          const uint32_t key = fa + deg[kbase + b];
          if (out < cap) { kcol[out] = make_uint2(kbase + (uint32_t)b, e); wkey[out] = key; }
          out++;
          kmin = min(kmin, key);
          kmax = max(kmax, key);
        }
      }
    }
  }
  block_minmax_store(kmin, kmax, blk_min, blk_max);
}

size_t event_bytes(uint64_t capacity) { return (size_t)capacity * 36 + EV_SHARDS * 4 + 64; }

EventList event_list(void* buf, uint64_t capacity, int W, uint32_t* fill, uint32_t* overflow_host) {
  EventList ev;
  const uint64_t cap = capacity / EV_SHARDS * EV_SHARDS;
  unsigned char* p = static_cast<unsigned char*>(buf);
  ev.m = reinterpret_cast<uint64_t*>(p); p += cap * 8;
  ev.wi = reinterpret_cast<uint32_t*>(p); p += cap * 4;
  ev.wj = reinterpret_cast<uint32_t*>(p); p += cap * 4;
  ev.a = reinterpret_cast<uint32_t*>(p); p += cap * 4;
  ev.b = reinterpret_cast<uint32_t*>(p); p += cap * 4;
  ev.e = reinterpret_cast<uint32_t*>(p); p += cap * 4;
  ev.rb = reinterpret_cast<uint32_t*>(p); p += cap * 4;
  ev.x = reinterpret_cast<uint32_t*>(p); p += cap * 4;
  ev.fill = fill;  // EV_SHARDS zeroed counters (control block)
  ev.shard_cap = cap / EV_SHARDS;
  ev.overflow = overflow_host;
  ev.W = W;
  return ev;
}

void launch_tri_count_events(const Graph& g, const Pruned& pr, const EdgeList& el, const EdgeCounts& ec, int rank_mode, const EventList& ev,
                             const OrdList& ord, const GramRefJob* ref, const Tuning& tn, hipStream_t st) {
  const uint64_t E = el.E_hint;  // (only the grid goes by it)
  if (E == 0) return;
  // lanes per edge: a lane walks (W - j / 64) / TG words one dependent round after the other, so wide rows want wide
  // groups (Tuning::tg_events forces one; measured r02: see DESIGN.md)
  // r04c, on the pruned graph (a third of the triangles of r03's: shorter walks, more edges per wave pay): 4 lanes between 65 and 128
  // words — C2 (79): stage B's bracket 101.5 -> 99.4 us in eight alternating pairs of runs, C4 (79): 138.6 vs 138.5 — but not
  // below: C1 (32 words) 68.3 -> 69.7 us with 4
  const int tg = tri_count_events_lanes(g, tn);
  const uint64_t per = 256 / tg;
  // the strong edges are a fraction of E that only the device knows (20 - 45 % on C1 .. C4): size the grid for ~E/3
  uint64_t nb = (E / 3 + per - 1) / per;
  if (nb < 256) nb = 256;
  if (nb > 4096) nb = 4096;
  if (tn.cnt_blocks >= 1 && tn.cnt_blocks <= 65535) nb = tn.cnt_blocks;
  const GramRefJob rj = ref ? *ref : GramRefJob{};
  if (rj.out) nb++;  // (workgroup 0 is the rider)
  auto launch = [&](auto lanes, auto ordered) {
    hipLaunchKernelGGL((tri_count_events_kernel<decltype(lanes)::value, decltype(ordered)::value>), dim3((unsigned)nb), dim3(256), 0, st,
                       member_bits(g, pr), g.W, g.deg, el.ebi, el.ebj, el.ei, el.ej, pr.sl, rank_mode, ec.tcnt, ev, ec.own, el.ebase, rj, ord);
  };
  with_lanes<8, 4, 16, 32, 64>(tg, [&](auto lanes) {
    if (ord.cnt) launch(lanes, std::true_type{}); else launch(lanes, std::false_type{});
  });
}

int tri_count_events_lanes(const Graph& g, const Tuning& tn) {
  return tn.tg_events ? tn.tg_events : (g.W <= 64 ? 8 : (g.W <= 128 ? 4 : (g.W <= 512 ? 16 : 32)));
}

// (ORD) the fall-back of an overflow scans tcnt: the entries of the weak edges, which no kernel of the ordered form writes
__global__ __launch_bounds__(256) void zero_weak_counts_kernel(const float* __restrict__ es, const float* __restrict__ smin,
                                                               uint64_t E, const uint64_t* __restrict__ E_dev,
                                                               uint32_t* __restrict__ tcnt) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const uint64_t Ea = E_dev ? (*E_dev > E ? 0ull : *E_dev) : E;
  if (e >= Ea || !(es[e] >= *smin)) tcnt[e] = 0u;
}
void launch_zero_weak_counts(const EdgeList& el, const Pruned& pr, const EdgeCounts& ec, hipStream_t st) {
  if (el.E == 0) return;
  hipLaunchKernelGGL(zero_weak_counts_kernel, dim3((unsigned)((el.E + 255) / 256)), dim3(256), 0, st, el.es, pr.smin, el.E, el.E_dev, ec.tcnt);
}

void launch_tri_keys_events(const Graph& g, const Pruned& pr, const EdgeList& el, const EdgeCounts& ec, int rank_mode, const EventList& ev,
                            const OrdList& ord, const KeyArrays& ka, uint64_t want, const KeyPassOpts& o, const Tuning& tn, hipStream_t st) {
  // (ordered strong list: every workgroup pays for the prefix over the chunk totals, and four fit a CU beside it — one round of them)
  int nb = ord.cnt ? 1024 : 2048;
  if (tn.keys_blocks >= 1 && tn.keys_blocks <= (uint32_t)TK_MAX_BLOCKS) nb = (int)tn.keys_blocks;
  const uint32_t* klb = o.window ? pr.klb : nullptr;  // (no bound to read — Pruned{} — : no preset, the key range is measured)
  SelectState* preset = klb ? ka.sel : nullptr;
  if (ord.cnt)
    hipLaunchKernelGGL(tri_keys_events_kernel<true>, dim3(nb), dim3(256), 0, st, g.bits, g.wpre, g.deg, el.es, ec.toff, rank_mode,
                       ev, ka.wkey, ka.kcol, ka.blk_minmax, ka.blk_minmax + TK_MAX_BLOCKS, preset, klb, want, el.E, ka.cap,
                       o.check_bound ? 1 : 0, ord, o.chunk_shift, o.host_total);
  else
    hipLaunchKernelGGL(tri_keys_events_kernel<false>, dim3(nb), dim3(256), 0, st, g.bits, g.wpre, g.deg, el.es, ec.toff, rank_mode,
                       ev, ka.wkey, ka.kcol, ka.blk_minmax, ka.blk_minmax + TK_MAX_BLOCKS, preset, klb, want, el.E, ka.cap,
                       o.check_bound ? 1 : 0, OrdList{}, 0, (uint64_t*)nullptr);
  if (!klb)  // no a-priori window: the key range comes from the per-block extremes
    hipLaunchKernelGGL(key_range_kernel, dim3(1), dim3(1024), 0, st, ka.blk_minmax, ka.blk_minmax + TK_MAX_BLOCKS, nb, ka.sel, want);
}

// ------------------------------------------------------------------------------------------------
// 4. radix select: window [lo, lo + SEL_BINS << shift), <= 3 rounds of SEL_BITS bits down to shift 0
// ------------------------------------------------------------------------------------------------
constexpr int SEL_BITS = 12;  // key bits resolved per round
constexpr int SEL_BINS = 1 << SEL_BITS;
constexpr int SEL_PER = SEL_BINS / 256;  // bins per thread of the picking block
constexpr int SEL_THREADS = 256;
constexpr int SEL_ITEMS = 16;

// current window of the select: keys in [lo, lo + 2^wbits), binned by (key - lo) >> shift into <= SEL_BINS bins
// rounds_left: launches still to come INCLUDING this one.  The window's bits are split evenly over them (at most
// SEL_BITS per round): a 16-bit window resolved in two rounds uses 256 bins per round, not 4096 — every block flushes its
// non-zero bins with global atomics, and all per-bin loops scale with the bin count.
struct SelWindow { uint32_t lo, wbits, shift, nbins; };
__device__ __forceinline__ SelWindow select_window(const SelectState* sel, const SelSnap& cur, int rounds_left) {
  SelWindow w;
  if (!cur.started) {  // first round: the window is the key range [kmin, kmax]
    w.lo = sel->kmin;
    const uint32_t range_m1 = sel->kmax - sel->kmin;
    w.wbits = range_m1 == 0 ? 0u : (uint32_t)(32 - __builtin_clz(range_m1));
  } else {
    w.lo = cur.lo;
    w.wbits = cur.wbits;
  }
  const uint32_t rl = rounds_left > 0 ? (uint32_t)rounds_left : 1u;
  uint32_t br = (w.wbits + rl - 1u) / rl;                    // this round's share of the bits
  if (br > (uint32_t)SEL_BITS) br = (uint32_t)SEL_BITS;
  if (w.wbits > br + (uint32_t)SEL_BITS * (rl - 1u)) br = (uint32_t)SEL_BITS;  // (cannot happen for wbits <= SEL_BITS * rl)
  w.shift = w.wbits > br ? w.wbits - br : 0u;
  w.nbins = 1u << (w.wbits - w.shift);                      // bins (key - lo) >> shift can reach
  return w;
}

__device__ __forceinline__ void hist_add(uint32_t* lh, bool in, uint32_t bin) {
  // wave-uniform fast path: heavy ties put a whole wave in one bin (one LDS atomic instead of a 64-way conflict)
  const uint32_t b = in ? bin : 0xFFFFFFFFu;
  const uint32_t b0 = __builtin_amdgcn_readfirstlane(b);
  const uint64_t same = __ballot(b == b0);
  const uint64_t active = __ballot(true);
  if (same == active) {
    if (b0 != 0xFFFFFFFFu && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(active))
      atomicAdd(&lh[b0], (uint32_t)__popcll(active));
  } else if (in) {
    atomicAdd(&lh[b], 1u);
  }
}

// (Tried and dropped, r01: an EXACT histogram of the keys in [certified bound, 3.0] — ~50 k distinct fp32 values on C2 —
// filled by the key kernel with one device-scope atomic per key and read by a single pick kernel, replacing both rounds:
// bit-exact, but the atomics cost the key kernel +20 us and the pick 10-50 us, against 26 us for the two rounds.)
// One select round: every block histograms its share of the keys into the window's bins (LDS, then one global add per non-zero
// bin).  Until r05 the LAST block to finish (device-scope ticket, release / acquire) walked the bins from the top, picked the bin
// holding the want-th key and narrowed the window; now the NEXT launch does that in every workgroup's prologue (select_resolve).
// four keys of the view at logical positions 4q .. 4q + 3 (entries beyond a segment's valid count read as 0, which
// no window and no threshold ever admits: real keys are positive)
// keys the view really holds (M_dev: the launch was sized before the host knew the count)
__device__ __forceinline__ uint64_t view_count(const KeyView& v) { return v.M_dev ? min(v.M, *v.M_dev) : v.M; }

template <bool SEG>
__device__ __forceinline__ uint4 view_load4(const KeyView& v, uint64_t q) {
  if (!SEG) return reinterpret_cast<const uint4*>(v.base)[q];
  const uint64_t x = q << 2, sg = x / v.seg_len, off = x - sg * v.seg_len;  // seg_len % 4 == 0: no straddling
  const uint64_t nv = v.valid[sg * v.valid_stride];
  uint4 k = make_uint4(0u, 0u, 0u, 0u);
  if (off < nv) {
    k = *reinterpret_cast<const uint4*>(v.base + sg * v.seg_stride + off);
    if (off + 1 >= nv) k.y = 0u;
    if (off + 2 >= nv) k.z = 0u;
    if (off + 3 >= nv) k.w = 0u;
  }
  return k;
}

// The state after round r from the state before it and the round's histogram.  Whole workgroup (SEL_THREADS threads, all
// arrive); lds: 10 words of 8 bytes.  Thread t owns `per` bins counted from the TOP: bins nbins - 1 - (per t + k).  The bins were
// filled by the previous launch's L2-side atomics: plain loads see them.  *shortfall: a pruning bound promised want_req keys at
// or above the window's floor and did not keep it (an estimate set too high — sc_tri_prune.hip 3c): the selection of this call proves
// nothing; the host repeats it with a certifying sample.
__device__ SelSnap select_resolve(const SelectState* __restrict__ sel, int r, int rounds, uint64_t* lds, bool* shortfall) {
  static_assert(SEL_THREADS == 256 && SEL_PER == 16, "256 threads, at most 16 bins each");
  const SelSnap prev = sel->st[r];
  *shortfall = false;
  if (prev.done) return prev;  // (an earlier round already came down to one key value: round r added nothing)
  const SelWindow win = select_window(sel, prev, rounds - r);
  const int nbins = (int)win.nbins;
  const int per = nbins >= SEL_THREADS ? nbins / SEL_THREADS : 1;
  const bool owner = (int)threadIdx.x * per < nbins;
  const uint32_t* __restrict__ hist = sel->hist[r];
  uint32_t h[SEL_PER];
  uint64_t mine = 0;
#pragma unroll
  for (int k = 0; k < SEL_PER; k++) {
    h[k] = (owner && k < per) ? hist[nbins - 1 - ((int)threadIdx.x * per + k)] : 0u;
    mine += h[k];
  }
  const uint64_t want = prev.want, above0 = prev.above;
  if (threadIdx.x == 0) { lds[8] = 0; lds[9] = above0; }
  uint64_t tot;
  const uint64_t before = above0 + block_exscan_u64(mine, lds, &tot);
  // A window may hold fewer than want - above0 keys only where a rank selects among ITS triangles alone (sharded
  // stage B: the certified bound promises T keys above it in the whole graph, not in one rank's share): then every key
  // of the window is taken.  (Unsharded, the window always holds enough and this changes nothing.)
  const uint64_t want_eff = want < above0 + tot ? want : above0 + tot;
  *shortfall = sel->want_req != 0 && above0 + tot < sel->want_req;
  // the crossing thread: before < want <= before + mine (exactly one: the window holds >= want - above0 keys)
  if (before < want_eff && want_eff <= before + mine) {
    uint64_t run = before;
#pragma unroll
    for (int k = 0; k < SEL_PER; k++) {
      if (k < per && run < want_eff && want_eff <= run + h[k]) { lds[8] = (uint64_t)(nbins - 1 - ((int)threadIdx.x * per + k)); lds[9] = run; }
      run += h[k];
    }
  }
  __syncthreads();
  const uint32_t bin = (uint32_t)lds[8];
  const uint64_t above = lds[9];
  __syncthreads();  // (lds is the caller's again)
  SelSnap nx;
  nx.lo = win.lo + (bin << win.shift);
  nx.wbits = win.shift;  // the chosen bin is the next window
  nx.started = 1u;
  nx.done = win.shift == 0 ? 1u : 0u;
  nx.want = want_eff;
  nx.above = above;
  nx.need_eq = nx.done ? want_eff - above : 0ull;
  nx.pad = 0;
  return nx;
}

// round r of `rounds` (see SelectState): resolve round r - 1, then add this launch's share of the keys into hist[r]
template <bool SEG>
__global__ __launch_bounds__(SEL_THREADS) void select_round_kernel(KeyView view, SelectState* __restrict__ sel,
                                                                   int r, int rounds, uint64_t* __restrict__ host_short) {
  const uint64_t M = view_count(view);
  const uint32_t* __restrict__ wkey = view.base;
  __shared__ uint32_t lh[SEL_BINS];
  __shared__ uint64_t lds[10];
  for (int b = threadIdx.x; b < SEL_BINS; b += SEL_THREADS) lh[b] = 0;
  SelSnap cur;
  if (r == 0) {
    cur = sel->st[0];
  } else {
    bool shortfall;
    cur = select_resolve(sel, r - 1, rounds, lds, &shortfall);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      sel->st[r] = cur;
      if (shortfall && host_short) publish_host(host_short, 1ull);
    }
  }
  if (cur.done) return;  // uniform over the grid
  const SelWindow win = select_window(sel, cur, rounds - r);
  const int nbins = (int)win.nbins;
  __syncthreads();
  const uint64_t width = 1ull << win.wbits;
  const uint64_t M4 = M >> 2;  // whole uint4 groups (wkey comes from hipMalloc: 16-byte aligned)
  const uint64_t stride = (uint64_t)gridDim.x * SEL_THREADS;
  auto bin4 = [&](const uint4& k4) {
    const uint32_t ks[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint64_t rel = (uint64_t)ks[c] - (uint64_t)win.lo;  // wraps huge when key < lo
      hist_add(lh, (ks[c] >= win.lo) && (rel < width), (uint32_t)(rel >> win.shift));
    }
  };
  // (hipcc does not carry loads across the trips of a loop: four grid-strided loads are issued together — a thread's SEL_ITEMS keys
  // used to be four dependent round trips, ~2 us of the launch's 6)
  uint64_t q = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
  for (; q + 3 * stride < M4; q += 4 * stride) {
    const uint4 a0 = view_load4<SEG>(view, q), a1 = view_load4<SEG>(view, q + stride), a2 = view_load4<SEG>(view, q + 2 * stride),
                a3 = view_load4<SEG>(view, q + 3 * stride);
    bin4(a0); bin4(a1); bin4(a2); bin4(a3);
  }
  for (; q < M4; q += stride) bin4(view_load4<SEG>(view, q));
  if (!SEG && blockIdx.x == 0 && threadIdx.x < (M & 3)) {  // tail (a segmented view is a whole number of groups)
    const uint32_t key = wkey[(M4 << 2) + threadIdx.x];
    const uint64_t rel = (uint64_t)key - (uint64_t)win.lo;
    if ((key >= win.lo) && (rel < width)) atomicAdd(&lh[(uint32_t)(rel >> win.shift)], 1u);
  }
  __syncthreads();
  uint32_t* __restrict__ hist = sel->hist[r];
  for (int b = threadIdx.x; b < nbins; b += SEL_THREADS) {
    const uint32_t v = lh[b];
    if (v) atomicAdd(&hist[b], v);
  }
}

KeyView plain_view(const uint32_t* wkey, uint64_t M) { return KeyView{wkey, M, 0, 0, nullptr, 0, nullptr}; }

void launch_select_rounds(const KeyView& view, SelectState* s, int rounds, uint64_t* host_short, const Tuning& tn, hipStream_t st) {
  const uint64_t M = view.M;
  if (M == 0) return;
  uint64_t blocks = (M + (uint64_t)SEL_THREADS * SEL_ITEMS - 1) / ((uint64_t)SEL_THREADS * SEL_ITEMS);
  // 256 blocks measured best on C2 (1.5 M keys): every block pays an agent-scope release for its ticket
  uint64_t cap = 256;
  if (tn.sel_blocks >= 1) cap = tn.sel_blocks;
  if (blocks > cap) blocks = cap;
  if (blocks == 0) blocks = 1;
  if (rounds > 3) rounds = 3;  // (SelectState::hist; 3 x SEL_BITS covers a 32-bit key)
  for (int round = 0; round < rounds; round++) {
    if (view.seg_len) hipLaunchKernelGGL(select_round_kernel<true>, dim3((unsigned)blocks), dim3(SEL_THREADS), 0, st, view, s, round, rounds, host_short);
    else hipLaunchKernelGGL(select_round_kernel<false>, dim3((unsigned)blocks), dim3(SEL_THREADS), 0, st, view, s, round, rounds, host_short);
  }
}

// ------------------------------------------------------------------------------------------------
// 5. compaction in ordinal order
// ------------------------------------------------------------------------------------------------
constexpr int CP_THREADS = 256;
constexpr int CP_ITEMS = 4;  // one 16-byte load per thread: every wave reads 1 KiB contiguous
constexpr int CP_TILE = CP_THREADS * CP_ITEMS;

size_t compact_blocks(uint64_t M) { return (size_t)((M + CP_TILE - 1) / CP_TILE); }

template <bool SEG>
__device__ __forceinline__ void load_tile_keys(const KeyView& view, uint64_t base, uint32_t keys[CP_ITEMS], int& valid) {
  const uint32_t* __restrict__ wkey = view.base;
  const uint64_t M = view_count(view);
  if (SEG) {  // CP_ITEMS == 4 and seg_len % 4 == 0: one group of the view
    const uint4 k4 = base < M ? view_load4<true>(view, base >> 2) : make_uint4(0u, 0u, 0u, 0u);
    keys[0] = k4.x; keys[1] = k4.y; keys[2] = k4.z; keys[3] = k4.w;
    valid = base < M ? CP_ITEMS : 0;
    return;
  }
  if (base + CP_ITEMS <= M) {
    const uint4 k4 = *reinterpret_cast<const uint4*>(wkey + base);
    keys[0] = k4.x; keys[1] = k4.y; keys[2] = k4.z; keys[3] = k4.w;
    valid = CP_ITEMS;
  } else {
    valid = base < M ? (int)(M - base) : 0;
#pragma unroll
    for (int k = 0; k < CP_ITEMS; k++) keys[k] = (k < valid) ? wkey[base + k] : 0u;
  }
}

static_assert(CP_ITEMS == 4, "load_tile_keys reads one uint4 group of a segmented view");
template <bool SEG>
__global__ __launch_bounds__(CP_THREADS) void compact_count_kernel(KeyView view, SelectState* __restrict__ sel, int rounds,
                                                                   uint32_t* __restrict__ blk_gt,
                                                                   uint32_t* __restrict__ blk_eq,
                                                                   uint64_t* __restrict__ host_short) {
  static_assert(CP_THREADS == SEL_THREADS, "select_resolve: one workgroup of SEL_THREADS");
  __shared__ uint32_t lds[2][4];
  __shared__ uint64_t rl[10];
  const uint64_t base = (uint64_t)blockIdx.x * CP_TILE + (uint64_t)threadIdx.x * CP_ITEMS;
  uint32_t keys[CP_ITEMS];
  int valid;
  load_tile_keys<SEG>(view, base, keys, valid);
  // the last select round's histogram -> k* (every workgroup by itself; workgroup 0 leaves the result for the launches after this one)
  bool shortfall;
  const SelSnap fin = select_resolve(sel, rounds - 1, rounds, rl, &shortfall);
  const uint32_t kstar = fin.done ? fin.lo : 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sel->kstar = kstar; sel->done = fin.done; sel->want = fin.want; sel->need_eq = fin.need_eq;
    if (shortfall && host_short) publish_host(host_short, 1ull);
  }
  uint32_t g = 0, q = 0;
#pragma unroll
  for (int k = 0; k < CP_ITEMS; k++)
    if (k < valid) { g += keys[k] > kstar; q += keys[k] == kstar; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { g += __shfl_xor(g, o); q += __shfl_xor(q, o); }
  if ((threadIdx.x & 63) == 0) { lds[0][threadIdx.x >> 6] = g; lds[1][threadIdx.x >> 6] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    blk_gt[blockIdx.x] = lds[0][0] + lds[0][1] + lds[0][2] + lds[0][3];
    blk_eq[blockIdx.x] = lds[1][0] + lds[1][1] + lds[1][2] + lds[1][3];
  }
}

void launch_compact_count(const KeyView& view, SelectState* s, int rounds, uint32_t* blk_gt, uint32_t* blk_eq, uint64_t* host_short,
                          hipStream_t st) {
  if (view.M == 0) return;
  if (rounds > 3) rounds = 3;
  const dim3 grid((unsigned)compact_blocks(view.M));
  if (view.seg_len) hipLaunchKernelGGL(compact_count_kernel<true>, grid, dim3(CP_THREADS), 0, st, view, s, rounds, blk_gt, blk_eq, host_short);
  else hipLaunchKernelGGL(compact_count_kernel<false>, grid, dim3(CP_THREADS), 0, st, view, s, rounds, blk_gt, blk_eq, host_short);
}

template <bool SEG>
__global__ __launch_bounds__(CP_THREADS) void compact_write_kernel(KeyView view,
                                                                   SelectState* __restrict__ sel,
                                                                   const uint32_t* __restrict__ blk_gt,
                                                                   const uint32_t* __restrict__ blk_eq,
                                                                   const uint64_t* __restrict__ off_gt,
                                                                   const uint64_t* __restrict__ off_eq,
                                                                   uint64_t* __restrict__ sel_ord,
                                                                   uint32_t* __restrict__ sel_key, uint64_t n_sel) {
  // n_sel: entries sel_ord / sel_key hold.  A position at or beyond it cannot come out of a consistent select; a call that
  // was launched before the host knew the counts (and is about to be repeated) may hold anything, and must stay in bounds.
  __shared__ uint64_t lds[8];
  const uint32_t kstar = sel->kstar;
  const uint64_t need_eq = sel->need_eq;
  // the select's histograms are all zero again behind it (no launch reads them any more; a call may select twice: sharded stage B)
  for (uint32_t z = blockIdx.x * CP_THREADS + threadIdx.x; z < 3u * 4096u; z += gridDim.x * CP_THREADS) (&sel->hist[0][0])[z] = 0u;
  // off_gt == nullptr: this block adds up the tile counts before it by itself (a few thousand u32 from L2) — saves
  // the scan launch in between; both sums ride one u64 (gt high, eq low: each below 2^32 since M < 2^32 here)
  uint64_t gt0, eq0;
  if (off_gt == nullptr) {
    uint64_t a = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += CP_THREADS) a += ((uint64_t)blk_gt[b] << 32) | blk_eq[b];
    a = block_reduce_u64(a, lds);
    gt0 = a >> 32; eq0 = a & 0xFFFFFFFFull;
  } else {
    gt0 = off_gt[blockIdx.x]; eq0 = off_eq[blockIdx.x];
  }
  // most tiles hold nothing to emit (T << M): skip them on the block counts alone, without touching the keys
  if (blk_gt[blockIdx.x] == 0 && (blk_eq[blockIdx.x] == 0 || eq0 >= need_eq)) return;
  const uint64_t base = (uint64_t)blockIdx.x * CP_TILE + (uint64_t)threadIdx.x * CP_ITEMS;
  uint32_t keys[CP_ITEMS];
  int valid;
  load_tile_keys<SEG>(view, base, keys, valid);
  uint32_t g = 0, q = 0;
#pragma unroll
  for (int k = 0; k < CP_ITEMS; k++)
    if (k < valid) { g += keys[k] > kstar; q += keys[k] == kstar; }
  uint64_t tot;
  // both counts ride one u64 scan: gt in the high half, eq in the low half (each <= 1024 per tile)
  const uint64_t ex = block_exscan_u64(((uint64_t)g << 32) | q, lds, &tot);
  uint64_t gt_before = gt0 + (ex >> 32);
  uint64_t eq_before = eq0 + (ex & 0xFFFFFFFFull);
#pragma unroll
  for (int k = 0; k < CP_ITEMS; k++) {
    if (k < valid) {
      const uint32_t key = keys[k];
      const bool isg = key > kstar, isq = key == kstar;
      if (isg || (isq && eq_before < need_eq)) {
        const uint64_t pos = gt_before + (eq_before < need_eq ? eq_before : need_eq);
        if (pos < n_sel) { sel_ord[pos] = base + k; sel_key[pos] = key; }
      }
      gt_before += isg;
      eq_before += isq;
    }
  }
}

void launch_compact_write(const KeyView& view, SelectState* s, const uint32_t* blk_gt, const uint32_t* blk_eq, const uint64_t* off_gt,
                          const uint64_t* off_eq, const Selection& out, hipStream_t st) {
  if (view.M == 0) return;
  const dim3 grid((unsigned)compact_blocks(view.M));
  if (view.seg_len)
    hipLaunchKernelGGL(compact_write_kernel<true>, grid, dim3(CP_THREADS), 0, st, view, s, blk_gt, blk_eq, off_gt, off_eq,
                       out.sel_ord, out.sel_key, out.n);
  else
    hipLaunchKernelGGL(compact_write_kernel<false>, grid, dim3(CP_THREADS), 0, st, view, s, blk_gt, blk_eq, off_gt, off_eq,
                       out.sel_ord, out.sel_key, out.n);
}

// ------------------------------------------------------------------------------------------------
// 5b. sharded stage B: candidate exchange
//
// A rank enumerates the triangles of ITS contiguous row range, selects its own top-T among them (the same select and
// compaction as above, on its own keys) and writes them — in (i,j,k) order — into a fixed-size record, the *blob*, that
// the caller all-gathers:  header (CAND_HDR_WORDS x u64) | keys[cap] u32 | recs[cap] uint4 {i, j, k, key}.
// The global top-T is a subset of the union of the ranks' top-T lists, and because the row ranges are contiguous and
// ascending with the rank, the concatenation of the blobs in rank order IS in global (i,j,k) order: the merge is the
// same exact select + ordinal-order compaction over the concatenated keys (a segmented KeyView), and every rank gets
// the identical selected list.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cand_emit_kernel(const uint64_t* __restrict__ sel_ord,
                                                        const uint32_t* __restrict__ sel_key,
                                                        const uint2* __restrict__ kcol,
                                                        const uint32_t* __restrict__ ei,
                                                        const uint32_t* __restrict__ ej,
                                                        const SelectState* __restrict__ sel,
                                                        const uint64_t* __restrict__ toff, uint64_t E,
                                                        uint64_t* __restrict__ hdr, uint32_t* __restrict__ keys,
                                                        uint4* __restrict__ recs, uint64_t cap,
                                                        uint64_t want_requested) {
  const uint64_t n_sent = sel->want < cap ? sel->want : cap;  // the select clamps want to what its window held
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    hdr[0] = toff[E];      // triangles this rank enumerated
    hdr[1] = n_sent;
    hdr[2] = sel->kstar;
    hdr[3] = sel->kmin;    // a range containing every key sent
    hdr[4] = sel->kmax;
    // cut: the rank has more triangles than it was allowed to select, and the select window held that many — so keys at
    // or below its threshold stayed behind (had the window held fewer, everything that can matter was sent)
    hdr[5] = (toff[E] > want_requested && sel->want >= want_requested) ? 1ull : 0ull;
  }
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_sent) return;
  const uint2 ke = kcol[sel_ord[p]];
  const uint32_t key = sel_key[p];
  keys[p] = key;
  recs[p] = make_uint4(ei[ke.y], ej[ke.y], ke.x, key);
}

size_t cand_cap(uint32_t T, uint32_t world, int level) {
  const size_t full = ((size_t)T + 1023) / 1024 * 1024;
  if (world <= 1) return full;
  size_t base = 2 * (((size_t)T + world - 1) / world);
  if (base < 4096) base = 4096;
  if (level > 0) base = level >= 30 ? full : base << level;
  if (level < 0) base = base >> (-level > 30 ? 30 : -level);
  size_t c = (base + 1023) / 1024 * 1024;
  if (c < 1024) c = 1024;
  return c < full ? c : full;
}
size_t cand_blob_bytes(size_t cap) { return CAND_HDR_WORDS * 8 + cap * (4 + 16); }

CandBlob cand_blob(void* blob, size_t cap) {
  CandBlob b;
  unsigned char* p = static_cast<unsigned char*>(blob);
  b.hdr = reinterpret_cast<uint64_t*>(p);
  b.cap = cap;
  b.keys = reinterpret_cast<uint32_t*>(p + CAND_HDR_WORDS * 8);
  b.recs = reinterpret_cast<uint4*>(p + CAND_HDR_WORDS * 8 + b.cap * 4);
  return b;
}

void launch_cand_emit(const Selection& sl, const KeyArrays& ka, const EdgeList& el, const EdgeCounts& ec, uint32_t n_max,
                      uint64_t want_requested, const CandBlob& b, hipStream_t st) {
  const unsigned blocks = n_max ? (n_max + 255) / 256 : 1;
  hipLaunchKernelGGL(cand_emit_kernel, dim3(blocks), dim3(256), 0, st, sl.sel_ord, sl.sel_key, ka.kcol, el.ei, el.ej, ka.sel, ec.toff, el.E,
                     b.hdr, b.keys, b.recs, (uint64_t)b.cap, want_requested);
}

__global__ __launch_bounds__(64) void merge_check_kernel(const uint64_t* __restrict__ blobs, uint64_t blob_words,
                                                         uint32_t world, const SelectState* __restrict__ sel,
                                                         uint64_t* __restrict__ host_flag) {
  bool bad = false;
  const uint32_t kstar = sel->kstar;
  for (uint32_t q = threadIdx.x; q < world; q += 64) {
    const uint64_t* h = blobs + (uint64_t)q * blob_words;
    if (h[5] != 0 && !(kstar > (uint32_t)h[2])) bad = true;  // a cut list whose threshold the merged one does not clear
  }
  const uint64_t any = __ballot(bad);
  if (threadIdx.x == 0) publish_host(host_flag, any ? 1ull : 0ull);
}

void launch_merge_check(const void* blobs, size_t blob_bytes, uint32_t world, const SelectState* sel, uint64_t* host_flag,
                        hipStream_t st) {
  hipLaunchKernelGGL(merge_check_kernel, dim3(1), dim3(64), 0, st, static_cast<const uint64_t*>(blobs),
                     (uint64_t)(blob_bytes / 8), world, sel, host_flag);
}

// One wave: adds up the headers of the `world` gathered blobs and arms the select state for the merge.
//   want = min(T, candidates sent);   window: [certified bound or 2.0, 3.0] when known a priori (fast != 0), else the
//   union of the ranks' key ranges.   host_out[0..1] (pinned): T_eff, triangles enumerated by all ranks.
__global__ __launch_bounds__(64) void merge_prepare_kernel(const uint64_t* __restrict__ blobs, uint64_t blob_words,
                                                           uint32_t world, uint32_t T, int fast,
                                                           const uint32_t* __restrict__ klb,
                                                           SelectState* __restrict__ sel,
                                                           uint64_t* __restrict__ host_out,
                                                           uint64_t* __restrict__ host_short) {
  const uint32_t r = threadIdx.x;
  uint64_t m = 0, ns = 0;
  uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
  for (uint32_t q = r; q < world; q += 64) {
    const uint64_t* h = blobs + (uint64_t)q * blob_words;
    m += h[0]; ns += h[1];
    if (h[1] != 0) { kmin = min(kmin, (uint32_t)h[3]); kmax = max(kmax, (uint32_t)h[4]); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m += __shfl_xor(m, o); ns += __shfl_xor(ns, o);
    kmin = min(kmin, (uint32_t)__shfl_xor(kmin, o)); kmax = max(kmax, (uint32_t)__shfl_xor(kmax, o));
  }
  if (r != 0) return;
  const uint64_t want = ns < (uint64_t)T ? ns : (uint64_t)T;
  sel->want_req = 0;
  if (fast) {
    const uint32_t lo = *klb ? *klb : 0x40000000u, hi = 0x40400000u;  // 2.0f, 3.0f
    const uint32_t range_m1 = hi - lo;
    sel->kmin = lo; sel->kmax = hi;
    sel->st[0] = SelSnap{lo, range_m1 == 0 ? 0u : (uint32_t)(32 - __builtin_clz(range_m1)), 1u, 0u, want, 0ull, 0ull, 0ull};
  } else {
    sel->kmin = kmin <= kmax ? kmin : 0u; sel->kmax = kmin <= kmax ? kmax : 0u;
    sel->st[0] = SelSnap{0u, 0u, 0u, 0u, want, 0ull, 0ull, 0ull};
  }
  sel->want = want;  // (what the candidate kernels read if no select runs: an empty view)
  // SC_FLAG_EST_BOUND: the bound in *klb was an estimate.  A rank only ever sends keys at or above it (its select window's
  // floor), so fewer than T entries in all means fewer than T triangles of the whole graph lie above it — unless it certified
  // nothing (0: no pruning) — and the top-T of the pruned graph proves nothing about the full one (sc_tri_prune.hip 3c)
  if (host_short && *klb != 0u && ns < (uint64_t)T) publish_host(host_short, 1ull);
  host_out[1] = m;
  publish_host(host_out, want);
}

void launch_merge_prepare(const void* blobs, size_t blob_bytes, uint32_t world, uint32_t T, bool fast, const uint32_t* klb,
                          SelectState* sel, uint64_t* host_out, uint64_t* host_short, hipStream_t st) {
  hipLaunchKernelGGL(merge_prepare_kernel, dim3(1), dim3(64), 0, st, static_cast<const uint64_t*>(blobs),
                     (uint64_t)(blob_bytes / 8), world, T, fast ? 1 : 0, klb, sel, host_out, host_short);
}

KeyView cand_view(const void* blobs, size_t blob_bytes, uint32_t world, size_t cap) {
  const unsigned char* p = static_cast<const unsigned char*>(blobs);
  KeyView v;
  v.base = reinterpret_cast<const uint32_t*>(p + CAND_HDR_WORDS * 8);
  v.seg_len = cap;
  v.M = (uint64_t)world * v.seg_len;
  v.seg_stride = blob_bytes / 4;
  v.valid = reinterpret_cast<const uint64_t*>(p) + 1;  // hdr[1] = entries sent
  v.valid_stride = blob_bytes / 8;
  v.M_dev = nullptr;
  return v;
}

// ------------------------------------------------------------------------------------------------
// 7. decode: selected position -> ordinal -> edge (binary search in toff) -> r-th common neighbour above j.
//    The list stays in ORDINAL order ((i,j,k) ascending): neighbouring threads hit neighbouring edges, and the hot
//    path never needs the ranked order (see score_argmax_kernel).  launch_rank_order produces it for the stage hook.
// ------------------------------------------------------------------------------------------------
// kcol[ordinal] = {third vertex, edge id}, stored by the key kernels: decode is two lookups, no search (the earlier
// form searched toff for the edge: 12 LDS + 7 global steps per position, 10 us at T = 50 k and 28 us at 400 k).
__global__ __launch_bounds__(256) void tri_decode_kernel(const uint32_t* __restrict__ ei,
                                                         const uint32_t* __restrict__ ej,
                                                         const uint2* __restrict__ kcol,
                                                         const uint64_t* __restrict__ sel_ord, uint32_t T,
                                                         uint32_t* __restrict__ tri) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const uint2 ke = kcol[sel_ord[t]];
  tri[3 * (size_t)t] = ei[ke.y];
  tri[3 * (size_t)t + 1] = ej[ke.y];
  tri[3 * (size_t)t + 2] = ke.x;
}

void launch_tri_decode(const EdgeList& el, const KeyArrays& ka, const Selection& sl, uint32_t T, uint32_t* tri, hipStream_t st) {
  if (T == 0) return;
  hipLaunchKernelGGL(tri_decode_kernel, dim3((T + 255) / 256), dim3(256), 0, st, el.ei, el.ej, ka.kcol, sl.sel_ord, T, tri);
}

// ---- ranked order for the stage hook: sort (~key, position), then gather
__global__ __launch_bounds__(256) void sortkey_kernel(const uint32_t* __restrict__ sel_key, uint32_t T,
                                                      uint64_t* __restrict__ sortkey) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t < T) sortkey[t] = ((uint64_t)(~sel_key[t]) << 32) | (uint64_t)t;
}
__global__ __launch_bounds__(256) void gather_ranked_kernel(const uint64_t* __restrict__ sorted,
                                                            const uint32_t* __restrict__ tri,
                                                            const uint32_t* __restrict__ sel_key, uint32_t T,
                                                            uint32_t* __restrict__ tri_ranked,
                                                            uint32_t* __restrict__ key_ranked) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const uint32_t src = (uint32_t)(sorted[t] & 0xFFFFFFFFull);
  tri_ranked[3 * (size_t)t] = tri[3 * (size_t)src];
  tri_ranked[3 * (size_t)t + 1] = tri[3 * (size_t)src + 1];
  tri_ranked[3 * (size_t)t + 2] = tri[3 * (size_t)src + 2];
  key_ranked[t] = sel_key[src];
}

void launch_rank_order(const uint32_t* tri, const Selection& sl, uint32_t T, uint64_t* sortkey, uint64_t* sorted,
                       void* sort_tmp, size_t sort_bytes, uint32_t* tri_ranked, uint32_t* key_ranked,
                       hipStream_t st) {
  if (T == 0) return;
  hipLaunchKernelGGL(sortkey_kernel, dim3((T + 255) / 256), dim3(256), 0, st, sl.sel_key, T, sortkey);
  launch_sort_u64(sortkey, sorted, T, sort_tmp, sort_bytes, st);
  hipLaunchKernelGGL(gather_ranked_kernel, dim3((T + 255) / 256), dim3(256), 0, st, sorted, tri, sl.sel_key, T,
                     tri_ranked, key_ranked);
}

}  // namespace sc
