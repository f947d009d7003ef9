// sc_rows.hip — stage B's first step, over the bit rows stage A (sc_compat.hip) wrote: the row statistics (deg, deg+, the word-prefix
// popcounts), their fused form with the CSR row offsets (decoupled look-back over 64-row tiles) and the shard split.  The unfused
// form's scans are sc_scan.hip; the fused edge kernel, which keeps its own copy of the row walk, is sc_tri_edges.hip.
#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_kernels.hpp"

namespace sc {

// What one wave learns from the words of row i (row_stats_kernel, row_stats_scan_kernel): it writes wpre[i][w] = #set bits of
// the row in words [0, w) and clears the row of zero_rows (optional); d_all = the row's degree (wave-uniform); d_up, cost = this
// LANE's share of deg+ (bits above i) and of the row's stage B cost (see rowcost below) — the caller sums them over the wave.
struct RowWordStats { uint32_t d_all, d_up; uint64_t cost; };
__device__ __forceinline__ RowWordStats row_word_stats(const uint64_t* __restrict__ bits, int i, int W, uint32_t* __restrict__ wpre,
                                                       uint64_t* __restrict__ zero_rows) {
  const int lane = threadIdx.x & 63;
  if (zero_rows)
    for (int w = lane; w < W; w += 64) zero_rows[(size_t)i * W + w] = 0ull;
  uint32_t d_all = 0, d_up = 0;
  uint64_t cost = 0;
  for (int wb = 0; wb < W; wb += 64) {
    const int w = wb + lane;
    const uint64_t v = w < W ? bits[(size_t)i * W + w] : 0ull;
    const uint32_t pc = (uint32_t)__popcll(v);
    const uint32_t inc = wave_inscan(pc);  // of the word popcounts
    if (w < W) {
      wpre[(size_t)i * W + w] = d_all + inc - pc;
      uint64_t up = v;
      if (w < (i >> 6)) up = 0;
      else if (w == (i >> 6)) up &= mask_above(i & 63);
      d_up += __popcll(up);
      cost += (uint64_t)__popcll(up) * (uint64_t)(W - w + 4);
    }
    d_all += __shfl(inc, 63);
  }
  return RowWordStats{d_all, d_up, cost};
}

// deg[i], degp[i] (bits above i) and wpre[i][w] = #set bits of row i in words [0, w): one wave per row.
// rowcost (optional): estimate of stage B's work for the edges (i, j), j > i, of row i — the words the counting pass
// ANDs for each of them plus a constant: sum over j of (W - j / 64 + 4), saturated to u32.  Its prefix over the rows
// splits the rows into contiguous, equally heavy ranges when stage B is sharded.
__global__ __launch_bounds__(256) void row_stats_kernel(const uint64_t* __restrict__ bits, int n, int W,
                                                        uint32_t* __restrict__ deg, uint32_t* __restrict__ degp,
                                                        uint32_t* __restrict__ wpre,
                                                        uint64_t* __restrict__ zero_rows,
                                                        uint32_t* __restrict__ rowcost) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  RowWordStats rs = row_word_stats(bits, i, W, wpre, zero_rows);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rs.d_up += __shfl_xor(rs.d_up, o);
  if (rowcost) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rs.cost += __shfl_xor(rs.cost, o);
  }
  if (lane == 0) {
    deg[i] = rs.d_all; degp[i] = rs.d_up;
    if (rowcost) rowcost[i] = rs.cost > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rs.cost;
  }
}

// row_stats + the prefix over the rows in ONE launch ("fold row_stats ..."): a workgroup takes RS_ROWS rows
// (16 waves x RS_RPW rows), computes what row_stats_kernel computes, scans its edge counts (and row costs) in one wave and
// gets the sums of the tiles before it by decoupled look-back (sc_block.hpp) — so edge_off (the CSR row offsets), the
// per-row CSR bases, the cost prefix and the edge count for the host all come out of the kernel that read the bit rows;
// the separate scan launch(es) and their extra pass over deg / deg+ disappear.  157 tiles at N = 5000, 625 at 20 000 (64-row tiles: 14.7 us on C2, fewer CUs busy).
constexpr int RS_ROWS = 32;           // rows per tile: 16 waves x RS_RPW rows
constexpr int RS_RPW = RS_ROWS / 16;  // rows a wave takes, one after the other
__global__ __launch_bounds__(1024) void row_stats_scan_kernel(const uint64_t* __restrict__ bits, int n, int W,
                                                             uint32_t* __restrict__ deg, uint32_t* __restrict__ degp,
                                                             uint32_t* __restrict__ wpre,
                                                             uint64_t* __restrict__ zero_rows,
                                                             uint64_t* __restrict__ edge_off,
                                                             uint32_t* __restrict__ ebase,
                                                             uint64_t* __restrict__ cost_pre, LbArgs lb,
                                                             uint64_t* __restrict__ host_total) {
  __shared__ uint32_t l_degp[RS_ROWS], l_dlow[RS_ROWS];
  __shared__ uint64_t l_cost[RS_ROWS];
  __shared__ uint32_t s_tile;
  uint32_t* ticket = lb.ticket;
  const uint32_t epoch = lb.epoch;
  if (threadIdx.x == 0) s_tile = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const uint32_t tile = s_tile, nb = gridDim.x;
  if (tile >= nb) return;  // (a ticket that was not zero at launch: never index memory with it)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int rr = 0; rr < RS_RPW; rr++) {
    const int slot = wave * RS_RPW + rr;
    const int i = (int)tile * RS_ROWS + slot;
    uint32_t d_all = 0, d_up = 0;
    uint64_t cost = 0;
    if (i < n) {  // wave-uniform
      const RowWordStats rs = row_word_stats(bits, i, W, wpre, zero_rows);
      d_all = rs.d_all; d_up = rs.d_up; cost = rs.cost;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { d_up += __shfl_xor(d_up, o); cost += __shfl_xor(cost, o); }
    }
    if (lane == 0) {
      if (i < n) { deg[i] = d_all; degp[i] = d_up; }
      l_degp[slot] = d_up; l_dlow[slot] = d_all - d_up; l_cost[slot] = cost;
    }
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;  // wave 0: scan of the tile's 64 rows, look-back, outputs
  const uint64_t mine_e = lane < RS_ROWS ? l_degp[lane] : 0u, mine_c = lane < RS_ROWS ? l_cost[lane] : 0ull;
  const uint64_t inc_e = wave_inscan(mine_e), inc_c = wave_inscan(mine_c);
  const uint64_t tot_e = __shfl(inc_e, 63), tot_c = __shfl(inc_c, 63);
  uint64_t* const desc[2] = {lb.desc, lb.desc + nb};
  const uint64_t own[2] = {tot_e, tot_c};
  uint64_t pre[2];
  lb_lookback<2>(desc, tile, epoch, own, pre, lb.err);
  const int i = (int)tile * RS_ROWS + lane;
  if (lane < RS_ROWS && i < n) {
    const uint64_t off = pre[0] + inc_e - mine_e;
    edge_off[i] = off;
    ebase[i] = (uint32_t)off - l_dlow[lane];  // (lane < RS_ROWS here)
    if (cost_pre) cost_pre[i] = pre[1] + inc_c - mine_c;
  }
  if (tile == nb - 1 && lane == 0) {
    edge_off[n] = pre[0] + tot_e;
    if (cost_pre) cost_pre[n] = pre[1] + tot_c;
    if (host_total) publish_host(host_total, pre[0] + tot_e);
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // every tile has taken its ticket
  }
}

size_t row_stats_scan_state_bytes(int n) { return (size_t)(2 * ((n + RS_ROWS - 1) / RS_ROWS)) * sizeof(uint64_t); }

void launch_row_stats_scan(const Points& pts, const uint64_t* bits, const RowStats& rs, const RowOffsets& ro, const LbArgs& lb,
                           uint64_t* host_total, hipStream_t st) {
  hipLaunchKernelGGL(row_stats_scan_kernel, dim3((pts.n + RS_ROWS - 1) / RS_ROWS), dim3(1024), 0, st, bits, pts.n,
                     pts.ld >> 6, rs.deg, rs.degp, rs.wpre, rs.zero_rows, ro.edge_off, ro.ebase, ro.cost_pre, lb, host_total);
}

// Contiguous row range of one rank: rows [lo, hi) with lo = first row whose cost prefix reaches rank / world of the
// total (row 0 for rank 0, n for the end of the last rank).  own_row[0..1] and the CSR edge range own_edge[0..1] of
// those rows go to the control block; every rank computes the same boundaries from the same replicated arrays.
__global__ __launch_bounds__(64) void shard_split_kernel(const uint64_t* __restrict__ cost_pre,
                                                         const uint64_t* __restrict__ edge_off, int n, uint32_t rank,
                                                         uint32_t world, uint32_t* __restrict__ own_row,
                                                         uint64_t* __restrict__ own_edge) {
  // one wave; both boundaries (lo = boundary `rank`, hi = boundary `rank + 1`) by a 64-ary search: every step the 64
  // lanes probe 64 evenly spaced rows at once (3 steps for n = 20 000 instead of 15 dependent loads)
  const int lane = threadIdx.x;
  const uint64_t total = cost_pre[n];
  for (int which = 0; which < 2; which++) {
    const uint32_t l = rank + (uint32_t)which;
    int row;
    if (l == 0) row = 0;
    else if (l >= world) row = n;
    else {
      const uint64_t target = (uint64_t)(((unsigned __int128)total * l) / world);
      int lo = 0, hi = n;  // invariant: the answer (first r in [0, n] with cost_pre[r] >= target) lies in [lo, hi]
      while (hi - lo > 0) {
        const int span = hi - lo, step = (span + 63) / 64;
        const int probe = lo + lane * step;                   // probes lo, lo + step, ... (those < hi are real)
        const bool ge = probe < hi ? (cost_pre[probe] >= target) : true;
        const uint64_t m = __ballot(ge);
        // first probe at or above the target; none (the last real probe is still below it): the answer lies above it
        const int first = m ? __builtin_ctzll(m) : 64;
        if (first == 0) { hi = lo; }                                                // cost_pre[lo] >= target
        else if (first == 64) { lo = lo + 63 * step + 1; }                          // in (probe[63], hi]
        else { const int plo = lo + (first - 1) * step + 1; hi = min(hi, lo + first * step); lo = plo; }  // in (probe[first-1], probe[first]]
      }
      row = lo;
    }
    if (lane == 0) { own_row[which] = (uint32_t)row; own_edge[which] = edge_off[row]; }
  }
}

void launch_row_stats(const Points& pts, const uint64_t* bits, const RowStats& rs, hipStream_t st) {
  hipLaunchKernelGGL(row_stats_kernel, dim3((pts.n + 3) / 4), dim3(256), 0, st, bits, pts.n, pts.ld >> 6, rs.deg, rs.degp,
                     rs.wpre, rs.zero_rows, rs.rowcost);
}

void launch_shard_split(const RowOffsets& ro, const ShardCut& cut, int n, hipStream_t st) {
  hipLaunchKernelGGL(shard_split_kernel, dim3(1), dim3(64), 0, st, (const uint64_t*)ro.cost_pre, (const uint64_t*)ro.edge_off, n, cut.rank,
                     cut.world, cut.own_row, cut.own_edge);
}

}  // namespace sc
