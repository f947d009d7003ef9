// sc_tri_edges.hip — stage B, the CSR edge list: edge_fill, edge_build and the row emitter they share (sc_tri.hpp: the pipeline).
#include "sc_tri.hpp"

namespace sc {

// A row's upper-triangle edges, as edge_fill_kernel and edge_build_kernel emit them.  RowSide: what every edge of row i
// needs of the row itself — its correspondence (wave-uniform: scalar loads), the AoS copy behind the planes that the
// other end is gathered from (8 floats per correspondence: two 16-byte loads) and the pair test's constants.
// EdgeOut: the CSR arrays and the entries they hold (writes beyond cap are dropped).
struct RowSide {
  int i;
  float px, py, pz, qx, qy, qz;
  const float4* __restrict__ aos4;
  Derived dv;
};
struct EdgeOut { uint32_t* __restrict__ ei; uint32_t* __restrict__ ej; float* __restrict__ es; uint64_t cap; };

__device__ __forceinline__ RowSide row_side(const float* __restrict__ planes, int ld, int i, const Derived& dv) {
  return RowSide{i, planes[i], planes[ld + i], planes[2 * ld + i], planes[3 * ld + i], planes[4 * ld + i], planes[5 * ld + i],
                 reinterpret_cast<const float4*>(planes + 6 * (size_t)ld), dv};
}

// One wave, one round of 64 words of the row: lane holds word w with only the bits above the diagonal left in v; the edges go
// to base, base + 1, ... in column order.  CH column indices are staged per chunk in l_j (this wave's); extra(e, j, weight)
// runs after the three stores of each edge.  Returns the number of edges of the round.
template <int CH, typename Extra>
__device__ __forceinline__ uint32_t row_edges_emit(uint32_t* l_j, uint64_t v, int w, uint64_t base, const RowSide& row,
                                                   const EdgeOut& out, Extra extra) {
  const int lane = threadIdx.x & 63;
  uint32_t tot;
  const uint32_t r = group_exscan<64>((uint32_t)__popcll(v), &tot);
  for (uint32_t c0 = 0; c0 < tot; c0 += CH) {  // wave-uniform; one chunk unless the row is very dense
    // (1) divergent part, LDS only: the columns of this chunk in ascending order
    uint64_t vv = v;
    uint32_t rr = r - c0;  // modular: positions outside [0, CH) are skipped
    while (vv) {
      const int b = __builtin_ctzll(vv);
      vv &= vv - 1;
      if (rr < (uint32_t)CH) l_j[rr] = (uint32_t)(w * 64 + b);
      rr++;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // LDS is in-order within a wave
    // (2) flat part, one lane per edge: gathers, weight, coalesced stores
    const uint32_t cnt = min((uint32_t)CH, tot - c0);
    for (uint32_t t = lane; t < cnt; t += 64) {
      const uint32_t j = l_j[t];
      const uint64_t e = base + c0 + t;
      if (e >= out.cap) continue;
      const float4 a4 = row.aos4[2 * (size_t)j], b4 = row.aos4[2 * (size_t)j + 1];
      const float dp = dist3(row.px, row.py, row.pz, a4.x, a4.y, a4.z);
      const float dq = dist3(row.qx, row.qy, row.qz, a4.w, b4.x, b4.y);
      bool edge;
      const float sw = pair_weight(dp, dq, row.dv.d_thr, row.dv.min_len, row.dv.neg_inv2sig2, edge);
      out.ei[e] = (uint32_t)row.i;
      out.ej[e] = j;
      out.es[e] = sw;
      extra(e, j, sw);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // l_j is rewritten by the next chunk
  }
  return tot;
}

// ------------------------------------------------------------------------------------------------
// 1. edge_fill: one wave per row
// ------------------------------------------------------------------------------------------------
// The edge weight is RECOMPUTED from the two correspondences with stage A's own chain (pair_weight over dist3: the
// same correctly rounded operations on the same operands give the same bits; the squares make the argument order
// irrelevant) instead of being gathered from S: a gather moves a 64-byte sector of the n x n matrix for 4 useful
// bytes (C3: 215 us), the recomputation is ~80 VALU operations on points that sit in L2.
__global__ __launch_bounds__(256) void edge_fill_kernel(const uint64_t* __restrict__ bits,
                                                        const float* __restrict__ planes, Derived dv,
                                                        int n, int ld, int W,
                                                        const uint64_t* __restrict__ edge_off,
                                                        uint32_t* __restrict__ ei, uint32_t* __restrict__ ej,
                                                        float* __restrict__ es,
                                                        const uint32_t* __restrict__ deg,
                                                        const uint32_t* __restrict__ degp,
                                                        uint32_t* __restrict__ ebase, int ebase_ready,
                                                        uint32_t* __restrict__ ebi,
                                                        uint32_t* __restrict__ ebj, uint64_t cap,
                                                        uint32_t* __restrict__ es_hist) {
  // cap: entries the edge arrays hold.  The host may launch this kernel BEFORE it knows the edge count (into the
  // arrays of the previous call, while it polls for the count); writes beyond cap are dropped and the host re-runs.
  // es_hist (optional): the 256-bin histogram of the edge weights that sizes the heaviest-edge pruning sample (§3b;
  // PR_HCOPIES global copies) — collected here, where the weights are made, instead of by a launch of its own (7 us).
  constexpr int CH = 512;  // column indices staged per wave and chunk
  __shared__ uint32_t l_j[4][CH];
  __shared__ uint32_t l_h[2][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (es_hist) {
    l_h[0][threadIdx.x] = 0u; l_h[1][threadIdx.x] = 0u;
    __syncthreads();
  }
  if (i < n) {
  uint64_t base = edge_off[i];
  // CSR base of row i: edge_off[i] - (# bits of row i at or below i) = edge_off[i] - (deg - deg+), modular u32.
  // ebase_ready: the (tiled) scan of deg+ wrote every row's base already, so the base of the OTHER end is one gather;
  // otherwise (small n: a one-block scan, where the extra loads cost more than they save here) it is derived on the fly
  // from three and this wave records its own row's.
  const uint32_t my_base = ebase_ready ? ebase[i] : (uint32_t)base - (deg[i] - degp[i]);
  if (!ebase_ready && lane == 0) ebase[i] = my_base;
  const int w0 = i >> 6;
  const RowSide row = row_side(planes, ld, i, dv);
  const EdgeOut out{ei, ej, es, cap};
  for (int wb = w0; wb < W; wb += 64) {
    const int w = wb + lane;
    uint64_t v = 0;
    if (w < W) {
      v = bits[(size_t)i * W + w];
      if (w == w0) v &= mask_above(i & 63);
    }
    base += row_edges_emit<CH>(l_j[wave], v, w, base, row, out, [&](uint64_t e, uint32_t j, float sw) {
      if (es_hist) atomicAdd(&l_h[lane & 1][weight_bin(__float_as_uint(sw), 0u, 0u)], 1u);  // integer sums: order-free
      // both CSR bases travel with the edge, so stage B fetches an edge in ONE memory level
      ebi[e] = my_base;
      ebj[e] = ebase_ready ? ebase[j] : (uint32_t)edge_off[j] - (deg[j] - degp[j]);
    });
  }
  }  // i < n
  if (es_hist) {
    __syncthreads();
    const uint32_t v = l_h[0][threadIdx.x] + l_h[1][threadIdx.x];
    if (v) atomicAdd(&es_hist[(size_t)(blockIdx.x & (PR_HCOPIES - 1)) * 256 + threadIdx.x], v);
  }
}

void launch_edge_fill(const Graph& g, const Points& pts, const Derived& dv, const uint64_t* edge_off, const EdgeList& el,
                      bool ebase_ready, uint32_t* es_hist, hipStream_t st) {
  hipLaunchKernelGGL(edge_fill_kernel, dim3((g.n + 3) / 4), dim3(256), 0, st, g.bits, pts.planes, dv, g.n, g.ld, g.W,
                     edge_off, el.ei, el.ej, el.es, g.deg, g.degp, el.ebase, ebase_ready ? 1 : 0, el.ebi, el.ebj, el.cap, es_hist);
}

// ------------------------------------------------------------------------------------------------
// 1'. edge_build (r04): everything between stage A and the estimating sample in ONE launch — the hot path's form of
//     row_stats_scan + edge_fill (two launches, 29.5 us at C2).
//
// What made the row kernel a launch of its own was the prefix over the rows: a wave cannot place row i's edges before it
// knows how many edges the rows before it hold, and counting them meant reading their bit rows.  Stage A now leaves
// deg+[i] behind (atomics where the adjacency words are made, sc_compat.hip), so a workgroup of EBK_ROWS waves sums
// deg+[0 .. its first row) itself — a few 16-byte loads per thread, no look-back, no cross-workgroup dependency — and then
// each wave, for its row: word-prefix popcounts (wpre), the CSR offset and base, the strong-bit row cleared, the row's
// edges with their recomputed weights (as edge_fill_kernel).
// (r04 also took the ESTIMATING sample here — sampled triangles recomputed from the correspondences through a per-wave LDS
// queue: 50.3 us against 16.4 + 13.7 for the two launches, a dense row being one wave's serial chain; removed in r05,
// profiles/r04_ab_edge_build.txt keeps the numbers.)
// The CSR bases of an edge's OTHER end (ebj) are not known here (row j's wave may not have run): the counting pass looks
// them up in ebase instead (one more gather, beside its row loads).  n <= 64 * EBK_WMAX only.
// ------------------------------------------------------------------------------------------------
constexpr int EBK_ROWS = 8;     // rows (waves) per workgroup
constexpr int EBK_CH = 256;     // column indices staged per wave and chunk
constexpr int EBK_WMAX = 320;   // words per bit row it can handle (n <= 20 480): NCH = 2 chunks of 64 words up to 8192, 5 beyond

template <int NCH>  // 64-word chunks of a bit row: W <= 64 NCH
__global__ __launch_bounds__(64 * EBK_ROWS) void edge_build_kernel(const uint64_t* __restrict__ bits,
                                                                   const float* __restrict__ planes, Derived dv, int n,
                                                                   int ld, int W, const uint32_t* __restrict__ degp,
                                                                   uint32_t* __restrict__ wpre,
                                                                   uint64_t* __restrict__ zero_rows,
                                                                   uint64_t* __restrict__ edge_off,
                                                                   uint32_t* __restrict__ ebase,
                                                                   uint32_t* __restrict__ ei, uint32_t* __restrict__ ej,
                                                                   float* __restrict__ es, uint64_t cap,
                                                                   uint64_t* __restrict__ host_total,
                                                                   uint64_t* __restrict__ live_range) {
  __shared__ uint64_t s_red[EBK_ROWS];
  __shared__ uint32_t l_j[EBK_ROWS][EBK_CH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * EBK_ROWS, i = r0 + wave;
  // edges of the rows before this workgroup's (r0 is a multiple of 4: whole 16-byte pieces)
  uint64_t acc = 0;
  {  // (four 16-byte loads in flight: the loop's trips were dependent round trips — up to three for the last rows at C2, ten at C3)
    constexpr int QS = 64 * EBK_ROWS * 4;
    int q = tid * 4;
    for (; q + 3 * QS < r0; q += 4 * QS) {
      const uint4 v0 = *reinterpret_cast<const uint4*>(degp + q), v1 = *reinterpret_cast<const uint4*>(degp + q + QS),
                  v2 = *reinterpret_cast<const uint4*>(degp + q + 2 * QS), v3 = *reinterpret_cast<const uint4*>(degp + q + 3 * QS);
      acc += ((uint64_t)v0.x + v0.y + v0.z + v0.w) + ((uint64_t)v1.x + v1.y + v1.z + v1.w) + ((uint64_t)v2.x + v2.y + v2.z + v2.w) +
             ((uint64_t)v3.x + v3.y + v3.z + v3.w);
    }
    uint4 w[3];
    int nw = 0;
#pragma unroll
    for (int u = 0; u < 3; u++) { const bool in = q + u * QS < r0; w[u] = in ? *reinterpret_cast<const uint4*>(degp + q + u * QS) : make_uint4(0u, 0u, 0u, 0u); nw += in; }
#pragma unroll
    for (int u = 0; u < 3; u++) acc += (uint64_t)w[u].x + w[u].y + w[u].z + w[u].w;
    (void)nw;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) s_red[wave] = acc;
  __syncthreads();
  if (i >= n) return;
  uint64_t my_off = 0;
#pragma unroll
  for (int w8 = 0; w8 < EBK_ROWS; w8++) my_off += s_red[w8];
  for (int r = r0; r < i; r++) my_off += degp[r];  // wave-uniform: scalar loads
  const int wi = i >> 6, bi = i & 63;
  const RowSide row = row_side(planes, ld, i, dv);
  const EdgeOut out{ei, ej, es, cap};
  // ---- the row's words: prefix popcounts, the strong row cleared (not sc_rows.hip's row_word_stats: this form keeps the
  // upper-triangle words in registers for the edges below and counts the bits BELOW the diagonal, for the CSR base)
  uint32_t d_all = 0, d_low = 0;
  uint64_t up[NCH];
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    const int w = 64 * c + lane;
    const uint64_t v = w < W ? bits[(size_t)i * W + w] : 0ull;
    const uint32_t pc = (uint32_t)__popcll(v);
    uint32_t tot;
    const uint32_t ex = group_exscan<64>(pc, &tot);
    if (w < W) {
      wpre[(size_t)i * W + w] = d_all + ex;
      zero_rows[(size_t)i * W + w] = 0ull;
    }
    d_all += tot;
    const uint64_t below = (1ull << bi) - 1ull;
    d_low += w < wi ? pc : (w == wi ? (uint32_t)__popcll(v & below) : 0u);
    up[c] = w < wi ? 0ull : (w == wi ? (v & mask_above(bi)) : v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d_low += __shfl_xor(d_low, o);
  const uint32_t my_base = (uint32_t)my_off - d_low;
  if (lane == 0) { edge_off[i] = my_off; ebase[i] = my_base; }
  // ---- edges, chunk by chunk
  uint64_t ebase_row = my_off;
#pragma unroll
  for (int c = 0; c < NCH; c++)
    ebase_row += row_edges_emit<EBK_CH>(l_j[wave], up[c], 64 * c + lane, ebase_row, row, out, [](uint64_t, uint32_t, float) {});
  if (i == n - 1 && lane == 0) {  // the last row's wave knows the edge count: the host polls for it
    edge_off[n] = ebase_row;
    if (live_range) { live_range[0] = 0ull; live_range[1] = ebase_row; }
    if (host_total) publish_host(host_total, ebase_row);  // (nullptr: a host-free call reads the count from edge_off[n] — DeferredPub)
  }
}

bool edge_build_fits(int n) { return n <= 64 * EBK_WMAX; }

void launch_edge_build(const Graph& g, const Points& pts, const Derived& dv, uint64_t* zero_rows, uint64_t* edge_off, const EdgeList& el,
                       uint64_t* host_total, uint64_t* live_range, hipStream_t st) {
  const dim3 grid((g.n + EBK_ROWS - 1) / EBK_ROWS), block(64 * EBK_ROWS);
  if (g.W <= 128)
    hipLaunchKernelGGL(edge_build_kernel<2>, grid, block, 0, st, g.bits, pts.planes, dv, g.n, g.ld, g.W, g.degp,
                       const_cast<uint32_t*>(g.wpre), zero_rows, edge_off, el.ebase, el.ei, el.ej, el.es, el.cap, host_total, live_range);
  else
    hipLaunchKernelGGL(edge_build_kernel<5>, grid, block, 0, st, g.bits, pts.planes, dv, g.n, g.ld, g.W, g.degp,
                       const_cast<uint32_t*>(g.wpre), zero_rows, edge_off, el.ebase, el.ei, el.ej, el.es, el.cap, host_total, live_range);
}

}  // namespace sc
