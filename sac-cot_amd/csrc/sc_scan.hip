// sc_scan.hip — the exclusive scan u32 -> u64 of the row counts (sc_rows.hip), the per-edge triangle counts, the compaction's tile
// counts and the sort's histograms: one block, look-back, or block sums + down-sweep, by size.  Stage A is sc_compat.hip.
#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_kernels.hpp"

namespace sc {

// ------------------------------------------------------------------------------------------------
// exclusive scan u32 -> u64: block sums, then a down-sweep whose blocks add up the sums before them (two launches);
// beyond SCAN_SELF_MAX tiles a one-block scan of the sums runs in between
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

// range (optional, device): [lo, hi) outside which every input is known to be zero (sharded stage B: the per-edge
// triangle counts of the edges other ranks enumerate) — tiles wholly outside are neither read nor written.
// ... and inside a tile that straddles an end of the range the elements outside it read as zero WITHOUT being read (r05: a host-free
// call's per-edge counts beyond its real edge count are never written — sc_capi.hip, ControlBlock::live_edges)
__device__ __forceinline__ bool scan_live(const uint64_t* __restrict__ range, size_t idx) {
  return !range || ((uint64_t)idx >= range[0] && (uint64_t)idx < range[1]);
}
__device__ __forceinline__ bool scan_tile_dead(const uint64_t* __restrict__ range, size_t tile) {
  if (!range) return false;
  const uint64_t t0 = (uint64_t)tile * SCAN_TILE;
  return t0 + SCAN_TILE <= range[0] || t0 >= range[1];
}

// ---- a tile of the scans, coalesced (r05).  By time stamps inside the look-back kernel's tiles a tile's life was 3 us of loads + local scan
// and 3 us of stores around 1 us of look-back: every thread owned SCAN_ITEMS CONSECUTIVE elements, so a wave's load touched 64 pieces 64
// bytes apart and its 8-byte stores 64 lines each, sixteen times over.  Now a tile is SCAN_SUB sub-tiles of 1024 elements and a thread takes
// four consecutive elements of each: a wave reads 1 KiB and writes 2 KiB at a stretch (C2: scan_lookback_kernel 11.7 -> 9.3 us).  A piece
// inside the array is loaded BEFORE `range` is looked at (its two words were a dependent round trip at the head of the chain) and masked
// afterwards: what lies beyond a host-free call's real edge count was never written, but it is the array's own memory.
constexpr int SCAN_SUB = SCAN_ITEMS / 4;
static_assert(SCAN_ITEMS % 4 == 0 && SCAN_THREADS == 256, "sub-tiles of 4 x 256 elements, four waves");
struct ScanTile { uint32_t v[SCAN_SUB][4]; uint64_t ex[SCAN_SUB]; uint64_t tot; bool dead; };
// loads + masks the tile's elements; returns with ex[r] = sum of the tile's elements before this thread's piece of sub-tile r and tot =
// the tile's sum.  wsum: 4 x SCAN_SUB words of LDS; one barrier; every thread of the workgroup calls it.
// (mask_dead: a tile wholly outside `range` reads as zeros — t.dead says so; `range` is looked at only AFTER the loads are on their way)
__device__ __forceinline__ void scan_tile_load(const uint32_t* __restrict__ in, size_t n, size_t tile, const uint64_t* __restrict__ range,
                                               bool mask_dead, uint64_t (*wsum)[SCAN_SUB], ScanTile& t) {
  const size_t tbase = tile * SCAN_TILE + (size_t)threadIdx.x * 4;
  if ((tile + 1) * SCAN_TILE <= n) {  // (block-uniform: ONE branch around all the loads — a branch per piece made the compiler wait for each)
    uint4 q[SCAN_SUB];
#pragma unroll
    for (int r = 0; r < SCAN_SUB; r++) q[r] = *reinterpret_cast<const uint4*>(in + tbase + (size_t)r * 1024);
#pragma unroll
    for (int r = 0; r < SCAN_SUB; r++) { t.v[r][0] = q[r].x; t.v[r][1] = q[r].y; t.v[r][2] = q[r].z; t.v[r][3] = q[r].w; }
  } else {
#pragma unroll
    for (int r = 0; r < SCAN_SUB; r++)
#pragma unroll
      for (int k = 0; k < 4; k++) { const size_t idx = tbase + (size_t)r * 1024 + k; t.v[r][k] = idx < n ? in[idx] : 0u; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool dead = mask_dead && scan_tile_dead(range, tile);  // block-uniform
  t.dead = dead;
  uint64_t inc[SCAN_SUB], mine[SCAN_SUB];
#pragma unroll
  for (int r = 0; r < SCAN_SUB; r++) {
    const size_t idx = tbase + (size_t)r * 1024;
    uint64_t a = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { t.v[r][k] = (!dead && scan_live(range, idx + k)) ? t.v[r][k] : 0u; a += t.v[r][k]; }
    mine[r] = a; inc[r] = a;
  }
  // (wave_inscan's steps for the SCAN_SUB values TOGETHER, step by step: one value after the other, hipcc waits for each sub-tile's
  // load in turn where this form has all four in flight — 19 more s_waitcnt in scan_lookback_kernel, the hot path's scan)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
#pragma unroll
    for (int r = 0; r < SCAN_SUB; r++) {
      const uint64_t x = __shfl_up(inc[r], o);
      if (lane >= o) inc[r] += x;
    }
  if (lane == 63)
#pragma unroll
    for (int r = 0; r < SCAN_SUB; r++) wsum[wave][r] = inc[r];
  __syncthreads();
  uint64_t tot = 0;
#pragma unroll
  for (int r = 0; r < SCAN_SUB; r++) {
    uint64_t before = tot;
#pragma unroll
    for (int w = 0; w < 4; w++) { const uint64_t x = wsum[w][r]; before += w < wave ? x : 0ull; tot += x; }
    t.ex[r] = before + inc[r] - mine[r];
  }
  t.tot = tot;
}
struct ScanEbase { const uint32_t* deg; const uint32_t* degp; uint32_t* ebase; };
// out[i] = pre + (exclusive prefix inside the tile) for the tile's elements below n; eb: see scan_downsweep_kernel
__device__ __forceinline__ void scan_tile_store(uint64_t* __restrict__ out, size_t n, size_t tile, uint64_t pre, const ScanTile& t, const ScanEbase& eb) {
  const size_t tbase = tile * SCAN_TILE + (size_t)threadIdx.x * 4;
  const bool whole = (tile + 1) * SCAN_TILE <= n;  // block-uniform
#pragma unroll
  for (int r = 0; r < SCAN_SUB; r++) {
    const size_t idx = tbase + (size_t)r * 1024;
    uint64_t o4[4], run = pre + t.ex[r];
#pragma unroll
    for (int k = 0; k < 4; k++) { o4[k] = run; run += t.v[r][k]; }
    if (whole) {
      typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
      u64x2* dst = reinterpret_cast<u64x2*>(out + idx);  // (idx is a multiple of 4: 32-byte aligned)
      dst[0] = u64x2{o4[0], o4[1]}; dst[1] = u64x2{o4[2], o4[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) if (idx + k < n) out[idx + k] = o4[k];
    }
    if (eb.ebase)
#pragma unroll
      for (int k = 0; k < 4; k++) if (idx + k < n) eb.ebase[idx + k] = (uint32_t)o4[k] - (eb.deg[idx + k] - eb.degp[idx + k]);
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_block_sums_kernel(const uint32_t* __restrict__ in, size_t n,
                                                                       uint64_t* __restrict__ bsum,
                                                                       const uint64_t* __restrict__ range) {
  __shared__ uint64_t wsum[4][SCAN_SUB];
  if (scan_tile_dead(range, blockIdx.x)) { if (threadIdx.x == 0) bsum[blockIdx.x] = 0; return; }
  ScanTile t;
  scan_tile_load(in, n, blockIdx.x, range, false, wsum, t);
  if (threadIdx.x == 0) bsum[blockIdx.x] = t.tot;
}

__global__ __launch_bounds__(1024) void scan_of_sums_kernel(uint64_t* __restrict__ bsum, size_t nb,
                                                            uint64_t* __restrict__ total_out,
                                                            uint64_t* __restrict__ host_total) {
  __shared__ uint64_t lds[16];
  uint64_t carry = 0;
  for (size_t b0 = 0; b0 < nb; b0 += 1024) {
    const size_t b = b0 + threadIdx.x;
    const uint64_t v = b < nb ? bsum[b] : 0;
    uint64_t tot;
    const uint64_t ex = block_exscan_u64(v, lds, &tot);
    if (b < nb) bsum[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    *total_out = carry;
    if (host_total) publish_host(host_total, carry);
  }
}

// SELF: every block sums the raw block sums before it by itself (<= SCAN_SELF_MAX of them, from L2) and the last one
// writes the total — the single-block scan-of-sums launch (a ~4.6 us floor) disappears.
// eb (optional): also ebase[i] = (u32) out[i] - (deg[i] - degp[i]), the CSR base of row i (see launch_edge_fill)
template <bool SELF>
__global__ __launch_bounds__(SCAN_THREADS) void scan_downsweep_kernel(const uint32_t* __restrict__ in, size_t n,
                                                                      const uint64_t* __restrict__ bsum,
                                                                      uint64_t* __restrict__ out,
                                                                      uint64_t* __restrict__ host_total,
                                                                      const uint64_t* __restrict__ range,
                                                                      ScanEbase eb) {
  __shared__ uint64_t lds[8];
  __shared__ uint64_t wsum[4][SCAN_SUB];
  const bool outside = scan_tile_dead(range, blockIdx.x);  // block-uniform
  if (outside && !(SELF && blockIdx.x == gridDim.x - 1)) return;  // (the last tile of the SELF form still owes out[n])
  ScanTile t;
  scan_tile_load(in, n, blockIdx.x, range, false, wsum, t);
  uint64_t pre;
  if (SELF) {
    uint64_t a = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += SCAN_THREADS) a += bsum[b];
    pre = block_reduce_u64(a, lds);
  } else {
    pre = bsum[blockIdx.x];
  }
  if (!outside) scan_tile_store(out, n, blockIdx.x, pre, t, eb);  // (a tile wholly outside the range is never written, in any form)
  if (SELF && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    out[n] = pre + t.tot;
    if (host_total) publish_host(host_total, pre + t.tot);
  }
}

// Single-pass form (decoupled look-back, sc_block.hpp): one launch instead of block sums + down-sweep.
// lb: ticket (zero between launches: the last tile resets it), error flag, one descriptor per tile, this launch's epoch.
__global__ __launch_bounds__(SCAN_THREADS) void scan_lookback_kernel(const uint32_t* __restrict__ in, size_t n,
                                                                     uint64_t* __restrict__ out, LbArgs lb,
                                                                     uint64_t* __restrict__ host_total,
                                                                     const uint64_t* __restrict__ range, ScanEbase eb) {
  __shared__ uint32_t s_tile;
  __shared__ uint64_t s_prefix;
  uint32_t* ticket = lb.ticket;
  const uint32_t epoch = lb.epoch;
  if (threadIdx.x == 0) s_tile = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const uint32_t tile = s_tile;
  if (tile >= gridDim.x) return;  // (a ticket that was not zero at launch: never index memory with it)
  __shared__ uint64_t wsum[4][SCAN_SUB];
  ScanTile t;
  scan_tile_load(in, n, tile, range, true, wsum, t);  // (a tile wholly outside the range: known zeros, never written)
  const bool dead = t.dead;
  const uint64_t tot = t.tot;
  if (threadIdx.x < 64) {
    uint64_t* const desc[1] = {lb.desc};
    const uint64_t own[1] = {tot};
    uint64_t pre[1];
    lb_lookback<1>(desc, tile, epoch, own, pre, lb.err);
    if (threadIdx.x == 0) s_prefix = pre[0];
  }
  __syncthreads();
  const uint64_t pre = s_prefix;
  if (!dead) scan_tile_store(out, n, tile, pre, t, eb);
  if (tile == gridDim.x - 1 && threadIdx.x == 0) {
    out[n] = pre + tot;
    if (host_total) publish_host(host_total, pre + tot);
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // every tile has taken its ticket
  }
}

// small inputs: ONE block scans up to two arrays in one launch (three launches of the tiled scan are pure latency there)
__global__ __launch_bounds__(1024) void scan_small_kernel(const uint32_t* __restrict__ in0, uint64_t* __restrict__ out0,
                                                          const uint32_t* __restrict__ in1, uint64_t* __restrict__ out1,
                                                          size_t n, uint64_t* __restrict__ host_total) {
  __shared__ uint64_t lds[16];
  constexpr int PER = 8;  // consecutive elements per thread and pass: 8192 per pass, so a few passes at most
  const int arrays = in1 ? 2 : 1;
  for (int a = 0; a < arrays; a++) {
    const uint32_t* in = a ? in1 : in0;
    uint64_t* out = a ? out1 : out0;
    uint64_t carry = 0;
    for (size_t b0 = 0; b0 < n; b0 += 1024 * PER) {
      const size_t base = b0 + (size_t)threadIdx.x * PER;
      uint32_t v[PER];
      uint64_t sum = 0;
#pragma unroll
      for (int k = 0; k < PER; k++) { v[k] = (base + k < n) ? in[base + k] : 0u; sum += v[k]; }
      uint64_t tot;
      uint64_t run = carry + block_exscan_u64(sum, lds, &tot);
#pragma unroll
      for (int k = 0; k < PER; k++) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
      }
      carry += tot;
    }
    if (threadIdx.x == 0) {
      out[n] = carry;
      if (a == 0 && host_total) publish_host(host_total, carry);
    }
  }
}

constexpr size_t SCAN_SMALL_MAX = 8192;  // one pass of the single block; beyond it the tiled form is faster (N = 20 000: 26 -> ~9 us)
// Tuning::scan_self_max (4096 tiles = 16.7 M elements): beyond it the scan of sums is its own launch

void launch_scan_u32_pair(const ScanWork& w, const ScanJob& a, const ScanJob& b, size_t n, hipStream_t st) {
  if (n <= SCAN_SMALL_MAX) {
    hipLaunchKernelGGL(scan_small_kernel, dim3(1), dim3(1024), 0, st, a.in, a.out, b.in, b.out, n, a.x.host_total);
  } else {
    launch_scan_u32(w, a.in, n, a.out, a.x, st);
    if (b.in) {
      ScanExtra xb = b.x;
      xb.host_total = nullptr;
      launch_scan_u32(w, b.in, n, b.out, xb, st);
    }
  }
}

bool scan_writes_ebase(size_t n) { return n > SCAN_SMALL_MAX; }

size_t scan_temp_bytes(size_t n) { return ((n + SCAN_TILE - 1) / SCAN_TILE + 4) * sizeof(uint64_t); }

void launch_scan_u32(const ScanWork& w, const uint32_t* in, size_t n, uint64_t* out, const ScanExtra& x, hipStream_t st) {
  const ScanEbase eb{x.deg, x.degp, x.ebase};
  const uint64_t* range = x.range;
  const Tuning& tn = w.tn;
  uint64_t* host_total = x.host_total;
  if (n <= SCAN_SMALL_MAX) {
    hipLaunchKernelGGL(scan_small_kernel, dim3(1), dim3(1024), 0, st, in, out, (const uint32_t*)nullptr,
                       (uint64_t*)nullptr, n, host_total);
    return;
  }
  uint64_t* bsum = static_cast<uint64_t*>(w.temp);
  const size_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
  if (nb == 0) return;  // n == 0 is handled by the small path above
  // single-pass form while the look-back stays shallow (r02: 116 tiles 10.6 us against 4.9 + 7.9; 781 tiles 16.4 against
  // 5.0 + 9.4 — every 64 tiles are one more dependent round of descriptor loads)
  if (x.lb.epoch && x.lb.desc && x.lb.ticket && tn.scan_self_max != 0 && nb <= (size_t)(range ? 512 : 256)) {  // (tiles outside a range publish a zero at once: a trimmed launch may be longer)
    hipLaunchKernelGGL(scan_lookback_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, st, in, n, out, x.lb, host_total,
                       range, eb);
    return;
  }
  hipLaunchKernelGGL(scan_block_sums_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, st, in, n, bsum, range);
  if (nb <= tn.scan_self_max) {  // (a test sets scan_self_max = 0 to force the three-kernel form)
    hipLaunchKernelGGL(scan_downsweep_kernel<true>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, st, in, n, bsum, out,
                       host_total, range, eb);
  } else {
    hipLaunchKernelGGL(scan_of_sums_kernel, dim3(1), dim3(1024), 0, st, bsum, nb, out + n, host_total);
    hipLaunchKernelGGL(scan_downsweep_kernel<false>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, st, in, n, bsum, out,
                       (uint64_t*)nullptr, range, eb);
  }
}


}  // namespace sc
