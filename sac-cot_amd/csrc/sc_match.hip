// sc_match.hip — descriptor matching (include/saccot.h, sc_match): brute-force nearest neighbours between two descriptor sets under a
// total order, then mutual / ratio test and an order-preserving compaction.  Two launches:
//
//   match_dist_kernel    all-pairs canonical distance + per-row selection.  Register-tiled like an SGEMM: a workgroup owns 128 source
//                        rows and a SLICE of the target columns, which it walks in tiles of 64; both tiles are staged in LDS in
//                        chunks of 16 components (transposed: component-major, so a thread reads its 8 rows and 4 columns of one
//                        component with three 16-byte reads), every thread carries an 8 x 4 block of sums in registers across the
//                        chunks (the last chunk is cut short at D) — the chain of a pair is sequential in c, D = 1024 needs no
//                        more LDS than D = 16.  The sums are held as pairs of adjacent columns (a 2-vector subtract, multiply, add per pair: no fused multiply-add,
//                        whatever the build's contraction setting).  Zero padding in c is exact: (0 - 0)^2 adds +0 to a sum >= 0.
//                        Selection: a row's KP smallest keys (distance bits << 32 | column) of the slice live in LDS and take
//                        candidates through a cascade of 64-bit minima — slot q keeps the smaller of (what it holds, what arrives)
//                        and passes the larger on to slot q + 1.  Every key goes through slot 0, so slot 0 ends as the minimum of
//                        all; what slot 1 sees is everything else; and so on: the KP smallest in order, whatever the interleaving.
//                        The slice's lists go to workspace (part); the column minima that SC_MATCH_MUTUAL needs combine through
//                        LDS and then global 64-bit atomic minima (a minimum is order-free: deterministic).  A non-finite
//                        descriptor clears the `clean` word: every element is read by some workgroup.
//   match_finish_kernel  one thread per source row: merges the row's slices under the same order, applies mutual / ratio, takes its
//                        output slots from a decoupled look-back over the tiles (sc_block.hpp, as peel_compact_kernel), writes
//                        corr / d2 in ascending (row, rank) order, gathers the matched points for sc_register_features, and the
//                        last tile writes the count and the non-finite flag.
//
// What the two kernels share with sc_match_batch.hip's is said once, in sc_match_tile.hpp: tile_step and top_insert, the finish
// kernel's row decision (row_kept) and entry write (entry_write, entry_resid), the pose-record accessors and the not-finite scan.
// The chunk loop, the selection block and the column-minimum flush stay written out in both distance kernels: moved into shared
// templates they cost this file's gated instantiations an occupancy step or, under a launch bound, time; as they stand the distance
// kernels compile to the instructions they had before the finish steps were shared.
//
// sc_match_guided (GUIDED) is the same pair of launches with a pose prior: a cell (i, j) is a candidate only where the canonical
// residual of the inlier test, resid2(Rt, src_pts[i], tgt_pts[j]) (sc_arith.hpp), is below gate2.  The distance launch stages the
// workgroup's 128 source points once and a tile's 64 target points per tile, every thread folds its 8 x 4 decisions into one 32-bit
// word BEFORE the descriptor chunks (the points are not live across the accumulate loop), an inadmissible cell offers no key — not to
// the row's list, not to the column minimum — and a tile in which no cell of the workgroup is admissible is skipped altogether: no
// descriptor load, no tile_step (the decision is a workgroup-wide OR behind a barrier every thread passes).  Because a skipped tile's
// descriptors are never staged, the finiteness rule is carried by a scan of its own in the same launch: every workgroup tests a
// grid-strided share of both descriptor arrays, both point arrays and the pose.  The finish launch can also emit g2 per entry.
//
// sc_match_guided_poses (GATE_POSES) gates by the union over up to 64 pose records: a cell is a candidate where SOME used record's
// residual is below gate2.  The records are staged once per workgroup in LDS (a record that SC_GUIDE_POSE_STATUS switches off stages
// nothing: its bit in s_used stays clear, its floats are neither read nor tested) and a cell walks the used records until one admits
// it — the pose lives in LDS, not in registers, so nothing of it is carried across the accumulate loop.  Everything behind the word
// `adm` is the single-pose kernel's.  The finish launch evaluates every used record for the at most ns * knn output entries only:
// label = the record of the smallest residual (ties: the lowest index), g2 = that minimum.
#include <cstddef>
#include <type_traits>

#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_kernels.hpp"
#include "sc_match_tile.hpp"

#pragma clang fp contract(off)  // the canonical distance rounds the product and the sum separately

namespace sc {

namespace {

constexpr int MT_ROWS = 128, MT_COLS = 64, MT_THREADS = 256;  // (MT_KC, the key, tile_step and top_insert: sc_match_tile.hpp, shared with sc_match_batch.hip)
constexpr int MT_LDA = MT_ROWS + 4, MT_LDB = MT_COLS + 4;  // 16-byte aligned rows; the pad spreads the transposing stores over the banks
constexpr int FIN_THREADS = 256;

// sc_match's kernel takes no guide: an empty argument
struct NoGuide {};

// the gate of a distance launch: none (sc_match), one pose (sc_match_guided), the union over pose records (sc_match_guided_poses)
// (plain ints, not an enum: the kernel's signature names the gate in an expression, and an unnamed type is numbered differently in
// the host's and the device's mangling — the stub would register a name the code object does not hold)
constexpr int GATE_NONE = 0, GATE_POSE = 1, GATE_POSES = 2;
constexpr int MT_POSES = (int)SC_GUIDE_MAX_POSES;
static_assert(MT_POSES == 64, "s_used is one 64-bit word, filled by one ballot of a 64-lane wave");

// The distance launch, said once.  GATE_NONE is sc_match's kernel; GATE_POSE adds the gate; GATE_POSES the gate of several poses.
// The chunk loop, the selection and the flush are this kernel's own text, as they are sc_match_batch.hip's: as shared templates they
// cost the gated instantiations a wave per SIMD, and under a launch bound that restored the wave 0.5 % of a call
// (profiles/match_shared.txt).
template <int KP, int GATE>
__global__ __launch_bounds__(MT_THREADS) void match_dist_kernel(const float* __restrict__ fsrc, uint32_t ns,
                                                                const float* __restrict__ ftgt, uint32_t nt, uint32_t D,
                                                                uint32_t tiles_per_slice, unsigned long long* __restrict__ part,
                                                                size_t ld_part, unsigned long long* __restrict__ colmin,
                                                                uint32_t* __restrict__ clean,
                                                                typename std::conditional<GATE != GATE_NONE, MatchGuide, NoGuide>::type gd) {
  constexpr bool GUIDED = GATE != GATE_NONE, POSES = GATE == GATE_POSES;
  __shared__ __attribute__((aligned(16))) float sA[MT_KC][MT_LDA];
  __shared__ __attribute__((aligned(16))) float sB[MT_KC][MT_LDB];
  __shared__ unsigned long long s_top[MT_ROWS][KP];
  __shared__ unsigned long long s_col[MT_COLS];
  __shared__ float sP[GUIDED ? 3 : 1][GUIDED ? MT_ROWS : 1];  // the workgroup's source points, component-major
  __shared__ float sQ[GUIDED ? 3 : 1][GUIDED ? MT_COLS : 1];  // the tile's target points
  __shared__ __attribute__((aligned(16))) float sM[POSES ? MT_POSES : 1][12];  // GATE_POSES: the used records' floats
  __shared__ unsigned long long s_used;                                        // ... and bit k: record k is used
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;  // the thread's 4 columns / 8 rows; also (component, row) when it loads
  const uint32_t row0 = blockIdx.x * MT_ROWS;
  const uint32_t n_tiles = (nt + MT_COLS - 1) / MT_COLS;
  const uint32_t tile_lo = blockIdx.y * tiles_per_slice;
  const uint32_t tile_hi = tile_lo + tiles_per_slice < n_tiles ? tile_lo + tiles_per_slice : n_tiles;
  for (int e = threadIdx.x; e < MT_ROWS * KP; e += MT_THREADS) (&s_top[0][0])[e] = KEY_NONE;
  bool bad = false;
  float M[POSES ? 1 : 12];  // GATE_POSE: the pose (wave-uniform)
  uint32_t adm = 0;         // GUIDED: bit r * 4 + cc: cell (row r, column cc) of this thread is admissible in this tile
  if constexpr (GUIDED) {
    if constexpr (POSES) {
      // every workgroup stages (and tests) the used records; the tiles' first barrier publishes them
      for (uint32_t e = threadIdx.x; e < gd.n_poses * 12u; e += MT_THREADS) {
        const uint32_t k = e / 12u, f = e % 12u;
        const float* rec = pose_record(gd, k);
        if (!pose_used(gd, rec)) continue;
        const float v = rec[f];
        bad = bad || not_finite(v);
        sM[k][f] = v;
      }
      if (threadIdx.x < 64) {  // (the first wave, whole)
        const unsigned long long used = __ballot(threadIdx.x < gd.n_poses && pose_used(gd, pose_record(gd, threadIdx.x)));
        if (threadIdx.x == 0) s_used = used;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 12; k++) { M[k] = gd.Rt[k]; bad = bad || not_finite(M[k]); }
    }
    // the finiteness rule depends on the input alone: every element is tested here, whatever tiles the gate drops below
    const size_t stride = (size_t)gridDim.x * gridDim.y * MT_THREADS;
    const size_t me = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * MT_THREADS + threadIdx.x;
    bad = scan_not_finite(fsrc, (size_t)ns * D, me, stride) || bad;
    bad = scan_not_finite(ftgt, (size_t)nt * D, me, stride) || bad;
    bad = scan_not_finite(gd.src, (size_t)ns * 3, me, stride) || bad;  // (either layout: 3 ns contiguous floats)
    bad = scan_not_finite(gd.tgt, (size_t)nt * 3, me, stride) || bad;
    for (int e = threadIdx.x; e < 3 * MT_ROWS; e += MT_THREADS) {
      const uint32_t comp = e / MT_ROWS, lr = e % MT_ROWS, row = row0 + lr;
      sP[comp][lr] = row < ns ? gd.src[(size_t)row * gd.s_elem + (size_t)comp * gd.s_comp] : 0.f;
    }
  }
  for (uint32_t tile = tile_lo; tile < tile_hi; tile++) {
    const uint32_t col0 = tile * MT_COLS;
    if (threadIdx.x < MT_COLS) s_col[threadIdx.x] = KEY_NONE;
    if constexpr (GUIDED) {
      // (nobody still reads the tile before: its last read of sQ is in front of that tile's OR barrier, which every thread has passed)
      if (threadIdx.x < 3 * MT_COLS) {
        const uint32_t comp = threadIdx.x / MT_COLS, lc = threadIdx.x % MT_COLS, col = col0 + lc;
        sQ[comp][lc] = col < nt ? gd.tgt[(size_t)col * gd.t_elem + (size_t)comp * gd.t_comp] : 0.f;
      }
      __syncthreads();  // sQ (and, first tile, sP, the lists' and s_col's initial values) are written
      // One cell at a time, rolled: unrolled, the 32 independent chains are scheduled side by side and the kernel needs 190 to 230
      // registers (two waves per SIMD instead of sc_match's three); rolled it stays within the accumulate loop's budget.  The reads
      // are conflict-free: a wave's 4 rows are 8 words apart, its 16 columns 4 words.
      adm = 0;
      if constexpr (POSES) {
        const unsigned long long used = s_used;  // (workgroup-uniform)
#pragma unroll 1
        for (int cell = 0; cell < 32; cell++) {
          const uint32_t lr = ty * 8 + (cell >> 2), lc = tx * 4 + (cell & 3);
          if (!(row0 + lr < ns && col0 + lc < nt)) continue;
          const float px = sP[0][lr], py = sP[1][lr], pz = sP[2][lr], qx = sQ[0][lc], qy = sQ[1][lc], qz = sQ[2][lc];
          // the OR over the used records of the single-pose test (the same chain, the pose read from LDS: a broadcast); the cell
          // leaves at its first admitting record
          bool ok = false;
#pragma unroll 1
          for (unsigned long long m = used; m != 0ull && !ok; m &= m - 1ull)
            ok = resid2(sM[__builtin_ctzll(m)], px, py, pz, qx, qy, qz) < gd.gate2;
          adm |= (ok ? 1u : 0u) << cell;
        }
      } else {
#pragma unroll 1
        for (int cell = 0; cell < 32; cell++) {
          const uint32_t lr = ty * 8 + (cell >> 2), lc = tx * 4 + (cell & 3);
          // a float <: a NaN or infinite residual is never admissible
          const bool ok = row0 + lr < ns && col0 + lc < nt &&
                          resid2(M, sP[0][lr], sP[1][lr], sP[2][lr], sQ[0][lc], sQ[1][lc], sQ[2][lc]) < gd.gate2;
          adm |= (ok ? 1u : 0u) << cell;
        }
      }
      // workgroup-uniform, and every thread passes this barrier on both paths; nothing of a skipped tile is a candidate
      if (!__syncthreads_or(adm != 0u)) continue;
    }
    f2 acc[8][2];
#pragma unroll
    for (int r = 0; r < 8; r++) { acc[r][0] = f2{0.f, 0.f}; acc[r][1] = f2{0.f, 0.f}; }
    for (uint32_t c0 = 0; c0 < D; c0 += MT_KC) {
      const uint32_t c = c0 + tx;
      float va[MT_ROWS / 16], vb[MT_COLS / 16];
#pragma unroll
      for (int it = 0; it < MT_ROWS / 16; it++) {
        const uint32_t row = row0 + ty + 16 * it;
        va[it] = (row < ns && c < D) ? fsrc[(size_t)row * D + c] : 0.f;
      }
#pragma unroll
      for (int it = 0; it < MT_COLS / 16; it++) {
        const uint32_t col = col0 + ty + 16 * it;
        vb[it] = (col < nt && c < D) ? ftgt[(size_t)col * D + c] : 0.f;
      }
      __syncthreads();  // the chunk before is consumed (and, first chunk: the lists' and s_col's initial values are written)
#pragma unroll
      for (int it = 0; it < MT_ROWS / 16; it++) { bad = bad || not_finite(va[it]); sA[tx][ty + 16 * it] = va[it]; }
#pragma unroll
      for (int it = 0; it < MT_COLS / 16; it++) { bad = bad || not_finite(vb[it]); sB[tx][ty + 16 * it] = vb[it]; }
      __syncthreads();
      // the last chunk of a descriptor is cut short (D = 33: 16 + 16 + 1 components, not 48); the bound is uniform
      const uint32_t lim = D - c0 < (uint32_t)MT_KC ? D - c0 : (uint32_t)MT_KC;
      if (lim == (uint32_t)MT_KC) {
#pragma unroll
        for (int k = 0; k < MT_KC; k++) tile_step(acc, &sA[k][ty * 8], &sB[k][tx * 4]);
      } else {
        for (uint32_t k = 0; k < lim; k++) tile_step(acc, &sA[k][ty * 8], &sB[k][tx * 4]);
      }
    }
    // selection.  (Every thread is behind the last chunk's second barrier: the lists and s_col hold at least their initial values.)
    const uint32_t colb = col0 + tx * 4;
    unsigned long long cmin[4] = {KEY_NONE, KEY_NONE, KEY_NONE, KEY_NONE};
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint32_t lr = ty * 8 + r, row = row0 + lr;
      if (row >= ns) continue;
      const float v[4] = {acc[r][0].x, acc[r][0].y, acc[r][1].x, acc[r][1].y};
      unsigned long long* list = &s_top[lr][0];
      // what the list's last slot holds only ever falls: an old value lets a candidate through that the cascade then passes out again
      const unsigned long long worst = *reinterpret_cast<volatile unsigned long long*>(&list[KP - 1]);
      unsigned long long best = KEY_NONE;
#pragma unroll
      for (int cc = 0; cc < 4; cc++) {
        if (colb + cc >= nt) continue;
        if constexpr (GUIDED) {
          if (!((adm >> (r * 4 + cc)) & 1u)) continue;  // an inadmissible cell offers no key
        }
        const unsigned long long hi = (unsigned long long)__float_as_uint(v[cc]) << 32;
        const unsigned long long key = hi | (colb + cc);
        const unsigned long long rkey = hi | row;
        cmin[cc] = rkey < cmin[cc] ? rkey : cmin[cc];
        if (KP == 1) best = key < best ? key : best;
        else if (key < worst) top_insert<KP>(list, key);
      }
      if (KP == 1 && best < worst) atomicMin(&list[0], best);
    }
    if (colmin) {
#pragma unroll
      for (int cc = 0; cc < 4; cc++)
        if (cmin[cc] != KEY_NONE) atomicMin(&s_col[tx * 4 + cc], cmin[cc]);
      __syncthreads();
      if (threadIdx.x < MT_COLS && col0 + threadIdx.x < nt) {
        const unsigned long long v = s_col[threadIdx.x];
        unsigned long long* g = &colmin[col0 + threadIdx.x];
        if (v < __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(g, v);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < MT_ROWS && row0 + threadIdx.x < ns) {
#pragma unroll
    for (int q = 0; q < KP; q++) part[((size_t)blockIdx.y * KP + q) * ld_part + row0 + threadIdx.x] = s_top[threadIdx.x][q];
  }
  if (bad) __hip_atomic_store(clean, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(FIN_THREADS) void match_finish_kernel(const unsigned long long* __restrict__ part, size_t ld_part,
                                                                   uint32_t slices, uint32_t kp, MatchJob job,
                                                                   const unsigned long long* __restrict__ colmin,
                                                                   const uint32_t* __restrict__ clean, int32_t* __restrict__ corr,
                                                                   float* __restrict__ d2, uint32_t* __restrict__ count,
                                                                   MatchGather g, LbArgs lb, uint64_t* host_word, MatchGuide gd,
                                                                   float* __restrict__ g2, int32_t* __restrict__ label) {
  __shared__ uint32_t s_tile;
  __shared__ uint64_t s_scan[FIN_THREADS / 64];
  __shared__ uint64_t s_prefix;
  if (threadIdx.x == 0) s_tile = __hip_atomic_fetch_add(lb.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const uint32_t tile = s_tile;
  if (tile >= gridDim.x) return;  // (a ticket that was not zero at launch: never index memory with it)
  const uint32_t i = tile * FIN_THREADS + threadIdx.x;
  const bool ok = __hip_atomic_load(clean, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
  unsigned long long top[4] = {KEY_NONE, KEY_NONE, KEY_NONE, KEY_NONE};
  uint32_t cnt = 0;
  if (ok && i < job.ns) {
    for (uint32_t s = 0; s < slices; s++) {
      for (uint32_t q = 0; q < kp; q++) {
        unsigned long long key = part[((size_t)s * kp + q) * ld_part + i];
        if (key >= top[3]) break;  // (a slice's list ascends)
#pragma unroll
        for (int w = 0; w < 4; w++) {
          const unsigned long long lo = key < top[w] ? key : top[w];
          key = key < top[w] ? top[w] : key;
          top[w] = lo;
        }
      }
    }
    cnt = row_kept(top, i, job.mutual, job.r2, job.knn, colmin, job.nt);
  }
  uint64_t tot;
  const uint64_t ex = block_exscan_u64(cnt, s_scan, &tot);
  if (threadIdx.x < 64) {
    uint64_t* const desc[1] = {lb.desc};
    const uint64_t own[1] = {tot};
    uint64_t pre[1];
    lb_lookback<1>(desc, tile, lb.epoch, own, pre, lb.err);
    if (threadIdx.x == 0) s_prefix = pre[0];
  }
  __syncthreads();
  const uint64_t pre = s_prefix;
  const size_t cap = (size_t)job.ns * job.knn;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    if (w >= (int)cnt) break;
    const size_t slot = (size_t)(pre + ex + w);
    const uint32_t j = (uint32_t)top[w];
    if (slot >= cap || j >= job.nt) break;  // (cannot happen: a row emits at most knn keys, each with a column of this call)
    entry_write(slot, i, top[w], corr, d2, g, 0u, 0u);
    if (gd.n_poses != 0u) {
      // sc_match_guided_poses: every used record's residual of the entry (the distance launch's chain on the same points); the
      // smallest, ties to the lowest index — a NaN never wins, and the entry is admissible: some residual is below gate2
      if (g2 || label) {
        float p[3], q[3];
        entry_points(gd, i, j, p, q);
        float best = __uint_as_float(0x7F800000u);
        int32_t best_k = 0;
        for (uint32_t k = 0; k < gd.n_poses; k++) {
          const float* rec = pose_record(gd, k);
          if (!pose_used(gd, rec)) continue;
          float M[12];
#pragma unroll
          for (int f = 0; f < 12; f++) M[f] = rec[f];
          const float r = resid2(M, p[0], p[1], p[2], q[0], q[1], q[2]);
          if (r < best) { best = r; best_k = (int32_t)k; }
        }
        if (g2) g2[slot] = best;
        if (label) label[slot] = best_k;
      }
    } else if (g2) {  // sc_match_guided: the gate residual of the entry, the distance launch's chain on the same points
      float M[12];
#pragma unroll
      for (int k = 0; k < 12; k++) M[k] = gd.Rt[k];
      g2[slot] = entry_resid(M, gd, i, j);
    }
  }
  if (tile == gridDim.x - 1 && threadIdx.x == 0) {
    const uint32_t n = ok ? (uint32_t)(pre + tot) : 0u;
    count[0] = n;
    count[1] = ok ? 0u : 1u;
    if (host_word) publish_host(host_word, (uint64_t)n | ((uint64_t)(ok ? 0u : 1u) << 32));
    __hip_atomic_store(lb.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // every tile has taken its ticket
  }
}

}  // namespace

MatchPlan match_plan(uint32_t ns, uint32_t nt, uint32_t knn, float r2) {
  MatchPlan p;
  p.kp = r2 > 0.f ? 2u : knn;  // the ratio test looks at the second-smallest key
  p.row_blocks = (ns + MT_ROWS - 1) / MT_ROWS;
  const uint32_t tiles = (nt + MT_COLS - 1) / MT_COLS;
  // enough workgroups to fill the device a few times over (256 CUs, several resident workgroups each); never more than 1024 slices:
  // the finish kernel reads slices * kp keys per row
  uint32_t want = (4096 + p.row_blocks - 1) / p.row_blocks;
  if (want > 1024) want = 1024;
  if (want > tiles) want = tiles;
  p.tiles_per_slice = (tiles + want - 1) / want;
  p.slices = (tiles + p.tiles_per_slice - 1) / p.tiles_per_slice;
  p.ld_part = (size_t)p.row_blocks * MT_ROWS;
  p.part_bytes = p.ld_part * p.slices * p.kp * sizeof(uint64_t);
  return p;
}

uint32_t match_finish_tiles(uint32_t ns) { return (ns + FIN_THREADS - 1) / FIN_THREADS; }

namespace {

// one distance launch under gate GATE: the dispatch over the lists' length
template <int GATE, class Guide>
void launch_dist(const MatchJob& job, const MatchPlan& plan, uint64_t* part, uint64_t* colmin, uint32_t* clean, const Guide& gd, hipStream_t st) {
  const auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(plan.row_blocks, plan.slices), dim3(MT_THREADS), 0, st, job.fsrc, job.ns, job.ftgt, job.nt, job.dim,
                       plan.tiles_per_slice, reinterpret_cast<unsigned long long*>(part), plan.ld_part,
                       reinterpret_cast<unsigned long long*>(colmin), clean, gd);
  };
  switch (plan.kp) {
    case 1: go(match_dist_kernel<1, GATE>); break;
    case 2: go(match_dist_kernel<2, GATE>); break;
    case 3: go(match_dist_kernel<3, GATE>); break;
    default: go(match_dist_kernel<4, GATE>); break;
  }
}

}  // namespace

void launch_match_dist(const MatchJob& job, const MatchPlan& plan, uint64_t* part, uint64_t* colmin, uint32_t* clean, const MatchGuide* gd,
                       hipStream_t st) {
  if (!gd) launch_dist<GATE_NONE>(job, plan, part, colmin, clean, NoGuide{}, st);
  else if (gd->n_poses != 0u) launch_dist<GATE_POSES>(job, plan, part, colmin, clean, *gd, st);
  else launch_dist<GATE_POSE>(job, plan, part, colmin, clean, *gd, st);
}

void launch_match_finish(const MatchJob& job, const MatchPlan& plan, const uint64_t* part, const uint64_t* colmin, const uint32_t* clean, LbArgs lb,
                         const MatchOut& o, hipStream_t st) {
  hipLaunchKernelGGL(match_finish_kernel, dim3(match_finish_tiles(job.ns)), dim3(FIN_THREADS), 0, st,
                     reinterpret_cast<const unsigned long long*>(part), plan.ld_part, plan.slices, plan.kp, job,
                     reinterpret_cast<const unsigned long long*>(colmin), clean, o.corr, o.d2, o.count, o.g, lb, o.host_word,
                     o.gd ? *o.gd : MatchGuide{}, o.gd ? o.g2 : nullptr, o.gd && o.gd->n_poses != 0u ? o.label : nullptr);
}

}  // namespace sc
