// sc_match_batch.hip — descriptor matching for a whole batch of small problems (include/saccot.h, sc_match_batch): the kernels.
// The arithmetic and the selection step are sc_match.hip's (tile_step, top_insert: sc_match_tile.hpp), so problem b's slot holds what
// sc_match returns for problem b alone, bit for bit; the finish kernel's row decision and entry write, the pose-record accessors and
// the not-finite scan are one text with sc_match.hip's, in the same header.  The chunk loop, the selection block and the
// column-minimum flush are written out here as they are there (sc_match.hip says why).  Two launches for the batch, whatever its size:
//
//   match_batch_dist_kernel    grid = the flattened list of (problem, tile of 64 source rows); the tile map comes from the host with
//                              the offsets, and a tile never spans two problems.  A workgroup of 128 threads walks ALL target
//                              columns of its problem in tiles of 64 — no slices: a row's KP smallest keys complete in the
//                              workgroup's LDS lists and go to `top` once.  Register tile 8 rows x 4 columns per thread, chunks of 16
//                              components staged transposed in LDS, zero padding in c and in rows (exact: (0 - 0)^2 adds +0).
//                              64 rows, not sc_match's 128: problems of 64 - 512 rows leave half as many padded rows on average
//                              (32 against 64), a batch of 16 problems of 256 rows still makes 64 workgroups, and 11 KB of LDS with
//                              two waves lets a compute unit hold many of them at once.  The column minima of SC_MATCH_MUTUAL combine in
//                              LDS, then by 64-bit atomic minima on colmin[tgt_off[b] + j] (a minimum is order-free: deterministic).
//                              A non-finite descriptor clears the problem's own `clean` word: a problem's tiles together read
//                              every element of it, and nothing of another problem.
//   match_batch_finish_kernel  a workgroup of 256 per problem: a thread per source row, 256 rows at a time with a running count —
//                              mutual / ratio per row, a workgroup scan, and the kept keys go into the problem's slot in ascending
//                              (row, rank) order with their indices local to the problem; the matched points are gathered
//                              beside them for sc_register_batch_features; thread 0 writes the count pair.  No look-back across
//                              problems: a slot's position is known on the host.
//
// Both kernels are written once for two arguments: MatchBatchJob — packed problems, addressed by their offsets — and MatchPairsJob
// (sc_match_pairs: listed pairs of shared sets, addressed by a record per pair, sc_kernels.hpp).  What differs is where a problem's
// rows, lists, column minima and slot start: MatchView, filled by view_of for either argument; everything behind it is one text, so
// a pair's slot holds what the packed form returns for the pair expanded.  The packed instantiation reads what it always read.
//
// sc_match_guided_batch (MatchGuidedBatchJob, MatchGuidedPairsJob: the same two arguments with a MatchBatchGuide behind them) is the
// same pair of launches with a pose prior per problem, as sc_match.hip's GUIDED is for one frame: problem b's pose goes into scalar
// registers, the tile's 64 source points into LDS once and a column tile's 64 target points per tile; every thread folds its 8 x 4
// decisions resid2(Rt_b, p_i, q_j) < gate2 into one 32-bit word BEFORE the descriptor chunks (a loop over its rows), an inadmissible
// cell offers no key — not to the row's list, not to the column minimum — and a tile in which no cell of the workgroup is admissible
// is skipped altogether (a workgroup-wide OR behind a barrier every thread passes).  A skipped tile's descriptors are never staged, so the
// finiteness rule is carried by a scan of its own: the ceil(ns_b / 64) workgroups of problem b share a strided scan of the problem's
// OWN descriptor and point ranges — nothing of a neighbour's — and each tests the pose.  A problem whose record carries a status
// other than SC_OK (SC_GUIDE_POSE_STATUS) returns before any of this.  GUIDED is a property of the job's type: the unguided
// instantiations keep their arguments and their code.
#include <cstddef>
#include <type_traits>

#include "sc_arith.hpp"

#include "sc_block.hpp"
#include "sc_kernels.hpp"
#include "sc_match_tile.hpp"

#pragma clang fp contract(off)  // the canonical distance rounds the product and the sum separately

namespace sc {

namespace {

constexpr int MB_ROWS = MATCH_BATCH_ROWS, MB_COLS = 64, MB_THREADS = 128;
constexpr int MB_LD = 64 + 4;  // 16-byte aligned rows; the pad spreads the transposing stores over the banks
constexpr int MBF_THREADS = 256;
static_assert(MB_ROWS == 64 && MB_THREADS == (MB_ROWS / 8) * (MB_COLS / 4), "a thread owns 8 rows x 4 columns of the tile");

// Where problem b's data starts.  top_row / col: the problem's first row of lists and first column minimum — the packed form's are
// its offsets, a pair's are its own (a set that is the target of two pairs has two ranges of minima).
struct MatchView {
  const float* fsrc; const float* ftgt;  // the problem's first descriptor row, either side
  uint32_t so, to, ns, nt;               // first point row and rows, either side (the gather's)
  size_t top_row, col, slot;
};
__device__ __forceinline__ MatchView view_of(const MatchBatchJob& job, uint32_t b) {
  const uint32_t so = job.src_off[b], to = job.tgt_off[b];
  return MatchView{job.fsrc + (size_t)so * job.dim, job.ftgt + (size_t)to * job.dim, so, to, job.src_off[b + 1] - so, job.tgt_off[b + 1] - to,
                   so, to, job.slot[b]};
}
__device__ __forceinline__ MatchView view_of(const MatchPairsJob& job, uint32_t p) {
  const uint32_t* r = job.rec + (size_t)PAIR_WORDS * p;
  return MatchView{job.feat + (size_t)r[PW_SRC] * job.dim, job.feat + (size_t)r[PW_TGT] * job.dim, r[PW_SRC], r[PW_TGT], r[PW_NS], r[PW_NT],
                   r[PW_TOP], (size_t)r[PW_COL_LO] | (size_t)r[PW_COL_HI] << 32, r[PW_SLOT]};
}

// is this job one of the guided forms?  (Decided by the type: the template arguments, hence the names, of the unguided kernels stay.)
template <class Job> struct guided_job : std::false_type {};
template <> struct guided_job<MatchGuidedBatchJob> : std::true_type {};
template <> struct guided_job<MatchGuidedPairsJob> : std::true_type {};

template <int KP, class Job>
__global__ __launch_bounds__(MB_THREADS) void match_batch_dist_kernel(const Job job) {
  constexpr bool GUIDED = guided_job<Job>::value;
  __shared__ __attribute__((aligned(16))) float sA[MT_KC][MB_LD];
  __shared__ __attribute__((aligned(16))) float sB[MT_KC][MB_LD];
  __shared__ unsigned long long s_top[MB_ROWS][KP];
  __shared__ unsigned long long s_col[MB_COLS];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;  // the thread's 4 columns / 8 rows; also (component, row) when it loads
  if (blockIdx.x >= job.n_tiles) return;
  const uint32_t b = job.tile_map[2 * blockIdx.x], row0 = job.tile_map[2 * blockIdx.x + 1];
  if (b >= job.n_problems) return;  // (cannot happen: the host built the map)
  float M[12];  // GUIDED: the problem's pose (workgroup-uniform: scalar registers)
  if constexpr (GUIDED) {
    const float* rec = pose_record(job.gd, b);
    if (!pose_used(job.gd, rec)) return;  // nothing else of a skipped problem is read or written
#pragma unroll
    for (int k = 0; k < 12; k++) M[k] = rec[k];
  }
  const MatchView v = view_of(job, b);
  const uint32_t ns = v.ns, nt = v.nt, D = job.dim;
  const float* __restrict__ fsrc = v.fsrc;
  const float* __restrict__ ftgt = v.ftgt;
  unsigned long long* const colmin = job.colmin ? reinterpret_cast<unsigned long long*>(job.colmin) + v.col : nullptr;
  const uint32_t n_tiles = (nt + MB_COLS - 1) / MB_COLS;
  for (int e = threadIdx.x; e < MB_ROWS * KP; e += MB_THREADS) (&s_top[0][0])[e] = KEY_NONE;
  bool bad = false;
  float(*sP)[MB_ROWS] = nullptr;  // GUIDED: the tile's source points, component-major
  float(*sQ)[MB_COLS] = nullptr;  // GUIDED: the column tile's target points
  uint32_t adm = 0;               // GUIDED: bit r * 4 + cc: cell (row r, column cc) of this thread is admissible in this column tile
  if constexpr (GUIDED) {
    __shared__ float s_src[3][MB_ROWS];
    __shared__ float s_tgt[3][MB_COLS];
    sP = s_src; sQ = s_tgt;
    const MatchBatchGuide& gd = job.gd;
#pragma unroll
    for (int k = 0; k < 12; k++) bad = bad || not_finite(M[k]);
    // The finiteness rule depends on the input alone: the problem's workgroups share every element of ITS descriptors and points,
    // whatever tiles the gate drops below.  (A point is read through the strides: in SoA a problem's points are three ranges.)
    const size_t stride = (size_t)((ns + MB_ROWS - 1) / MB_ROWS) * MB_THREADS, me = (size_t)(row0 / MB_ROWS) * MB_THREADS + threadIdx.x;
    bad = scan_not_finite(fsrc, (size_t)ns * D, me, stride) || bad;
    bad = scan_not_finite(ftgt, (size_t)nt * D, me, stride) || bad;
    for (size_t e = me; e < (size_t)ns * 3; e += stride)
      bad = bad || not_finite(gd.src[((size_t)v.so + e / 3) * gd.s_elem + (e % 3) * gd.s_comp]);
    for (size_t e = me; e < (size_t)nt * 3; e += stride)
      bad = bad || not_finite(gd.tgt[((size_t)v.to + e / 3) * gd.t_elem + (e % 3) * gd.t_comp]);
    for (int e = threadIdx.x; e < 3 * MB_ROWS; e += MB_THREADS) {
      const uint32_t comp = e / MB_ROWS, lr = e % MB_ROWS, row = row0 + lr;
      sP[comp][lr] = row < ns ? gd.src[((size_t)v.so + row) * gd.s_elem + (size_t)comp * gd.s_comp] : 0.f;
    }
  }
  for (uint32_t tile = 0; tile < n_tiles; tile++) {
    const uint32_t col0 = tile * MB_COLS;
    if (threadIdx.x < MB_COLS) s_col[threadIdx.x] = KEY_NONE;
    if constexpr (GUIDED) {
      const MatchBatchGuide& gd = job.gd;
      // (nobody still reads the tile before: its last read of sQ is in front of that tile's OR barrier, which every thread has passed)
      for (int e = threadIdx.x; e < 3 * MB_COLS; e += MB_THREADS) {
        const uint32_t comp = e / MB_COLS, lc = e % MB_COLS, col = col0 + lc;
        sQ[comp][lc] = col < nt ? gd.tgt[((size_t)v.to + col) * gd.t_elem + (size_t)comp * gd.t_comp] : 0.f;
      }
      __syncthreads();  // sQ (and, first tile, sP, the lists' and s_col's initial values) are written
      // The thread's 4 target points in registers, its 8 rows rolled.  (All 32 cells unrolled cost sc_match.hip's kernel 60+ registers
      // and a wave per SIMD; this kernel runs two waves per SIMD with or without a gate, and the half-rolled form stays within them:
      // profiles/match_shared.txt has the registers.  The cell's indices are constants here and a row's point is read once for 4 cells: measured 7 % faster
      // than the loop over 32 cells)
      adm = 0;
      {
        float qx[4], qy[4], qz[4];
#pragma unroll
        for (int cc = 0; cc < 4; cc++) { qx[cc] = sQ[0][tx * 4 + cc]; qy[cc] = sQ[1][tx * 4 + cc]; qz[cc] = sQ[2][tx * 4 + cc]; }
#pragma unroll 1
        for (int r = 0; r < 8; r++) {
          const uint32_t lr = ty * 8 + r;
          const float px = sP[0][lr], py = sP[1][lr], pz = sP[2][lr];
          const bool row_in = row0 + lr < ns;
#pragma unroll
          for (int cc = 0; cc < 4; cc++) {
            // a float <: a NaN or infinite residual is never admissible
            const bool in = row_in && col0 + tx * 4 + cc < nt && resid2(M, px, py, pz, qx[cc], qy[cc], qz[cc]) < gd.gate2;
            adm |= (in ? 1u : 0u) << (r * 4 + cc);
          }
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
      float va[MB_ROWS / 8], vb[MB_COLS / 8];
#pragma unroll
      for (int it = 0; it < MB_ROWS / 8; it++) {
        const uint32_t row = row0 + ty + 8 * it;
        va[it] = (row < ns && c < D) ? fsrc[(size_t)row * D + c] : 0.f;
      }
#pragma unroll
      for (int it = 0; it < MB_COLS / 8; it++) {
        const uint32_t col = col0 + ty + 8 * it;
        vb[it] = (col < nt && c < D) ? ftgt[(size_t)col * D + c] : 0.f;
      }
      __syncthreads();  // the chunk before is consumed (and, first chunk: the lists' and s_col's initial values are written)
#pragma unroll
      for (int it = 0; it < MB_ROWS / 8; it++) { bad = bad || not_finite(va[it]); sA[tx][ty + 8 * it] = va[it]; }
#pragma unroll
      for (int it = 0; it < MB_COLS / 8; it++) { bad = bad || not_finite(vb[it]); sB[tx][ty + 8 * it] = vb[it]; }
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
      const float d[4] = {acc[r][0].x, acc[r][0].y, acc[r][1].x, acc[r][1].y};
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
        const unsigned long long hi = (unsigned long long)__float_as_uint(d[cc]) << 32;
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
      if (threadIdx.x < MB_COLS && col0 + threadIdx.x < nt) {
        const unsigned long long m = s_col[threadIdx.x];
        unsigned long long* g = &colmin[col0 + threadIdx.x];
        if (m < __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(g, m);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < MB_ROWS && row0 + threadIdx.x < ns) {
    unsigned long long* out = reinterpret_cast<unsigned long long*>(job.top) + (v.top_row + row0 + threadIdx.x) * KP;
#pragma unroll
    for (int q = 0; q < KP; q++) out[q] = s_top[threadIdx.x][q];
  }
  if (bad) __hip_atomic_store(&job.clean[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class Job>
__global__ __launch_bounds__(MBF_THREADS) void match_batch_finish_kernel(const Job job) {
  __shared__ uint64_t s_scan[MBF_THREADS / 64];
  constexpr bool GUIDED = guided_job<Job>::value;
  const uint32_t b = blockIdx.x;
  float M[12];  // GUIDED: the problem's pose
  if constexpr (GUIDED) {
    const float* rec = pose_record(job.gd, b);
    if (!pose_used(job.gd, rec)) {  // (0, 0), and nothing else of the problem is read or written
      if (threadIdx.x == 0) { job.count[2 * b] = 0u; job.count[2 * b + 1] = 0u; }
      return;
    }
#pragma unroll
    for (int k = 0; k < 12; k++) M[k] = rec[k];
  }
  const MatchView v = view_of(job, b);
  const uint32_t so = v.so, to = v.to, ns = v.ns, nt = v.nt;
  const size_t slot = v.slot, cap = (size_t)ns * job.knn;
  const bool ok = job.clean[b] != 0u;  // (written by the launch before this one)
  const unsigned long long* __restrict__ top = reinterpret_cast<const unsigned long long*>(job.top) + v.top_row * job.kp;
  const unsigned long long* __restrict__ colmin = job.colmin ? reinterpret_cast<const unsigned long long*>(job.colmin) + v.col : nullptr;
  const MatchGather g = job.g;
  uint32_t run = 0;  // kept so far, by the rows before this step's
  for (uint32_t base = 0; ok && base < ns; base += MBF_THREADS) {
    const uint32_t i = base + threadIdx.x;
    unsigned long long key[4] = {KEY_NONE, KEY_NONE, KEY_NONE, KEY_NONE};
    uint32_t cnt = 0;
    if (i < ns) {
#pragma unroll
      for (int q = 0; q < 4; q++)
        if (q < (int)job.kp) key[q] = top[(size_t)i * job.kp + q];
      cnt = row_kept(key, i, job.mutual, job.r2, job.knn, colmin, nt);
    }
    uint64_t tot;
    const uint64_t ex = block_exscan_u64(cnt, s_scan, &tot);
#pragma unroll
    for (int w = 0; w < 4; w++) {
      if (w >= (int)cnt) break;
      const size_t m = (size_t)run + ex + w;
      const uint32_t j = (uint32_t)key[w];
      if (m >= cap || j >= nt) break;  // (cannot happen: a row emits at most knn keys, each with a column of its problem)
      const size_t e = slot + m;
      entry_write(e, i, key[w], job.corr, job.d2, g, so, to);
      if constexpr (GUIDED) {
        if (job.gd.g2) job.gd.g2[e] = entry_resid(M, job.gd, (size_t)so + i, (size_t)to + j);  // the gate residual of the entry
      }
    }
    run += (uint32_t)tot;
  }
  if (threadIdx.x == 0) {
    job.count[2 * b] = ok ? run : 0u;
    job.count[2 * b + 1] = ok ? 0u : 1u;
  }
}

}  // namespace

template <class Job>
void launch_match_batch_dist(const Job& job, hipStream_t st) {
  const dim3 grid(job.n_tiles), block(MB_THREADS);
  switch (job.kp) {
    case 1: hipLaunchKernelGGL((match_batch_dist_kernel<1, Job>), grid, block, 0, st, job); break;
    case 2: hipLaunchKernelGGL((match_batch_dist_kernel<2, Job>), grid, block, 0, st, job); break;
    case 3: hipLaunchKernelGGL((match_batch_dist_kernel<3, Job>), grid, block, 0, st, job); break;
    default: hipLaunchKernelGGL((match_batch_dist_kernel<4, Job>), grid, block, 0, st, job); break;
  }
}
template <class Job>
void launch_match_batch_finish(const Job& job, hipStream_t st) {
  hipLaunchKernelGGL(match_batch_finish_kernel<Job>, dim3(job.n_problems), dim3(MBF_THREADS), 0, st, job);
}
template void launch_match_batch_dist(const MatchBatchJob&, hipStream_t);
template void launch_match_batch_dist(const MatchPairsJob&, hipStream_t);
template void launch_match_batch_dist(const MatchGuidedBatchJob&, hipStream_t);
template void launch_match_batch_dist(const MatchGuidedPairsJob&, hipStream_t);
template void launch_match_batch_finish(const MatchBatchJob&, hipStream_t);
template void launch_match_batch_finish(const MatchPairsJob&, hipStream_t);
template void launch_match_batch_finish(const MatchGuidedBatchJob&, hipStream_t);
template void launch_match_batch_finish(const MatchGuidedPairsJob&, hipStream_t);

}  // namespace sc
