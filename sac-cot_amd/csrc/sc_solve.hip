// sc_solve.hip — the kernels of sc_pairs_solve (include/saccot.h): Gauss-Newton on a pair list's pose graph, the linear system of a
// step solved by block-Jacobi preconditioned conjugate gradients.  5 + max_outer * (4 + 2 * max_inner) launches on data the host
// staged once (sc_cycles_check.hpp's image: the records, the sorted neighbour entries and the list starts):
//
//   prepare   a thread per pair: the prologue every pair-list entry shares (sc_pose64.hpp: validity, status, the pose widened ONCE
//             into the two oriented fp64 transforms), use, the info record and whether both sets are known — one word a pair —,
//             and the sets' tallies of usable pairs.
//   sets      a thread per set: X_0 into buffer 0, the set's state, its record of tallies.
//   linearise a thread per pair, a workgroup per chunk of 64 pairs: at X_j the pair's error, its cost, W_p and g_p; the chunk's
//             cost sum.  (Launch j serves step j + 1 and is the cost evaluation of step j.)
//   decide    one workgroup: c_j from the chunk sums and the verdict on step j.  A verdict ends every later launch at once.
//   factor    a WAVE per set, a workgroup per chunk of 64 sets: G and the diagonal block as sums over the set's sorted
//             list — a lane IS a slot of the header's sum, the fold a butterfly of xor shuffles, as in sc_sync.hip —, the LDL^T
//             factor, r = -G, z, x = 0 and the chunk's sum of r.z.
//   product   the hot launch, a wave per set as above: p = z + beta p formed on the fly for the set and for every neighbour,
//             q = H p over the sorted list (W_p, 288 bytes, and the neighbour's vectors), the chunk's sum of p.q.
//   update    a thread per set, a workgroup per chunk: x, r, z and the chunk's sum of r.z.
//   step      a thread per set: X_j from X_{j-1} and x into the other buffer, the changed tally.
//   finish    the records and the summary.
//
// The grand sums.  A chunk's sum is formed inside ONE workgroup, through LDS, by one thread in the header's order; the grand sum is
// formed from the chunk sums by EVERY workgroup of the launch that needs it, again by one thread in the header's order (the other
// threads stage the sums in LDS).  So no workgroup ever reads what another wrote in the same launch: the kernel boundary is the only
// hand-off, and there is no atomic on a double, no ticket, no spin.  The scalars a later launch needs (rz_i, rz_0, the live words)
// are written by workgroup 0 alone, into words that no workgroup of the same launch reads (SolveCtl, sc_kernels.hpp).
// Nothing is fused: the library is built with -ffp-contract=off and this file says so again.
#include <cstddef>

#include "sc_arith.hpp"
#include "sc_kernels.hpp"
#include "sc_pose64.hpp"
#include "sc_rot.hpp"
#include "sc_solve_check.hpp"

#pragma clang fp contract(off)

namespace sc {

static_assert(sizeof(SolveSetRecord) == sizeof(sc_solve_set) && sizeof(SolveSetRecord) == 160 && offsetof(SolveSetRecord, status) == offsetof(sc_solve_set, status) &&
              offsetof(SolveSetRecord, status) == 48 && offsetof(SolveSetRecord, state) == offsetof(sc_solve_set, state) &&
              offsetof(SolveSetRecord, degenerate) == offsetof(sc_solve_set, degenerate) && offsetof(SolveSetRecord, X) == offsetof(sc_solve_set, X) &&
              offsetof(SolveSetRecord, X) == 64 && offsetof(sc_sync_set, X) == 64 && offsetof(sc_sync_set, status) == 48 && sizeof(sc_sync_set) == 160,
              "SolveSetRecord is sc_solve_set, 160 bytes, and both it and sc_sync_set are init records");
static_assert(sizeof(SolvePairRecord) == sizeof(sc_solve_pair) && sizeof(SolvePairRecord) == 48 && offsetof(SolvePairRecord, cost) == offsetof(sc_solve_pair, cost) &&
              offsetof(SolvePairRecord, w2) == offsetof(sc_solve_pair, w2) && offsetof(SolvePairRecord, v2) == offsetof(sc_solve_pair, v2) &&
              offsetof(SolvePairRecord, reserved) == offsetof(sc_solve_pair, reserved), "SolvePairRecord is sc_solve_pair, 48 bytes");
static_assert(sizeof(SolveSummary) == sizeof(sc_solve_summary) && sizeof(SolveSummary) == 64 && offsetof(SolveSummary, cost0) == offsetof(sc_solve_summary, cost0) &&
              offsetof(SolveSummary, held_last) == offsetof(sc_solve_summary, held_last) && offsetof(SolveSummary, rz0) == offsetof(sc_solve_summary, rz0),
              "SolveSummary is sc_solve_summary, 64 bytes");
static_assert(sizeof(SolveCtl) <= SOLVE_CTL_BYTES && SOLVE_OUTER_MAX == SOLVE_MAX_OUTER && SOLVE_INNER_MAX == SOLVE_MAX_INNER && SOLVE_PRODUCT_MAX == SOLVE_MAX_PRODUCT,
              "the control words fit their area");
static_assert(sizeof(SolveInfo) == 16 && offsetof(sc_pose_info_result, status) == SOLVE_INFO_STATUS_AT && sizeof(sc_pose_info_result) == 320,
              "a set's tallies are 16 bytes; sc_pose_info_result is an info record");

namespace {

constexpr int ST = 256;              // threads of a workgroup of the flat launches (prepare, sets, step, finish)
constexpr int CH = (int)SOLVE_CHUNK; // a chunk: 64 pairs or sets, the workgroup of linearise and update
constexpr int WT = 1024;             // threads of a workgroup of product: 16 waves, four of the chunk's sets each
constexpr int FT = 256;              // of factor, whose waves hold a 6 x 6 block and its factor: 4 waves, sixteen sets each

__device__ __forceinline__ double dot6(const double* a, const double* b) {
  double s = a[0] * b[0];
#pragma unroll
  for (int c = 1; c < 6; c++) s = s + a[c] * b[c];
  return s;
}

__device__ __forceinline__ bool init_known(const SolveJob& job, uint32_t s) {
  const char* const rec = static_cast<const char*>(job.init) + (size_t)s * job.init_stride;
  bool ok = *reinterpret_cast<const int32_t*>(rec + 48) == SC_OK;
  const double* const X = reinterpret_cast<const double*>(rec + 64);
#pragma unroll
  for (int c = 0; c < 12; c++) ok = ok && finite64(X[c]);
  return ok;
}

// The grand sum of n chunk sums, in increasing order from +0.0, by thread 0; every thread of the workgroup gets it.  sh: CH doubles
// and one more.  (The chunk sums are an earlier launch's.)
__device__ __forceinline__ double block_grand_sum(const double* __restrict__ v, uint32_t n, double* sh) {
  double s = 0.0;
  for (uint32_t base = 0; base < n; base += CH) {
    if (threadIdx.x < CH && base + threadIdx.x < n) sh[threadIdx.x] = v[base + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t m = n - base < (uint32_t)CH ? n - base : (uint32_t)CH;
      for (uint32_t k = 0; k < m; k++) s = s + sh[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) sh[CH] = s;
  __syncthreads();
  s = sh[CH];
  __syncthreads();
  return s;
}
// A chunk's sum: sh[0 .. CH) hold the chunk's values (+0.0 past the end), summed by thread 0 from +0.0 in increasing order.
__device__ __forceinline__ void chunk_sum_store(const double* sh, double* out) {
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < CH; k++) s = s + sh[k];
    *out = s;
  }
}

// z = Hd^-1 r by the stored factor: L row-major below the diagonal (15), then D (6)
__device__ __forceinline__ void solve6(const double* __restrict__ fac, const double (&r)[6], double (&z)[6]) {
  double L[6][6], D[6], y[6];
  int at = 0;
#pragma unroll
  for (int i = 1; i < 6; i++)
#pragma unroll
    for (int k = 0; k < i; k++) L[i][k] = fac[at++];
#pragma unroll
  for (int i = 0; i < 6; i++) D[i] = fac[15 + i];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double a = r[i];
#pragma unroll
    for (int k = 0; k < i; k++) a = a - L[i][k] * y[k];
    y[i] = a;
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double a = y[i] / D[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) a = a - L[k][i] * z[k];
    z[i] = a;
  }
}

__global__ __launch_bounds__(ST) void solve_prepare_kernel(const SolveJob job) {
  const uint32_t p = blockIdx.x * ST + threadIdx.x;
  bool usable = false;
  if (p < job.n_pairs) {
    bool edge;
    const int status = pair_prologue(job.pose, job.pose_stride, job.status, job.rec, job.wide, p, &edge);
    const uint32_t* const r = job.rec + (size_t)CYCLES_REC_WORDS * p;
    const bool use = pair_use(job.use, job.use_stride, p);
    bool info_ok = true;
    if (job.info) {
      const char* const rec = static_cast<const char*>(job.info) + (size_t)p * job.info_stride;
      const double* const I = reinterpret_cast<const double*>(rec);
      for (int c = 0; c < 36; c++) info_ok = info_ok && finite64(I[c]);
      if (job.info_status) info_ok = info_ok && *reinterpret_cast<const int32_t*>(rec + SOLVE_INFO_STATUS_AT) == SC_OK;
    }
    usable = edge && use && info_ok && init_known(job, r[CW_LO]) && init_known(job, r[CW_HI]);
    job.usable[p] = usable ? 1u : 0u;
    job.pair[p].status = status;  // (the rest of the record is finish's)
    if (usable) {
      atomicAdd(&job.deg[r[CW_LO]], 1u);
      atomicAdd(&job.deg[r[CW_HI]], 1u);
    }
  }
  const uint32_t n = (uint32_t)__popcll(__ballot(usable));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&job.ctl->used_pairs, n);
}

__global__ __launch_bounds__(ST) void solve_sets_kernel(const SolveJob job) {
  const uint32_t s = blockIdx.x * ST + threadIdx.x;
  bool is_free = false;
  if (s < job.n_sets) {
    const char* const rec = static_cast<const char*>(job.init) + (size_t)s * job.init_stride;
    const double* const X = reinterpret_cast<const double*>(rec + 64);
#pragma unroll
    for (int c = 0; c < 12; c++) job.X[(size_t)12 * s + c] = X[c];  // X_0, bit for bit (buffer 1 is written whole by step 1)
    SolveInfo si{};
    si.status = *reinterpret_cast<const int32_t*>(rec + 48);
    si.state = !init_known(job, s) ? SC_SOLVE_UNKNOWN : s == job.anchor ? SC_SOLVE_ANCHOR : job.deg[s] == 0 ? SC_SOLVE_ISOLATED : SC_SOLVE_FREE;
    is_free = si.state == SC_SOLVE_FREE;
    job.sinfo[s] = si;
  }
  const uint32_t n = (uint32_t)__popcll(__ballot(is_free));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&job.ctl->free_sets, n);
}

__global__ __launch_bounds__(CH) void solve_lin_kernel(const SolveJob job, const uint32_t j) {
  if (job.ctl->stop) return;
  __shared__ double sh[CH];
  const uint32_t p = blockIdx.x * CH + threadIdx.x;
  const double* const __restrict__ X = job.X + (size_t)(j & 1) * 12 * job.n_sets;
  double cost = 0.0, w2 = 0.0, v2 = 0.0;
  if (p < job.n_pairs && job.usable[p]) {
    const uint32_t* const rc = job.rec + (size_t)CYCLES_REC_WORDS * p;
    const StoredPair sp = stored_pair(rc);
    const T64 Xb = load_t64(X + (size_t)12 * sp.b);
    const T64 D = compose_t64(inverse_t64(Xb), load_t64(X + (size_t)12 * sp.a));
    const T64 E = compose_t64(D, load_t64(job.wide + (size_t)24 * p + (sp.fwd ? 12 : 0)));  // T_p(b -> a): higher -> lower at 12
    double xi[6], y[6], info[36];
    xi[0] = (E.R[7] - E.R[5]) / 2.0;
    xi[1] = (E.R[2] - E.R[6]) / 2.0;
    xi[2] = (E.R[3] - E.R[1]) / 2.0;
    xi[3] = E.t[0]; xi[4] = E.t[1]; xi[5] = E.t[2];
    if (job.info) {
      const double* const I = reinterpret_cast<const double*>(static_cast<const char*>(job.info) + (size_t)p * job.info_stride);
#pragma unroll
      for (int c = 0; c < 36; c++) info[c] = I[c];
    } else {
#pragma unroll
      for (int c = 0; c < 36; c++) info[c] = (c % 7 == 0) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
      double s = info[6 * i] * xi[0];
#pragma unroll
      for (int k = 1; k < 6; k++) s = s + info[6 * i + k] * xi[k];
      y[i] = s;
    }
    cost = dot6(xi, y);
    w2 = (xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2];
    v2 = (xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5];
    // A = Ad(X(b)^-1)
    double A[6][6];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double c[3] = {Xb.R[i], Xb.R[3 + i], Xb.R[6 + i]};  // column i of R
      double ct[3];
      cross3(c, Xb.t, ct);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        A[i][k] = c[k]; A[3 + i][3 + k] = c[k];
        A[i][3 + k] = 0.0;
        A[3 + i][k] = -ct[k];
      }
    }
    double* const W = job.W + (size_t)36 * p;
    double* const g = job.g + (size_t)6 * p;
    double M[6][6];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int c = 0; c < 6; c++) {
        double s = info[6 * i] * A[0][c];
#pragma unroll
        for (int k = 1; k < 6; k++) s = s + info[6 * i + k] * A[k][c];
        M[i][c] = s;
      }
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
      for (int c = i; c < 6; c++) {
        double s = A[0][i] * M[0][c];
#pragma unroll
        for (int k = 1; k < 6; k++) s = s + A[k][i] * M[k][c];
        W[6 * i + c] = s;
        W[6 * c + i] = s;
      }
      double s = A[0][i] * y[0];
#pragma unroll
      for (int k = 1; k < 6; k++) s = s + A[k][i] * y[k];
      g[i] = s;
    }
  }
  if (p < job.n_pairs) {
    double* const e = job.err + ((size_t)(j & 1) * job.n_pairs + p) * 3;
    e[0] = cost; e[1] = w2; e[2] = v2;
  }
  sh[threadIdx.x] = cost;
  chunk_sum_store(sh, job.costc + blockIdx.x);
}

__global__ __launch_bounds__(ST) void solve_decide_kernel(const SolveJob job, const uint32_t j) {
  SolveCtl* const ctl = job.ctl;
  if (ctl->stop) return;
  __shared__ double sh[CH + 1];
  const double c = block_grand_sum(job.costc, (uint32_t)solve_chunks(job.n_pairs), sh);
  if (threadIdx.x != 0) return;
  if (j == 0) {
    ctl->cost[0] = c;
    if (ctl->free_sets == 0) { ctl->K = 0; ctl->stop = SC_SOLVE_STOP_CONVERGED; }
    return;
  }
  uint32_t inner = 0;
  for (uint32_t i = 1; i <= job.max_inner; i++) inner += ctl->live_u[(j - 1) * job.max_inner + i] != 0 ? 1u : 0u;
  ctl->inner[j] = inner;
  ctl->J = j;
  if (!(c <= ctl->cost[j - 1])) { ctl->K = j - 1; ctl->stop = SC_SOLVE_STOP_ROSE; return; }  // (a NaN as well)
  ctl->cost[j] = c;
  ctl->K = j;
  if (ctl->changed[j] == 0 || ctl->rz0[j] == 0.0) ctl->stop = SC_SOLVE_STOP_CONVERGED;
  else if (j == job.max_outer) ctl->stop = SC_SOLVE_STOP_MAX_OUTER;
}

__global__ __launch_bounds__(FT) void solve_factor_kernel(const SolveJob job, const uint32_t j) {
  if (job.ctl->stop) return;
  __shared__ double sh[CH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t* const __restrict__ ent = job.entries;
  for (int k = 0; k < CH / (FT / 64); k++) {
    const int local = wave + (FT / 64) * k;
    const uint32_t s = blockIdx.x * CH + local;
    double rz = 0.0;
    if (s < job.n_sets && job.sinfo[s].state == SC_SOLVE_FREE) {  // (wave-uniform)
      const uint32_t begin = job.off[s], end = job.off[s + 1];
      double G[6], H[21];
#pragma unroll
      for (int c = 0; c < 6; c++) G[c] = 0.0;
#pragma unroll
      for (int c = 0; c < 21; c++) H[c] = 0.0;
      for (uint32_t i = begin + lane; i < end; i += 64) {  // slot `lane`: entries lane, lane + 64, ... in this order
        const uint64_t e = ent[i];
        const uint32_t p = cycles_entry_pair(e);
        if (!job.usable[p]) continue;
        const double* const __restrict__ W = job.W + (size_t)36 * p;
        const double* const __restrict__ g = job.g + (size_t)6 * p;
        if (cycles_entry_forward(e)) {
#pragma unroll
          for (int c = 0; c < 6; c++) G[c] = G[c] + g[c];
        } else {
#pragma unroll
          for (int c = 0; c < 6; c++) G[c] = G[c] - g[c];
        }
        int at = 0;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
          for (int c = r; c < 6; c++) { H[at] = H[at] + W[6 * r + c]; at++; }
      }
#pragma unroll
      for (int h = 32; h > 0; h >>= 1) {
#pragma unroll
        for (int c = 0; c < 6; c++) G[c] = G[c] + __shfl_xor(G[c], h);
#pragma unroll
        for (int c = 0; c < 21; c++) H[c] = H[c] + __shfl_xor(H[c], h);
      }
      // the factor, on every lane alike
      double Hm[6][6], L[6][6], D[6], u[6];
      {
        int at = 0;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
          for (int c = r; c < 6; c++) { Hm[r][c] = H[at]; Hm[c][r] = H[at]; at++; }
      }
      bool held = false;
#pragma unroll
      for (int c = 0; c < 6; c++) {
        double a = Hm[c][c];
#pragma unroll
        for (int q = 0; q < c; q++) { u[q] = L[c][q] * D[q]; a = a - L[c][q] * u[q]; }
        D[c] = a;
        held = held || !(a > 0.0 && a < __builtin_inf());
#pragma unroll
        for (int i = c + 1; i < 6; i++) {
          double b = Hm[i][c];
#pragma unroll
          for (int q = 0; q < c; q++) b = b - L[i][q] * u[q];
          L[i][c] = b / a;
        }
      }
      double f[21];  // the factor as it is stored: L row-major below the diagonal, then D
      {
        int at = 0;
#pragma unroll
        for (int i = 1; i < 6; i++)
#pragma unroll
          for (int q = 0; q < i; q++) f[at++] = L[i][q];
#pragma unroll
        for (int i = 0; i < 6; i++) f[15 + i] = D[i];
      }
      double r[6], z[6];
#pragma unroll
      for (int c = 0; c < 6; c++) { r[c] = -G[c]; z[c] = 0.0; }
      if (!held) {
        solve6(f, r, z);
        rz = dot6(r, z);
      }
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 21; c++) job.fac[(size_t)21 * s + c] = f[c];
      }
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) { job.x[(size_t)6 * s + c] = 0.0; job.r[(size_t)6 * s + c] = r[c]; job.z[(size_t)6 * s + c] = z[c]; }
        SolveInfo* const si = job.sinfo + s;
        si->active = held ? 0u : 1u;
        if (held) { si->degenerate = si->degenerate + 1; atomicAdd(&job.ctl->held[j], 1u); }
      }
    }
    if (lane == 0) sh[local] = rz;
  }
  chunk_sum_store(sh, job.rzc + blockIdx.x);  // rz_0's chunk sums: buffer 0
}

// p of iteration i for set n (any lane may ask for any set): z where i == 1, else z + beta * the p of iteration i - 1; +0.0 where
// the set is not active
__device__ __forceinline__ void form_p(const SolveJob& job, uint32_t n, uint32_t i, double beta, double (&p)[6]) {
  if (!job.sinfo[n].active || job.sinfo[n].state != SC_SOLVE_FREE) {
#pragma unroll
    for (int c = 0; c < 6; c++) p[c] = 0.0;
    return;
  }
  const double* const __restrict__ z = job.z + (size_t)6 * n;
  if (i == 1) {
#pragma unroll
    for (int c = 0; c < 6; c++) p[c] = z[c];
  } else {
    const double* const __restrict__ pp = job.p + ((size_t)((i - 1) & 1) * job.n_sets + n) * 6;
#pragma unroll
    for (int c = 0; c < 6; c++) p[c] = z[c] + beta * pp[c];
  }
}

__global__ __launch_bounds__(WT) void solve_product_kernel(const SolveJob job, const uint32_t j, const uint32_t i) {
  SolveCtl* const ctl = job.ctl;
  if (ctl->stop) return;
  const uint32_t idx = (j - 1) * job.max_inner + i;
  if (i > 1 && ctl->live_u[idx - 1] == 0) return;  // the iteration before was not applied, or never multiplied
  __shared__ double sh[CH + 1];
  const uint32_t nch = (uint32_t)solve_chunks(job.n_sets);
  const double rz_prev = block_grand_sum(job.rzc + (size_t)((i - 1) & 1) * nch, nch, sh);  // rz_{i-1}
  double beta = 0.0;
  if (i == 1) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->rz0[j] = rz_prev;
    if (rz_prev == 0.0) return;
  } else {
    if (rz_prev <= job.cg2 * ctl->rz0[j]) return;  // the solve ended behind iteration i - 1
    beta = rz_prev / ctl->rz[i - 2];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->rz[i - 1] = rz_prev; ctl->live_p[idx] = 1; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t* const __restrict__ ent = job.entries;
  for (int k = 0; k < CH / (WT / 64); k++) {
    const int local = wave + (WT / 64) * k;
    const uint32_t s = blockIdx.x * CH + local;
    double pq = 0.0;
    if (s < job.n_sets && job.sinfo[s].state == SC_SOLVE_FREE && job.sinfo[s].active) {  // (wave-uniform)
      double ps[6], acc[6];
      form_p(job, s, i, beta, ps);
#pragma unroll
      for (int c = 0; c < 6; c++) acc[c] = 0.0;
      const uint32_t begin = job.off[s], end = job.off[s + 1];
      for (uint32_t t = begin + lane; t < end; t += 64) {  // slot `lane`: entries lane, lane + 64, ... in this order
        const uint64_t e = ent[t];
        const uint32_t nb = cycles_entry_set(e), p = cycles_entry_pair(e);
        if (!job.usable[p]) continue;
        double pn[6], d[6];
        form_p(job, nb, i, beta, pn);
#pragma unroll
        for (int c = 0; c < 6; c++) d[c] = ps[c] - pn[c];
        const double* const __restrict__ W = job.W + (size_t)36 * p;
#pragma unroll
        for (int r = 0; r < 6; r++) {
          double u = W[6 * r] * d[0];
#pragma unroll
          for (int c = 1; c < 6; c++) u = u + W[6 * r + c] * d[c];
          acc[r] = acc[r] + u;
        }
      }
#pragma unroll
      for (int h = 32; h > 0; h >>= 1)
#pragma unroll
        for (int c = 0; c < 6; c++) acc[c] = acc[c] + __shfl_xor(acc[c], h);
      pq = dot6(ps, acc);
      if (lane == 0) {
        double* const po = job.p + ((size_t)(i & 1) * job.n_sets + s) * 6;
#pragma unroll
        for (int c = 0; c < 6; c++) { po[c] = ps[c]; job.q[(size_t)6 * s + c] = acc[c]; }
      }
    }
    if (lane == 0) sh[local] = pq;
  }
  chunk_sum_store(sh, job.pqc + blockIdx.x);
}

__global__ __launch_bounds__(CH) void solve_update_kernel(const SolveJob job, const uint32_t j, const uint32_t i) {
  SolveCtl* const ctl = job.ctl;
  if (ctl->stop) return;
  const uint32_t idx = (j - 1) * job.max_inner + i;
  if (ctl->live_p[idx] == 0) return;
  __shared__ double sh[CH + 1];
  const uint32_t nch = (uint32_t)solve_chunks(job.n_sets);
  const double pq = block_grand_sum(job.pqc, nch, sh);
  if (!(pq > 0.0 && pq < __builtin_inf())) return;  // the solve ends; this iteration is not applied
  const double alpha = ctl->rz[i - 1] / pq;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->live_u[idx] = 1;
  const uint32_t s = blockIdx.x * CH + threadIdx.x;
  double rz = 0.0;
  if (s < job.n_sets && job.sinfo[s].state == SC_SOLVE_FREE && job.sinfo[s].active) {
    const double* const __restrict__ p = job.p + ((size_t)(i & 1) * job.n_sets + s) * 6;
    double r[6], z[6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
      job.x[(size_t)6 * s + c] = job.x[(size_t)6 * s + c] + alpha * p[c];
      r[c] = job.r[(size_t)6 * s + c] - alpha * job.q[(size_t)6 * s + c];
    }
    solve6(job.fac + (size_t)21 * s, r, z);
#pragma unroll
    for (int c = 0; c < 6; c++) { job.r[(size_t)6 * s + c] = r[c]; job.z[(size_t)6 * s + c] = z[c]; }
    rz = dot6(r, z);
  }
  sh[threadIdx.x] = rz;
  chunk_sum_store(sh, job.rzc + (size_t)(i & 1) * nch + blockIdx.x);
}

__global__ __launch_bounds__(ST) void solve_step_kernel(const SolveJob job, const uint32_t j) {
  if (job.ctl->stop) return;
  const uint32_t s = blockIdx.x * ST + threadIdx.x;
  bool changed = false;
  if (s < job.n_sets) {
    const double* const __restrict__ prev = job.X + ((size_t)((j - 1) & 1) * job.n_sets + s) * 12;
    double* const __restrict__ cur = job.X + ((size_t)(j & 1) * job.n_sets + s) * 12;
    const T64 old = load_t64(prev);
    T64 out = old;
    SolveInfo* const si = job.sinfo + s;
    if (si->state == SC_SOLVE_FREE && si->active) {
      const double* const x = job.x + (size_t)6 * s;
      const double I[9] = {1.0, -x[2], x[1], x[2], 1.0, -x[0], -x[1], x[0], 1.0};
      T64 Q;
      rot_plain(I, Q.R);
      Q.t[0] = x[3]; Q.t[1] = x[4]; Q.t[2] = x[5];
      const T64 M = compose_t64(Q, old);
      T64 N;
      rot_plain(M.R, N.R);
      bool fin = true;
#pragma unroll
      for (int c = 0; c < 9; c++) fin = fin && finite64(N.R[c]);
#pragma unroll
      for (int c = 0; c < 3; c++) { N.t[c] = M.t[c]; fin = fin && finite64(N.t[c]); }
      if (fin) {
        double dR2 = 0.0, dt2 = 0.0;
#pragma unroll
        for (int c = 0; c < 9; c++) { const double d = N.R[c] - old.R[c]; dR2 = c ? dR2 + d * d : d * d; }
#pragma unroll
        for (int c = 0; c < 3; c++) { const double d = N.t[c] - old.t[c]; dt2 = c ? dt2 + d * d : d * d; }
        changed = dR2 > job.r2_max || dt2 > job.e2_max;
        out = N;
      } else {
        si->degenerate = si->degenerate + 1;
      }
    }
    store_t64(cur, out);
  }
  const uint32_t n = (uint32_t)__popcll(__ballot(changed));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&job.ctl->changed[j], n);
}

__global__ __launch_bounds__(ST) void solve_finish_kernel(const SolveJob job) {
  const SolveCtl* const ctl = job.ctl;
  const uint32_t K = ctl->K, J = ctl->J;
  const uint32_t i = blockIdx.x * ST + threadIdx.x;
  if (i < job.n_sets) {
    const double* const __restrict__ X = job.X + ((size_t)(K & 1) * job.n_sets + i) * 12;
    const SolveInfo si = job.sinfo[i];
    SolveSetRecord out;
#pragma unroll
    for (int c = 0; c < 12; c++) { out.Rt[c] = (float)X[c]; out.X[c] = X[c]; }
    out.status = si.status; out.state = si.state; out.degenerate = si.degenerate; out.reserved = 0;
    job.set[i] = out;
  }
  if (i < job.n_pairs) {
    const double* const e = job.err + ((size_t)(K & 1) * job.n_pairs + i) * 3;
    SolvePairRecord* const out = job.pair + i;  // (status: prepare's)
    out->used = job.usable[i]; out->cost = e[0]; out->w2 = e[1]; out->v2 = e[2];
#pragma unroll
    for (int c = 0; c < 4; c++) out->reserved[c] = 0;
  }
  if (i == 0) {
    SolveSummary s{};
    s.outer = K; s.stop = ctl->stop; s.free_sets = ctl->free_sets; s.used_pairs = ctl->used_pairs;
    for (uint32_t k = 1; k <= J; k++) s.inner_total += ctl->inner[k];
    s.inner_last = J ? ctl->inner[J] : 0u; s.held_last = J ? ctl->held[J] : 0u;
    s.cost0 = ctl->cost[0]; s.cost = ctl->cost[K]; s.rz0 = J ? ctl->rz0[J] : 0.0; s.reserved2 = 0.0;
    *job.sum = s;
  }
}

}  // namespace

void launch_pairs_solve(const SolveJob& job, hipStream_t st) {
  const uint32_t pair_flat = (job.n_pairs + ST - 1) / ST, set_flat = (job.n_sets + ST - 1) / ST, most = pair_flat > set_flat ? pair_flat : set_flat,
                 pair_chunks = (uint32_t)solve_chunks(job.n_pairs), set_chunks = (uint32_t)solve_chunks(job.n_sets);
  hipLaunchKernelGGL(solve_prepare_kernel, dim3(pair_flat), dim3(ST), 0, st, job);
  hipLaunchKernelGGL(solve_sets_kernel, dim3(set_flat), dim3(ST), 0, st, job);
  hipLaunchKernelGGL(solve_lin_kernel, dim3(pair_chunks), dim3(CH), 0, st, job, 0u);
  hipLaunchKernelGGL(solve_decide_kernel, dim3(1), dim3(ST), 0, st, job, 0u);
  for (uint32_t j = 1; j <= job.max_outer; j++) {
    hipLaunchKernelGGL(solve_factor_kernel, dim3(set_chunks), dim3(FT), 0, st, job, j);
    for (uint32_t i = 1; i <= job.max_inner; i++) {
      hipLaunchKernelGGL(solve_product_kernel, dim3(set_chunks), dim3(WT), 0, st, job, j, i);
      hipLaunchKernelGGL(solve_update_kernel, dim3(set_chunks), dim3(CH), 0, st, job, j, i);
    }
    hipLaunchKernelGGL(solve_step_kernel, dim3(set_flat), dim3(ST), 0, st, job, j);
    hipLaunchKernelGGL(solve_lin_kernel, dim3(pair_chunks), dim3(CH), 0, st, job, j);
    hipLaunchKernelGGL(solve_decide_kernel, dim3(1), dim3(ST), 0, st, job, j);
  }
  hipLaunchKernelGGL(solve_finish_kernel, dim3(most), dim3(ST), 0, st, job);
}

}  // namespace sc
