// sc_compat.hip — stage A (compat_graph): the tiles of the compatibility matrix and their adjacency words,
// the XCD-aware block order, launch_compat.  Input staging is sc_stage.hip; the row statistics and the shard split (stage B's first
// step) are sc_rows.hip; the exclusive scan is sc_scan.hip.
//
// Stage A's output is 4 N^2 bytes of weights + N^2/8 bytes of adjacency bits (103 MB at N = 5000): the HBM write
// roofline is its bound; see the stage-A section below for the tiling that gets the arithmetic out of the way.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "sc_arith.hpp"
#include "sc_block.hpp"
#include "sc_kernels.hpp"

namespace sc {

// ------------------------------------------------------------------------------------------------
// stage A
//
// The matrix is symmetric and the pair arithmetic is bit-symmetric (dist3(a,b) == dist3(b,a)), so only tiles on or
// above the diagonal are evaluated: one wave = one tile of TILE_R rows x 64 columns (lane = column).
//   * direct half:   S[i][j] is stored row by row (256 B contiguous per wave store); __ballot of the edge predicate
//                    IS the adjacency word of row i for this column block — lane r keeps the word of row r;
//   * mirrored half: the tile goes through an LDS transpose and S[j][i0..i0+31] is stored as 128-B row segments; the
//                    mirrored adjacency half-word of row j accumulates in lane j (bit r = edge with row i0 + r);
//   * tiles crossing the diagonal evaluate their full rectangle and write the direct half only.
// PMC on the previous one-sided kernel: WRITE_SIZE == algorithmic bytes, VALU-bound (74 VALU per pair); evaluating
// each pair once halves that work, which is what moves the kernel toward the HBM write roofline.
// deg / deg+ / word-prefix popcounts come from the bit rows in a second, tiny kernel.
// ------------------------------------------------------------------------------------------------
struct alignas(32) RowPt { float px, py, pz, qx, qy, qz, pad0, pad1; };  // the AoS copy written by stage_points_kernel

// value of `v` in lane `src` (wave-uniform src) as a scalar: v_readlane_b32 works on the bit pattern
__device__ __forceinline__ float bcast(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}


// S stores: 16 bytes per lane by default (4 consecutive floats of one row piece: a quarter of the store instructions
// and of the addresses the texture path has to process), optionally non-temporal (S is never read again on this
// path: no reason to keep it in L2 / Infinity Cache).  `mode` bit 0: 4-byte stores (round 1's form: better on small
// matrices, see launch_compat), bit 1: non-temporal.
typedef float f32x4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_s4(float* p, float a, float b, float c, float d, bool nt) {
  const f32x4s v = {a, b, c, d};
  if (nt) __builtin_nontemporal_store(v, reinterpret_cast<f32x4s*>(p));
  else *reinterpret_cast<f32x4s*>(p) = v;
}
__device__ __forceinline__ void store_s1(float* p, float a, bool nt) {
  if (nt) __builtin_nontemporal_store(a, p);
  else *p = a;
}

// The staging kernel's per-workgroup coordinate statistics -> the FX_MX_WORDS words of the call (one wave; the rows were written by
// the launch before this one: plain loads).  Lane = (row group lane / 16, word lane % 16).
struct StatsJob { const uint32_t* part; uint32_t rows; uint32_t* out; };
__device__ __forceinline__ void stats_reduce_wave(const StatsJob& sj, int lane) {
  const uint32_t c = (uint32_t)lane & 15u;
  uint32_t best = 0;
  if (c < 14)
    for (uint32_t r = (uint32_t)lane >> 4; r < sj.rows; r += 4) best = max(best, sj.part[(size_t)r * 16 + c]);
  best = max(best, (uint32_t)__shfl_xor((int)best, 16));
  best = max(best, (uint32_t)__shfl_xor((int)best, 32));
  if (lane < 14) sj.out[lane] = best;
}

// TILE_R rows per tile (16 or 64): 64 / TILE_R tiles stack into one 64-row block.
// DENSE: write the weight matrix S (false: SC_FLAG_NO_DENSE_S — adjacency bits only, no LDS tile image, no S traffic).
// RECT:  one-sided form for a ROW BLOCK [row0, row1) x all columns (stage A sharded by row blocks):
//        every tile writes its direct half only — the mirrored half belongs to another rank — and S holds the rows
//        of the block only (row i at S[(i - row0) * ld]).  Bit rows go to `bits` at their global row index.
template <int TILE_R, int COMPAT_WAVES, bool DENSE, bool RECT>
__global__ __launch_bounds__(64 * COMPAT_WAVES) void compat_tiles_kernel(const float* __restrict__ planes, int n,
                                                                         int ld, float d_thr, float min_len,
                                                                         float nis, float* __restrict__ S,
                                                                         uint64_t* __restrict__ bits, int n_tiles,
                                                                         int two_phase, int row0, int row1,
                                                                         int mode, uint32_t* __restrict__ degp,
                                                                         const uint32_t* __restrict__ wg_map, StatsJob sj) {
  constexpr int TILE_PAD = TILE_R + 1;  // LDS row stride of the transposed tile: conflict-free both ways
  constexpr int SUB = 64 / TILE_R;      // tiles per 64-row block
  __shared__ float tileT[DENSE ? COMPAT_WAVES : 1][DENSE ? 64 * TILE_PAD : 1];  // [column][row] per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // a host-free call's coordinate statistics: reduced HERE, by one wave of this launch, instead of by a workgroup of the staging
  // launch that stays behind for it (release + ticket + acquire: ~2.5 us of that launch); nothing before stage B's vote reads them
  if (sj.part && blockIdx.x == 0 && wave == COMPAT_WAVES - 1) stats_reduce_wave(sj, lane);
  // wg_map (whole-matrix form, COMPAT_WAVES == SUB: a workgroup = one 64 x 64 block of the matrix): which block this
  // workgroup takes — the XCD-aware order of compat_wg_map() below; ~0: a padding workgroup
  const uint32_t wg = wg_map ? wg_map[blockIdx.x] : blockIdx.x;
  if (wg == 0xFFFFFFFFu) return;
  const int t = (int)wg * COMPAT_WAVES + wave;
  if (t >= n_tiles) return;  // whole wave; no block-level barrier is used below
  const int W = ld >> 6;
  const bool nt = (mode & 2) != 0, st4 = (mode & 1) != 0;
  int J, h;
  if (RECT) {
    // column block fastest: consecutive waves write adjacent 256-byte pieces of the same rows
    J = t % W;
    h = t / W + row0 / TILE_R;  // row0 is a multiple of 64
  } else {
    // tile t -> (column block J, row sub-block h):  t = SUB J (J + 1) / 2 + h,  0 <= h < SUB (J + 1)
    J = (int)((__builtin_sqrtf(8.0f * (float)(t / SUB) + 1.0f) - 1.0f) * 0.5f);
    while (SUB * (J + 1) * (J + 2) / 2 <= t) J++;
    while (SUB * J * (J + 1) / 2 > t) J--;
    h = t - SUB * J * (J + 1) / 2;
  }
  const int rlim = RECT ? row1 : n;     // rows at or beyond it are not this launch's
  const int srow = RECT ? row0 : 0;     // S row offset
  const int i0 = h * TILE_R;
  const int j = J * 64 + lane;
  const bool diag = (h / SUB) == J;
  const float* px = planes;
  const float* py = planes + ld;
  const float* pz = planes + 2 * (size_t)ld;
  const float* qx = planes + 3 * (size_t)ld;
  const float* qy = planes + 4 * (size_t)ld;
  const float* qz = planes + 5 * (size_t)ld;
  const float jpx = px[j], jpy = py[j], jpz = pz[j], jqx = qx[j], jqy = qy[j], jqz = qz[j];
  const int i0s = __builtin_amdgcn_readfirstlane(i0);  // provably wave-uniform row base
  float* myT = tileT[DENSE ? wave : 0];
  uint64_t rowword = 0;      // lane r: adjacency word of row i0 + r over this column block
  uint64_t colword = 0;      // lane c: bit r = edge (row i0 + r, column j)
  // Interior tiles (every row and column real, not on the diagonal) are ~97 % of the work.
  const bool interior = !diag && (i0 + TILE_R <= rlim) && (J * 64 + 64 <= n);
  if (interior && two_phase) {
    // ---- two-phase form ----------------------------------------------------------------------------------
    // Only ~4 % of the pairs are edges, yet the exact chain (two correctly rounded square roots, the exponential)
    // is ~60 of the ~83 VALU instructions a pair used to cost, and the kernel was VALU-issue-bound.  Phase 1 computes
    // the two squared lengths (the same fp32 values the exact chain starts from) and a CONSERVATIVE candidate test in
    // squared quantities — no sqrt, no exp; phase 2 runs the exact chain on the queued candidates only and scatters
    // weights and adjacency bits into the LDS image of the tile, which is then written out as before.
    // Candidate test (theta = d_thr, L = min_len, A = sqrt(n2p), B = sqrt(n2q) as reals):
    //   an edge has |dp - dq| <= theta (1 + 2^-24) with dp = A (1 + e1), dq = B (1 + e2), |e| <= 2^-24, hence
    //   A^2 + B^2 - theta^2 - sigma <= 2 A B  with  sigma = (theta^2 + A^2 + B^2) 2^-21  (generous).
    //   a = fma(RN(n2p + n2q), 1 - 2^-20, -theta^2 (1 + 2^-20)) is <= that left side; so an edge has a <= 0 or
    //   a^2 <= 4 n2p n2q (1 + 2^-18).  Products so small that they could round to zero count as candidates.
    //   dp >= L needs n2p >= L^2 (1 - 2^-23); the test uses L^2 (1 - 2^-20), rounded down.
    // False positives cost a queue slot; a false negative is impossible, so the output is bit-identical.
    // Measured (r01): C2 29.4 -> 26.6 us, C3 ~400 -> ~385 us.  Ablation on C3 (N = 20 000, 1.65 GB of S): arithmetic
    // and LDS work alone 187 us, the stores alone 334 us (4.9 TB/s: 256-byte row pieces + 64-byte mirrored pieces; a
    // plain fill of the same bytes runs at 6.8 TB/s), both 383 us — the store PATTERN is the limiter now, not VALU.
    // A one-sided row kernel (1 KiB zero-fill stores per instruction + 4-byte patches of the edges, both triangles
    // evaluated) was built and was bit-exact but no faster: 234 us of arithmetic + ~190 us of stores that did not
    // overlap (423 us); 64-row tiles (256-byte mirrored pieces, SC_COMPAT_ROWS=64) change nothing on C3 either.
    constexpr int QCAP = 320;  // candidate queue per wave (a row adds <= 64; drained above QCAP - 64)
    __shared__ uint16_t queue[COMPAT_WAVES][QCAP];
    __shared__ unsigned long long rowbits[COMPAT_WAVES][TILE_R];
    __shared__ unsigned long long colbits[COMPAT_WAVES][64];
    uint16_t* myQ = queue[wave];
    unsigned long long* myRB = rowbits[wave];
    unsigned long long* myCB = colbits[wave];
    if (DENSE)
      for (int k = lane; k < 64 * TILE_PAD; k += 64) myT[k] = 0.0f;
    if (lane < TILE_R) myRB[lane] = 0ull;
    if (!RECT) myCB[lane] = 0ull;
    const RowPt* __restrict__ aos = reinterpret_cast<const RowPt*>(planes + 6 * (size_t)ld);
    // lane r (< TILE_R) keeps row point i0 + r in registers: phase 2 fetches both points of a candidate with
    // ds_bpermute (no memory latency in the drain — with ~1.5 tiles per wave slot the kernel's time is a wave's latency)
    const RowPt mine = aos[i0 + (lane & (TILE_R - 1))];
    const float theta2 = d_thr * d_thr;
    const float c1 = 1.0f - 0x1p-20f;
    const float c2 = theta2 * (1.0f + 0x1p-20f) * (1.0f + 0x1p-22f);  // rounded up a little: never below theta^2 (1 + 2^-20)
    const float k4 = 4.0f + 0x1p-16f;                                   // 4 (1 + 2^-18), exact
    const float Lc = (min_len * min_len) * (1.0f - 0x1p-20f) * (1.0f - 0x1p-22f);
    uint32_t cnt = 0;  // queued candidates (wave-uniform)
    auto drain = [&]() {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // LDS is in-order within a wave
      for (uint32_t q0 = 0; q0 < cnt; q0 += 64) {  // wave-uniform trips: ds_bpermute reads 0 from inactive lanes
        const bool valid = q0 + lane < cnt;
        const uint32_t code = valid ? myQ[q0 + lane] : 0u;
        const int r = (int)(code >> 6), c = (int)(code & 63);
        const float dp = dist3_fast(__shfl(mine.px, r), __shfl(mine.py, r), __shfl(mine.pz, r), __shfl(jpx, c),
                                    __shfl(jpy, c), __shfl(jpz, c));
        const float dq = dist3_fast(__shfl(mine.qx, r), __shfl(mine.qy, r), __shfl(mine.qz, r), __shfl(jqx, c),
                                    __shfl(jqy, c), __shfl(jqz, c));
        bool edge;
        const float s = pair_weight(dp, dq, d_thr, min_len, nis, edge);
        if (valid && edge) {
          if (DENSE) myT[c * TILE_PAD + r] = s;
          atomicOr(&myRB[r], 1ull << c);
          if (!RECT) atomicOr(&myCB[c], 1ull << r);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      cnt = 0;
    };
    // The scalar unit (one per CU) was the limiter of the first two-phase form (666 SALU + 101 SMEM per wave): one
    // 32-byte scalar load per row, and the test folded into VALU selects so that ONE compare produces a lane mask.
    const float INF = __builtin_inff(), QNAN = __builtin_nanf("");
    RowPt nxt = aos[i0s];  // wave-uniform address: scalar load, issued one row ahead of its use
#pragma unroll 4
    for (int r = 0; r < TILE_R; r++) {
      const RowPt rp = nxt;
      nxt = aos[i0s + ((r + 1) & (TILE_R - 1))];
      const float dxp = rp.px - jpx, dyp = rp.py - jpy, dzp = rp.pz - jpz;
      const float dxq = rp.qx - jqx, dyq = rp.qy - jqy, dzq = rp.qz - jqz;
      const float n2p = fma_(dzp, dzp, fma_(dyp, dyp, dxp * dxp));  // exactly dist3's radicand
      const float n2q = fma_(dzq, dzq, fma_(dyq, dyq, dxq * dxq));
      const float m = fmaxf(fma_(n2p + n2q, c1, -c2), 0.0f);        // a <= 0 or a^2 <= R  <=>  max(a,0)^2 <= R
      const float t = n2p * n2q;
      const float R = (t < 0x1p-100f) ? INF : t * k4;               // vanishing products: candidate
      const float lhs = (fminf(n2p, n2q) >= Lc) ? m * m : QNAN;     // too short: NaN never compares true
      const bool cand = lhs <= R;
      const uint64_t bal = __ballot(cand);
      if (bal != 0) {  // wave-uniform
        if (cand)
          myQ[cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] =
              (uint16_t)((r << 6) | lane);
        cnt += (uint32_t)__popcll(bal);
        if (cnt > (uint32_t)(QCAP - 64)) drain();
      }
    }
    if (cnt) drain();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // direct half from the tile image ([column][row], stride TILE_PAD): 16 bytes per lane — lane (r', c4) stores four
    // consecutive columns of row r' (four rows x 256 bytes per instruction; the LDS reads are conflict-free:
    // bank = 4 (lane % 16) + 17 u + lane / 16) — or, mode bit 0, one 256-byte row per instruction with 4-byte stores
    if (DENSE) {
      if (!st4) {
        const int c4 = (lane & 15) * 4, rr = lane >> 4;
#pragma unroll 4
        for (int q = 0; q < TILE_R; q += 4) {
          const int r = q + rr;
          store_s4(&S[(size_t)(i0 - srow + r) * ld + J * 64 + c4], myT[c4 * TILE_PAD + r], myT[(c4 + 1) * TILE_PAD + r],
                   myT[(c4 + 2) * TILE_PAD + r], myT[(c4 + 3) * TILE_PAD + r], nt);
        }
      } else {
#pragma unroll 4
        for (int r = 0; r < TILE_R; r++) store_s1(&S[(size_t)(i0 - srow + r) * ld + j], myT[lane * TILE_PAD + r], nt);
      }
    }
    if (lane < TILE_R) bits[(size_t)(i0 + lane) * W + J] = myRB[lane];
    // deg+ (edges to higher indices) of the tile's rows, accumulated where the adjacency words are made (degp zeroed by the
    // staging kernel): the row kernel that used to re-read the whole bit matrix for it is gone from the hot path — the
    // tiles on or above the diagonal hold exactly the upper triangle.  Integer sums: order-free.
    if (!RECT && degp && lane < TILE_R) {
      const uint32_t pc = (uint32_t)__popcll(myRB[lane]);
      if (pc) atomicAdd(&degp[i0 + lane], pc);
    }
    if (!RECT) {
      colword = myCB[lane];
      if (DENSE) {
        if (!st4) {
          // mirrored half: row J*64 + cc of S, columns i0 .. i0 + TILE_R - 1; a row piece is TILE_R / 4 lanes x 16 bytes
          constexpr int LP = TILE_R / 4, RPI = 64 / LP;  // lanes per piece, pieces (output rows) per instruction
          const int r4 = (lane % LP) * 4, co = lane / LP;
#pragma unroll 4
          for (int c = 0; c < 64; c += RPI) {
            const int cc = c + co;
            store_s4(&S[(size_t)(J * 64 + cc) * ld + i0 + r4], myT[cc * TILE_PAD + r4], myT[cc * TILE_PAD + r4 + 1],
                     myT[cc * TILE_PAD + r4 + 2], myT[cc * TILE_PAD + r4 + 3], nt);
          }
        } else {
          const int r = lane & (TILE_R - 1), hi = lane / TILE_R;
#pragma unroll 4
          for (int c = 0; c < 64; c += SUB) {
            const int cc = c + hi;
            store_s1(&S[(size_t)(J * 64 + cc) * ld + i0 + r], myT[cc * TILE_PAD + r], nt);
          }
        }
      }
      if (TILE_R == 64) bits[(size_t)j * W + (i0 >> 6)] = colword;
      else if (TILE_R == 32) reinterpret_cast<uint32_t*>(bits)[((size_t)j * W + (i0 >> 6)) * 2 + (h % SUB)] = (uint32_t)colword;
      else reinterpret_cast<uint16_t*>(bits)[((size_t)j * W + (i0 >> 6)) * 4 + (h % SUB)] = (uint16_t)colword;
    }
    return;
  }
  auto row_pair = [&](int r, auto guarded) {
    constexpr bool G = decltype(guarded)::value;
    float dpa, dqa, dpb, dqb;
    {  // row operands: wave-uniform addresses -> scalar loads, no VALU work
      const float ipx = px[i0s + r], ipy = py[i0s + r], ipz = pz[i0s + r], iqx = qx[i0s + r], iqy = qy[i0s + r],
                  iqz = qz[i0s + r];
      dpa = dist3_fast(ipx, ipy, ipz, jpx, jpy, jpz);
      dqa = dist3_fast(iqx, iqy, iqz, jqx, jqy, jqz);
    }
    {
      const float ipx = px[i0s + r + 1], ipy = py[i0s + r + 1], ipz = pz[i0s + r + 1], iqx = qx[i0s + r + 1],
                  iqy = qy[i0s + r + 1], iqz = qz[i0s + r + 1];
      dpb = dist3_fast(ipx, ipy, ipz, jpx, jpy, jpz);
      dqb = dist3_fast(iqx, iqy, iqz, jqx, jqy, jqz);
    }
    const int ia = i0 + r, ib = ia + 1;
    const float da = fabsf(dpa - dqa), db = fabsf(dpb - dqb);
    bool ea = (da <= d_thr) && (dpa >= min_len) && (dqa >= min_len);
    bool eb = (db <= d_thr) && (dpb >= min_len) && (dqb >= min_len);
    if (G) {
      ea = ea && (j != ia) && (j < n) && (ia < rlim);
      eb = eb && (j != ib) && (j < n) && (ib < rlim);
    }
    const uint64_t worda = __ballot(ea), wordb = __ballot(eb);
    float sa = 0.0f, sb = 0.0f;
    if ((worda | wordb) != 0) {
      const float va = sc_expf((da * da) * nis), vb = sc_expf((db * db) * nis);
      sa = ea ? va : 0.0f;
      sb = eb ? vb : 0.0f;
    }
    if (DENSE) {
      if (!G || ia < rlim) store_s1(&S[(size_t)(ia - srow) * ld + j], sa, nt);
      if (!G || ib < rlim) store_s1(&S[(size_t)(ib - srow) * ld + j], sb, nt);
    }
    if (lane == r) rowword = worda;
    if (lane == r + 1) rowword = wordb;
    if (!RECT) {
      colword |= (ea ? (1ull << r) : 0ull) | (eb ? (2ull << r) : 0ull);
      if (DENSE && !diag) { myT[lane * TILE_PAD + r] = sa; myT[lane * TILE_PAD + r + 1] = sb; }
    }
  };
  if (interior) {
#pragma unroll 2
    for (int r = 0; r < TILE_R; r += 2) row_pair(r, std::false_type{});
  } else {
#pragma unroll 2
    for (int r = 0; r < TILE_R; r += 2) row_pair(r, std::true_type{});
  }
  if (lane < TILE_R && i0 + lane < rlim) bits[(size_t)(i0 + lane) * W + J] = rowword;
  if (!RECT && degp && lane < TILE_R && i0 + lane < rlim) {  // (a tile on the diagonal: only the columns beyond the row itself)
    const int b = (i0 + lane) & 63;
    const uint64_t up = diag ? (b == 63 ? 0ull : (rowword & (~0ull << (b + 1)))) : rowword;
    const uint32_t pc = (uint32_t)__popcll(up);
    if (pc) atomicAdd(&degp[i0 + lane], pc);
  }
  if (!RECT && !diag) {
    // mirrored half: row j of S, columns i0 .. i0 + TILE_R - 1; SUB output rows per instruction
    if (DENSE) {
      const int r = lane & (TILE_R - 1), hi = lane / TILE_R;
#pragma unroll 4
      for (int c = 0; c < 64; c += SUB) {
        const int cc = c + hi;
        const float v = myT[cc * TILE_PAD + r];
        const int jj = J * 64 + cc;
        if (jj < n) store_s1(&S[(size_t)jj * ld + i0 + r], v, nt);
      }
    }
    // mirrored adjacency: row j, piece (h % SUB) of word (i0 / 64)
    if (j < n) {
      if (TILE_R == 64) bits[(size_t)j * W + (i0 >> 6)] = colword;
      else if (TILE_R == 32) reinterpret_cast<uint32_t*>(bits)[((size_t)j * W + (i0 >> 6)) * 2 + (h % SUB)] = (uint32_t)colword;
      else reinterpret_cast<uint16_t*>(bits)[((size_t)j * W + (i0 >> 6)) * 4 + (h % SUB)] = (uint16_t)colword;
    }
  }
}

// rows [row0, row1) of the graph (row0 a multiple of 64, row1 <= n); the whole matrix (symmetric tiles, each pair
// evaluated once) when the range is [0, n).  S == nullptr: adjacency bits only (SC_FLAG_NO_DENSE_S).  For a proper
// sub-range S holds the rows of the range only (row i at S + (i - row0) * ld).
// XCD-aware order of the 64 x 64 blocks (m, J), m <= J, of the symmetric form.  A 64-byte line of a bit row holds 8 adjacency
// words, and they are written by 8 DIFFERENT workgroups: row block m's words J = 8 k .. 8 k + 7 by the direct halves of (m, 8 k ..),
// and — the mirrored half — column block J's words m = 8 k' .. by (8 k' .., J).  Workgroups go to the 8 XCDs round-robin by
// index, each XCD has its own L2, and a line assembled in eight L2s leaves each of them as a partial write: the bits-only
// form of the kernel wrote 12.2 MB for 3.2 MB of bit rows (profiles/r03_pmc_compat_writes.txt).  So the blocks are dealt to
// the XCDs by 8 x 8 SUPER-blocks (all eight writers of a line in one super-block, hence one L2, and close together in its
// dispatch order): entry b of the map is the block workgroup b takes — workgroup b runs on XCD b % 8 —, ~0 pads the XCDs'
// lists to one length.  Super-blocks are dealt largest first to the XCD with the least work so far.
std::vector<uint32_t> compat_wg_map(int W) {
  const int SB = (W + 7) / 8;
  struct Super { int sj, sm; int tiles; };
  std::vector<Super> sup;
  for (int sj = 0; sj < SB; sj++)
    for (int sm = 0; sm <= sj; sm++) {
      int tiles = 0;
      for (int J = sj * 8; J < W && J < sj * 8 + 8; J++)
        for (int m = sm * 8; m <= J && m < sm * 8 + 8; m++) tiles++;
      if (tiles) sup.push_back(Super{sj, sm, tiles});
    }
  std::stable_sort(sup.begin(), sup.end(), [](const Super& a, const Super& b) { return a.tiles > b.tiles; });
  std::vector<uint32_t> lists[8];
  for (const Super& su : sup) {
    int best = 0;
    for (int x = 1; x < 8; x++) if (lists[x].size() < lists[best].size()) best = x;
    for (int J = su.sj * 8; J < W && J < su.sj * 8 + 8; J++)
      for (int m = su.sm * 8; m <= J && m < su.sm * 8 + 8; m++) lists[best].push_back((uint32_t)(J * (J + 1) / 2 + m));
  }
  size_t len = 0;
  for (int x = 0; x < 8; x++) len = lists[x].size() > len ? lists[x].size() : len;
  std::vector<uint32_t> map(8 * len, 0xFFFFFFFFu);
  for (int x = 0; x < 8; x++)
    for (size_t k = 0; k < lists[x].size(); k++) map[8 * k + x] = lists[x][k];
  return map;
}

void launch_compat(const Points& pts, const CompatOpts& o, const Derived& dv, float* S, uint64_t* bits, int row0, int row1,
                   const Tuning& tn, hipStream_t st) {
  const StatsJob sj{o.stat_part, o.stat_part ? (uint32_t)((pts.ld + 255) / 256) : 0u, o.stat_out};
  const int W = pts.ld >> 6;
  const int two_phase = tn.compat_one_phase ? 0 : 1;  // the one-phase interior form stays for A/B and parity
  const bool rect = !(row0 == 0 && row1 >= pts.n);
  // S stores, measured r02 (profiles/r02_ab_compat_stores.txt): on the first box 16 bytes per lane paid on the big matrix
  // (C3, N = 20 000: 346 vs 404 us, alternating with the form four times in one process) and cost a little on the small
  // one, where the kernel's time is a wave's latency (C2: 25.8 vs 23.7 us); on another box, later, C3 ran 400-420 us in
  // EVERY form.  So: 16-byte stores from ~N = 8000 on (never slower there), 4-byte below; non-temporal stores changed
  // nothing anywhere.  Tuning::compat_store_mode forces a form (bit 0: 4-byte, bit 2: 16-byte), bit 1 adds the nt hint.
  const long long tiles_all = rect ? (long long)((row1 - row0 + 15) / 16) * W : 2ll * W * (W + 1);
  int mode = (tiles_all >= 32768 || rect) ? 0 : 1;
  if (tn.compat_store_mode & 1u) mode = 1;
  if (tn.compat_store_mode & 4u) mode = 0;
  mode |= (int)(tn.compat_store_mode & 2u);
#define SC_COMPAT_ARGS pts.planes, pts.n, pts.ld, dv.d_thr, dv.min_len, dv.neg_inv2sig2, S, bits, n_tiles, two_phase, row0, row1, mode, o.degp, map_arg, sj
  const uint32_t* map_arg = nullptr;  // (only the symmetric 16- and 32-row forms take the map: there a workgroup is a 64 x 64 block)
  if (rect) {
    if (row1 <= row0) return;
    // one-sided 16-row tiles over the rectangle (every pair of the block evaluated by this rank)
    const int n_tiles = ((row1 - row0 + 15) / 16) * W;
    if (S) hipLaunchKernelGGL((compat_tiles_kernel<16, 4, true, true>), dim3((n_tiles + 3) / 4), dim3(256), 0, st, SC_COMPAT_ARGS);
    else hipLaunchKernelGGL((compat_tiles_kernel<16, 4, false, true>), dim3((n_tiles + 3) / 4), dim3(256), 0, st, SC_COMPAT_ARGS);
    return;
  }
  // tile height: 16 rows (4.3 KiB LDS image per wave, 4 waves per workgroup), 32 rows (8.4 KiB, 2 waves per workgroup) or
  // 64 rows (16.6 KiB, one wave per workgroup; the mirrored half is then written as full 256-byte segments).  Measured: C2 28 vs 49 us, C3 432 vs
  // 435 us — bigger mirrored pieces do not pay for the lost occupancy.  Tuning::compat_rows = 64 selects it (experiments).
  // r02, by size (HIP-event bracket around the kernel, alternating in one process): N = 6000 31 vs 40 us, 8000 52 vs 58,
  // 10 000 97 vs 91, 12 000 137 vs 129, 16 000 264 vs 226, 20 000 (C3) 430 vs 372 for 16- vs 32-row tiles: from ~10 000
  // correspondences on the launch has enough tiles that the taller tile's lower occupancy no longer shows, and its
  // 128-byte mirrored pieces and half as many row operands per pair do.
  const int tr = tn.compat_rows == 64 ? 64 : (tn.compat_rows == 32 ? 32 : (tn.compat_rows == 16 ? 16 : (pts.n >= 10000 ? 32 : 16)));
  if (tr == 32) {
    const int n_tiles = 2 * W * (W + 1) / 2;
    map_arg = o.wg_map;
    const unsigned grid = o.wg_map ? o.wg_map_len : (unsigned)((n_tiles + 1) / 2);
    if (S) hipLaunchKernelGGL((compat_tiles_kernel<32, 2, true, false>), dim3(grid), dim3(128), 0, st, SC_COMPAT_ARGS);
    else hipLaunchKernelGGL((compat_tiles_kernel<32, 2, false, false>), dim3(grid), dim3(128), 0, st, SC_COMPAT_ARGS);
  } else if (tr == 64) {
    const int n_tiles = W * (W + 1) / 2;
    if (S) hipLaunchKernelGGL((compat_tiles_kernel<64, 1, true, false>), dim3(n_tiles), dim3(64), 0, st, SC_COMPAT_ARGS);
    else hipLaunchKernelGGL((compat_tiles_kernel<64, 1, false, false>), dim3(n_tiles), dim3(64), 0, st, SC_COMPAT_ARGS);
  } else {
    const int n_tiles = 4 * W * (W + 1) / 2;
    map_arg = o.wg_map;
    const unsigned grid = o.wg_map ? o.wg_map_len : (unsigned)((n_tiles + 3) / 4);
    if (S) hipLaunchKernelGGL((compat_tiles_kernel<16, 4, true, false>), dim3(grid), dim3(256), 0, st, SC_COMPAT_ARGS);
    else hipLaunchKernelGGL((compat_tiles_kernel<16, 4, false, false>), dim3(grid), dim3(256), 0, st, SC_COMPAT_ARGS);
  }
#undef SC_COMPAT_ARGS
}

}  // namespace sc
