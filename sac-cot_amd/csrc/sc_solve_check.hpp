// sc_solve_check.hpp — the host-only rules of sc_pairs_solve (include/saccot.h) that sc_pairs_sync does not already have: what is
// refused of sc_solve_params, of the four strides and of the anchor, the three thresholds, and where the workspace areas lie.  The
// list's rules, the adjacency, the staged image (the records, the entries, the list starts) and the rules every pair-list entry
// shares are sc_cycles_check.hpp's, the pose records every pose entry's (sc_pose_check.hpp).  No HIP: sc_capi_solve.hip includes it, and so does
// tests/native/solve_check_main.cpp, a program of its own that runs these functions under the sanitizers on the CPU.
#pragma once
#include "sc_sync_check.hpp"

namespace sc {

constexpr uint32_t SOLVE_MAX_OUTER = 32, SOLVE_MAX_INNER = 256, SOLVE_MAX_PRODUCT = 2048;
constexpr uint32_t SOLVE_INFO_BYTES = 288, SOLVE_INFO_STATUS_AT = 296, SOLVE_INIT_BYTES = 160;

inline bool solve_reads_status(const sc_solve_params* sp) { return (sp->flags & SC_SOLVE_STATUS) != 0; }
inline bool solve_reads_info_status(const sc_solve_params* sp) { return (sp->flags & SC_SOLVE_INFO_STATUS) != 0; }

// What a call refuses of its parameter block, of the strides and of the anchor — the rule that is broken, for the caller to put its
// name in front of; nullptr: they are fine.
inline const char* solve_params_error(const sc_solve_params* sp) {
  if (sp->size != sizeof(sc_solve_params)) return "params->size is not sizeof(sc_solve_params)";
  if (sp->max_outer < 1 || sp->max_outer > SOLVE_MAX_OUTER) return "max_outer must be 1 .. 32";
  if (sp->max_inner < 1 || sp->max_inner > SOLVE_MAX_INNER) return "max_inner must be 1 .. 256";
  if (sp->max_outer * sp->max_inner > SOLVE_MAX_PRODUCT) return "max_outer * max_inner must not exceed 2048";
  if (const char* what = pairs_tol_error(sp->rot_tol, sp->trans_tol)) return what;
  if (!(sp->cg_tol >= 0.f && sp->cg_tol < 1.f)) return "cg_tol must be finite and in [0, 1)";
  if (sp->flags & ~(SC_SOLVE_STATUS | SC_SOLVE_INFO_STATUS)) return "an unknown flag";
  return nullptr;
}
inline const char* solve_stride_error(const sc_solve_params* sp, uint32_t pose_stride, bool has_use, uint32_t use_stride, bool has_info,
                                      uint32_t info_stride, uint32_t init_stride) {
  if (!pose_stride_ok(pose_stride, solve_reads_status(sp))) return "pose_stride must be a multiple of 4 and at least 48 (52 with SC_SOLVE_STATUS)";
  if (const char* what = pairs_use_stride_error(has_use, use_stride)) return what;
  if (has_info && (info_stride % 8 != 0 || info_stride < (solve_reads_info_status(sp) ? SOLVE_INFO_STATUS_AT + 4 : SOLVE_INFO_BYTES)))
    return "info_stride must be a multiple of 8 and at least 288 (300 with SC_SOLVE_INFO_STATUS)";
  if (init_stride % 8 != 0 || init_stride < SOLVE_INIT_BYTES) return "init_stride must be a multiple of 8 and at least 160";
  return nullptr;
}
inline const char* solve_anchor_error(const sc_solve_params* sp, uint32_t n_sets) { return pairs_anchor_error(sp->anchor, n_sets); }

// The three thresholds a call uses (of parameters that solve_params_error accepts): r2_max and e2_max from where sync_thresholds
// takes them, and cg2.
inline void solve_thresholds(const sc_solve_params* sp, double out[3]) {
  out[0] = pairs_r2_max(sp->rot_tol);
  out[1] = pairs_e2_max(sp->trans_tol);
  out[2] = (double)sp->cg_tol * (double)sp->cg_tol;
}

// Bytes of the info and init arrays a call reads: a record's head at byte k * stride.
inline uint64_t solve_info_bytes_read(uint64_t n_pairs, uint32_t info_stride, bool reads_status) {
  return n_pairs == 0 ? 0 : (n_pairs - 1) * info_stride + (reads_status ? SOLVE_INFO_STATUS_AT + 4 : SOLVE_INFO_BYTES);
}
inline uint64_t solve_init_bytes_read(uint64_t n_sets, uint32_t init_stride) { return n_sets == 0 ? 0 : (n_sets - 1) * init_stride + SOLVE_INIT_BYTES; }

// ---- the device workspace behind the staged words (sync_meta_bytes of them), three areas; every array starts on 8 bytes.
//   pair  per pair: the oriented fp64 poses (192 bytes), W_p (288), g_p (48), the errors of two states (2 x 24), the usable word
//         (8 with its pad): 584 bytes.
//   set   per set: X twice (2 x 96), x, r, z, q (48 each), p twice (2 x 48), the factor (168), SolveInfo (16): 664 bytes.
//   ctl   the control words (SolveCtl, sc_kernels.hpp) in SOLVE_CTL_BYTES, the sets' tallies of usable pairs behind them — the two
//         are zeroed by one memset —, then the chunk sums: 3 doubles per chunk of 64 sets, one per chunk of 64 pairs.
constexpr uint32_t SOLVE_CTL_BYTES = 19456;
constexpr uint32_t SOLVE_CHUNK = 64;
constexpr uint64_t solve_chunks(uint64_t n) { return (n + SOLVE_CHUNK - 1) / SOLVE_CHUNK; }
struct SolveLayout {
  uint64_t wide, W, g, err, usable, pair_bytes;          // in the pair area
  uint64_t X, x, r, z, q, p, fac, sinfo, set_bytes;      // in the set area
  uint64_t deg, zero_bytes, rzc, pqc, costc, ctl_bytes;  // in the ctl area (zero_bytes: what the memset clears, from byte 0)
};
inline SolveLayout solve_layout(uint32_t n_sets, uint32_t n_pairs) {
  SolveLayout l{};
  const uint64_t P = n_pairs, S = n_sets;
  l.wide = 0; l.W = l.wide + 192 * P; l.g = l.W + 288 * P; l.err = l.g + 48 * P; l.usable = l.err + 48 * P; l.pair_bytes = l.usable + 8 * P;
  l.X = 0; l.x = l.X + 192 * S; l.r = l.x + 48 * S; l.z = l.r + 48 * S; l.q = l.z + 48 * S; l.p = l.q + 48 * S; l.fac = l.p + 96 * S;
  l.sinfo = l.fac + 168 * S; l.set_bytes = l.sinfo + 16 * S;
  l.deg = SOLVE_CTL_BYTES; l.zero_bytes = (l.deg + 4 * S + 15) / 16 * 16;
  l.rzc = l.zero_bytes; l.pqc = l.rzc + 16 * solve_chunks(S); l.costc = l.pqc + 8 * solve_chunks(S); l.ctl_bytes = l.costc + 8 * solve_chunks(P);
  return l;
}

}  // namespace sc
