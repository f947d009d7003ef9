// sc_kernels.hpp — launchers of the hand-written gfx950 kernels (one per SURVEY.md §8(a) row).
// Every launcher only enqueues on `st`; none allocates, frees or synchronises (capture-safe).
#pragma once
#include <cstddef>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "../../include/saccot.h"
#include "sc_chunks.hpp"

namespace sc {

std::vector<uint32_t> compat_wg_map(int W);  // sc_compat.hip (run_compat, sc_capi_compat.hip, caches it per row width): which 64 x 64 block workgroup b of stage A takes (XCD-aware)

// Derived fp32 constants, computed once per call on the host in fp64.
struct Derived {
  float d_thr;         // sigma * sqrt(-2 ln t_cmp)
  float neg_inv2sig2;  // -1 / (2 sigma^2)
  float tau2;          // tau^2
  float min_len;
  float inv_tau2;      // 1 / tau^2   (score modes MSE / MAE, include/saccot.h)
  float inv_tau;       // 1 / tau
};
// what score_term compares against (`thr` of the scoring kernels): tau^2, 1 / tau^2 or 1 / tau by score_mode
__host__ __device__ __forceinline__ float score_thr(const Derived& dv, int score_mode) {
  const float inv_tau2 = dv.inv_tau2, inv_tau = dv.inv_tau, tau2 = dv.tau2;  // (read first: a choice among values, not among addresses)
  return score_mode == SC_SCORE_MSE ? inv_tau2 : (score_mode == SC_SCORE_MAE ? inv_tau : tau2);
}

// Scheduling / fallback knobs of the kernels.  The shipped library reads NO environment variable: these defaults are
// what runs, and only sc_set_debug() (include/saccot.h, test and tuning hook) changes them, per context.  None of them
// can change a result — only the launch geometry or which of two bit-identical code paths runs.
struct Tuning {
  bool no_events = false;          // row-walking count / key kernels instead of the event list
  uint64_t event_cap = 0;          // forced event capacity (0: the context's own, grown after an overflow)
  size_t compact_self_max = 4096;  // tiles up to which compact_write adds up the tile counts by itself
  size_t scan_self_max = 4096;     // tiles up to which the scan's down-sweep adds up the block sums by itself
  uint32_t cnt_blocks = 0, keys_blocks = 0, sel_blocks = 0;  // grid sizes (0: automatic)
  int tg_count = 8, tg_keys = 8, tg_sample = 0;              // lanes per edge (tg_sample 0: by row width)
  int tg_events = 0;               // lanes per edge of the event-recording counting pass (0: by row width)
  uint32_t sample_mode = 0;        // pruning sample: 0 by size (launch_sample_hist), 1 every stride-th edge, 2 the heaviest edges (both CERTIFY their bound)
  bool no_edge_build = false;      // row statistics and edge list as separate launches (not launch_edge_build)
  bool compat_linear_order = false;  // stage A's 64 x 64 blocks in index order (r03) instead of the XCD-aware order
  bool no_estimate = false;        // never prune by an ESTIMATED bound (sc_tri_prune.hip 3c): always one of the certifying samples
  uint32_t est_margin_pct = 0;     // the estimate aims at the (pct / 100 x T)-th key (0: 200; tests force failures with a small one)
  uint32_t sample_blocks = 0;      // grid of the heaviest-edge sample (0: one block per 256 edges)
  bool rows_unfused = false;       // row_stats and the scan(s) of the row counts as separate launches (round 1's form)
  uint64_t sample_edges = 0;       // edges of the pruning sample (0: automatic, ~5T/8)
  uint32_t score_split = 0;        // share (of 256) of the hypotheses scored on the matrix pipe
  uint32_t score_filter = 0;       // C2, inlier count: 0 = by size and scale (plain kernel / linear filter / Gram filter), 1 = plain kernel, 2 = linear filter, 3 = Gram filter
  uint32_t filter_splits = 0;      // grid.y of the filter (0: by size)
  uint32_t filter_queue_cap = 0;   // entries of the filter's global queue (0: by size; tests force overflows with a small one)
  uint32_t filter_lds_queue = 0;   // entries of a wave's LDS queue, 64 .. 256 (0: 256)
  uint32_t filter_variant = 0;     // body of the filter kernel (sc_filter.hip): 0 default, bit-identical scheduling variants, >= 16 timing-only ablations
  uint32_t gram_kappa_q4 = 0;      // the Gram filter's cut: hypotheses whose reach stays under (value / 16) tau' count as NEAR the reference (0 = GX_KAPPA = 8; 1 = practically no cut)
  bool gram_ref_late = false;      // the Gram filter's reference frame is voted after the selection, in a launch of its own (what every path but the hot one does anyway), instead of under the counting pass
  bool no_fast = false;            // sc_register_device never enqueues host-free (always waits for stage B's two counts)
  bool no_lane = false;            // a host-free sc_register_device_async frame stays on the caller's stream (never on the context's lane)
  bool gram_guard_fail = false;    // the matrix-pipe probe reports a violation (tests of the guard)
  bool filter_blind = false;       // the host decides C2's kernel WITHOUT the coordinate maxima (as if they had not arrived yet)
  bool compat_one_phase = false;   // exact chain on every pair of an interior tile
  bool scan_ordinals = false;      // stage B's hot path keeps the scan of the per-edge counts (no ordered strong list: sc_tri.hip 2c)
  uint32_t ord_chunk_max = 0;      // chunks of the ordered strong list the key kernel accepts (0: ORD_CHUNK_MAX; tests force the fallback with a small one)
  int compat_rows = 0;             // tile height of stage A: 0 = by size (16 below 10 000 correspondences, 32 from there), 16, 32, 64
  uint32_t compat_store_mode = 0;  // 0: by size; bit 0: force 4-byte S stores, bit 2: force 16-byte, bit 1: non-temporal
};

// LbArgs: what a look-back launch needs from its caller.  desc: the tile descriptors (8 bytes per tile and value) in a
// persistent area that ONLY look-back launches write — zeroed once, and again whenever the 12-bit epoch wraps; epochs
// 1 .. 4095 are handed out one per launch, so words of earlier launches read as "nothing yet".  ticket / err: two
// words that are NEVER descriptor storage (a ticket that aliased an old descriptor would hand out garbage tile
// indices): the ticket is zero between launches (the last tile of a launch resets it).
// A descriptor carries 50 bits of value (sc_block.hpp): every prefix of a look-back launch, its total included, stays below
// 2^50.  desc is 8-byte aligned; one area serves launches of any tile count, each under an epoch of its own.
struct LbArgs {
  uint32_t* ticket = nullptr;
  uint32_t* err = nullptr;
  uint64_t* desc = nullptr;
  uint32_t epoch = 0;
};

// Device view of the padded SoA point planes: px py pz qx qy qz, each `ld` floats (ld = roundup(n,64)),
// zero-filled beyond n — followed, at planes + 6 * ld, by an AoS copy of 8 floats per correspondence
// (px py pz qx qy qz 0 0; 32-byte aligned) for the consumers that fetch one whole correspondence at a time.
struct Points {
  const float* planes;  // (6 + 8) * ld
  int n;
  int ld;
};

// ---- input staging -----------------------------------------------------------------------------
// user layout (AoS n x 3 or SoA 3 x n) -> padded planes; sets *bad_flag != 0 when a value is not finite.
// bad_flag may be host-pinned memory: it is only touched (atomicOr) when a non-finite value is found.
// zero[0]: a buffer (the per-call control block) the kernel clears on the way — saves a memset launch; zero[1]: a second one.
// coord_max (optional, 2 x u32): atomicMax of the bit patterns of max |src coordinate| and max |tgt coordinate|; with it:
// coord_max_next (the pair the NEXT call uses: cleared by the last block), mx_ticket (a zeroed u32, left zero; nullptr: the rows
// of coord_part stay unreduced — launch_compat's stat_part) and
// host_max (pinned u64: receives max|tgt| << 32 | max|src| once every block is done).
// The coordinate statistics are FX_MX_WORDS u32 (coord_max, WRITTEN — not accumulated — by the last block of the launch):
// [0] max |src coordinate|, [1] max |tgt coordinate| (bit patterns), [2 + c] / [8 + c]: float_key of the largest / of minus
// the smallest value of coordinate c (px py pz qx qy qz): the bounding boxes.  coord_part: 16 u32 per block of the launch
// (stage_part_words(ld)), scratch.  host_box (pinned, 6 x u64, optional): (key of -min) << 32 | key of max per
// coordinate, written before host_max.
constexpr int FX_MX_WORDS = 16;
inline size_t stage_part_words(int ld) { return (size_t)((ld + 255) / 256) * 16; }
// The launch's views (host-side; stage_inputs, sc_capi_compat.hip, fills them): where the coordinate statistics go, and the buffers cleared on the way.
struct CoordStatsOut { uint32_t* coord_max; uint32_t* coord_part; uint32_t* mx_ticket; uint64_t* host_max; uint64_t* host_box; };
struct ZeroSpan { uint32_t* p; uint32_t words; };
void launch_stage_points(const CoordStatsOut& cs, const ZeroSpan (&zero)[2], const float* d_src, const float* d_tgt, int n, int ld,
                         int layout, float* planes, uint32_t* bad_flag, hipStream_t st);
// order-preserving map float -> u32 (all finite floats and infinities; 0 is below every float) and back
__host__ __device__ inline uint32_t float_key(float f) {
  union { float f; uint32_t u; } x; x.f = f;
  return (x.u & 0x80000000u) ? ~x.u : (x.u | 0x80000000u);
}
__host__ __device__ inline float float_unkey(uint32_t k) {
  union { float f; uint32_t u; } x; x.u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  return x.f;
}
// can C2's filter bound its error at this tau?  (the host-side twin of the test every wave of the filter makes; maxima as
// the staging kernel published them, ~0 = not known: assume yes)
bool filter_in_range(uint64_t host_max, float tau2);

// ---- stage A: compat_graph -----------------------------------------------------------------------
// S: n x ld fp32 (row-major, symmetric, zero diagonal / pad columns); bits: n x (ld/64) u64;
// rows [row0, row1) (row0 a multiple of 64): the whole matrix by symmetric tiles for [0, n), one-sided tiles for a
// row block (then S, if given, holds the rows of the block only).  S == nullptr: adjacency bits only.
// degp (optional, whole-matrix form only; n u32, ZEROED): also accumulates deg+[i] = edges (i, j) with j > i (atomics).
// wg_map / wg_map_len (optional, whole-matrix form): the XCD-aware order of the 64 x 64 blocks, compat_wg_map(ld / 64) on the
// device — the launch then has wg_map_len workgroups.
// stat_part / stat_out (optional): the staging launch was given no ticket (mx_ticket == nullptr) and left its per-workgroup rows
// of coordinate statistics unreduced: one wave of this launch reduces them into the FX_MX_WORDS words.
struct CompatOpts { uint32_t* degp; const uint32_t* wg_map; uint32_t wg_map_len; const uint32_t* stat_part; uint32_t* stat_out; };  // (CompatOpts{}: none)
void launch_compat(const Points& pts, const CompatOpts& o, const Derived& dv, float* S, uint64_t* bits, int row0, int row1,
                   const Tuning& tn, hipStream_t st);
// The row arrays as the launches see them — RowStats, RowOffsets, ShardCut: plain host-side views, as stage B's are, each filled by one
// accessor of the host driver (sc_capi_compat.hip: rows_of, offsets_of; sc_capi_tri.hip: cut_of), behind the last ENSURE of what it names.
//
// deg[i] = edges of i; degp[i] = edges (i,j) with j > i; wpre: n x (ld/64) u32, set bits of row i in words [0,w).
// zero_rows (optional): an n x W u64 matrix cleared on the way (the pruned bit matrix of stage B).
// rowcost (optional, n u32): per-row estimate of stage B's work (see row_stats_kernel), for launch_shard_split.
struct RowStats { uint32_t* deg; uint32_t* degp; uint32_t* wpre; uint64_t* zero_rows; uint32_t* rowcost; };
// edge_off (n + 1 CSR row offsets), ebase (n per-row CSR bases), cost_pre (optional, n + 1: prefix of the row costs)
struct RowOffsets { uint64_t* edge_off; uint32_t* ebase; uint64_t* cost_pre; };
// one rank's share of the rows: own_row[0..1] and the CSR edge range own_edge[0..1] (ControlBlock), written by either split
struct ShardCut { uint32_t rank, world; uint32_t* own_row; uint64_t* own_edge; };
void launch_row_stats(const Points& pts, const uint64_t* bits, const RowStats& rs, hipStream_t st);
// row_stats and the prefixes over the rows in one launch (decoupled look-back over 64-row tiles): also ro (rs.rowcost is not written:
// the costs go straight into ro.cost_pre) and the edge count
// into host_total.  lb: row_stats_scan_state_bytes(n) of the caller's look-back state area and this launch's epoch.
size_t row_stats_scan_state_bytes(int n);
void launch_row_stats_scan(const Points& pts, const uint64_t* bits, const RowStats& rs, const RowOffsets& ro, const LbArgs& lb,
                           uint64_t* host_total, hipStream_t st);
// this rank's contiguous, equally heavy row range (own_row[0..1]) and its CSR edge range (own_edge[0..1])
// from the exclusive prefix of rowcost (ro.cost_pre, n + 1 entries) — device-side, identical on every rank.
void launch_shard_split(const RowOffsets& ro, const ShardCut& cut, int n, hipStream_t st);

// ---- exclusive scan u32 -> u64 (out has n+1 entries; out[n] = total) -----------------------------
// Extras a scan can do on its way (all optional; ScanExtra{}: none):
//   host_total: host-pinned u64 that also receives the total, written by the kernel itself — the host
//     reads it after its next stream synchronise, with no copy kernel in between;
//   range (device, [lo, hi)): outside it every input is known to be zero — tiles wholly outside are neither read nor
//     written (sharded stage B: the triangle counts of the edges other ranks enumerate); out[n] is still the total;
//   deg / degp / ebase: also ebase[i] = (u32) out[i] - (deg[i] - degp[i]), the CSR base of row i (launch_edge_fill).
//   lb.epoch != 0: the single-pass (decoupled look-back) form.  PRECONDITION: the total is below 2^50 (the value field of a
//     descriptor, see LbArgs) — the forms without look-back carry 64 bits and have no such limit.
// Alignment (every form, and the select / compaction kernels' key arrays likewise): `in` / wkey and `out` are 16-byte aligned —
// whole tiles are read as uint4 and written as pairs of u64.  The one-block form (n <= 8192) does not look at `range`: there the
// inputs outside it ARE zero.
struct ScanExtra {
  LbArgs lb;
  const uint64_t* range = nullptr;
  const uint32_t* deg = nullptr;
  const uint32_t* degp = nullptr;
  uint32_t* ebase = nullptr;
  uint64_t* host_total = nullptr;
};
// what every scan of a caller works with: temp (scan_temp_bytes(n) of scratch) and the knobs
struct ScanWork { void* temp; const Tuning& tn; };
struct ScanJob { const uint32_t* in; uint64_t* out; ScanExtra x; };
size_t scan_temp_bytes(size_t n);
void launch_scan_u32(const ScanWork& w, const uint32_t* in, size_t n, uint64_t* out, const ScanExtra& x, hipStream_t st);
// two arrays of the same length in one go (one launch when n is small); b.in may be null (ScanJob{}: no second array); host_total:
// of array a only (b's is not looked at)
void launch_scan_u32_pair(const ScanWork& w, const ScanJob& a, const ScanJob& b, size_t n, hipStream_t st);

// ---- stage B: triangles_topT ---------------------------------------------------------------------
struct Graph {
  const uint64_t* bits;  // n x W
  const float* S;        // n x ld
  const uint32_t* deg;
  const uint32_t* degp;  // edges to higher indices
  const uint32_t* wpre;  // n x W word-prefix popcounts of `bits`
  int n, ld, W;
};
// The context's stage-B arrays as the launches see them — EdgeList, EdgeCounts, Pruned, KeyArrays, Selection: plain views, each
// filled by one accessor of the host driver (sc_capi_tri.hip: edges_of, counts_of, pruned_of, keys_of, selection_of).  A launcher
// takes the views it reads or writes, then what is per launch, then the stream.
//
// CSR edge list of the upper triangle, rows ascending, columns ascending: ei/ej/es (es = S[i][j]).
// ebase[i] (u32, modular): CSR index of edge (i,k), k > i, is ebase[i] + wpre[i][k/64] + popc(bits[i][k/64] below k).
// ebi[e] / ebj[e]: the bases of both ends of edge e (so an edge is fetched in one memory level).  ebi == ebj == nullptr: the
// fused edge kernel (launch_edge_build) made the list and wrote no per-edge bases — whoever wants them looks them up in ebase.
// E: the edge count — or, in a host-free call (launched before the host knows it, sc_capi_tri.hip), what the grids and the arrays
// COVER: the true count is then *E_dev (device; nullptr on a waited call) and the kernels work on min(E, *E_dev) edges.
// E_hint: the count that host-side choices which only cost time go by (the sample's form and stride, the counting pass's grid): E,
// or a host-free call's last known count.  cap: entries the arrays hold (the kernels that fill them drop writes beyond it).
struct EdgeList {
  uint32_t* ei; uint32_t* ej; float* es;
  uint32_t* ebi; uint32_t* ebj; uint32_t* ebase;
  uint64_t E; const uint64_t* E_dev; uint64_t E_hint;
  uint64_t cap;
};
// Per-edge triangle counts and what their scan makes of them: toff[e] = triangles of the edges before e, toff[E] = all of them.
// own (optional, device; sharded stage B): [lo, hi) of the edges this rank enumerates — the others count 0.
struct EdgeCounts {
  uint32_t* tcnt; uint64_t* toff; const uint64_t* own;
  // toff as its 2 E + 2 u32 words: where an OrdList's tloc and ctot live (no scan writes toff then; the count still lands in toff[E])
  uint32_t* words() const { return reinterpret_cast<uint32_t*>(toff); }
};
// ebase_ready: the per-row CSR bases were written by the scan of deg+ (ScanExtra, tiled form) and are READ here;
// otherwise they are derived on the fly and this kernel writes them.  scan_writes_ebase(n) tells which.
bool scan_writes_ebase(size_t n);
void launch_edge_fill(const Graph& g, const Points& pts, const Derived& dv, const uint64_t* edge_off, const EdgeList& el,
                      bool ebase_ready, uint32_t* es_hist, hipStream_t st);  // es_hist: see launch_sample_hist (optional)
// The hot path's form (r04; n <= 20 480, weight ranking, estimated pruning bound): row statistics (wpre), CSR offsets and
// bases from g.degp — which launch_compat accumulated —, the strong-bit rows cleared and the edge list (ei / ej / es; NO ebi /
// ebj: launch_tri_count_events looks the bases up), in one launch.  The edge count lands in edge_off[n] and, where given, in
// host_total (pinned) and as [0, edge count) in live_range (device, 2 x u64).
bool edge_build_fits(int n);
void launch_edge_build(const Graph& g, const Points& pts, const Derived& dv, uint64_t* zero_rows, uint64_t* edge_off, const EdgeList& el,
                       uint64_t* host_total, uint64_t* live_range, hipStream_t st);
// Compact list of the strong edges (those of the pruned graph), written by the pruning kernel in ST_SHARDS regions of
// `cap` entries (fill[r] = entries of region r; ST_SHARDS zeroed counters of the control block).  list == nullptr: off.
constexpr int ST_SHARDS = 256;
struct StrongList {
  uint32_t* list;
  uint32_t* fill;
  uint32_t cap;
  // 0: region r takes the pruning kernel's blocks with block % 256 == r.  > 0: region r takes `region_blocks` CONSECUTIVE
  // blocks (256 edges each), so a region is a contiguous range of edge ids — a rank of the sharded stage B then walks only the
  // regions its own edge range touches (the pruning kernel also zeroes every tcnt entry in this form)
  uint32_t region_blocks;
  // != nullptr: the ORDERED form (sc_tri.hip 2c; region_blocks == 0, one rank, at most ORD_MAX_BLOCKS blocks).  Block b writes its
  // strong edges in ascending order into its own slot list[ORD_BLOCK_EDGES b ..] and their number into cnt[b]: no atomic, and the slots'
  // runs one after the other are the strong edges in edge order.  fill is not touched, and no tcnt entry is zeroed.
  uint32_t* cnt = nullptr;
};
uint32_t strong_list_cap(uint64_t E);
size_t strong_list_bytes(uint64_t E);
// What the pruning leaves (launch_prune_bits): the strong upper-triangle bit matrix mbits (n x W), the strong-edge threshold *smin
// (device float; -1 = nothing certified), *klb (key of the bound or 0) and the strong list.  All null (Pruned{}): no pruning —
// membership is the graph's own bit rows (member_bits) and every edge counts.
struct Pruned {
  uint64_t* mbits;
  float* smin;
  uint32_t* klb;
  StrongList sl;
};
inline const uint64_t* member_bits(const Graph& g, const Pruned& pr) { return pr.mbits ? pr.mbits : g.bits; }
// tcnt[e] = #k > j adjacent (in member_bits) to both ends of edge e = (i,j); edges with es[e] < *smin count 0
void launch_tri_count(const Graph& g, const Pruned& pr, const EdgeList& el, const EdgeCounts& ec, const Tuning& tn, hipStream_t st);

// Certified pruning (weight ranking), two launches:
//  launch_sample_hist: the triangles of every R-th edge go into `hist` (256 u32, zeroed by the caller); `part` of
//    `parts`: this launch takes every parts-th SAMPLED edge starting at `part` (one process per GPU: the histograms of
//    all parts are summed before launch_prune_bits sees them).  key_floor: a value at or below the smallest possible
//    triangle weight.
//  launch_prune_bits: derives *smin and *klb from the histogram, builds the strong bit matrix (already zero), and
//    with sl.list set also compacts the strong edges and zeroes tcnt of the weak ones.
void launch_sample_hist(const Graph& g, const EdgeList& el, uint64_t want, float key_floor, uint32_t part, uint32_t parts,
                        uint32_t* hist, uint32_t* es_hist, const Tuning& tn, hipStream_t st);
// The ESTIMATING sample (r04, sc_tri_prune.hip 3c): one sampled 64-column word in `rate` of every edge's row pair, its triangles'
// keys into `hist` — a uniform 1-in-rate sample of ALL the graph's triangles.  launch_prune_bits then takes the bin where
// rate x (count from the top) reaches margin x T as the bound: an estimate, not a certificate — the select verifies it
// (SelectState::want_req) and the caller repeats the call with a certifying sample when it was too high.
struct SamplePlan {
  bool estimate;       // true: launch_sample_estimate / hist_want below; false: launch_sample_hist (certifying), hist_want = T
  uint32_t rate;       // power of two
  uint64_t hist_want;  // what launch_prune_bits looks for in the histogram
};
SamplePlan sample_plan(uint64_t want, bool allow_estimate, const Tuning& tn, uint64_t E, int W);  // E, W: the graph (0: not known: rate <= 64)
struct SampleCands {  // (off: none kept)
  uint4* cand = nullptr;  // sample_estimate_blocks() entries: the best-keyed triangle each workgroup sampled {key bits, i, j, k} — the voters of stage C2's reference frame (sc_gramref.hpp)
  unsigned long long* slot = nullptr;  // ControlBlock::ref_slot
};
void launch_sample_estimate(const Graph& g, const EdgeList& el, uint32_t rate, uint32_t* hist, const SampleCands& cands, const Tuning& tn,
                            hipStream_t st);
uint32_t sample_estimate_blocks(uint64_t E, const Tuning& tn);  // workgroups launch_sample_estimate uses
uint32_t sample_candidate_blocks(uint64_t E, const Tuning& tn);  // ... of which the first so many leave a candidate behind
// es_hist: PR_HCOPIES x 256 words (control block): the weight histogram of the heaviest-edge sample, filled by launch_edge_fill
// launch_sample_hist ALWAYS accumulates into PR_HCOPIES x 256 words (`hist` = the control block's copies);
// launch_hist_reduce sums them into one 256-bin histogram (the exchanged form); launch_prune_bits reads either
// (hist_is_copies).
void launch_hist_reduce(const uint32_t* copies, uint32_t* out, hipStream_t st);
struct PruneOpts {
  bool logbins = false;  // hist comes from launch_sample_estimate (logarithmic bins of 3.0 - key)
  bool trimmed = false;  // (with el.E_dev) the scan that follows skips the counts beyond *E_dev: the workgroups there leave at once
};
// (with el.E_dev and sl.list the tcnt entries of [*E_dev, E) are zeroed too; ec.own: only this rank's strong edges are listed)
void launch_prune_bits(const Graph& g, const uint32_t* hist, bool hist_is_copies, const EdgeList& el, uint64_t want, float key_floor,
                       const Pruned& pr, const EdgeCounts& ec, const PruneOpts& o, hipStream_t st);
// sharded stage B, after the certificate: work estimate per row of the PRUNED graph (strong_rowcost_kernel), and — in one
// single-block launch — its prefix and this rank's row / edge range (the rule of launch_shard_split)
void launch_strong_rowcost(const Graph& g, const Pruned& pr, uint32_t* rowcost, hipStream_t st);
void launch_cost_split(const RowOffsets& ro, const ShardCut& cut, const uint32_t* rowcost, int n, hipStream_t st);  // (reads ro.edge_off only)

// Event list of stage B (sc_tri.hip 2b): one record per non-zero member word of a strong edge, SoA, split into
// EV_SHARDS regions of shard_cap records; fill[shard] = records appended to that region.
struct EventList {
  uint64_t* m;       // member word (bits = common neighbours k of the edge inside this 64-column word)
  uint32_t* wi;      // word offset of row i: i * W + w   (into bits / wpre)
  uint32_t* wj;      // word offset of row j
  uint32_t* a;       // weight ranking: ebase[i];  degree ranking: deg[i] + deg[j]
  uint32_t* b;       // weight ranking: ebase[j]
  uint32_t* e;       // edge index
  uint32_t* rb;      // rank of the word's first triangle inside its edge
  uint32_t* x;       // position of the edge in the flat ordered strong list (written with an OrdList only)
  uint32_t* fill;    // EV_SHARDS counters
  uint64_t shard_cap;
  uint32_t* overflow;  // host-pinned flag, set when a region is full
  int W;
};
// Ordinals from the ORDERED strong list (sc_tri.hip 2c): no scan of the per-edge counts between the counting pass and the key kernel.
// The counting pass takes the flat list in chunks of 256 / (lanes per edge) consecutive positions per workgroup and trip; it leaves
// tloc[x] = triangles of the earlier edges of x's chunk and ctot[c] = triangles of chunk c, and every workgroup of the key kernel
// makes the prefix over the chunk totals by itself.  cnt == nullptr: off (tcnt -> scan -> toff).
constexpr uint32_t ORD_BLOCK_EDGES = 1024;  // edges a block of the pruning kernel takes in this form: its slot of the list
constexpr uint32_t ORD_MAX_BLOCKS = 1024;   // ... and the blocks whose counts a workgroup's prologue sums, four per thread (one 16-byte load)
constexpr uint32_t ORD_CHUNK_MAX = 8192;   // chunk totals a workgroup of the key kernel holds (LDS, u32: ordinals below 2^32 are a precondition of the path)
struct OrdList {
  uint32_t* cnt = nullptr;      // StrongList::cnt (ORD_MAX_BLOCKS entries; only those of the blocks that hold a live edge are read)
  uint32_t* tloc = nullptr;     // one entry per position of the flat strong list
  uint32_t* ctot = nullptr;     // one entry per chunk
  uint32_t* n_strong = nullptr; // ControlBlock::n_strong: strong edges, written by the counting pass
  uint64_t* total = nullptr;    // where the scan would leave the triangle count (toff[E]): written by workgroup 0 of the key kernel
  uint64_t E = 0;               // edges the launches cover ...
  const uint64_t* E_dev = nullptr;  // ... and (host-free calls) the edges there are
  uint32_t chunk_max = ORD_CHUNK_MAX;
};
struct GramRefJob;
size_t event_bytes(uint64_t capacity);
EventList event_list(void* buf, uint64_t capacity, int W, uint32_t* fill, uint32_t* overflow_host);
// counting pass that also emits the events (replaces launch_tri_count when an event buffer is available).  The grid goes by el.E_hint.
// ord (cnt != nullptr): the strong list is ordered (pr.sl.cnt) — also leave what the key kernel makes the ordinals from.
// ref (optional): one extra workgroup votes for stage C2's reference frame (sc_gramref.hpp)
void launch_tri_count_events(const Graph& g, const Pruned& pr, const EdgeList& el, const EdgeCounts& ec, int rank_mode, const EventList& ev,
                             const OrdList& ord, const GramRefJob* ref, const Tuning& tn, hipStream_t st);
// lanes per edge launch_tri_count_events uses (a chunk of an OrdList is 256 / this many positions)
int tri_count_events_lanes(const Graph& g, const Tuning& tn);
// tcnt[e] = 0 for the edges below *smin: what the pruning kernel leaves out in the ordered form, for the scan of an overflow's fall-back
void launch_zero_weak_counts(const EdgeList& el, const Pruned& pr, const EdgeCounts& ec, hipStream_t st);

// Radix-select state.  Lives in the context's control block, which the staging kernel zeroes per call.
// r05: no workgroup of a select round stays behind to "pick": a round only adds its keys into hist[r], and the NEXT launch —
// round r + 1, or the compaction's counting kernel after the last round — resolves that histogram in every workgroup's prologue
// (select_resolve: 16 loads per thread + one block scan, ~1 us, overlapped with its first key loads); its workgroup 0 stores the
// resolved state for the launches after it.  The release + ticket + last workgroup's pass this replaces were ~4 us of a round's 8.
struct SelSnap {           // the select after some rounds: keys in [lo, lo + 2^wbits) still undecided, `above` keys above it
  uint32_t lo, wbits;      // valid once started != 0 (before: the window is the key range [kmin, kmax])
  uint32_t started, done;  // done: the window is one key value, lo = k*
  uint64_t want;           // number of keys to keep (clamped to what the window holds)
  uint64_t above;          // keys strictly above the window
  uint64_t need_eq;        // done: how many keys == k* to keep (lowest ordinals first)
  uint64_t pad;
};
struct SelectState {
  uint32_t kmin, kmax;     // key range
  uint32_t kstar, done;    // the result (compact_count_kernel's workgroup 0 writes it; every later kernel reads these)
  uint64_t want;           //   keys kept
  uint64_t need_eq;        //   how many keys == kstar among them
  uint64_t want_req;       // != 0: the window's floor is a bound that must have this many keys at or above it (whoever resolves a
                           // round reports a shortfall: an ESTIMATED pruning bound that was too high, sc_tri_prune.hip 3c)
  uint64_t pad;
  SelSnap st[4];           // st[r]: the state BEFORE round r (st[0]: key_range_kernel / the key kernel's preset / merge_prepare_kernel)
  uint32_t hist[3][4096];  // hist[r]: round r's bins; all zero between selects (compact_write_kernel clears them behind the select)
};
static_assert(offsetof(SelectState, hist) % 16 == 0, "SelectState::hist must be 16-byte aligned");

constexpr int PR_HCOPIES = 4;  // global copies of the pruning-sample histogram (block b adds into copy b % 4): with one
                               // copy a thousand blocks' adds into the same 256 words serialise (C2 sample 34 -> 27 us);
                               // with 16 the readers' 16 loads per bin cost prune_bits what the sample gained
// Per-call control block (device memory, zeroed by the staging kernel at the start of every call).
struct ControlBlock {
  uint32_t ev_fill[1024];    // event-list region fill counters (EV_SHARDS)
  uint32_t prune_hist[PR_HCOPIES * 256];  // sampled key histogram of the certified pruning, PR_HCOPIES partial copies
  uint32_t es_hist[PR_HCOPIES * 256];     // edge-weight histogram (which edges the sample takes), same layout
  uint32_t st_fill[256];     // strong-edge list region fill counters (ST_SHARDS)
  float smin;                // strong-edge threshold (written by prune_bits_kernel)
  uint32_t amx_ticket;       // blocks-finished counter of score_argmax_kernel
  uint32_t klb;              // key of the certified lower bound of the pruning (0: none)
  uint32_t pad_fin[2];
  uint32_t own_row[2];       // sharded stage B: this rank's row range [lo, hi) ...
  uint32_t n_strong;         // ordered strong list (OrdList): strong edges, written by the counting pass
  uint32_t pad0[8];
  uint64_t key2[2];          // internal winner key pair (sc_register_device)
  unsigned long long fin_word;  // finalize_kernel: workgroups finished << 32 | rank count so far — ONE returning atomic per workgroup (left zero)
  uint64_t own_edge[2];      // ... and its CSR edge range (launch_shard_split)
  uint64_t live_edges[2];    // host-free calls: [0, edges of the graph) — written by launch_edge_build; the scan of the per-edge counts skips the tiles beyond it
  uint64_t pad1[1];
  SelectState sel;
  // stage C2's reference frame (sc_gramref.hpp): slot v = the best (key bits << 32 | workgroup) among the workgroups = v (mod 64) of the
  // estimating sample — its voter v is that workgroup's candidate triangle
  alignas(8) unsigned long long ref_slot[64];
};
static_assert(offsetof(ControlBlock, sel) % 16 == 0, "ControlBlock::sel must be 16-byte aligned");

// key of every triangle, in ordinal (lexicographic i,j,k) order: wkey[toff[e] + r]; kcol[ordinal] = {the triangle's third vertex, its
// edge id}.  cap: entries wkey / kcol hold.  blk_minmax: 2 * 8192 u32 scratch (per-block key min / max, reduced into sel->kmin /
// sel->kmax; sel->want = want).  sel: the select state of the control block.
struct KeyArrays { uint32_t* wkey; uint2* kcol; uint64_t cap; uint32_t* blk_minmax; SelectState* sel; };
// the selection: sel_ord[g] = ordinal of the g-th selected triangle, (i,j,k) ascending, sel_key[g] its key; n: entries both hold
struct Selection { uint64_t* sel_ord; uint32_t* sel_key; uint64_t n; };
void launch_tri_keys(const Graph& g, const Pruned& pr, const EdgeList& el, const EdgeCounts& ec, int rank_mode, const KeyArrays& ka,
                     uint64_t want, const Tuning& tn, hipStream_t st);
// keys from the event list (replaces launch_tri_keys when no region overflowed): ka.cap keys at most (writes beyond are dropped);
// want is clipped to toff[E].  ord (cnt != nullptr): ordinals from the ordered strong list (toff unused)
struct KeyPassOpts {
  // (weight ranking, every edge weight >= 2/3) the kernel presets the select window to [*pr.klb or 2.0, 3.0] and no key-range pass
  // runs; two select rounds then always suffice
  bool window = false;  // (needs pr.klb: with Pruned{} there is no bound to read and the key range is measured as without it)
  bool check_bound = false;  // with a pruning bound in *pr.klb the select must find `want` keys at or above it (SelectState::want_req)
  int chunk_shift = 0;       // (with ord) chunk = 1 << chunk_shift positions
  uint64_t* host_total = nullptr;  // (with ord) pinned word that receives the triangle count, as the scan's would
};
void launch_tri_keys_events(const Graph& g, const Pruned& pr, const EdgeList& el, const EdgeCounts& ec, int rank_mode, const EventList& ev,
                            const OrdList& ord, const KeyArrays& ka, uint64_t want, const KeyPassOpts& o, const Tuning& tn, hipStream_t st);
// A key array as the select / compaction kernels see it.  Plain (seg_len == 0): M keys at base.  Segmented (the
// all-gathered candidate blobs of sharded stage B): M = segments x seg_len logical entries, seg_len a multiple of 1024;
// segment s holds valid[s * valid_stride] real keys at base + s * seg_stride, the rest of it reads as 0.
struct KeyView {
  const uint32_t* base;
  uint64_t M;
  uint64_t seg_len;
  uint64_t seg_stride;    // u32 words between segment starts
  const uint64_t* valid;  // real keys of segment s: valid[s * valid_stride]
  uint64_t valid_stride;  // u64 words
  // plain view only, optional (device): the true key count when the host launched before it knew it — the kernels then
  // look at min(M, *M_dev) keys; M is what the grids cover (host-free path, sc_capi.hip)
  const uint64_t* M_dev;
};
KeyView plain_view(const uint32_t* wkey, uint64_t M);
// `rounds` launches (one histogram of <= 12 key bits each; round r + 1 — and launch_compact_count after the last — resolves round r:
// see SelectState) find the exact threshold key
// host_short (optional, pinned u64): set to 1 when SelectState::want_req keys were promised above the window's floor and
// fewer are there
void launch_select_rounds(const KeyView& view, SelectState* s, int rounds, uint64_t* host_short, const Tuning& tn, hipStream_t st);
// compaction of the selected keys in ordinal order
size_t compact_blocks(uint64_t M);
// rounds: what launch_select_rounds was given (the counting kernel resolves the last round's histogram; host_short as there)
void launch_compact_count(const KeyView& view, SelectState* s, int rounds, uint32_t* blk_gt, uint32_t* blk_eq, uint64_t* host_short,
                          hipStream_t st);
void launch_compact_write(const KeyView& view, SelectState* s, const uint32_t* blk_gt, const uint32_t* blk_eq, const uint64_t* off_gt,
                          const uint64_t* off_eq, const Selection& out, hipStream_t st);

// ---- sharded stage B: the candidate blob a rank sends, and the merge of the gathered blobs ----
constexpr int CAND_HDR_WORDS = 32;  // u64 words: [0] triangles enumerated, [1] entries sent, [2] local threshold key,
                                    // [3] / [4] a key range containing every key sent, [5] 1 = the rank had more
                                    // candidates than the blob holds (its list is cut at its local threshold key)
struct CandBlob {
  uint64_t* hdr;
  uint32_t* keys;  // cap entries, (i,j,k) ascending
  uint4* recs;     // cap entries {i, j, k, key}
  size_t cap;
};
// Entries per blob.  A rank can contribute up to T triangles to the global top-T, but with equally heavy row ranges it
// contributes about T / world: the blob holds twice that (at least 4096), times 2^level — `level` (sc_params.
// shard_cand_level) is raised by the caller after SC_ERETRY, i.e. when the merge found that a cut list could have
// mattered (launch_merge_check); negative levels shrink the blob (tests).  Never more than T rounded up to 1024.
size_t cand_cap(uint32_t T, uint32_t world, int level);
size_t cand_blob_bytes(size_t cap);  // bytes per rank
CandBlob cand_blob(void* blob, size_t cap);
// this rank's selection (n_max an upper bound of its length) -> blob
void launch_cand_emit(const Selection& sl, const KeyArrays& ka, const EdgeList& el, const EdgeCounts& ec, uint32_t n_max,
                      uint64_t want_requested, const CandBlob& b, hipStream_t st);
// sums the gathered headers, arms `sel` for the merge select; host_out[0] <- T_eff (polled), host_out[1] <- triangles
// host_short (pinned, optional): set when *klb is an ESTIMATED bound and fewer than T candidates came
void launch_merge_prepare(const void* blobs, size_t blob_bytes, uint32_t world, uint32_t T, bool fast, const uint32_t* klb,
                          SelectState* sel, uint64_t* host_out, uint64_t* host_short, hipStream_t st);
KeyView cand_view(const void* blobs, size_t blob_bytes, uint32_t world, size_t cap);
// After the merge select: a rank whose list was cut sent everything above its local threshold key k_r; the merged
// selection is exact iff the merged threshold k* lies strictly above k_r for every such rank (everything it did not send
// is then below k*).  Otherwise *host_flag = 1 (pinned; 0 is written otherwise): the call must be repeated with bigger blobs.
void launch_merge_check(const void* blobs, size_t blob_bytes, uint32_t world, const SelectState* sel, uint64_t* host_flag,
                        hipStream_t st);
// ranked order: sortkey ascending = (key desc, ordinal asc).  A hand-written stable LSD radix sort of the HIGH 32 bits (sc_sort.hip):
// the low halves must already ascend (they are the input positions).  temp: sort_temp_bytes(n); less, and nothing is launched.
size_t sort_temp_bytes(size_t n);
void launch_sort_u64(const uint64_t* in, uint64_t* out, size_t n, void* temp, size_t temp_bytes, hipStream_t st);
// selected position -> (i,j,k); the list stays in ordinal ((i,j,k) ascending) order
void launch_tri_decode(const EdgeList& el, const KeyArrays& ka, const Selection& sl, uint32_t T, uint32_t* tri, hipStream_t st);
// ranked order (key desc, ordinal asc) of the ordinal-ordered list: only the stage hook needs it
void launch_rank_order(const uint32_t* tri, const Selection& sl, uint32_t T, uint64_t* sortkey, uint64_t* sorted,
                       void* sort_tmp, size_t sort_bytes, uint32_t* tri_ranked, uint32_t* key_ranked, hipStream_t st);

// ---- stage C ---------------------------------------------------------------------------------------
struct Shard {
  uint32_t T_eff;   // ranked triangles in total
  uint32_t block;   // dealing granularity
  uint32_t rank, world;
  uint32_t n_local; // hypotheses of this rank
  uint32_t ld_local;// roundup(n_local, 256): plane stride of RtSoA / partial counts
};
uint32_t shard_local_count(uint32_t T_eff, uint32_t block, uint32_t rank, uint32_t world);
// Where stage C finds triangle g of the selected list: the selection itself (position -> ordinal -> {third vertex,
// edge} -> edge ends) — the hot path never materialises the T x 3 list (only the stage hook does, launch_tri_decode).
struct TriSource {
  const uint64_t* sel_ord;
  const uint2* kcol;
  const uint32_t* ei;
  const uint32_t* ej;
  // sharded stage B: sel_ord[g] is a logical position in the gathered candidate blobs; its record {i, j, k, key}
  // is cand_recs[(pos / cand_seg) * cand_stride + pos % cand_seg]   (cand_recs == nullptr: the local form above)
  const uint4* cand_recs;
  uint64_t cand_seg, cand_stride;  // entries per blob; uint4 units between blob record arrays
  // host-free calls only (0: unchecked): what a looked-up {vertex, edge} must stay below — a call that turns out to have
  // been launched on wrong assumptions (and is repeated) may find anything in the selection, and must not follow it
  uint32_t lim_vertex, lim_edge;
  uint64_t lim_ord;
};
// The context's stage-C arrays as the launches see them — Hyps, FilterBufs, Partial, ArgmaxOut, and the Stamps of a timed launch:
// plain host-side views, as stage B's are, each filled by one accessor of the host driver (sc_capi.hip: hyps_of, filter_of; run_score
// fills the Partial).  A view is taken after the last ENSURE of every buffer it names and is not kept across one.
//
// This rank's hypotheses.  soa: RtSoA[c * ld_local + l], c = 0..11, for the local hypotheses of the shard (global rank index derived).
// aos (null where no exact pass reads it): also 12 consecutive floats per local hypothesis (ld_local x 12), for the lane =
// correspondence kernel.
// t_eff_dev (null on waited, certified calls; device u64): the true length of the selection when the host launched with sh.T_eff =
// the requested T before it knew (host-free path): positions at or beyond it are treated as padding and never looked up
struct Hyps { Shard sh; float* soa; float* aos; const uint64_t* t_eff_dev; };
// What C2 leaves for the arg-max: rows x ld_local u32 counts
struct Partial { uint32_t* counts; uint32_t rows; };
// first / last (both or neither): start and stop timestamps taken from the dispatch packets of the stage's first and last kernel
// (hipExtLaunchKernelGGL) — no extra packet on the stream, unlike a bracket of hipEventRecord calls (~4.5 us each on this part).
// mid (optional): stop timestamp of the FILTER kernel's own dispatch (first .. mid = that kernel alone).  Stamps{}: plain launches.
struct Stamps { hipEvent_t first, last, mid; };
// C1 writes h.soa and, where given, h.aos.
// tile_job (optional): the filter's tile kernel rides in the same launch as extra workgroups (C1 alone leaves most of the
// chip idle: T / 256 workgroups), which saves a launch on the critical path.
struct FilterTileJob;
void launch_kabsch(const Points& pts, const TriSource& ts, const Hyps& h, const FilterTileJob* tile_job, hipStream_t st);
// C1 on an explicit triangle list to AoS T x 12 (stage hook)
void launch_kabsch_aos(const Points& pts, const uint32_t* tri, uint32_t T, float* Rt, hipStream_t st);
// AoS T x 12 -> SoA planes (stage hook for sc_score_host)
void launch_rt_to_soa(const float* Rt, uint32_t T, uint32_t ld_local, float* RtSoA, hipStream_t st);
// C2: inlier counts.  out.counts: n_chunks * ld_local u32 scratch.
// The plain C2 kernel: lane = hypothesis with the points in LDS (every score mode, the matrix-pipe share).
// score_chunks: point chunks that launch will use (out.rows).
uint32_t score_chunks(int n, uint32_t ld_local);
// score_mode: 0 inlier count, 1 truncated squared residual, 2 truncated absolute residual (include/saccot.h)
void launch_score(const Points& pts, const Hyps& h, const Partial& out, const Stamps& ev, const Derived& dv, int score_mode,
                  const Tuning& tn, hipStream_t st);
// C2, inlier count, by filter + exact fix-up (sc_filter.hip): which calls use it, what it needs, and its two launches.
// The tile (fp16 image of the correspondences) depends on the points only: launch_filter_tile runs once per call, any
// time after launch_stage_points (whose atomicMax fills mx_cur); mx_cur / mx_next are two u32 pairs that alternate
// from call to call (the tile kernel clears the next call's).  partial: fp.splits rows of ld_local counts.
// Two filters share the machinery (tile of the correspondences, queue of undecided tests, recount bitmap, exact pass):
//   mode 1, "linear":  the MFMA gives the three residual components of 8 hypotheses x 32 correspondences, the vector
//                      pipe squares and tests them (4.75 vector instructions per test);
//   mode 2, "Gram":    the MFMA gives the SQUARED residual itself — |R p + t - q|^2 expanded into a 48-term dot product
//                      of per-correspondence features and per-hypothesis coefficients, 32 hypotheses x 32 correspondences
//                      per three chained MFMAs — and the vector pipe only tests its sign (1.6 instructions per test).
//                      Squaring by inner products cancels: usable while tau is not too small against the clouds' extent.
struct FilterPlan {
  uint32_t mode;  // 1 linear, 2 Gram
  uint32_t windows, splits, n_waves, rows, queue_cap;
  size_t tile_bytes, state_bytes, coef_bytes;  // coef_bytes: the Gram filter's per-hypothesis coefficients and its two permutations (0 for the linear one)
};
// The filter's plan and buffers: tile (plan.tile_bytes), state (plan.state_bytes), coef (plan.coef_bytes; Gram), frame (gram_frame_bytes();
// Gram) and mx, the FX_MX_WORDS coordinate statistics the staging kernel wrote.
struct FilterBufs { FilterPlan plan; void* tile; void* state; void* coef; void* frame; const uint32_t* mx; };
// Gram filter: what its waves load instead of computing it (made once per call: launch_kabsch's threads, or launch_gram_coef).
// Rows are PERMUTED: hypotheses near the call's reference frame first (sc_filter.hip, "the cut"); so are the tile's rows.
struct GramFrame;
struct GramCoef {
  void* A;            // 64 bytes per row: fp16 halves of its 16 coefficients
  float* C;           // accumulator start value per row
  float* W;           // shell width per row (0: not filtered)
  uint32_t* flag;     // bit 0 filtered, bit 1 recount, bits 8.. log2 of the largest alpha
  uint32_t* hperm;    // coefficient row -> hypothesis of this rank's shard
  uint32_t* pperm;    // tile row -> correspondence
  GramFrame* frame;   // the call's frame and the four class counters (in the filter's state buffer)
};
GramCoef gram_coef_view(void* buf, uint32_t ld_local, void* frame);
// which kernel stage C2 runs: 0 = plain fp32 kernel, 1 = linear filter, 2 = Gram filter.  By score mode, size, the knobs of
// sc_debug and — unless forced — by whether tau is on a scale the filter can bound (host_max / host_box: the coordinate
// maxima and bounding boxes the staging kernel published; ~0 = not known: assume the linear filter applies, never Gram).
int score_filter_mode(int score_mode, const Tuning& tn, int n, uint32_t ld_local, uint64_t host_max, const uint64_t* host_box,
                      float tau2);
FilterPlan filter_plan(int n, uint32_t ld_local, const Tuning& tn, uint32_t mode);
struct FilterTileJob {  // what the tile kernel needs (filter_tile_job fills it)
  uint32_t rows; const uint32_t* mx_cur; uint32_t* mx_next; void* tile; void* info; uint32_t* zero; uint32_t zero_words; uint32_t mode;
  GramCoef coef; float tau2;  // mode 2: the Kabsch threads of the same launch also write their hypotheses' coefficients
};
FilterTileJob filter_tile_job(const FilterBufs& fb, uint32_t ld_local, float tau2);  // (mx_cur = fb.mx; mx_next stays null)
// Gram filter: the call's reference frame (sc_gramref.hpp; `frame`: gram_frame_bytes() of device memory, per context).  One
// workgroup votes for it among 64 hypotheses and clears the class counters — BEFORE the tile and the coefficients are made.  In a
// launch of its own (launch_gram_ref: ts == nullptr: the hypotheses exist already — stage hook — and are read from h.soa; else
// they are solved from the selection `*ts`), or, on the hot path, as an extra workgroup of the counting pass
// (launch_tri_count_events, `ref`) fed by the candidate triangles the estimating sample leaves behind (launch_sample_estimate, `cand`).
size_t gram_frame_bytes();
struct GramRefJob;
GramRefJob gram_ref_job(const Points& pts, const FilterBufs& fb, float tau2, const Tuning& tn);  // (fb.mx and fb.frame only; source left empty)
void launch_gram_ref(const Points& pts, const TriSource* ts, const Hyps& h, const FilterBufs& fb, float tau2, const Tuning& tn, hipStream_t st);
// the coefficients on their own (stage hook sc_score_host, which has no Kabsch launch)
void launch_gram_coef(const Hyps& h, float tau2, const GramCoef& coef, hipStream_t st);
void launch_filter_tile(const Points& pts, const FilterTileJob& job, hipStream_t st);  // on its own (stage hook sc_score_host)
// h.aos: 12 consecutive floats per hypothesis (what the exact pass loads; launch_kabsch / the stage hook write them); out: fb.plan.splits rows
void launch_score_filter(const Points& pts, const Hyps& h, const FilterBufs& fb, const Partial& out, const Stamps& ev, const Derived& dv,
                         const Tuning& tn, hipStream_t st);
// Run-time probe of the matrix pipe's accumulation arithmetic (the model the Gram filter's bound assumes; sc_gram_guard.hip):
// blocking, ~1e6 cancelling dot products.  scratch: 16 bytes of device memory.  worst_units: largest |hardware - exact| /
// largest term seen, in units of 2^-24 (the bound assumes 18.5; gram_guard_limit() is what a context tolerates).
hipError_t gram_guard_probe(void* scratch, hipStream_t st, float* worst_units, bool* subnormals_kept, uint32_t* compared);
float gram_guard_limit();
bool filter_ablations_built();  // -DSC_ABLATIONS: the scheduling / timing-only variants of the filter kernels exist (Tuning::filter_variant)
// diagnostics (sc_debug_last): what the filter of the last launch handed to the exact pass.  Blocking copies on `st`.
hipError_t filter_read_counters(const void* state, const FilterPlan& fp, hipStream_t st, uint64_t* undecided, uint64_t* recounts);
// Gram filter: {near correspondences, near hypotheses, hypotheses in the grid, the reference's position in the shard (~0: none), its vote x 256}
hipError_t filter_read_frame(const void* frame, hipStream_t st, uint32_t out[5]);
// Winner key pair key2[0..1] (written, not accumulated: no zeroing needed):
//   key2[0] = max over hypotheses with count > 0 of  (count << 32) | second,   second = sel_key[g] (the triangle's
//             ranking key) or, when sel_key == nullptr, 0xFFFFFFFF - g;
//   key2[1] = max of (0xFFFFFFFF - g) over the hypotheses attaining key2[0]  (only when sel_key != nullptr).
// With g the position in the ordinal-ordered list this picks: most inliers, then best ranking key, then lowest
// (i,j,k) — exactly "ties -> best-ranked triangle" of SURVEY §8a, without ever sorting the list.
// cnt (n_local u32): the per-hypothesis counts (the stage hook returns them).  pairs: argmax_scratch_bytes() of
// per-block (key, position) pairs; ticket: a zeroed u32 in the control block (left zero).
size_t argmax_scratch_bytes(uint32_t ld_local);
uint32_t argmax_blocks(uint32_t ld_local);  // workgroups of launch_argmax = pairs it leaves when key2 == nullptr
struct ArgmaxOut { const uint32_t* sel_key; uint32_t* cnt; uint64_t* pairs; uint32_t* ticket; uint64_t* key2; };
void launch_argmax(const Shard& sh, const Partial& in, const ArgmaxOut& out, hipStream_t st);
// C3 (sc_final.hip): winner decode + re-solve + mask.  Rt12 receives R (row-major) and t; identity / zero mask when key2[0] == 0.
// sel_key / T: the ordinal-ordered ranking keys (for the winner's rank index); host_out (pinned, 2 x u64) receives
// [1] = rank index << 32 | position (all ones: the key pair decodes to nothing of the selection) and then, released, [0] = key2[0].
// key2: npairs key pairs (all-gathered, one per rank; 1 = already reduced); key_out (2 x u64, optional) receives the
// reduced pair.
// sh / RtSoA: this rank's shard and the (R,t) planes phase 1 produced — a locally scored winner is looked up there.
// dp (optional; host-free calls): what the call's earlier kernels would have published to the host one by one — stage B's two counts
// (device words; they go to dp->host[HW_EDGES] as ONE word: edges | triangles << 32, ~0 if either needs more than 32 bits) and, with_stats,
// the staging kernel's coordinate statistics (FX_MX_WORDS words -> HW_COORD_MAX, HW_BOX .. + 5) — written by THIS kernel, before
// the winner.  Those kernels then publish nothing: a system-scope store costs the kernel that makes it ~0.5 us.
// The host words: one host-pinned area of HW_COUNT x u64 per context (sc_ctx::pinned), through which the kernels hand single results to
// the host.  The host ARMS a word it will poll (all ones: "pending"), or CLEARS a flag a kernel only ever sets; the kernel named
// writes it with a system-scope store; the host reads it after polling it, or after the winner word — the last store of a call.
enum HostWord : int {
  HW_EDGES = 0,         // edge count.  Armed by run_row_stats / run_edges, written by the scan (or fused row / edge kernel), polled by run_edges.
                        // Host-free call: edges | triangles << 32 in ONE word, written by the finalize kernel (DeferredPub), read by finalize_wait
  HW_BAD_INPUT = 1,     // non-finite input coordinate.  Cleared by stage_inputs, set (low half) by the staging kernel, read by run_edges / finalize_wait / the hooks
  HW_TRIANGLES = 2,     // triangle count (of the pruned graph when pruning).  Armed and polled by run_select, written by the scan of the counts
  HW_TOTAL = 4,         // 3-cliques of the unpruned graph (SC_FLAG_EXACT_TOTAL).  Written by its scan in run_edges, read by run_select behind HW_TRIANGLES
  HW_EV_OVERFLOW = 5,   // an event-list region was full.  Cleared by run_select, set (low half) by the counting pass, read by run_select / finalize_wait; high half: the ordered strong list had too many chunks (chunk_overflow)
  HW_MERGED_T = 6,      // sharded select: merged T_eff.  Armed and polled by sc_shard_score_device, written by merge_prepare ...
  HW_MERGED_M = 7,      // ... together with the number of candidates merged (written before HW_MERGED_T)
  HW_WINNER = 8,        // the winner's key: the last word a call writes.  Armed by finalize_enqueue, written by the finalize kernel, polled by finalize_wait
  HW_WINNER_POS = 9,    // rank << 32 | position of the winner (all ones: the pair decodes to nothing).  Written before HW_WINNER, read behind it
  HW_PEEL_ALIVE = 10,   // sc_peel, truncated score modes: correspondences a round's compaction kept.  Armed and polled by the round, written by the compaction kernel
  HW_MATCH = 11,        // sc_match / sc_register_features: matches kept | non-finite flag << 32.  Armed and polled by the host entries, written by the finish kernel
  HW_CAND_CUT = 12,    // a cut candidate list mattered (SC_ERETRY).  Cleared by sc_shard_score_device, set by merge_check, read by finalize_wait
  HW_COORD_MAX = 13,    // max|tgt| << 32 | max|src|.  Armed by stage_inputs, written by the staging kernel (host-free: by the finalize kernel, every 64th
                        // call), read with acquire by read_coord_stats; sc_score_host polls it
  HW_SELECT_SHORT = 14, // the select found fewer keys above the pruning bound than promised.  Cleared by run_edges, set by select / compaction, read by finalize_wait
  HW_MERGE_SHORT = 15,  // the merged candidates hold fewer than T keys above an estimated bound.  Cleared by sc_shard_score_device, set by merge_prepare, read by finalize_wait
  HW_BOX = 16,          // .. 21: the two bounding boxes, (key of -min) << 32 | key of max per axis.  Written BEFORE HW_COORD_MAX by the same kernel, read behind it
  HW_COUNT = 22
};
struct DeferredPub {
  const uint64_t* dev_edges;
  const uint64_t* dev_triangles;
  const uint32_t* coord_max;
  unsigned long long* host;
  int with_stats;
};
// Frame end: what a winner launch (launch_finalize, launch_peel_winner) decodes — keys: the npairs key pairs (`key2` above) — and
// what it leaves.  h: this rank's shard and hypotheses (h.sh / h.soa: `sh / RtSoA` above; h.soa null: nothing scored locally).
struct WinnerIn { const uint32_t* sel_key; uint32_t T; const uint64_t* keys; int npairs; };
struct WinnerOut { float* Rt12; uint8_t* mask; uint64_t* host_out; };
void launch_finalize(const Points& pts, const TriSource& ts, const Hyps& h, const WinnerIn& in, const WinnerOut& out, float tau2,
                     uint64_t* key_out, unsigned long long* fin_word, const DeferredPub* dp, hipStream_t st);
// SURVEY §8f-2 (SC_FLAG_REFINE): fp64 least-squares refit of Rt12 over the inlier mask; no-op when key2[0] == 0 or
// fewer than 3 inliers.  scratch: refine_scratch_bytes(n).
size_t refine_scratch_bytes(int n);
void launch_refine(const Points& pts, const uint8_t* mask, const uint64_t* key2, double* scratch, float* Rt12,
                   hipStream_t st);
// mask of an explicit hypothesis (stage hook)
void launch_mask(const Points& pts, const float* Rt12, float tau2, uint8_t* mask, hipStream_t st);

// ---- rounds on a scored frame (sc_peel; sc_peel.hip) ---------------------------------------------------
// The device words of a context's rounds (zeroed once; every kernel leaves the counters zero)
struct PeelWords {
  unsigned long long fin_word;  // peel_winner_kernel: workgroups finished << 32 | rank count so far (as ControlBlock::fin_word)
  unsigned long long key2[2];   // the round's reduced winner pair (launch_refine reads [0])
  uint32_t n_alive;             // peel_compact_kernel: correspondences it kept
  uint32_t pad;
};
// claim + compact, ONE launch: claimed[m] |= (|R p_m + t - q_m|^2 < tau2) for the hypothesis at position prev_pos of h.soa (the
// winner of the round before; prev_pos == ~0u: nothing to fold in), then the correspondences still unclaimed go, order preserved,
// into the six planes of `alive` (stride pts.ld).  fresh: `claimed` holds nothing yet (round 1): read as zeros, written whole.
// lb: a look-back launch of peel_compact_tiles(n) tiles (8 bytes of descriptor each).  host_alive (optional, pinned): receives the
// number kept (the host needs it to size the scoring launch where the scores do not tell it: the truncated score modes).
uint32_t peel_compact_tiles(int n);
struct PeelSets { uint8_t* claimed; float* alive; uint64_t* host_alive; };
void launch_peel_compact(const Points& pts, const Hyps& h, const PeelSets& ps, uint32_t prev_pos, float tau2, bool fresh,
                         PeelWords* words, LbArgs lb, hipStream_t st);
// winner + mask of a round: finalize_kernel's work on ONE shard (the hypothesis at position g is h.soa[.. + g]) with
// mask[m] = !claimed[m] && inlier.  in.keys / in.npairs: what launch_argmax left (key2 == nullptr form); npairs == 0: no hypothesis
// (identity, zero mask).  out.host_out as launch_finalize's.
void launch_peel_winner(const Points& pts, const Hyps& h, const WinnerIn& in, const WinnerOut& out, const uint8_t* claimed, float tau2,
                        PeelWords* words, hipStream_t st);
// label[m] = value where mask[m] (sc_register_instances: one launch per accepted motion)
void launch_peel_label(const uint8_t* mask, int n, int32_t value, int32_t* label, hipStream_t st);

// ---- refits iterated to a fixed point on a scored frame (sc_polish; sc_polish.hip) ---------------------------------
// One candidate: sc_polish_cand of include/saccot.h, field for field (sc_capi_polish.hip asserts the size).
struct PolishCand {
  float Rt[12];              // select: the frame's fp32 (R, t); polish: the last iterate
  uint32_t rank;             // position in the ranked list
  uint32_t score0, score;    // frame score; score of the last iterate over all n (the frame's score_mode)
  uint16_t iters, reserved;  // refits that changed (R, t)
};
static_assert(sizeof(PolishCand) == 64, "sc_polish_cand is 64 bytes");
constexpr uint32_t POLISH_MAX_CAND = 64;
// The candidate set as the three launches see it (sc_capi_polish.hip fills it): cand holds POLISH_MAX_CAND records, *n_cand = K of them
// filled, want = the candidates asked for.
struct PolishSet { PolishCand* cand; uint32_t* n_cand; uint32_t want; };
// The first K = min(want, hypotheses with cnt > 0) of the T hypotheses under (cnt desc, sel_key desc, position asc) — the frame's
// total order — into cand[0 .. K) in that order, with their rank in the ranked list; cand[K .. want) zeroed; *n_cand = K.  One workgroup.
void launch_polish_select(const PolishSet& ps, const uint32_t* cnt, const uint32_t* sel_key, uint32_t T, const float* RtSoA, uint32_t ld_local,
                          hipStream_t st);
// One workgroup per candidate, every iteration inside the launch: mask of (R, t) -> refit in refine_kernel's canonical order -> again,
// until the refit is declined, returns the same bits, or max_iter refits are done; then the score of the last iterate.
// scratch: want * chunk_scratch_bytes(n) (sc_chunks.hpp).  thr: tau^2, 1 / tau^2 or 1 / tau by score_mode.
void launch_polish(const Points& pts, const PolishSet& ps, uint32_t max_iter, float tau2, float thr, int score_mode, double* scratch,
                   hipStream_t st);
// The candidate with the largest score (ties: the earlier one) -> out.Rt12, out.mask; the records and their number -> out_cand / out_n (either
// may be null); out.host_out (pinned, 2 x u64): [1] = rank << 32 | score, then, released, [0] = winner index << 32 | K (0: no candidate).
void launch_polish_winner(const Points& pts, const PolishSet& ps, const WinnerOut& out, PolishCand* out_cand, uint32_t* out_n, float tau2,
                          hipStream_t st);

// ---- descriptor matching (sc_match; sc_match.hip) -------------------------------------------------------
// One call: fsrc ns x dim, ftgt nt x dim (row-major fp32, device); knn 1 .. 4; mutual / r2 (> 0: the ratio test, r2 = ratio^2) with
// knn == 1 only.  A key is (bits of the canonical squared distance) << 32 | index.
struct MatchJob {
  const float* fsrc; const float* ftgt;
  uint32_t ns, nt, dim, knn, mutual;
  float r2;
};
// How the distance launch is cut: row_blocks x slices workgroups, a slice = tiles_per_slice column tiles; every (row, slice) leaves kp
// ascending keys in `part` (key q of slice s of row i at part[(s * kp + q) * ld_part + i]; all ones: none), part_bytes in all.
struct MatchPlan {
  uint32_t kp, row_blocks, slices, tiles_per_slice;
  size_t ld_part, part_bytes;
};
MatchPlan match_plan(uint32_t ns, uint32_t nt, uint32_t knn, float r2);
// sc_register_features: the matched points, gathered by the finish launch into two n x 3 arrays (gsrc == nullptr: no gather).
// Point i of src is src[i * s_elem + c * s_comp] (either layout of sc_params).
struct MatchGather {
  const float* src; const float* tgt;
  uint32_t s_elem, s_comp, t_elem, t_comp;
  float* gsrc; float* gtgt;
};
// sc_match_guided: the keypoints of both sets (point i of src is src[i * s_elem + c * s_comp], as MatchGather's), the pose prior (12
// floats in HBM, read in stream order) and gate2; cell (i, j) is a candidate only where resid2(Rt, src[i], tgt[j]) < gate2.
// sc_match_guided_poses (n_poses > 0; Rt is not read): n_poses records in HBM, pose_stride bytes apart, float Rt[12] at byte 0 and —
// use_status — an int32 status at byte 48; a record whose status is not SC_OK is skipped.  Cell (i, j) is a candidate where SOME
// used record's residual is below gate2; the finish launch labels every entry with the used record of the smallest residual.
struct MatchGuide {
  const float* src; const float* tgt;
  uint32_t s_elem, s_comp, t_elem, t_comp;
  const float* Rt;
  float gate2;
  const void* pose;
  uint32_t pose_stride, n_poses, use_status;
};
// colmin (SC_MATCH_MUTUAL, else nullptr): nt keys (distance << 32 | row), all ones at launch.  clean: one word, non-zero at launch,
// cleared when a non-finite descriptor is read — with a guide (gd != nullptr: sc_match_guided) when any descriptor, any point or the
// pose is not finite, whatever the gate excludes.
void launch_match_dist(const MatchJob& job, const MatchPlan& plan, uint64_t* part, uint64_t* colmin, uint32_t* clean, const MatchGuide* gd,
                       hipStream_t st);
// What a match call writes, and the optional parts it may carry; a caller names what it sets and leaves the rest zero.
struct MatchOut {
  int32_t* corr; float* d2;  // n x 2 int32 and n, in device memory
  uint32_t* count;           // count[0] = n, count[1] = 1 if something not finite was read
  bool to_host;              // match_enqueue: a host form — count and host_word are filled in there (match_words, HW_MATCH armed)
  uint64_t* host_word;       // optional, pinned: receives n | flag << 32
  MatchGather g;             // optional: the gather
  const MatchGuide* gd;      // optional: the gate
  const float* h_Rt;         // with gd, match_enqueue only: the pose as 12 host floats, copied behind the memset (nullptr: gd->Rt / gd->pose in HBM)
  float* g2;                 // optional with gd: g2[m] = the gate residual of entry m
  int32_t* label;            // optional with gd->n_poses > 0: label[m] = the used record with the smallest residual of entry m, g2[m] that minimum
};
// merge + mutual / ratio + compaction in (row, rank) order; with the flag raised n = 0 and nothing else is written.  lb: a look-back
// launch of match_finish_tiles(ns) tiles (8 bytes of descriptor each).
uint32_t match_finish_tiles(uint32_t ns);
void launch_match_finish(const MatchJob& job, const MatchPlan& plan, const uint64_t* part, const uint64_t* colmin, const uint32_t* clean, LbArgs lb,
                         const MatchOut& o, hipStream_t st);

// ---- many small registrations in one launch (sc_register_batch; sc_batch.hip) ------------------------------
// One problem's result: sc_batch_result of include/saccot.h, field for field (sc_batch.hip asserts the size).
struct BatchRecord {
  float Rt[12];
  int32_t status;
  uint32_t n, edges, tri_kept;
  uint64_t tri_total;
  uint32_t best_rank, best_count;
};
constexpr int BATCH_MAX_N = 512;
// Problem b owns rows [offset[b], offset[b + 1]) of src / tgt (n x 3 row-major, or with soa three planes of `total`) and of mask;
// 3 <= rows <= BATCH_MAX_N, checked by the caller.  Everything in device memory.
struct BatchJob {
  const float* src; const float* tgt;
  const uint32_t* offset;
  uint32_t n_problems, total;
  int soa;
  uint32_t T;
  int rank_mode, score_mode;
  Derived dv;
  BatchRecord* res;
  uint8_t* mask;
};
// sc_register_batch_features: the problems sit in SLOTS — job.offset[b] is where problem b starts, count[2b] how many correspondences
// it holds (at most BATCH_MAX_N: the slots' capacities, checked by the caller) and count[2b + 1] != 0 says its match read a
// non-finite descriptor.  The kernel then writes the records of the flagged (SC_EINVAL, n = 0) and the short (n < 3: SC_ENOHYP)
// problems itself.  A type of its own, so that the plain form's kernel argument — and with it its code — stays what it was.
struct BatchSlotJob {
  BatchJob job;
  const uint32_t* count;
};
// One workgroup per problem; every record and mask range is written (complete in stream order).
void launch_batch_register(const BatchJob& job, hipStream_t st);
void launch_batch_register_slots(const BatchSlotJob& job, hipStream_t st);
// sc_register_instances_batch: the same kernel, followed inside the workgroup by up to max_instances - 1 rounds of sc_peel.  job.res
// holds max_instances planes of n_problems records, motion-major; job.mask is not used: label (int32, positioned like the mask) says
// which motion claimed a correspondence, -1 for none; nfound: a word per problem.  Types of their own again, so that the kernels of
// sc_register_batch keep their arguments and their code.
constexpr uint32_t INSTANCES_BATCH_MAX = 16;
struct BatchRounds {
  uint32_t max_instances, min_score;
  int32_t* label;
  uint32_t* nfound;
};
struct InstBatchJob {
  BatchJob job;
  BatchRounds rounds;
};
struct InstBatchSlotJob {
  BatchJob job;
  BatchRounds rounds;
  const uint32_t* count;  // as BatchSlotJob's
};
void launch_instances_batch(const InstBatchJob& job, hipStream_t st);
void launch_instances_batch_slots(const InstBatchSlotJob& job, hipStream_t st);

// ---- iterated fp64 refits for a batch's winners (sc_polish_batch; sc_polish_batch.hip) ----------------------
// One problem's result: sc_polish_batch_result of include/saccot.h, field for field (sc_polish_batch.hip asserts the size).
struct PolishBatchRecord {
  float Rt[12];
  int32_t status;
  uint32_t score0, score;
  uint16_t iters, stop;
};
// Problem b owns rows [offset[b], offset[b + 1]) of src / tgt and of mask, as in BatchJob; in[b].status and in[b].Rt are the
// input pose (read, never written), out[b] the result.  thr: tau^2, 1 / tau^2 or 1 / tau by score_mode.  Everything in device memory.
struct PolishBatchJob {
  const float* src; const float* tgt;
  const uint32_t* offset;
  uint32_t n_problems, total;
  int soa, score_mode;
  uint32_t max_iter;
  float tau2, thr;
  const BatchRecord* in;
  PolishBatchRecord* out;
  uint8_t* mask;
};
// The slot form (behind sc_register_batch_features): job.src / job.tgt are the problems' POINTS (job.offset = src_off, job.total =
// total_s; tgt_off, total_t for the other side), and correspondence m of problem b is (src point corr[2 (slot[b] + m)], tgt point
// corr[2 (slot[b] + m) + 1]), indices local to the problem, m < count[2b]; count[2b + 1] != 0: the match flagged the problem.
// Mask bytes at slot[b] + m.  A type of its own, so that the plain form's kernel argument and code do not depend on it.
struct PolishBatchSlotJob {
  PolishBatchJob job;
  const uint32_t* tgt_off; const uint32_t* slot;
  const int32_t* corr; const uint32_t* count;
  uint32_t knn, total_t;
};
// The pairs form (behind sc_register_pairs_features): job.src == job.tgt are the POINTS of the table of sets (job.total its rows;
// job.offset is not read), and pair p's two sets, its slot and its correspondences are what rec + PAIR_WORDS * p says (PairWord,
// below); corr, count and the mask bytes as in the slot form.  A third type, for the same reason.
struct PolishBatchPairsJob {
  PolishBatchJob job;
  const uint32_t* rec;
  const int32_t* corr; const uint32_t* count;
  uint32_t knn;
};
// One workgroup per problem, every refit inside the launch; every record and mask range is written (complete in stream order).
void launch_polish_batch(const PolishBatchJob& job, hipStream_t st);
void launch_polish_batch_slots(const PolishBatchSlotJob& job, hipStream_t st);
void launch_polish_batch_pairs(const PolishBatchPairsJob& job, hipStream_t st);

// ---- the fp64 information matrix of a batch's poses (sc_pose_info_batch; sc_info_batch.hip) ------------------
// One problem's result: sc_pose_info_result of include/saccot.h, field for field (sc_info_batch.hip asserts the size).
struct PoseInfoRecord {
  double info[36];
  double sse;
  int32_t status;
  uint32_t inliers;
  uint32_t reserved[4];
};
// THE POSE RECORDS of every entry from here to sc_settle_poses, said once.  `pose` is the caller's array of records, pose_stride bytes
// apart: float Rt[12] at byte 0 and — where the entry reads it — an int32 status at byte 48; read, never written, and nothing of a
// record behind that is read (sc_pose_check.hpp has the rule of the stride and the bytes a call reads).  A frame form has n_poses
// records, pose k at byte k * pose_stride, and reads the status only with `status`; out[k] is pose k's result.  A batch form reads the
// status always; sc_pose_info_batch has one record per problem (problem b at byte b * pose_stride, out[b]), the others n_poses planes
// of n_problems records, motion-major: pose k of problem b at byte (k * n_problems + b) * pose_stride, out[k * n_problems + b].
// Problem b of a batch owns rows [offset[b], offset[b + 1]) of src / tgt (and of label), as in BatchJob.  thr: tau^2, 1 / tau^2 or
// 1 / tau by score_mode.  scratch: n_poses * chunk_scratch_bytes(pts.n) (sc_chunks.hpp).  Everything in device memory.
// Both heads hold the entry's OWN word — max_iter of the entries that iterate, the mode of sc_assign_poses — where every job had it,
// between the score and the poses: the kernels' arguments keep their layout, so the kernels compile to the code they were.
struct PoseFrameHead {  // what every frame form's job opens with (sc_capi_pose.hpp fills it from the context's pass, but the own word)
  Points pts;  // the frame's staged planes, in the caller's indexing
  float tau2, thr;
  int score_mode;
  union { uint32_t max_iter, mode; };
  uint32_t n_poses;
  const void* pose;
  uint32_t pose_stride;
  int status;
};
struct PoseBatchHead {  // ... and every motion-major batch form's (from sc_params and the offsets)
  const float* src; const float* tgt;
  const uint32_t* offset;
  uint32_t n_problems, total;
  int soa, score_mode;
  float tau2, thr;
  union { uint32_t max_iter, mode; };
  uint32_t n_poses;
  const void* pose;
  uint32_t pose_stride;
};
// sc_pose_info_batch: one record per problem, no score.  Its kernels take the job inside the slot and pairs types below, so it
// keeps its own fields.
struct PoseInfoJob {
  const float* src; const float* tgt;
  const uint32_t* offset;
  uint32_t n_problems, total;
  int soa;
  float tau2;
  const void* pose;
  uint32_t pose_stride;
  PoseInfoRecord* out;
};
// The slot form and the pairs form: what PolishBatchSlotJob and PolishBatchPairsJob say, field for field.  Types of their own, so
// that the plain form's kernel argument and code do not depend on them.
struct PoseInfoSlotJob {
  PoseInfoJob job;
  const uint32_t* tgt_off; const uint32_t* slot;
  const int32_t* corr; const uint32_t* count;
  uint32_t knn, total_t;
};
struct PoseInfoPairsJob {
  PoseInfoJob job;
  const uint32_t* rec;
  const int32_t* corr; const uint32_t* count;
  uint32_t knn;
};
// One workgroup per problem; every record is written (complete in stream order).
void launch_pose_info_batch(const PoseInfoJob& job, hipStream_t st);
void launch_pose_info_batch_slots(const PoseInfoSlotJob& job, hipStream_t st);
void launch_pose_info_batch_pairs(const PoseInfoPairsJob& job, hipStream_t st);

// ---- the same on a scored frame (sc_pose_info_frame; sc_info_frame.hip) -----------------------------------------
// sel by sel_mode (SC_POSE_INFO_SEL_*): nullptr, n bytes, or n int32 compared with label0 + k.  (thr, score_mode and the own word
// are not read.)
struct PoseInfoFrameJob : PoseFrameHead {
  const void* sel;
  uint32_t sel_mode;
  int32_t label0;
  double* scratch;
  PoseInfoRecord* out;
};
// ONE launch, a workgroup of 1024 threads per pose; every record is written (complete in stream order).
void launch_pose_info_frame(const PoseInfoFrameJob& job, hipStream_t st);

// ---- caller-supplied poses refitted on a scored frame (sc_polish_poses; sc_polish_poses.hip) ----------------------
// mask bytes [k * n, (k + 1) * n) are pose k's mask (mask == nullptr: none).  sel by sel_mode (SC_POLISH_POSES_SEL_*): nullptr, n
// bytes, or n int32 compared with label0 and label0 + k.
struct PolishPosesJob : PoseFrameHead {
  const void* sel;
  uint32_t sel_mode;
  int32_t label0;
  double* scratch;
  PolishBatchRecord* out;
  uint8_t* mask;
};
// ONE launch, a workgroup of 1024 threads per pose; every record (and mask) is written (complete in stream order).
void launch_polish_poses(const PolishPosesJob& job, hipStream_t st);

// ---- correspondences labelled by the pose that fits best (sc_assign_poses; sc_assign_frame.hip, sc_assign_batch.hip) ----------
// One pose's result: sc_assign_result of include/saccot.h, field for field (sc_assign_frame.hip asserts the size and the offsets).
struct AssignRecord {
  int32_t status;
  uint32_t count;
  uint64_t score;
  uint32_t reserved[4];
};
// The frame form.  sel: nullptr or n bytes.  label: n int32; d2: n floats or nullptr.  out: n_poses records, ZERO at launch (the
// workgroups add their tallies into count and score; workgroup 0 stores the status words).
struct AssignFrameJob : PoseFrameHead {
  const uint8_t* sel;
  int32_t* label;
  float* d2;
  AssignRecord* out;
};
// bytes of dynamic LDS of a launch: a pose's twelve floats and its two tally words
inline size_t assign_frame_lds_bytes(uint32_t n_poses) { return (size_t)n_poses * (48 + 8); }
// ONE launch, a workgroup per tile of ASSIGN_TILE correspondences (sc_assign.hpp); every label (and d2) is written.
void launch_assign_frame(const AssignFrameJob& job, hipStream_t st);
// The batch form.
struct AssignBatchJob : PoseBatchHead {
  int32_t* label;
  AssignRecord* out;
};
// ONE launch, a workgroup per problem; every label of a problem's range and every record is written (complete in stream order).
void launch_assign_batch(const AssignBatchJob& job, hipStream_t st);

// ---- poses relabelled and refitted until stable (sc_settle_poses; sc_settle.hpp, sc_settle_frame.hip, sc_settle_batch.hip) ----
// The frame form.  sel: nullptr or n bytes.  label: n int32 (every pass stores it; the last pass's stores are the output); d2: n
// floats or nullptr; out: n_poses records; rounds: two words or nullptr.  scratch: PolishPosesJob's, the same buffer.
struct SettleFrameJob : PoseFrameHead {
  const uint8_t* sel;
  double* scratch;
  PolishBatchRecord* out;
  int32_t* label;
  float* d2;
  uint32_t* rounds;
};
// ONE launch of ONE workgroup of 1024 threads; every label (and d2), every record and the two words are written.
void launch_settle_frame(const SettleFrameJob& job, hipStream_t st);
// The batch form.  rounds: two words per problem or nullptr.
struct SettleBatchJob : PoseBatchHead {
  PolishBatchRecord* out;
  int32_t* label;
  uint32_t* rounds;
};
// ONE launch, a workgroup per problem; every label of a problem's range, every record and word pair is written.
void launch_settle_batch(const SettleBatchJob& job, hipStream_t st);

// ---- duplicate poses found and folded (sc_merge_poses; sc_merge.hpp, sc_merge_frame.hip, sc_merge_batch.hip) -----------------
// One pose's record: sc_merge_pose of include/saccot.h, field for field (sc_merge_frame.hip asserts the size and the offsets).
struct MergeRecord {
  float Rt[12];
  int32_t status, index;
  uint32_t count, score;
};
// What both forms read of sc_merge_params.
struct MergeRule {
  uint32_t measure, num, den, min_count;
  int compact;
};
// The frame form.  sel: nullptr or n bytes.  rows: n_poses x merge_row_words(n) u64, every word written by the support launch.
// tally: 2 x n_poses words — the counts, then the scores —, ZERO at launch (the workgroups of the support launch add into them).
// overlap: n_poses x n_poses words, the caller's or the workspace's.  out, parent: n_poses; count: two words or nullptr.
struct MergeFrameJob : PoseFrameHead {
  const uint8_t* sel;
  MergeRule rule;
  uint64_t* rows;
  uint32_t* tally;
  uint32_t* overlap;
  MergeRecord* out;
  int32_t* parent;
  uint32_t* count;
};
__host__ __device__ inline size_t merge_row_words(int n) { return ((size_t)n + 63) / 64; }
// THREE launches: support (a workgroup per tile of MERGE_TILE correspondences: the bit rows and the tallies), overlap (a workgroup
// per tile of pose pairs j <= k: the table, mirrored), decide (ONE workgroup: the strength order, the fold, every output).
void launch_merge_frame(const MergeFrameJob& job, hipStream_t st);
// The batch form.  out, parent: n_poses x n_problems, motion-major; count: two words per problem or nullptr.
struct MergeBatchJob : PoseBatchHead {
  MergeRule rule;
  MergeRecord* out;
  int32_t* parent;
  uint32_t* count;
};
// ONE launch, a workgroup per problem; every record, parent and word pair is written (complete in stream order).
void launch_merge_batch(const MergeBatchJob& job, hipStream_t st);

// ---- loop consistency of a pair list's poses (sc_pairs_cycles; sc_cycles.hip) -------------------------------------------------
// One pair's record and the summary: sc_cycle_result and sc_cycle_summary of include/saccot.h, field for field (sc_cycles.hip
// asserts the sizes and the offsets).
struct CycleRecord {
  int32_t status;
  uint32_t cycles, ok, ok_alive, alive, dropped_round;
  double min_trace, max_e2;
  uint32_t reserved[2];
};
struct CycleSummary {
  uint32_t rounds, stable, alive, edges;
  uint64_t triangles, consistent;
};
// The round words, ZERO at launch: dropped[k], k = 1 .. max_rounds, the pairs round k dropped — a round's launch returns at once
// when the round before dropped none, and writes nothing, so every later word stays 0 as well; dropped[0] is never read.
struct CyclesCtl {
  uint32_t dropped[65];
  uint32_t edges;                  // pairs in alive_0
  uint64_t triangles, consistent;  // of alive_0, each counted by its pair on the two lowest sets
};
// rec: the pairs' records, entries: the sorted neighbour lists (sc_cycles_check.hpp); pose: the caller's records; keep: nullptr or
// n_pairs bytes; wide: 2 x 12 doubles a pair; alive: 2 x n_pairs bytes, buffer k & 1 holds alive_k; res: n_pairs; sum: one.
struct CyclesJob {
  const uint32_t* rec;
  const uint64_t* entries;
  const void* pose;
  const uint8_t* keep;
  double* wide;
  uint8_t* alive;
  CyclesCtl* ctl;
  CycleRecord* res;
  CycleSummary* sum;
  double tr_min, e2_max;
  uint32_t n_pairs, pose_stride, min_ok, max_rounds;
  int status;  // a record holds a status at byte 48
};
// max_rounds + 2 launches: prepare (validity, the oriented fp64 poses, alive_0, every record's head), a launch per round (a wave per
// pair: its two sorted lists intersected, the loops composed, the verdict), finish (the summary).
void launch_pairs_cycles(const CyclesJob& job, hipStream_t st);

// ---- absolute poses of a pair list's sets (sc_pairs_sync; sc_sync.hip) --------------------------------------------------------
// The three output records: sc_sync_set, sc_sync_pair and sc_sync_summary of include/saccot.h, field for field (sc_sync.hip asserts
// the sizes and the offsets).
struct SyncSetRecord {
  float Rt[12];
  int32_t status;
  uint32_t known_round, used, degenerate;
  double X[12];
};
struct SyncPairRecord {
  int32_t status;
  uint32_t used;
  double r2, e2;
  uint32_t reserved[2];
};
struct SyncSummary {
  uint32_t rounds, converged, known, used, changed_last, reserved[3];
};
// A set's state in one of the two buffers (buffer k & 1 holds X_k and known_k): 104 bytes.
struct SyncState {
  double X[12];
  uint32_t known, pad;
};
// What a set's own wave keeps about it across the rounds (one writer: no second buffer).
struct SyncInfo {
  uint32_t known_round, used, degenerate, pad;
};
// The round words, ZERO at launch: changed[k], k = 1 .. max_rounds, the sets round k changed — a round's launch returns at once when
// the round before changed none, and writes nothing, so every later word stays 0 as well; changed[0] is never read.  known, used,
// done: the finish launch's tallies and its ticket.
struct SyncCtl {
  uint32_t changed[257];
  uint32_t known, used, done;
};
// rec, entries: the pairs' records and the sorted neighbour lists (sc_cycles_check.hpp), off: the n_sets + 1 list starts; pose, use,
// weight: the caller's (use, weight: nullptr or an array); wide: 2 x 12 doubles a pair; wt: a double a pair, 0.0 where the pair is
// not usable; state: 2 x n_sets; info: n_sets.
struct SyncJob {
  const uint32_t* rec;
  const uint64_t* entries;
  const uint32_t* off;
  const void* pose;
  const void* use;
  const float* weight;
  double* wide;
  double* wt;
  SyncState* state;
  SyncInfo* info;
  SyncCtl* ctl;
  SyncSetRecord* set;
  SyncPairRecord* pair;
  SyncSummary* sum;
  double r2_max, e2_max;
  uint32_t n_sets, n_pairs, pose_stride, use_stride, anchor, max_rounds;
  int status;  // a record holds a status at byte 48
};
// max_rounds + 2 launches: prepare (a thread per pair: validity, use, weight, the oriented fp64 poses; a thread per set: X_0), a
// launch per round (a wave per set, a lane per slot of the header's sum), finish (the set records, the residuals, the summary).
void launch_pairs_sync(const SyncJob& job, hipStream_t st);

// ---- Gauss-Newton pose-graph solve of a pair list's sets (sc_pairs_solve; sc_solve.hip) ---------------------------------------
// The three output records: sc_solve_set, sc_solve_pair and sc_solve_summary of include/saccot.h, field for field (sc_solve.hip
// asserts the sizes and the offsets).
struct SolveSetRecord {
  float Rt[12];
  int32_t status;
  uint32_t state, degenerate, reserved;
  double X[12];
};
struct SolvePairRecord {
  int32_t status;
  uint32_t used;
  double cost, w2, v2;
  uint32_t reserved[4];
};
struct SolveSummary {
  uint32_t outer, stop, inner_total, inner_last, free_sets, used_pairs, held_last, reserved;
  double cost0, cost, rz0, reserved2;
};
constexpr uint32_t SOLVE_OUTER_MAX = 32, SOLVE_INNER_MAX = 256, SOLVE_PRODUCT_MAX = 2048;
// The control words, ZERO at launch.  A word is written by ONE workgroup of a launch (or added to by atomics) and read by LATER
// launches only, never by the launch that writes it: nothing depends on the order in which a launch's workgroups run.
//   stop, K, J     the decide launch's verdict: stop != 0 ends every later launch at once.
//   free_sets, used_pairs   tallies of the sets and prepare launches.
//   changed[j], held[j], inner[j]   tallies of step j: sets changed by the step launch, sets held by the factor launch, and the
//                  iterations applied (the decide launch counts them from live_u).
//   live_p[x], live_u[x], x = (j - 1) * max_inner + i: iteration i of step j is to be multiplied (written by its product launch,
//                  read by its update launch) / has been applied (written by its update launch, read by the next product launch).
//                  A word left 0 ends the chain: every later launch of the step finds its predecessor's word 0.
//   cost[j]        c_j;  rz0[j]: rz_0 of step j;  rz[i]: rz_i of the step in hand.
struct SolveCtl {
  uint32_t stop, K, J, free_sets, used_pairs, pad[3];
  uint32_t changed[SOLVE_OUTER_MAX + 1], held[SOLVE_OUTER_MAX + 1], inner[SOLVE_OUTER_MAX + 1], pad2;
  double cost[SOLVE_OUTER_MAX + 1], rz0[SOLVE_OUTER_MAX + 1], rz[SOLVE_INNER_MAX + 1];
  uint32_t live_p[SOLVE_PRODUCT_MAX + 2], live_u[SOLVE_PRODUCT_MAX + 2];
};
// What a set's launches keep about it: its state (SC_SOLVE_*), whether it is active in the step in hand, the init status, and the
// steps in which it was held or stepped to no finite pose.
struct SolveInfo {
  uint32_t state, active;
  int32_t status;
  uint32_t degenerate;
};
// rec, entries, off: as SyncJob's; pose, use, info, init: the caller's (use, info: nullptr or an array).  Per pair: wide 2 x 12
// doubles, usable a word, W 36 doubles, g 6, err 2 x 3 (cost_p, w2, v2 of state j & 1).  Per set: X 2 x 12 doubles (buffer j & 1
// holds X_j), x, r, z, q 6 each, p 2 x 6 (buffer i & 1 holds the p of iteration i), fac 21 (L row-major below the diagonal, then D),
// sinfo; deg: the usable pairs that name it (a tally, zeroed with ctl).  Chunk sums: rzc 2 x set chunks (buffer i & 1: rz_i), pqc
// set chunks, costc pair chunks.
struct SolveJob {
  const uint32_t* rec;
  const uint64_t* entries;
  const uint32_t* off;
  const void* pose;
  const void* use;
  const void* info;
  const void* init;
  double* wide;
  uint32_t* usable;
  double* W;
  double* g;
  double* err;
  double* X;
  double* x;
  double* r;
  double* z;
  double* q;
  double* p;
  double* fac;
  SolveInfo* sinfo;
  uint32_t* deg;
  double* rzc;
  double* pqc;
  double* costc;
  SolveCtl* ctl;
  SolveSetRecord* set;
  SolvePairRecord* pair;
  SolveSummary* sum;
  double r2_max, e2_max, cg2;
  uint32_t n_sets, n_pairs, pose_stride, use_stride, info_stride, init_stride, anchor, max_outer, max_inner;
  int status, info_status;  // a pose record holds a status at byte 48; an info record one at byte 296
};
// 5 + max_outer * (4 + 2 * max_inner) launches: prepare, sets, linearise, decide; per step: factor, (product, update) per inner
// iteration, step, linearise, decide; finish.
void launch_pairs_solve(const SolveJob& job, hipStream_t st);

// ---- descriptor matching for a batch of small problems (sc_match_batch; sc_match_batch.hip) -----------------
// Problem b owns rows [src_off[b], src_off[b + 1]) of fsrc and [tgt_off[b], tgt_off[b + 1]) of ftgt (1 .. MATCH_BATCH_MAX_N rows
// each, checked by the caller) and the output slot that starts at entry slot[b] = src_off[b] * knn.  tile_map: n_tiles pairs
// (problem, first row of the tile inside it), tiles of MATCH_BATCH_ROWS source rows, none across two problems.  Everything in
// device memory.  kp = knn, 2 with the ratio test (r2 > 0).
constexpr int MATCH_BATCH_ROWS = 64;
constexpr int MATCH_BATCH_MAX_N = 4096;
struct MatchBatchJob {
  const float* fsrc; const float* ftgt;
  const uint32_t* src_off; const uint32_t* tgt_off; const uint32_t* slot; const uint32_t* tile_map;
  uint32_t n_problems, n_tiles, dim, knn, kp, mutual;
  float r2;
  uint64_t* top;     // kp keys per source row, row src_off[b] + i at top + (src_off[b] + i) * kp: written by the distance launch
  uint64_t* colmin;  // SC_MATCH_MUTUAL, else nullptr: a key per target row (distance << 32 | source row of the problem), all ones at launch
  uint32_t* clean;   // a word per problem, non-zero at launch, cleared when the problem reads a non-finite descriptor
  int32_t* corr; float* d2; uint32_t* count;  // the slots, and 2 words per problem: n_b, the non-finite flag
  MatchGather g;     // sc_register_batch_features: packed points in, slot-positioned n x 3 arrays out (gsrc == nullptr: no gather)
};
// (its two launches: launch_match_batch_dist / _finish, below, for the four job types)

// ---- the same for listed pairs of shared sets (sc_match_pairs; sc_match_batch.hip, sc_polish_batch.hip) ----------------
// One table of sets, feat (total x dim), and a list of pairs drawn from it: the problems of the launches are the PAIRS.  A set
// serves many pairs, so nothing of a pair can be addressed by its sets' rows: pair p has a record of PAIR_WORDS words (built on the
// host, sc_pairs_check.hpp) with the first row and the size of both its sets in the table and the bases that are the pair's OWN —
// its rows' lists in `top`, its column minima in `colmin` (two pairs that share a target set do not share minima), its slot.
enum PairWord : int {
  PW_SRC = 0, PW_NS,   // the source set: first row in the table, rows (1 .. MATCH_BATCH_MAX_N, checked by the caller)
  PW_TGT, PW_NT,       // the target set
  PW_TOP,              // the pair's first row in `top`: the source rows of the pairs before it (slot / knn)
  PW_SLOT,             // the pair's first output entry: knn x PW_TOP
  PW_COL_LO, PW_COL_HI,  // the pair's first key in `colmin`: the target rows of the pairs before it (64 bits: it may pass 2^32)
  PAIR_WORDS
};
// A type of its own, so that the packed form's kernel argument and code stay what they were.  tile_map: n_tiles pairs (pair, first
// row of the tile inside its source set); g.src == g.tgt: the table's points.
struct MatchPairsJob {
  const float* feat;
  const uint32_t* rec; const uint32_t* tile_map;
  uint32_t n_problems, n_tiles, dim, knn, kp, mutual;
  float r2;
  uint64_t* top; uint64_t* colmin; uint32_t* clean;  // as MatchBatchJob's, at the pair's own bases; a `clean` word per pair
  int32_t* corr; float* d2; uint32_t* count;
  MatchGather g;
};

// ---- both forms under a pose prior per problem (sc_match_guided_batch; sc_match_batch.hip) ---------------------------
// The keypoints of the batch (point so + i of src is src[(so + i) * s_elem + c * s_comp], as MatchGather's; the pairs form: src ==
// tgt, the table), one pose record per problem — 12 floats at byte pose_stride * b of `pose`, with use_status an int32 status at
// byte 48 of the record — and gate2; cell (i, j) of problem b is a candidate only where resid2(Rt_b, src[i], tgt[j]) < gate2.  A
// problem whose status is not SC_OK is skipped: its count pair is (0, 0) and nothing else of it is read or written.  g2 (optional):
// the gate residual of every output entry, slot-positioned like d2.
struct MatchBatchGuide {
  const float* src; const float* tgt;
  uint32_t s_elem, s_comp, t_elem, t_comp;
  const void* pose;
  uint32_t pose_stride, use_status;
  float gate2;
  float* g2;
};
// Types of their own, so that the unguided forms' kernel arguments and code stay what they were; everything the base says holds, and
// `clean` is also cleared when a point of the problem or its pose is not finite, whatever the gate excludes.
struct MatchGuidedBatchJob : MatchBatchJob { MatchBatchGuide gd; };
struct MatchGuidedPairsJob : MatchPairsJob { MatchBatchGuide gd; };
// The two launches of every form, on the job type (instantiated in sc_match_batch.hip for the four above).
// dist: a workgroup per tile: the canonical distances of its rows to every target row of the problem, the rows' kp smallest keys -> top
// finish: a workgroup per problem: mutual / ratio per row, compaction inside the slot in ascending (row, rank) order, the count pair, the gather
template <class Job> void launch_match_batch_dist(const Job& job, hipStream_t st);
template <class Job> void launch_match_batch_finish(const Job& job, hipStream_t st);

}  // namespace sc
