// sc_ctx.hpp — private to the host side of the C ABI (sc_capi*.hip): the context and its call state, the status macros, and the
// host helpers that more than one of those files uses.  No kernel source includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <type_traits>

#include "../../include/saccot.h"
#include "../../include/saccot_debug.h"
#include "sc_frame_check.hpp"
#include "sc_kernels.hpp"
#include "sc_match_batch_check.hpp"

namespace sc {

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  template <class T> T* as() const { return static_cast<T*>(p); }
};

constexpr int N_EVENTS = 12;  // 0..8 stage brackets, 9..10 the key kernel (all reused by calibrate_events), 11 the stop of stage C2's filter kernel (SC_FLAG_TIMING_HOT)
constexpr int N_PINNED = HW_COUNT;  // the host words (sc_kernels.hpp, HostWord)
static_assert(HW_MERGED_M == HW_MERGED_T + 1 && HW_WINNER_POS == HW_WINNER + 1, "merge_prepare and the finalize kernel write word pairs");

// How a pass is enqueued: decided by the entry point BEFORE the pass starts and handed to hyp_begin, which stores it in the fresh pass.
struct PassMode {
  // the entry point can repeat the call (sc_register*), or its caller does (sc_hypothesize_device with SC_FLAG_EST_BOUND): stage B
  // may prune by an ESTIMATED bound (sc_tri_prune.hip 3c); the select verifies it, finalize_wait reads the verdict (frame_end)
  bool may_estimate = false;
  // host-free enqueue (include/saccot.h): a call of the last one's shape does not wait for stage B's two counts; its launches cover E_cov
  // edges / M_cov keys (fast_plan) and read the real counts from device memory; finalize_wait validates, and the call is repeated the waiting
  // way when a count outgrew the cover.  pass_end takes host_free back; the covers stay for sc_debug_last.
  bool host_free = false;
  uint64_t E_cov = 0, M_cov = 0;
};

// Stage B's form: which of its kernels a call runs, in which variant.  Each field is decided ONCE, by the function named above it
// (sc_capi_tri.hip; the reasons stand there), and every later line of run_edges / run_select reads it here.  run_edges starts from
// StageBForm{} — but for `build`, which stage A's launches read before, and `ord_state`, which run_select sets — so a stage hook, which
// starts no pass, finds nothing of the call before.
struct StageBForm {
  // ---- hyp_begin (before stage A: stage_inputs, run_compat and run_row_stats read it); a stage hook clears it
  bool build = false;       // launch_edge_build: row statistics + edge list + estimating sample in one launch
  // ---- form_begin, at the top of run_edges
  bool spec = false;        // host-free (PassMode): no wait; E and M are what the launches COVER, the kernels read the real counts from device memory
  bool own_sample = false;  // the whole sample goes into the context's own histogram (no exchanged histogram, one part); run_select must be handed the same
  bool fused = false;       // edge_off / ebase are made by the row kernel (run_row_stats) or by the fused edge kernel: no scan of the degrees
  bool est_local = false;   // the bound may be an estimate: the call can be repeated and the whole sample is taken here
  bool est_shard = false;   // ... sharded, SC_FLAG_EST_BOUND: every rank takes the whole sample, the merge verifies
  // ---- form_counted, behind the edge count
  bool pruned = false;      // certified pruning (sc_tri_prune.hip 3b)
  bool use_events = false;  // counting pass + event list (sc_tri.hip 2b)
  bool have_total = false;  // SC_FLAG_EXACT_TOTAL: the 3-cliques of the whole graph are counted as well (HW_TOTAL)
  bool est_active = false;  // stage B prunes by an estimate (Pass::plan.estimate)
  // ---- form_select, at the top of run_select (these need the edge count)
  uint64_t spec_cap = 0;    // keys the speculative key pass may write (0: no speculative pass)
  bool ord_on = false;      // ordinals from the ordered strong list (sc_tri.hip 2c): no scan of the per-edge counts
  bool recut = false;       // sharded event path: the ranks' edge ranges are cut again after the certificate
  bool trimmed = false;     // host-free on the fused edge kernel: pruning kernel and scan stop at the real edge count
  int ord_state = 0;        // 0 ordinals from the scan of the per-edge counts, 1 from the ordered strong list, 2 that form, then an overflow's fall-back through the scan (read_triangle_count raises it; sc_debug_last)
  // ---- form_keys, behind the triangle count
  bool events_ok = false;   // the event list holds every event (no region overflowed)
  bool fast_window = false; // the select takes the a-priori window [2, 3]: two rounds, and an estimated bound is verified by the first
  bool keys_done = false;   // the speculative key pass wrote every key: no second pass
};

// One run through hyp_begin (or sc_shard_compat_device) to finalize_wait (sc_capi_frame.hip).  Assigned Pass{} in pass_begin and
// nowhere else: what a pass did not set itself reads as "no".  Fields are READ after the pass as well — by a finalize call that comes
// later (have_hyp links the two, and it may come twice), by note_completed (E, M, n, params, form.use_events), by fill_stats and
// sc_debug_last (counts, covers, filter_*, est_state, form.ord_state, hot_ext) — so nothing is cleared when a pass ends except
// mode.host_free.  The stage hooks (sc_*_host) start no pass: they run single kernels on the context's buffers and touch only what
// host_to_planes says.
struct Pass {
  PassMode mode;
  int n = 0, ld = 0; uint32_t T_eff = 0;
  uint64_t E = 0, M = 0, M_total = 0;  // stage B's counts (host-free: the covers until finalize_wait has validated, then the real ones)
  StageBForm form;          // stage B's decisions (above)
  Derived dv{}; Shard sh{};
  bool begun = false, have_hyp = false;  // sc_hypothesize_begin_device is done (_end may follow); the hypothesize half is done (finalize may follow)
  sc_params params{};
  bool timing = false, timing_hot = false, timed_trikeys = false, refine = false;
  int timing_one = -1;      // SC_FLAG_TIMING_ONE: the one stage bracket recorded (0 .. 6), -1: none
  bool hot_ext = false;     // SC_FLAG_TIMING_HOT took its timestamps from the kernels' dispatch packets (run_stage_c)
  uint32_t amx_blocks = 0;  // workgroups of the arg-max launch whose pairs this context's finalize step reduces itself (0: one reduced pair in `key`)
  uint64_t* bits_cur = nullptr;  // the adjacency bit matrix: the context's own buffer, or — sharded stage A — the caller's all-gathered one
  bool rows_fused = false;  // run_row_stats already produced edge_off / ebase / cost_pre and armed the edge count
  bool regular = false;     // every assumption of the host-free form was met (run_select, apply_verdict): note_completed files it as fast_ok
  bool est_void = false;    // stage B's estimate (form.est_active) could not be verified on the path taken (event overflow): repeat
  int est_state = 0;        // 0 certified bound (or no pruning), 1 estimated and verified: apply_verdict sets it, count_frame reads it
  SamplePlan plan{false, 1u, 0};
  // stage C2's reference frame (sc_gramref.hpp): on the hot path the estimating sample leaves candidate triangles behind (ref_cand_n of
  // them) and the counting pass carries the vote as an extra workgroup (ref_done); everywhere else stage C votes in a launch of its own
  uint32_t ref_cand_n = 0; bool ref_done = false;
  bool filter_on = false;   // C2 goes through a matrix-pipe filter (decided ONCE per pass: decide_filter)
  int filter_mode = 0;      // ... which: 1 linear, 2 Gram (0: the plain fp32 kernel)
  FilterPlan fx_plan{};     // ... with this plan
  // sharded A + B (sc_shard_*_device): the phase reached (0: none) and the gathered candidate blobs
  bool sharded_ab = false; int shard_phase = 0;
  const void* cand_all = nullptr; size_t cand_bytes = 0;
  // rounds on this pass's frame (sc_peel): set where a frame's status becomes SC_OK (sc_wait, whichever way the frame ran), gone with
  // the pass (pass_begin) or when any other computing entry is called (peel_end)
  bool peelable = false;
  uint32_t peel_round = 0;           // rounds done
  uint32_t peel_prev = 0xFFFFFFFFu;  // position of the winner whose mask the next round's claim step folds in (all ones: none)
  uint32_t peel_claimed = 0;         // inlier-count mode: correspondences claimed so far (the best_counts add up to it)
};

// The outstanding half of sc_register_device_async / sc_finalize_gathered_device_async (at most one per context; sc_wait ends it)
enum class Outstanding {
  None,
  Enqueued,  // a host-free register: sc_wait validates it and may repeat it the waiting way (PendingCall)
  Complete,  // a waited register: done, its status held (Frame::held_rc)
  Finalize,  // the second half of sc_finalize_gathered_device_async: no repeat inside the library
};
// the arguments of an Enqueued call, kept for its repeat
struct PendingCall {
  const float* src = nullptr; const float* tgt = nullptr; int64_t n = 0; sc_params p{};
  float* Rt = nullptr; uint8_t* mask = nullptr;
};

// One call of an entry point as its caller sees it: it survives the library's own repeat of the call (sc_wait -> register_waited: a
// second pass) and ends in count_frame.  Assigned Frame{} in frame_begin and nowhere else.
struct Frame {
  int fast_state = 0;            // 0 waited, 1 host-free and valid, 2 host-free, failed validation, repeated
  bool lane = false;             // its host-free enqueue ran on the context's lane (sc_ctx::lane_fork)
  bool est_failed_call = false;  // a pass of this frame saw its estimate fail (sc_debug_last: prune_bound 2); the repeat must not forget it
  Outstanding outstanding = Outstanding::None;  // set by leave_outstanding, taken back by sc_wait (sc_capi_frame.hip)
  int held_rc = 0;               // Complete: the status sc_wait delivers
  PendingCall call;
  sc_stats pend_stats{};         // the library's own copy of the call's statistics: sc_wait hands it to the caller
};

// What a host form may stage at once (HostArrays, below): sc_register_batch_features has nine arrays
constexpr int N_HOST_ARR = 9;

// The grow-only device workspace: Buf members and nothing else.  sc_destroy walks it as an array (workspace_bufs), so a Buf declared
// here is freed; there is no second list to keep in step.
struct Workspace {
  Buf in_src, in_tgt, planes, S, bits, deg, degp, wpre, ebase, edge_off, scan_tmp, ei, ej, es, ebi, ebj, tcnt, toff, wkey, kcol, ctl, events, blk_gt,
      blk_eq, blk_minmax, bits2, off_gt, off_eq, sel_ord, sel_key, sortkey, sorted, sort_tmp, tri, tri_rk, key_rk, rt, rt_aos, partial, cnt, key, rt12,
      mask, refine_tmp, amx_pairs, strong, ord_cnt, rowcost, cost_pre, lb_state, lb_ticket, fx_tile, fx_state, fx_mx, fx_part, fx_coef, guard_tmp, fx_frame, ref_cand,
      // sc_peel / sc_register_instances: allocated by the first round, never by a frame.  peel_cnt: a round's scores — the frame's own stay
      // in `cnt`, where sc_polish reads them whether or not rounds have run
      peel_planes, peel_claimed, peel_words, peel_label, peel_cnt,
      // sc_polish: allocated by the first polish, never by a frame.  cand: 64 candidate records, then the word that counts them;
      // tmp: the chunk sums, candidates x chunk_scratch_bytes(n)
      polish_cand, polish_tmp,
      // sc_match / sc_register_features: allocated by the first match, never by a frame.  part: the slices' partial lists; words: the
      // "clean" word, the host entries' count pair, the guided host entries' pose, then the column minima; the rest: device copies of
      // the host entries' arrays (g2: the guided host entries' only, allocated by the first of them)
      match_part, match_words, match_fsrc, match_ftgt, match_psrc, match_ptgt, match_corr, match_d2, match_gsrc, match_gtgt, match_g2,
      // sc_match_guided_poses, the host forms' device copies of the pose records and of the labels: allocated by the first of them
      match_pose, match_label,
      // The staging pool of every other host form (HostArrays, below): slot k holds the device copy of the k-th array the form
      // declares.  Allocated by the first host form that needs the slot, never by a frame or a device form; alive for one host form
      // at a time, dead on its return.
      host_arr[N_HOST_ARR],
      // ---- what follows is allocated by the first call of the entry named, host or device form, never by a frame or by another entry
      // sc_register_batch.  off: the copy of the caller's offsets
      batch_off,
      // sc_match_batch / sc_register_batch_features, and sc_match_pairs / sc_register_pairs_features (a pair is a problem of theirs,
      // found through a record).  meta: the copies of both offset arrays, the slot starts and the tile map (pairs: the pairs' records,
      // the slot starts, the tile map); top: the rows' lists between the two launches; words: a "clean" word per problem, then the
      // column minima; gsrc / gtgt: the gathered points, slot-positioned
      mbatch_meta, mbatch_top, mbatch_words, mbatch_gsrc, mbatch_gtgt,
      // sc_polish_batch.  off: the copy of the caller's offsets (the slot form: both arrays and the slot starts; the pairs form: the
      // pairs' records)
      pbatch_off,
      // sc_register_instances_batch.  off: the copy of the caller's offsets (the features form holds what
      // sc_register_batch_features_device holds, in the mbatch buffers)
      ibatch_off,
      // sc_pose_info_batch.  off: the copy of the caller's offsets (the slot form: both arrays and the slot starts; the pairs form:
      // the pairs' records)
      pinfo_off,
      // sc_pose_info_frame.  tmp: the chunk sums and bit words, n_poses x chunk_scratch_bytes(n) — not polish_tmp: a polish may be
      // enqueued behind the call
      pinfo_frame_tmp,
      // sc_polish_poses.  tmp: the chunk sums and bit words, n_poses x chunk_scratch_bytes(n) — not polish_tmp and not
      // pinfo_frame_tmp: either call may be enqueued behind this one.  sc_settle_poses's frame form keeps its member bits and chunk
      // sums here as well: one layout (sc_chunks.hpp), and the calls are stream-ordered, so one serves both
      ppose_tmp,
      // sc_assign_poses, sc_settle_poses, sc_merge_poses.  off: the batch form's copy of the caller's offsets (assign's frame form
      // needs no buffer: the tallies are added into the caller's records).  mrg_rows: merge's frame form's support sets, n_poses x
      // ceil(n / 64) u64, and behind them the 2 x n_poses tally words; mrg_table: its overlap table where the caller passes none
      asg_off, stl_off, mrg_off, mrg_rows, mrg_table,
      // sc_pairs_cycles.  meta: the pairs' records and the sorted neighbour entries (sc_cycles_check.hpp); wide: the oriented fp64
      // poses; state: the round words and the two buffers of alive bytes
      cyc_meta, cyc_wide, cyc_state,
      // sc_pairs_sync.  meta: the pairs' records, the sorted neighbour entries and the list starts; wide: the oriented fp64 poses and
      // the pairs' weights; state: the round words, the two buffers of the sets' states and their tallies (sc_sync_check.hpp)
      sync_meta, sync_wide, sync_state,
      // sc_pairs_solve.  meta: as sync_meta; pair: the oriented fp64 poses, W_p, g_p, the errors of two states and the usable words;
      // set: the two states, the vectors of the inner solve, the factors and the sets' tallies; ctl: the control words, the sets'
      // tallies of usable pairs and the chunk sums (sc_solve_check.hpp)
      solve_meta, solve_pair, solve_set, solve_ctl;
};
constexpr size_t N_WORKSPACE_BUFS = sizeof(Workspace) / sizeof(Buf);
static_assert(std::is_standard_layout<Workspace>::value && alignof(Workspace) == alignof(Buf) && sizeof(Workspace) == N_WORKSPACE_BUFS * sizeof(Buf),
              "Workspace holds Buf members only: it is walked as an array of them");
inline Buf* workspace_bufs(Workspace* w) { return reinterpret_cast<Buf*>(w); }

}  // namespace sc

// The context.  What lives as long as it does is a direct member; the call in flight is `frame` and, inside it, `pass`.
struct sc_ctx : sc::Workspace {  // (the workspace buffers are direct members too: c->planes)
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // A caller's stream is set (sc_set_stream; SC_STREAM_DEFAULT included): outputs are stream-ordered, nothing synchronises.  NOT
  // "stream != own_stream": a frame on its lane (below) has the private stream as `stream` and still belongs to a caller's.
  bool caller_stream = false;
  // The lane: a host-free frame of a direct sc_register_device_async call on a caller's stream runs on own_stream — idle whenever
  // a caller's stream is set — beside that stream: lane_fork is recorded on the caller's stream at the call and the lane waits
  // for it; lane_join is recorded behind the frame's last launch and the caller's stream waits for it in sc_wait (lane_join_caller).
  // While the frame is outstanding `stream` is the lane and lane_home the caller's stream.
  hipEvent_t lane_fork = nullptr, lane_join = nullptr;
  hipStream_t lane_home = nullptr;
  bool on_lane = false;
  uint64_t n_lane = 0;  // frames that ran on the lane (sc_debug_last)
  std::string last_error;
  size_t held = 0;
  uint64_t cap_bytes = 64ull << 30;  // what ensure() holds `held` against: every entry point sets it from its sc_params
  hipEvent_t ev[sc::N_EVENTS] = {};
  float ev_overhead_us = -1.f;  // cost of one event record inside a bracket (calibrate_events); < 0: not measured yet (on this stream)
  uint64_t* pinned = nullptr;  // N_PINNED x u64 host-pinned area the kernels write results into, indexed by HostWord

  // the XCD-aware block orders of stage A (compat_wg_map), one per row width met so far: a context that alternates between a few
  // sizes must not rebuild and upload the map on every call (that cost 2 ms per call in bench.py's varying-n leg)
  static constexpr int N_WG_MAPS = 8;
  struct WgMap { int W = 0; uint32_t len = 0; sc::Buf buf; uint64_t used = 0; } wg_maps[N_WG_MAPS];
  uint64_t wg_map_clock = 0;
  // sc_register (host arrays in, host arrays out): pinned, device-mapped staging areas — the staging kernel reads the
  // correspondences straight from host memory and the finalize kernel writes (R, t, mask) straight into it: no copies
  void* h_in = nullptr; size_t h_in_cap = 0;
  void* h_out = nullptr; size_t h_out_cap = 0;
  // sc_register_batch: the pinned staging area the caller's offsets pass through on their way to batch_off, and the event behind the
  // copy out of it (the next batch call waits for it before it overwrites the area)
  void* h_batch_off = nullptr; size_t h_batch_off_cap = 0;
  hipEvent_t batch_off_ev = nullptr;
  bool host_arr_live = false;  // a host form is between its room and its return: host_arr is its (HostArrays::run)
  uint64_t ev_capacity = 1ull << 21;  // event records (32 B each); doubled after an overflow
  sc::Tuning tn;  // defaults unless sc_set_debug() changed them; the library reads no environment variable
  // decoupled look-back launches (single-pass scan, fused compaction): their state area and its epoch
  uint32_t lb_epoch = 0; void* lb_zeroed = nullptr; size_t lb_zeroed_cap = 0;
  // run-time probe of the matrix pipe's accumulation model (sc_gram_guard.hip): 0 not run, 1 holds, 2 violated
  int gram_guard = 0; float gram_guard_worst = 0.f;

  // ---- history: what a completed call leaves for the next one (note_completed and apply_verdict, sc_capi_frame.hip, write it;
  // fast_plan, the array growers and edge_build_ok, sc_capi_tri.hip, read it).  The two rules are sc_frame_check.hpp's.
  bool fast_ok = false;      // the last completed call was regular (events, a-priori window, T triangles found): the next may be enqueued host-free
  sc::ShapeHistory shape;    // the last call's counts and shape, the window of maxima the covers are sized by
  sc::EstHistory est;        // an estimate failed on this context: it certifies for a while (sc_set_debug resets)
  // a call's ordered strong list (sc_tri.hip 2c) had more chunks than the key kernel holds and fell back through the scan: the context
  // takes the scan form from then on — such a graph would overflow again (sc_set_debug resets)
  bool ord_off = false;
  // the coordinate maxima and boxes the staging kernel of the last completed call published (use_filter): what a host-free call
  // picks stage C2's kernel by when it is enqueued before its own staging kernel has run — a second frame in flight on the stream
  uint64_t mx_last = ~0ull, box_last[6] = {0, 0, 0, 0, 0, 0};
  // cumulative over the context's life (sc_debug_last): how its sc_register_device(_async) / host-free sc_hypothesize_device calls
  // were enqueued and how stage B's pruning bound fared — what a stream of frames reports (a per-call field would only say the last)
  uint64_t n_frames = 0, n_fast_ok = 0, n_fast_repeat = 0, n_est_ok = 0, n_est_fail = 0;
  uint64_t n_spec_grow = 0;  // buffers re-allocated (a stream synchronisation each) inside host-free enqueues

  sc::Frame frame;  // the call in flight, as the caller sees it
  sc::Pass pass;    // ... and the library's current (or last) run through the stages for it
};

namespace sc {

int fail_hip(sc_ctx* c, hipError_t e, const char* what);
// evaluate; a HIP error (with its text in last_error as SC_EHIP), or a status other than SC_OK, is the caller's status
#define HIPCHK(c, expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) return fail_hip((c), _e, #expr); } while (0)
#define SC_TRY(expr) do { const int _rc = (expr); if (_rc != SC_OK) return _rc; } while (0)
#define ENSURE(c, buf, bytes) SC_TRY(ensure((c), (buf), (bytes)))
#define ENSURE_ROOM(c, buf, need, room) SC_TRY(ensure_room((c), (buf), (need), (room)))

// ---- defined in sc_capi.hip, used by the other host files as well (what each does is said at its definition)
int ensure(sc_ctx* c, Buf& b, size_t bytes);
int ensure_room(sc_ctx* c, Buf& b, size_t need, size_t room);
int check_params(const sc_params* p);
Derived derive(const sc_params* p);
inline uint64_t workspace_cap(const sc_params* p) { return p->max_workspace ? p->max_workspace : (64ull << 30); }
inline Points points_of(const sc_ctx* c) { return Points{c->planes.as<float>(), c->pass.n, c->pass.ld}; }
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
int lb_next(sc_ctx* c, size_t bytes, int slot, size_t desc_off, LbArgs* out);
int rec(sc_ctx* c, int i);
float ev_us(sc_ctx* c, int a, int b);
inline void arm_word(sc_ctx* c, HostWord w) { c->pinned[w] = PIN_PENDING; }
// HW_EV_OVERFLOW's high half: the overflow (low half) was the ordered strong list's chunk count, not — or not only — an event region
inline bool chunk_overflow(const sc_ctx* c) { return chunks_overflowed(c->pinned[HW_EV_OVERFLOW]); }
int wait_word(sc_ctx* c, HostWord idx);
// "who: what" into last_error; the status of a refused call
inline int refuse(sc_ctx* c, const char* who, const char* what) {
  c->last_error = std::string(who) + ": " + what;
  return SC_EINVAL;
}
// a refused NULL argument, named (the context is there: sc_last_error can say which)
#define SC_NOT_NULL(c, who, arg) do { if (!(arg)) return refuse((c), (who), #arg " is NULL"); } while (0)
// an sc_register_device_async / sc_finalize_gathered_device_async call is outstanding on this context
inline int busy(sc_ctx* c) { return c->frame.outstanding != Outstanding::None ? (c->last_error = "a call is outstanding on this context (sc_wait first)", SC_EINVAL) : SC_OK; }
// Any computing entry other than sc_peel* ends the frame the context may hold (include/saccot.h, sc_peel)
inline void peel_end(sc_ctx* c) { c->pass.peelable = false; }
// ... and sc_wait opens one where a frame's status is SC_OK.  The same state whichever way the frame ran (waited, host-free, repeated
// after a miss): the winner's words are those of the pass that delivered the outputs
inline void peel_open(sc_ctx* c) {
  c->pass.peelable = true; c->pass.peel_round = 0;
  c->pass.peel_prev = (uint32_t)c->pinned[HW_WINNER_POS];
  c->pass.peel_claimed = (uint32_t)(c->pinned[HW_WINNER] >> 32);
}
void fill_stats(const sc_ctx* c, sc_stats* s);

// What an entry point checks before it touches the context, always in this order: peel_end, busy, check_params(p), p->shard_world == 1.
// Each entry names the ones that apply to it; one whose own order is another (sc_register_device_async, sc_register_instances,
// sc_compat_host) spells that out itself.
enum EntryCheck : unsigned { ENDS_FRAME = 1u, NOT_BUSY = 2u, PARAMS = 4u, ONE_RANK = 8u };
int entry_checks(sc_ctx* c, const sc_params* p, unsigned checks);
// the caller's sc_stats, if it gave one of this library's size, from the context's copy
inline void copy_stats(sc_stats* stats, const sc_stats& from) { if (stats && stats->size == sizeof(sc_stats)) *stats = from; }
// n x 3 host arrays -> in_src / in_tgt (enqueued; the arrays must stay until the stream has passed the copies)
int points_to_device(sc_ctx* c, const float* src, const float* tgt, int64_t n);
// rt12 and n bytes of mask -> the caller's host arrays (R and t split); the stream is idle on return
int outputs_to_host(sc_ctx* c, size_t n, float R[9], float t[3], uint8_t* mask);

// ---- defined in sc_capi_match.hip / sc_capi_batch.hip, used by the other batch files as well
// the rules of sc_match_params and of ns, nt; fills everything of *job but the descriptor pointers
int match_check(sc_ctx* c, const sc_match_params* mp, int64_t ns, int64_t nt, MatchJob* job);
// The steps of a match on one pair of sets (sc_capi_match.hip; sc_capi_match_guided_poses.hip runs the same sequence).
// match_enqueue: the memset and the two launches, writing what `o` names (MatchOut, sc_kernels.hpp; o.to_host: a host form)
int match_enqueue(sc_ctx* c, const MatchJob& job, MatchOut o);
// What a host form brings: its arrays, and which parts it has.  The sequence match_host runs for all of them: the keypoints ->
// match_psrc / match_ptgt (a guided form; room for g2 with them), the descriptors -> match_fsrc / match_ftgt, the pose records ->
// match_pose, match_enqueue, the ONE wait (HW_MATCH: the count, or SC_EINVAL for something not finite), the read-back of that many
// entries of corr and d2 and — where asked for — g2 and label, and the wait for the stream.  A features form (p: the gather into
// match_gsrc / match_gtgt) gets all but the last: its read-backs are enqueued, and match_register_gathered goes on from there.
struct MatchHost {
  const float* fsrc; const float* ftgt;        // descriptors
  const float* src_pts; const float* tgt_pts;  // keypoints: the guided and the features forms
  MatchGuide* gd;                              // a guided form: the guide but for its pointers (guide_check / poses_check), in layout `layout`
  uint32_t layout;
  const float* Rt;                             // sc_match_guided: the pose, 12 host floats
  const void* pose;                            // sc_match_guided_poses: the records, as given
  const sc_params* p;                          // a features form
  int32_t* corr; float* d2; float* g2; int32_t* label;  // the caller's arrays (g2, label: optional)
};
int match_host(sc_ctx* c, MatchJob job, const MatchHost& h, uint32_t* found);
// the tail of a features form: fewer than 3 matches -> the identity and SC_ENOHYP; else sc_register_device on the gathered points
// (n x 3 whatever the caller's layout) and its outputs -> the caller's
int match_register_gathered(sc_ctx* c, const sc_params* p, uint32_t found, float R[9], float t[3], uint8_t* mask, sc_stats* stats);
// the caller's points (either layout of sc_params, src_rows / tgt_rows of them) -> two n x 3 arrays, as a finish kernel is told
inline MatchGather gather_of(const float* src, uint32_t src_rows, const float* tgt, uint32_t tgt_rows, int layout, float* gsrc, float* gtgt) {
  const bool soa = layout == SC_SOA;
  return MatchGather{src, tgt, soa ? 1u : 3u, soa ? src_rows : 1u, soa ? 1u : 3u, soa ? tgt_rows : 1u, gsrc, gtgt};
}
// the points of both sets in a guide's layout, as the kernels are told (MatchGuide, MatchBatchGuide: MatchGather's strides)
template <class Guide>
void guide_points(Guide* gd, const float* src, size_t src_rows, const float* tgt, size_t tgt_rows, uint32_t layout) {
  const MatchGather g = gather_of(src, (uint32_t)src_rows, tgt, (uint32_t)tgt_rows, (int)layout, nullptr, nullptr);
  gd->src = g.src; gd->tgt = g.tgt;
  gd->s_elem = g.s_elem; gd->s_comp = g.s_comp; gd->t_elem = g.t_elem; gd->t_comp = g.t_comp;
}
// a guided features entry's keypoints are one pair of arrays: the gate and the gather read them the same way
inline int layouts_agree(sc_ctx* c, const char* who, const sc_guide_params* gp, const sc_params* p) {
  if ((int32_t)gp->layout != p->layout) return refuse(c, who, "guide->layout must be params->layout: the keypoints are one pair of arrays");
  return SC_OK;
}
// what a batch entry refuses of sc_params (shard_world != 1, refit, timing, an estimated bound); `who` opens the message
int batch_params_check(sc_ctx* c, const sc_params* p, const char* who);
// what a batch entry refuses of the caller's offsets (sizes 3 .. SC_BATCH_MAX_N, nothing decreasing, a total of 2^31 at most): the
// rule that is broken, for the caller to put its name in front of; nullptr: they are fine
const char* batch_offsets_error(const uint32_t* offset, uint32_t n_problems);
// what the registration kernels read of sc_params (the pointers and sizes are the caller's; a slot form then sets soa = 0)
inline BatchJob batch_job_of(const sc_params* p) {
  BatchJob job{};
  job.soa = p->layout == SC_SOA; job.T = p->max_triangles; job.rank_mode = p->rank_mode; job.score_mode = p->score_mode;
  job.dv = derive(p);
  return job;
}
// The pinned staging area that host words of a batch call (offsets, maps) pass through on their way to the device.  begin: the area
// holds `bytes` and the copy out of the call before is done (an event behind that copy — not behind that call's kernel); the caller
// fills c->h_batch_off; send: area -> dst (enqueued), and the event behind it.
int batch_staging_begin(sc_ctx* c, size_t bytes);
int batch_staging_send(sc_ctx* c, Buf& dst, size_t bytes);
// the caller's offsets (n_problems + 1 words) through that area into dst (enqueued)
inline size_t batch_offsets_bytes(uint32_t n_problems) { return ((size_t)n_problems + 1) * 4; }
int batch_offsets_to_device(sc_ctx* c, const uint32_t* offset, uint32_t n_problems, Buf& dst);

// The host-array form of an entry (defined in sc_capi_batch.hip).  The entry declares its arrays — an input is copied in, an output
// copied out, each with its byte count said once — and gets a handle for each; the k-th array declared is staged in slot k of the
// context's pool (Workspace::host_arr), whichever entry declares it.  An optional array the caller did not pass is declared all the
// same, with its host pointer NULL: it keeps its slot, needs no room, is not copied, and `at` gives nullptr for it.  `also` names a
// workspace buffer of the entry's own (its scratch, its copy of the offsets) that its enqueue is going to ENSURE.  Then
//   run(enqueue): room for every staged array, in declaration order, then for every `also` buffer — nothing is enqueued before the
//   last one has its room, so SC_ENOMEM leaves no copy from the caller's memory in flight -> the copies in, in declaration order ->
//   enqueue(), the device form's sequence on at<T>(handle) -> the copies out — those declared `first` before the others, each group
//   in declaration order -> the wait for the stream.  A step that fails behind the room is waited for as well: whatever a host form
//   returns, no copy from or into the caller's memory is in flight.
// One HostArrays is alive per context (sc_ctx::host_arr_live); between its return and the next one's room the pool holds nothing.
struct HostArrays {
  static constexpr int MAX = N_HOST_ARR;
  static constexpr int MAX_ALSO = 2;  // sc_merge_poses_frame: its rows and its own table
  explicit HostArrays(sc_ctx* ctx) : c(ctx) {}
  int in(const void* host, size_t bytes) { return add(Arr{host, nullptr, bytes, false}); }
  int out(void* host, size_t bytes, bool first = false) { return add(Arr{nullptr, host, bytes, first}); }
  // k arrays that only the family's other form has (a frame form's src, tgt; a batch form's sel): their slots stay theirs.  The two
  // forms of a family declare ONE list in ONE order, so that an array has the same slot in both — as it had one buffer in both
  void absent(int k = 1) { while (k-- > 0) add(Arr{nullptr, nullptr, 0, false}); }
  void also(Buf& b, size_t bytes) { if (n_also < MAX_ALSO) { more[n_also] = &b; more_bytes[n_also] = bytes; } n_also++; }
  // the device copy of a declared array, once run has made its room (nullptr: the caller did not pass it)
  template <class T> T* at(int k) const { return k < MAX && (arr[k].from || arr[k].to) ? c->host_arr[k].as<T>() : nullptr; }
  template <class Enqueue> int run(Enqueue enqueue) {
    SC_TRY(room());
    int rc = send();
    if (rc == SC_OK) rc = enqueue();
    return finish(rc);
  }

 private:
  struct Arr { const void* from; void* to; size_t bytes; bool first; };
  int add(const Arr& a) { if (n < MAX) arr[n] = a; return n++; }  // (room refuses an entry that declared more)
  int room();
  int send();
  int fetch();
  int finish(int rc);
  sc_ctx* c;
  Arr arr[MAX];
  Buf* more[MAX_ALSO];
  size_t more_bytes[MAX_ALSO];
  int n = 0, n_also = 0;
};

// ---- the batched match sequence: defined in sc_capi_match_batch.hip but for the template, used by sc_capi_instances_batch.hip
// (the packed form) and sc_capi_pairs.hip (a pair is a problem, found through a record) as well
struct MatchBatchSizes {
  uint32_t n_problems, n_tiles;
  size_t total_s, total_t, slots;  // rows of fsrc, rows of ftgt, output entries (total_s * knn)
  BatchMetaLayout meta;            // the metadata of the form (sc_match_batch_check.hpp): its words, where the slot starts and the tile map sit
};
// The arrays every host form of a match declares, always these seven in this order (their slots are the same in every form): the
// descriptors and keypoints of both sides — NULL for what a form has not: a match alone has no keypoints, a pairs form one table
// (its rows in fsrc / psrc: one copy serves both sides) — and the three outputs of the match.
struct MatchBatchArrays { int fsrc, ftgt, psrc, ptgt, corr, d2, count; };
inline MatchBatchArrays mbatch_arrays(HostArrays& h, const MatchBatchSizes& sz, uint32_t dim, const float* fsrc, size_t src_rows, const float* ftgt,
                                      size_t tgt_rows, const float* psrc, const float* ptgt, int32_t* corr, float* d2, uint32_t* count) {
  MatchBatchArrays a;
  a.fsrc = h.in(fsrc, src_rows * dim * 4);
  a.ftgt = h.in(ftgt, tgt_rows * dim * 4);
  a.psrc = h.in(psrc, src_rows * 12);
  a.ptgt = h.in(ptgt, tgt_rows * 12);
  a.corr = h.out(corr, sz.slots * 8);
  a.d2 = h.out(d2, sz.slots * 4);
  a.count = h.out(count, (size_t)sz.n_problems * 8);
  return a;
}
// every refusal of a packed batched match; `p` only for a features entry, whose name for the messages is `features` (nullptr: the
// match alone).  Fills *job (but its pointers) and *sz.
int mbatch_check(sc_ctx* c, const uint32_t* src_off, const uint32_t* tgt_off, uint32_t n_problems, const sc_match_params* mp,
                 const sc_params* p, const char* features, MatchJob* job, MatchBatchSizes* sz);
// the workspace of the match itself (gather: and of the gathered points)
int mbatch_room(sc_ctx* c, const MatchJob& mj, const MatchBatchSizes& sz, bool gather);
// bytes of the "clean" words in front of the column minima in mbatch_words
inline size_t mbatch_clean_bytes(const MatchBatchSizes& sz) { return (((size_t)sz.n_problems + 1) / 2) * 8; }
// The staging copy, the memset and the two launches (mbatch_room has been called).  The form passes what is its own: `fill` writes
// sz.meta.words words of metadata into the staging area; `job` arrives with its inputs and with its pointers into mbatch_meta, but
// the tile map, set; its launch pair follows from its type.  Everything else of the job — the fields MatchBatchJob and MatchPairsJob
// share by name — is filled here.
template <class Job, class Fill>
int mbatch_enqueue(sc_ctx* c, const MatchJob& mj, const MatchBatchSizes& sz, Job job, Fill fill, int32_t* d_corr, float* d_d2, uint32_t* d_count,
                   const MatchGather& g) {
  const size_t meta_bytes = sz.meta.words * 4;
  SC_TRY(batch_staging_begin(c, meta_bytes));
  fill(static_cast<uint32_t*>(c->h_batch_off));
  SC_TRY(batch_staging_send(c, c->mbatch_meta, meta_bytes));
  const size_t clean_bytes = mbatch_clean_bytes(sz), words_bytes = clean_bytes + (mj.mutual ? sz.total_t * 8 : 0);
  HIPCHK(c, hipMemsetAsync(c->mbatch_words.p, 0xFF, words_bytes, c->stream));
  job.tile_map = c->mbatch_meta.as<uint32_t>() + sz.meta.map_at;
  job.n_problems = sz.n_problems; job.n_tiles = sz.n_tiles; job.dim = mj.dim; job.knn = mj.knn; job.kp = mj.r2 > 0.f ? 2u : mj.knn;
  job.mutual = mj.mutual; job.r2 = mj.r2;
  job.top = c->mbatch_top.as<uint64_t>();
  job.colmin = mj.mutual ? reinterpret_cast<uint64_t*>(static_cast<char*>(c->mbatch_words.p) + clean_bytes) : nullptr;
  job.clean = c->mbatch_words.as<uint32_t>();
  job.corr = d_corr; job.d2 = d_d2; job.count = d_count; job.g = g;
  launch_match_batch_dist(job, c->stream);
  launch_match_batch_finish(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}
// the packed form of it: both offset arrays, the slot starts and the tile map; MatchBatchJob and its launches.  A features entry
// passes its sc_params and the problems' points, for the gather into mbatch_gsrc / _gtgt (p == nullptr: the match alone)
int mbatch_enqueue_packed(sc_ctx* c, const MatchJob& mj, const MatchBatchSizes& sz, const float* d_fsrc, const float* d_ftgt,
                          const uint32_t* src_off, const uint32_t* tgt_off, int32_t* d_corr, float* d_d2, uint32_t* d_count,
                          const sc_params* p = nullptr, const float* d_src_pts = nullptr, const float* d_tgt_pts = nullptr);
// the registration kernel's argument on the slots the match filled (the gathered points, the slot starts), but for its outputs
BatchJob mbatch_slots_job(const sc_ctx* c, const MatchBatchSizes& sz, const sc_params* p);
// sc_batch.hip's kernel on those slots (the count pairs are the caller's)
int mbatch_register(sc_ctx* c, const MatchBatchSizes& sz, const sc_params* p, const uint32_t* d_count, sc_batch_result* d_res, uint8_t* d_mask);

// ---- defined in sc_capi_pairs.hip, used by the pairs entries of sc_capi_match_guided_batch.hip as well
// every refusal of a pairs entry; `p` only for the features entries, whose name for the messages is `features`.  Fills *job (but its
// pointers) and *sz (n_problems: the pairs; total_s / total_t: the source / target rows of all pairs).
int pairs_check(sc_ctx* c, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp,
                const sc_params* p, const char* features, MatchJob* job, MatchBatchSizes* sz);

// ---- defined in sc_capi_polish_batch.hip, used by sc_capi_pairs.hip as well
// sc_polish_params as a batch takes them (one candidate per problem); `who` opens the message
int pbatch_pparams_check(sc_ctx* c, const sc_polish_params* pp, const char* who);
// what the polish kernel reads of the two parameter blocks (the pointers are the caller's)
PolishBatchJob pbatch_job(const sc_params* p, const sc_polish_params* pp);

// ---- a call on a scored frame (sc_peel, sc_polish): what the two share in front of their launches and behind them
// The entry checks, `busy` first, then "is there a frame"; the refusal names the caller.  Then the context's device.
inline int scored_frame_begin(sc_ctx* c, const char* who) {
  SC_TRY(busy(c));
  if (!c->pass.peelable) {
    c->last_error = std::string(who) + ": no frame on this context (it follows an sc_register* call that returned SC_OK with shard_world == 1; any other computing call ends the frame)";
    return SC_EINVAL;
  }
  HIPCHK(c, hipSetDevice(c->device));
  return SC_OK;
}
// Behind the last launch: outputs complete on return with the private stream, stream-ordered with a caller's (as sc_register_device);
// then the winner's two host words (HW_WINNER, armed by the caller, and HW_WINNER_POS) are there.
inline int scored_frame_wait(sc_ctx* c) {
  if (c->pass.timing || !c->caller_stream) HIPCHK(c, hipStreamSynchronize(c->stream));
  SC_TRY(wait_word(c, HW_WINNER));
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}
// The caller's sc_stats: the frame's n, edges, tri_*; the winner's count and rank index; if the frame asked for SC_FLAG_TIMING, this call's
// brackets — events 0 - 1 us_stage, 1 - 2 us_score, 2 - 3 us_argmax (when last_ev == 4), last_ev - 1 .. last_ev us_mask; the others zero.
inline void scored_frame_stats(sc_ctx* c, sc_stats* stats, uint32_t best_count, uint32_t best_rank, int last_ev) {
  if (!stats || stats->size != sizeof(sc_stats)) return;
  fill_stats(c, stats);
  stats->best_count = best_count;
  stats->best_rank = best_rank;
  if (!c->pass.timing) return;
  stats->us_stage = ev_us(c, 0, 1);
  stats->us_score = ev_us(c, 1, 2);
  stats->us_argmax = last_ev == 4 ? ev_us(c, 2, 3) : 0.f;
  stats->us_mask = ev_us(c, last_ev - 1, last_ev);
  stats->us_compat = stats->us_triangles = stats->us_trikeys = stats->us_kabsch = 0.f;
  stats->us_total = stats->us_stage + stats->us_score + stats->us_argmax + stats->us_mask;
}

// the stage sequencers the stage hooks run one at a time (sc_capi_hooks.hip): stage A's three are defined in sc_capi_compat.hip,
// run_triangles in sc_capi_tri.hip
int stage_inputs(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p);
int run_compat(sc_ctx* c, bool dense);
int run_row_stats(sc_ctx* c, bool will_prune, bool hot = false);
inline bool may_prune(const sc_params* p) { return p->rank_mode == SC_RANK_WEIGHT && !(p->flags & SC_FLAG_NO_PRUNE); }
int run_triangles(sc_ctx* c, const sc_params* p, bool want_list);

// ---- stage B's host side: defined in sc_capi_tri.hip, called by sc_capi.hip (what each does is said at its definition).  SC_LOCAL:
// shared by the host files and no part of the library's dynamic symbol table.
#define SC_LOCAL __attribute__((visibility("hidden")))
SC_LOCAL int run_edges(sc_ctx* c, const sc_params* p, uint32_t* hist, uint32_t part, uint32_t parts);
SC_LOCAL int run_select(sc_ctx* c, const sc_params* p, const uint32_t* hist, bool want_list);
// the views of the context's stage-B arrays (sc_kernels.hpp): the one place each Buf becomes a typed pointer
SC_LOCAL EdgeList edges_of(const sc_ctx* c);
SC_LOCAL EdgeCounts counts_of(const sc_ctx* c);
SC_LOCAL KeyArrays keys_of(const sc_ctx* c);
SC_LOCAL Selection selection_of(const sc_ctx* c);
// ... and of the row arrays (defined in sc_capi_compat.hip; scan_degrees and graph_of use them too)
SC_LOCAL RowStats rows_of(const sc_ctx* c);
SC_LOCAL RowOffsets offsets_of(const sc_ctx* c);
SC_LOCAL int ensure_compaction(sc_ctx* c, size_t nb, size_t nb_room, uint32_t T_eff);
SC_LOCAL int run_compaction(sc_ctx* c, const KeyView& view, size_t nb, int rounds, uint64_t* host_short);
inline int select_rounds(bool window) { return window ? 2 : 3; }  // the a-priori window spares the round that measures the key range
SC_LOCAL bool window_known(const sc_params* p);
SC_LOCAL uint32_t select_want(const sc_ctx* c, const sc_params* p);
SC_LOCAL bool edge_build_ok(const sc_ctx* c, const sc_params* p, int64_t n, bool may_estimate);
SC_LOCAL int ensure_frame(sc_ctx* c);
// the pass in hand continues the shape of the last completed call
inline bool shape_continues(const sc_ctx* c) { return c->shape.continues(c->pass.n, &c->pass.params); }
// what a host-free frame assumes (one page of sc_capi_tri.hip): the plan, and what the completed call leaves (the validation at its
// end is sc_frame_check.hpp's hostfree_valid)
SC_LOCAL bool fast_plan(const sc_ctx* c, int64_t n, const sc_params* p, PassMode* mode);
SC_LOCAL bool hostfree_next_ok(const sc_ctx* c, bool regular);

// ---- a frame's end is sc_capi_frame.hip; what it calls of sc_capi.hip (what each does is said at its definition)
SC_LOCAL int frame_begin(sc_ctx* c);
SC_LOCAL int continue_pass(sc_ctx* c, bool in_order, const char* otherwise);
SC_LOCAL bool pass_end(sc_ctx* c);
SC_LOCAL int hyp_begin(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p, uint32_t* d_hist, uint32_t part,
                       uint32_t parts, const PassMode& mode);
SC_LOCAL int hyp_end(sc_ctx* c, const uint32_t* d_hist, uint64_t* d_key, sc_stats* stats);
SC_LOCAL TriSource tri_source_of(const sc_ctx* c);
struct CoordStats { uint64_t mx, box[6]; };
SC_LOCAL CoordStats read_coord_stats(const sc_ctx* c);
// stage brackets as (first event, second event): stage, compat, triangles, kabsch, score, argmax, mask
constexpr int STAGE_EV[7][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {7, 8}};
SC_LOCAL float ev_us_raw(sc_ctx* c, int a, int b);

int decide_filter(sc_ctx* c, const sc_params* p, const Shard& sh);
// the views of the context's stage-C arrays (sc_kernels.hpp; what each is taken behind is said at its definition)
SC_LOCAL Hyps hyps_of(const sc_ctx* c);
SC_LOCAL FilterBufs filter_of(const sc_ctx* c);
int run_score(sc_ctx* c, const sc_params* p, const Hyps& h, Partial* out, bool tile_done, const Stamps& ev);

}  // namespace sc
