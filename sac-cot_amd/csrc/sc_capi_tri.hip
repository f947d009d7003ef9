// sc_capi_tri.hip — stage B's host side: which of stage B's kernels (sc_tri_edges.hip, sc_tri_prune.hip, sc_tri.hip) a call runs, in what order, into which arrays.  Host-only, on
// the context (sc_ctx.hpp); sc_capi.hip's entries and the stage hooks call run_edges / run_select / run_triangles.
//
// Four jobs, each in its own place:
//   1. the FORM of the call (StageBForm, sc_ctx.hpp) is decided by form_begin / form_counted / form_select / form_keys — one function
//      per moment at which more is known — and read by everything else;
//   2. the arrays are grown by grow_edge_arrays / grow_key_arrays (+ ensure_compaction): "need now, room for the next host-free
//      call", and "an array that was re-allocated lost what the speculative launch wrote" (Caps);
//   3. the launches are one function per step; run_edges and run_select are the step lists, in launch order;
//   4. the two waits (read_edge_count, read_triangle_count) and the repairs of what ran speculatively follow them.
// What a host-free frame assumes is said once, at the end of the file.
#include <cmath>

#include "sc_ctx.hpp"
#include "sc_gramref.hpp"

namespace sc {

// ---- sizes and small answers ---------------------------------------------------------------------------------------------------

// entries the edge arrays hold (what fast_plan caps a host-free call's edge cover by)
static uint64_t edge_capacity(const sc_ctx* c, bool build) {
  uint64_t cap = c->es.cap / 4 >= 2 ? c->es.cap / 4 - 2 : 0;  // es carries two pad entries
  for (const Buf* b : {&c->ei, &c->ej}) cap = b->cap / 4 < cap ? b->cap / 4 : cap;
  if (!build) for (const Buf* b : {&c->ebi, &c->ebj}) cap = b->cap / 4 < cap ? b->cap / 4 : cap;
  return cap;
}

// The smallest key a triangle can have in weight ranking: every edge has s >= t_cmp up to rounding (0.1 % slack), so w >= ~3 t_cmp — what
// the select's a-priori window and the pruning samples' floors rest on.  NOT when -1 / (2 sigma^2) overflowed fp32 (sigma below 2^-64.5 =
// 3.8e-20): (d * d) * -inf is -inf or NaN, sc_expf clamps both to its floor, every weight is e^-87 and nothing bounds the keys from below
// (tests/test_gpu_range.py: the select then returned keys of its window, [2, 3], that no triangle has).
static float key_floor(const sc_params* p) {
  const float nis = (float)(-1.0 / (2.0 * (double)p->sigma * (double)p->sigma));  // derive()'s neg_inv2sig2
  return std::isfinite(nis) ? 3.0f * p->t_cmp * 0.999f : 0.0f;
}
// ... and whether that floor puts every key into the a-priori window [2, 3]: what the select, the estimating sample, the fused edge
// kernel and the host-free form all go by — one answer for all of them
// (weight keys of a graph whose edges all weigh >= 2/3 (0.1 % slack) lie in [2.0, 3.0]: window known a priori)
bool window_known(const sc_params* p) { return p->rank_mode == SC_RANK_WEIGHT && key_floor(p) >= 2.0f; }

static Graph graph_of(const sc_ctx* c) {
  const RowStats rs = rows_of(c);
  return Graph{c->pass.bits_cur, c->S.as<float>(), rs.deg, rs.degp, rs.wpre, c->pass.n, c->pass.ld, c->pass.ld >> 6};
}

// how many triangles stage B selects: T — or, when B is sharded, what one candidate blob holds (this rank's own best)
uint32_t select_want(const sc_ctx* c, const sc_params* p) {
  if (!c->pass.sharded_ab) return p->max_triangles;
  const uint32_t cap = (uint32_t)cand_cap(p->max_triangles, (uint32_t)p->shard_world, p->shard_cand_level);
  return cap < p->max_triangles ? cap : p->max_triangles;
}

// The views of the context's stage-B arrays (sc_kernels.hpp), as they stand NOW: taken again behind whatever grows an array.
// The edge list: E is c->pass.E (read_edge_count sets it); a host-free call's real count sits in edge_off[n]; the fused edge kernel
// writes no per-edge bases
EdgeList edges_of(const sc_ctx* c) {
  const StageBForm& f = c->pass.form;
  return EdgeList{c->ei.as<uint32_t>(), c->ej.as<uint32_t>(), c->es.as<float>(),
                  f.build ? nullptr : c->ebi.as<uint32_t>(), f.build ? nullptr : c->ebj.as<uint32_t>(), c->ebase.as<uint32_t>(),
                  c->pass.E, f.spec ? c->edge_off.as<uint64_t>() + c->pass.n : nullptr, f.spec ? c->shape.E_last : c->pass.E,
                  edge_capacity(c, f.build)};
}
// the per-edge counts; sharded stage B: the device-side edge range [lo, hi) this rank enumerates (nullptr: every edge)
EdgeCounts counts_of(const sc_ctx* c) {
  return EdgeCounts{c->tcnt.as<uint32_t>(), c->toff.as<uint64_t>(), c->pass.sharded_ab ? c->ctl.as<ControlBlock>()->own_edge : nullptr};
}
// the key arrays (cap: what fast_plan caps its key cover by, and the speculative key pass may write)
KeyArrays keys_of(const sc_ctx* c) {
  return KeyArrays{c->wkey.as<uint32_t>(), c->kcol.as<uint2>(), c->wkey.cap / 4 < c->kcol.cap / 8 ? c->wkey.cap / 4 : c->kcol.cap / 8,
                   c->blk_minmax.as<uint32_t>(), &c->ctl.as<ControlBlock>()->sel};
}
Selection selection_of(const sc_ctx* c) {
  return Selection{c->sel_ord.as<uint64_t>(), c->sel_key.as<uint32_t>(), c->sel_ord.cap / 8 < c->sel_key.cap / 4 ? c->sel_ord.cap / 8 : c->sel_key.cap / 4};
}
// what the pruning kernel writes (no strong list yet: prune() says which form)
static Pruned pruned_of(const sc_ctx* c) {
  ControlBlock* ctl = c->ctl.as<ControlBlock>();
  return Pruned{c->bits2.as<uint64_t>(), &ctl->smin, &ctl->klb, StrongList{nullptr, nullptr, 0u, 0u}};
}
// the host word of "the select found fewer keys above the pruning bound than it promised" (sharded: the merge's word says it)
// this rank's share of the rows, as either split writes it into the control block
static ShardCut cut_of(const sc_ctx* c, const sc_params* p) {
  ControlBlock* ctl = c->ctl.as<ControlBlock>();
  return ShardCut{(uint32_t)p->shard_rank, (uint32_t)p->shard_world, ctl->own_row, ctl->own_edge};
}
static uint64_t* select_short_word(sc_ctx* c) { return c->pass.sharded_ab ? nullptr : &c->pinned[HW_SELECT_SHORT]; }

// "Did any of these arrays move?"  An array that was re-allocated — for this call's count, or only for the ROOM the next calls
// want — has lost what the speculative launch wrote into it.  By CAPACITY, not by address: hipFree + hipMalloc hand the same
// address back often enough.
struct Caps {
  static constexpr int MAX = 5;
  const Buf* buf[MAX]; size_t cap[MAX]; int n = 0;
  void add(const Buf& b) { buf[n] = &b; cap[n++] = b.cap; }
  bool moved() const { for (int k = 0; k < n; k++) if (buf[k]->cap != cap[k]) return true; return false; }
};

// the Gram filter's frame (sc_gramref.hpp): 512 bytes per context
int ensure_frame(sc_ctx* c) {
  if (!c->fx_frame.p) {
    ENSURE(c, c->fx_frame, gram_frame_bytes());
    HIPCHK(c, hipMemsetAsync(c->fx_frame.p, 0, gram_frame_bytes(), c->stream));
  }
  return SC_OK;
}

// The hot path's fused form of row_stats_scan + edge_fill + the estimating sample (sc_tri_edges.hip 1'): where the pruning bound
// will be an estimate (the same conditions as form_begin's and form_counted's, minus what only the edge count decides) and the
// bit rows are short enough for the kernel.  hyp_begin asks — with "the whole sample, own histogram" (StageBForm::own_sample) —
// before stage A, and fast_plan, because the fused kernel writes no per-edge bases.
bool edge_build_ok(const sc_ctx* c, const sc_params* p, int64_t n, bool may_estimate) {
  return may_estimate && !c->est.failed && window_known(p) && may_prune(p) && !c->tn.no_events && !c->tn.no_estimate &&
         c->tn.sample_mode == 0 && !c->tn.no_edge_build && !c->tn.rows_unfused && edge_build_fits((int)n) &&  // (stage C may be dealt over ranks: shard_world)
         p->max_triangles != 0;
}

// ---- the form, first half ------------------------------------------------------------------------------------------------------

// What is known before anything is launched: how the call is enqueued, where its sample goes, who made the row offsets.
static int form_begin(sc_ctx* c, const sc_params* p, const uint32_t* hist, uint32_t parts) {
  StageBForm f{};
  f.build = c->pass.form.build;          // (hyp_begin's, or a stage hook's "no")
  f.ord_state = c->pass.form.ord_state;  // (run_select's: a call without edges never gets there, and sc_debug_last goes on showing the last one's)
  f.spec = c->pass.mode.host_free;
  f.own_sample = hist == nullptr && parts == 1;
  if (f.build && !f.own_sample) { c->last_error = "internal: the fused edge kernel was chosen for a call that shares its sample"; return SC_EHIP; }
  f.fused = c->pass.rows_fused || f.build;
  c->pass.rows_fused = false;
  // An ESTIMATED bound where the call can be repeated should the select find it too high (sc_tri_prune.hip 3c): the common
  // form only — event list, a-priori select window (the check rides the window's first round), the whole sample here
  // (sharded, SC_FLAG_EST_BOUND: every rank takes the WHOLE sample — it is cheaper than the latency of the all-reduce that
  // would sum the ranks' shares — and the merge of the candidates verifies the bound: sc_shard_score_device)
  f.est_local = c->pass.mode.may_estimate && !c->est.failed && f.own_sample && !c->pass.sharded_ab;
  f.est_shard = c->pass.sharded_ab && hist != nullptr && (p->flags & SC_FLAG_EST_BOUND) != 0;
  c->pass.form = f;
  return SC_OK;
}

// What the edge count decides (E: the count, or a host-free call's cover): pruning, the event path, the sample's plan.
static void form_counted(sc_ctx* c, const sc_params* p, const Graph& g, uint64_t E) {
  StageBForm& f = c->pass.form;
  // certified pruning (sc_tri_prune.hip 3b): weight ranking only; pointless on tiny graphs
  f.pruned = may_prune(p) && E >= 4096;
  // counting pass + event list (sc_tri.hip 2b) on the pruned graph; Tuning::no_events keeps the row-walking pair
  f.use_events = f.pruned && !c->tn.no_events;
  f.have_total = f.pruned && (p->flags & SC_FLAG_EXACT_TOTAL) != 0;  // statistics only: 3-cliques of the whole graph
  // the smallest possible weight is ~3 t_cmp (every edge has s >= t_cmp up to rounding); 0.1 % slack
  c->pass.plan = f.pruned ? sample_plan(p->max_triangles, (f.est_local || f.est_shard) && f.use_events && window_known(p), c->tn,
                                        f.spec ? c->shape.E_last : E, g.W)
                          : SamplePlan{false, 1u, p->max_triangles};
  f.est_active = c->pass.plan.estimate;
}

// ---- run_edges' steps ----------------------------------------------------------------------------------------------------------

// The scan of deg+ -> edge_off (and the per-row CSR bases edge_fill reads), unless a fused kernel made them; sharded: also the
// prefix of the per-row work estimate and, from it, this rank's contiguous row / edge range.
// read-back #1: the scan kernel itself writes the edge count to host-pinned memory (no copy kernel)
static int scan_degrees(sc_ctx* c, const sc_params* p) {
  const StageBForm& f = c->pass.form;
  const size_t n = c->pass.n;
  hipStream_t st = c->stream;
  ENSURE(c, c->edge_off, (n + 1) * sizeof(uint64_t));
  ENSURE(c, c->scan_tmp, scan_temp_bytes(n));
  if (!f.fused || f.build) arm_word(c, HW_EDGES);
  ENSURE(c, c->ebase, n * 4);
  if (c->pass.sharded_ab) ENSURE(c, c->cost_pre, (n + 1) * sizeof(uint64_t));  // (sharded) the prefix of the per-row work estimate
  const RowStats rs = rows_of(c);
  const RowOffsets ro = offsets_of(c);
  const ScanWork work{c->scan_tmp.p, c->tn};
  ScanExtra xe;  // the scan of deg+ also writes the per-row CSR bases edge_fill reads
  xe.deg = rs.deg; xe.degp = rs.degp; xe.ebase = ro.ebase; xe.host_total = &c->pinned[HW_EDGES];
  ScanExtra xc;  // (sharded) the scan of the row costs
  if (!f.fused && scan_writes_ebase(n)) {  // tiled scans: the single-pass form, each on its own half of the state area
    const size_t half = scan_temp_bytes(n);
    SC_TRY(lb_next(c, 2 * half, 0, 0, &xe.lb));
    if (c->pass.sharded_ab) SC_TRY(lb_next(c, 2 * half, 1, half, &xc.lb));  // (same size: the area stays)
  }
  if (c->pass.sharded_ab) {
    // also the prefix of the per-row work estimate and, from it, this rank's contiguous row / edge range
    if (!f.fused)
      launch_scan_u32_pair(work, ScanJob{rs.degp, ro.edge_off, xe}, ScanJob{c->rowcost.as<uint32_t>(), ro.cost_pre, xc}, n, st);
    launch_shard_split(ro, cut_of(c, p), c->pass.n, st);
  } else if (!f.fused) {
    launch_scan_u32(work, rs.degp, n, ro.edge_off, xe, st);
  }
  return SC_OK;
}

// The edge list, into arrays that hold el.cap entries (writes beyond are dropped by the kernel).  The fused kernel also makes the
// row statistics and the count itself.
// the weight histogram of the heaviest-edge pruning sample is collected by the same kernel (sc_debug.sample_mode = ...
// any: it costs edge_fill ~1 us and saves a launch whenever that sample is chosen)
static void fill_edges(sc_ctx* c, const Graph& g, const EdgeList& el) {
  const StageBForm& f = c->pass.form;
  ControlBlock* ctl = c->ctl.as<ControlBlock>();
  if (f.build)  // (the count: to the host that waits for it, or — host-free — as the range the scan of the counts stops at)
    launch_edge_build(g, points_of(c), c->pass.dv, c->bits2.as<uint64_t>(), c->edge_off.as<uint64_t>(), el,
                      f.spec ? nullptr : &c->pinned[HW_EDGES], f.spec ? ctl->live_edges : nullptr, c->stream);
  else
    launch_edge_fill(g, points_of(c), c->pass.dv, c->edge_off.as<uint64_t>(), el, f.fused || scan_writes_ebase((size_t)c->pass.n),
                     ctl->es_hist, c->stream);
}

// The first wait.  Host-free call (fast_plan() made sure E_cov <= the arrays' capacity): no wait.  E is then what the launches and
// arrays COVER; the kernels take the real count from edge_off[n] (EdgeList::E_dev) and the end of the call validates it.
// Sets c->pass.E, the form's second part, and "nothing yet" for what run_select delivers.
static int read_edge_count(sc_ctx* c, const sc_params* p, const Graph& g, uint32_t* hist) {
  const bool spec = c->pass.form.spec;
  if (!spec) {
    SC_TRY(wait_word(c, HW_EDGES));
    if ((uint32_t)c->pinned[HW_BAD_INPUT] != 0) { c->last_error = "non-finite input coordinate"; return SC_EINVAL; }
  }
  const uint64_t E = c->pass.E = spec ? c->pass.mode.E_cov : c->pinned[HW_EDGES];
  c->pass.M = 0; c->pass.M_total = 0; c->pass.T_eff = 0; c->pass.est_void = false;
  form_counted(c, p, g, E);
  c->pinned[HW_SELECT_SHORT] = 0;  // "the select found fewer keys above the pruning bound than it promised" (select_round_kernel)
  // an exchanged histogram is written on every path (zeros where no sample runs: the control block's copies are zero)
  if (hist && !c->pass.form.pruned) launch_hist_reduce(c->ctl.as<ControlBlock>()->prune_hist, hist, c->stream);
  // edge ids, CSR bases and the strong list are u32 (include/saccot.h, limits): a graph beyond that is refused, not wrapped
  if (E >= (1ull << 32)) { c->last_error = "the compatibility graph has 2^32 or more edges"; return SC_ETOOMANY; }
  return SC_OK;
}

// Every array indexed by the edge count: E entries now, and on a waited call room for the next host-free ones.  *moved: an edge
// array was re-allocated (Caps) — what the speculative fill wrote is gone.
static int grow_edge_arrays(sc_ctx* c, uint64_t E, bool* moved) {
  const StageBForm& f = c->pass.form;
  // (a waited call leaves room for what a host-free repetition of its shape will want to cover: fast_plan caps by these arrays)
  const uint64_t E_room = f.spec ? E : c->shape.room(E, ShapeHistory::EDGES, shape_continues(c));
  Caps edge_arrays;
  edge_arrays.add(c->ei); edge_arrays.add(c->ej); edge_arrays.add(c->es);
  if (!f.build) { edge_arrays.add(c->ebi); edge_arrays.add(c->ebj); }
  ENSURE_ROOM(c, c->ei, E * 4, E_room * 4);
  ENSURE_ROOM(c, c->ej, E * 4, E_room * 4);
  ENSURE_ROOM(c, c->es, (E + 2) * 4, (E_room + 2) * 4);  // +1: the 4-way unrolled gathers of idle slots may touch index E
  if (!f.build) { ENSURE_ROOM(c, c->ebi, E * 4, E_room * 4); ENSURE_ROOM(c, c->ebj, E * 4, E_room * 4); }
  // every other array indexed by the edge count gets room for whatever the edge arrays can hold — that is what fast_plan caps a
  // host-free call's cover by, so no such call ever has to grow one of them (a re-allocation synchronises the stream: 0.35 ms in
  // the middle of bench.py's stream, once per array and rise of the cover)
  const uint64_t E_hold = f.spec ? E : edge_capacity(c, f.build);
  ENSURE_ROOM(c, c->tcnt, E * 4, E_hold * 4);
  ENSURE_ROOM(c, c->toff, (E + 1) * 8, (E_hold + 1) * 8);
  ENSURE_ROOM(c, c->scan_tmp, scan_temp_bytes(E), scan_temp_bytes(E_hold));
  if (!f.spec) {
    ENSURE_ROOM(c, c->strong, strong_list_bytes(E), strong_list_bytes(E_hold));
    ENSURE_ROOM(c, c->lb_state, scan_temp_bytes(E), 2 * scan_temp_bytes(E_hold));
  }
  *moved = edge_arrays.moved();
  return SC_OK;
}

// The pruning sample — this process's share (`part` of `parts`), or the whole of it — into the control block's histogram, and from
// there into `hist` where the histogram is exchanged; before it, where asked for, the exact count of the whole graph's 3-cliques.
static int run_sample(sc_ctx* c, const sc_params* p, const Graph& g, const EdgeList& el, uint32_t* hist, uint32_t part, uint32_t parts) {
  const StageBForm& f = c->pass.form;
  if (!f.pruned) return SC_OK;
  hipStream_t st = c->stream;
  ControlBlock* ctl = c->ctl.as<ControlBlock>();
  if (f.have_total) {  // the whole graph, every rank's edges
    EdgeCounts all = counts_of(c);
    all.own = nullptr;
    launch_tri_count(g, Pruned{}, el, all, c->tn, st);
    ScanExtra xt;
    xt.host_total = &c->pinned[HW_TOTAL];
    launch_scan_u32(ScanWork{c->scan_tmp.p, c->tn}, all.tcnt, el.E, all.toff, xt, st);
  }
  if (f.build && !f.est_active) { c->last_error = "internal: the fused edge kernel ran but the bound is not an estimate"; return SC_EHIP; }
  if (f.est_active) {
    // an estimating sample (the single-GPU hot path; sharded, SC_FLAG_EST_BOUND: every rank takes the whole of it), inlier count, a call
    // big enough for stage C2's Gram filter to be in question: the sample also
    // leaves its workgroups' best triangles behind — the voters of that filter's reference frame (count_triangles passes them on)
    SampleCands cands;
    if ((f.est_local || f.est_shard) && p->score_mode == 0 && c->tn.score_filter != 1 && c->tn.score_filter != 2 && !c->tn.gram_ref_late &&
        (uint64_t)p->max_triangles * (uint64_t)c->pass.n >= (1ull << 27)) {
      if (!c->ref_cand.p) {
        ENSURE(c, c->ref_cand, 4096 * sizeof(uint4));
        HIPCHK(c, hipMemsetAsync(c->ref_cand.p, 0, 4096 * sizeof(uint4), st));
      }
      cands = SampleCands{c->ref_cand.as<uint4>(), ctl->ref_slot};
      c->pass.ref_cand_n = sample_candidate_blocks(el.E, c->tn);
    }
    launch_sample_estimate(g, el, c->pass.plan.rate, ctl->prune_hist, cands, c->tn, st);
  } else {
    // SC_FLAG_EST_BOUND on the phase API where the plan is NOT an estimate (select window unknown: t_cmp below ~0.668; sc_debug's
    // no_events / no_estimate / sample_mode): the caller still skips the histogram all-reduce, so every rank must end up with the
    // SAME histogram — each takes the WHOLE certifying sample, not its share (with shares the ranks derived different
    // bounds, cut the strong list differently, and the merged top-T could miss triangles)
    const bool whole = f.est_shard;
    launch_sample_hist(g, el, p->max_triangles, key_floor(p), whole ? 0u : part, whole ? 1u : parts, ctl->prune_hist, ctl->es_hist,
                       c->tn, st);
  }
  if (hist) launch_hist_reduce(ctl->prune_hist, hist, st);  // the exchanged form: one 256-bin histogram
  return SC_OK;
}

// Stage B, first half: CSR edge list and this process's share (`part` of `parts`) of the pruning sample, accumulated
// into `hist` (256 u32 on the device, already zero; nullptr = the control block's own histogram).  Sets c->pass.E and the
// decisions the second half needs (c->pass.form).
int run_edges(sc_ctx* c, const sc_params* p, uint32_t* hist, uint32_t part, uint32_t parts) {
  c->pass.ref_cand_n = 0; c->pass.ref_done = false;
  SC_TRY(form_begin(c, p, hist, parts));
  const StageBForm& f = c->pass.form;
  SC_TRY(scan_degrees(c, p));
  // While the host polls for the edge count, edge_fill already runs into the edge arrays this context holds from
  // earlier calls (it needs no host-side count: one wave per row, offsets from the scan).  Writes beyond their
  // capacity are dropped by the kernel; in that case, or on a first call, it runs (again) after the read-back.
  const Graph g = graph_of(c);
  const uint64_t spec_cap = edge_capacity(c, f.build);
  if (spec_cap || f.build) fill_edges(c, g, edges_of(c));  // (the fused kernel also makes the row statistics and the count itself)
  SC_TRY(read_edge_count(c, p, g, hist));
  const uint64_t E = c->pass.E;
  if (E == 0) return SC_OK;
  bool edge_arrays_moved = false;
  SC_TRY(grow_edge_arrays(c, E, &edge_arrays_moved));
  const EdgeList el = edges_of(c);  // (the count is known, the arrays hold it)
  if (E > spec_cap || edge_arrays_moved) {  // first call, or the graph outgrew the arrays (just re-allocated above)
    if (spec_cap && !f.build)  // the partial run's counts
      HIPCHK(c, hipMemsetAsync(c->ctl.as<ControlBlock>()->es_hist, 0, sizeof(uint32_t) * PR_HCOPIES * 256, c->stream));
    fill_edges(c, g, el);
  }
  return run_sample(c, p, g, el, hist, part, parts);
}

// ---- the form, second half -----------------------------------------------------------------------------------------------------

// What run_select decides before its first launch; E is known (run_edges).
static int form_select(sc_ctx* c, const sc_params* p, const uint32_t* hist) {
  StageBForm& f = c->pass.form;
  const uint64_t E = c->pass.E;
  if ((hist == nullptr) != f.own_sample) { c->last_error = "internal: the select was handed another histogram than the edges' sample went into"; return SC_EHIP; }
  // The key kernel runs speculatively in the common form only — events, a-priori select window — and not when every stage
  // is bracketed by events; spec_cap: the keys the arrays of the earlier calls hold (0: none yet, no speculative pass).
  f.spec_cap = 0;
  if (f.use_events && window_known(p) && !c->pass.timing)
    f.spec_cap = f.spec ? c->pass.mode.M_cov : keys_of(c).cap;  // (M_cov <= that capacity: fast_plan)
  // Exactly those calls, on one rank, take their ordinals from an ORDERED strong list (sc_tri.hip
  // 2c): no scan of the per-edge counts, the key kernel leaves the triangle count where the scan would.  While the pruning kernel's
  // grid stays within what a workgroup's prologue sums (C3 does not), and until a call's list had more chunks than the key kernel
  // holds (sc_ctx::ord_off); sc_debug.scan_ordinals keeps the scan.
  f.ord_on = f.spec_cap != 0 && !c->pass.sharded_ab && f.own_sample && p->shard_world == 1 &&
             !c->tn.scan_ordinals && !c->ord_off && (E + ORD_BLOCK_EDGES - 1) / ORD_BLOCK_EDGES <= ORD_MAX_BLOCKS;
  f.ord_state = f.ord_on ? 1 : 0;
  // Sharded (event path): the ranks' row ranges are cut AFTER the certificate, by the work of the pruned graph (VERDICT r02
  // #5: a correspondence list in keypoint order puts nearly every strong edge into a few rows).  Every rank holds the
  // whole strong matrix, so every rank computes the same cut: the pruning kernel lists EVERY strong edge, two small
  // launches make the cut, and the counting pass skips the edges of the other ranks.
  f.recut = f.pruned && c->pass.sharded_ab && p->shard_world > 1 && f.use_events;
  // a host-free call on the fused edge kernel: the launches cover E edges, the graph has fewer — the pruning kernel's workgroups
  // beyond them leave without writing their counts, and the scan skips those tiles (counts_range)
  f.trimmed = f.spec && f.build && !c->pass.sharded_ab;
  return SC_OK;
}

// What the triangle count decides: whether the event list stands, which window the select takes, whether the speculative key pass
// already wrote every key.  key_arrays_moved: grow_key_arrays re-allocated one (what that pass wrote is gone).
static void form_keys(sc_ctx* c, const sc_params* p, uint64_t M, bool key_arrays_moved) {
  StageBForm& f = c->pass.form;
  // a region overflowed: this call walks the rows again
  f.events_ok = f.use_events && !(!f.spec && (uint32_t)c->pinned[HW_EV_OVERFLOW] != 0);
  // weight keys of a graph whose edges all weigh >= 2/3 (0.1 % slack) lie in [2.0, 3.0]: window known a priori
  f.fast_window = f.events_ok && window_known(p);
  f.keys_done = f.spec_cap != 0 && f.events_ok && M <= f.spec_cap && !key_arrays_moved;  // the speculative pass wrote every key
}

// ---- run_select's steps --------------------------------------------------------------------------------------------------------

// what the steps hand on to each other
struct SelectArgs {
  Graph g;
  EdgeList el;       // (E = el.E: the count, or a host-free call's cover)
  EdgeCounts cnt;
  Pruned pr{};       // the bit rows the counting pass walks and the weight bound: none until prune() has pruned
  OrdList ord{};
  EventList ev{};
  ScanExtra xr;                     // the range of the scan of the per-edge counts (counts_range)
  int chunk_shift = 0;              // an OrdList's chunk: the positions a workgroup of the counting pass takes per trip
};

// Prune with the (summed) sample histogram: the strong bit rows, the strong list — ordered where the ordinals come from it — and,
// sharded, the second cut of the ranks' ranges.
static int prune(sc_ctx* c, const sc_params* p, const uint32_t* hist, SelectArgs& a) {
  const StageBForm& f = c->pass.form;
  if (!f.pruned) return SC_OK;
  const uint64_t E = a.el.E;
  hipStream_t st = c->stream;
  ControlBlock* ctl = c->ctl.as<ControlBlock>();
  a.pr = pruned_of(c);
  if (f.use_events) {  // the pruning kernel also compacts the strong edges for the counting pass
    ENSURE(c, c->strong, strong_list_bytes(E));  // (a waited call: run_edges left room)
    ENSURE(c, c->ord_cnt, ORD_MAX_BLOCKS * sizeof(uint32_t));  // (by every call of the event path: a host-free one finds it)
    a.pr.sl = StrongList{c->strong.as<uint32_t>(), ctl->st_fill, strong_list_cap(E), 0u};
  }
  if (f.ord_on) {
    // tloc and ctot live where the scan's offsets would: toff holds 2 E + 2 words, tloc takes E of them, ctot at most E / 4 + 4
    // from the next multiple of four (E >= 4096), and the count lands in toff[E] as ever
    uint32_t* words = a.cnt.words();
    a.ord.cnt = c->ord_cnt.as<uint32_t>(); a.ord.tloc = words; a.ord.ctot = words + ((E + 3) & ~(uint64_t)3);
    a.ord.n_strong = &ctl->n_strong; a.ord.total = a.cnt.toff + E; a.ord.E = E; a.ord.E_dev = a.el.E_dev;
    a.ord.chunk_max = c->tn.ord_chunk_max && c->tn.ord_chunk_max < ORD_CHUNK_MAX ? c->tn.ord_chunk_max : ORD_CHUNK_MAX;
    a.pr.sl.cnt = a.ord.cnt;
  }
  // contiguous regions: a rank walks only the regions its own edge range touches (unsharded the modulo form stays: the
  // counting pass is no faster with contiguous regions at C2 / C4 and 20 us slower at C3)
  if (f.recut) a.pr.sl.region_blocks = a.pr.sl.cap / 256;
  EdgeCounts listed = a.cnt;  // (recut: EVERY rank's strong edges are listed — the cut comes behind the list)
  if (f.recut) listed.own = nullptr;
  PruneOpts po;
  po.logbins = f.est_active; po.trimmed = f.trimmed;
  launch_prune_bits(a.g, f.own_sample ? ctl->prune_hist : hist, f.own_sample, a.el,
                    f.est_active ? c->pass.plan.hist_want : (uint64_t)p->max_triangles, key_floor(p), a.pr, listed, po, st);
  if (f.recut) {
    ENSURE(c, c->rowcost, ((size_t)c->pass.n + 4 + 1024) * 4);  // (cost_split_kernel reads whole 16-byte pieces)
    launch_strong_rowcost(a.g, a.pr, c->rowcost.as<uint32_t>(), st);
    launch_cost_split(offsets_of(c), cut_of(c, p), c->rowcost.as<uint32_t>(), c->pass.n, st);
  }
  return SC_OK;
}

// The counting pass: per-edge triangle counts — with the event list, and under the same launch the vote for stage C2's reference
// frame, or walking the rows.
static int count_triangles(sc_ctx* c, const sc_params* p, SelectArgs& a) {
  const StageBForm& f = c->pass.form;
  hipStream_t st = c->stream;
  if (!f.use_events) {
    launch_tri_count(a.g, a.pr, a.el, a.cnt, c->tn, st);
    return SC_OK;
  }
  // Tuning::event_cap (test hook) forces a (too) small buffer for THIS call without touching the context's own
  // capacity, which only grows (after an overflow)
  const uint64_t ev_cap = c->tn.event_cap >= 256 ? c->tn.event_cap : c->ev_capacity;
  ENSURE(c, c->events, event_bytes(ev_cap));
  c->pinned[HW_EV_OVERFLOW] = 0;
  a.ev = event_list(c->events.p, ev_cap, a.g.W, c->ctl.as<ControlBlock>()->ev_fill,
                    reinterpret_cast<uint32_t*>(&c->pinned[HW_EV_OVERFLOW]));
  GramRefJob ref{};
  if (c->pass.ref_cand_n) {  // (run_sample) one extra workgroup votes for stage C2's reference frame under this launch
    SC_TRY(ensure_frame(c));
    ref = gram_ref_job(points_of(c), filter_of(c), c->pass.dv.tau2, c->tn);  // (reads the statistics and the frame only: the plan and the other buffers are stage C's to make)
    ref.src.cand = c->ref_cand.as<uint4>(); ref.src.n_cand = c->pass.ref_cand_n; ref.src.cand_slot = c->ctl.as<ControlBlock>()->ref_slot;
    c->pass.ref_done = true;
  }
  launch_tri_count_events(a.g, a.pr, a.el, a.cnt, p->rank_mode, a.ev, a.ord, ref.out ? &ref : nullptr, c->tn, st);
  return SC_OK;
}

// the edges whose counts the scan reads.  sharded: the counts outside this rank's edge range are zero — their tiles are skipped;
// trimmed (form_select): the tiles beyond the real edges
static void counts_range(sc_ctx* c, SelectArgs& a) {
  a.xr.range = c->pass.form.trimmed ? c->ctl.as<ControlBlock>()->live_edges : a.cnt.own;
}

// read-back #2: triangle count (of the pruned graph when pruning), written to pinned memory by the scan of the per-edge counts ->
// toff (host-free: not written, the kernels read toff[E])
static int scan_counts(sc_ctx* c, SelectArgs& a) {
  arm_word(c, HW_TRIANGLES);
  SC_TRY(lb_next(c, scan_temp_bytes(a.el.E), 0, 0, &a.xr.lb));
  a.xr.host_total = c->pass.form.spec ? nullptr : &c->pinned[HW_TRIANGLES];
  launch_scan_u32(ScanWork{c->scan_tmp.p, c->tn}, a.cnt.tcnt, a.el.E, a.cnt.toff, a.xr, c->stream);
  return SC_OK;
}

// The key pass over the event list, into the key arrays as they stand (writes beyond what they hold are dropped); want / window:
// what the select's first round is told (window: the a-priori one); host_count: the pinned word that receives the triangle count,
// as the scan's would.
static void key_pass(sc_ctx* c, const sc_params* p, const SelectArgs& a, uint64_t want, bool window, uint64_t* host_count) {
  KeyPassOpts o;
  o.window = window; o.check_bound = !c->pass.sharded_ab; o.chunk_shift = a.chunk_shift; o.host_total = host_count;
  launch_tri_keys_events(a.g, a.pr, a.el, a.cnt, p->rank_mode, a.ev, a.ord, keys_of(c), want, o, c->tn, c->stream);
}

// The second wait.  Host-free call: none — M is what the key arrays and the launches cover, T_eff the requested T; the kernels
// read the real count from toff[E] (= the scan's total: the counts of [real E, E) are zero) and sc_wait validates.  Sets
// c->pass.M and M_total.
static int read_triangle_count(sc_ctx* c, SelectArgs& a) {
  StageBForm& f = c->pass.form;
  if (!f.spec) SC_TRY(wait_word(c, HW_TRIANGLES));
  if (f.ord_on && !f.spec && (uint32_t)c->pinned[HW_EV_OVERFLOW] != 0) {
    // an event region was full, or the list has more chunks than the key kernel holds: the row-walking key kernel needs toff —
    // the scan runs after all, here and only here, over counts whose weak entries nobody has written yet
    launch_zero_weak_counts(a.el, a.pr, a.cnt, c->stream);
    SC_TRY(scan_counts(c, a));
    SC_TRY(wait_word(c, HW_TRIANGLES));
    f.ord_state = 2;
    if (chunk_overflow(c)) c->ord_off = true;
  }
  c->pass.M_total = f.spec ? c->pass.mode.M_cov : (f.have_total ? c->pinned[HW_TOTAL] : c->pinned[HW_TRIANGLES]);
  c->pass.M = f.spec ? c->pass.mode.M_cov : c->pinned[HW_TRIANGLES];
  return SC_OK;
}

// The compaction's buffers: nb tiles now, room for nb_room (a caller without the room rule passes nb); the selection's T_eff entries.
int ensure_compaction(sc_ctx* c, size_t nb, size_t nb_room, uint32_t T_eff) {
  ENSURE_ROOM(c, c->blk_gt, nb * 4, nb_room * 4);
  ENSURE_ROOM(c, c->blk_eq, nb * 4, nb_room * 4);
  ENSURE_ROOM(c, c->off_gt, (nb + 1) * 8, (nb_room + 1) * 8);
  ENSURE_ROOM(c, c->off_eq, (nb + 1) * 8, (nb_room + 1) * 8);
  ENSURE(c, c->scan_tmp, scan_temp_bytes(nb));
  ENSURE(c, c->sel_ord, (size_t)T_eff * 8);
  ENSURE(c, c->sel_key, (size_t)T_eff * 4);
  return SC_OK;
}

// Every array indexed by the triangle count: M keys now, and on a waited call room for the next host-free ones; the compaction's
// buffers for whatever the key arrays can hold (fast_plan's cap).  *moved: a key array was re-allocated (Caps) — what the
// speculative key pass wrote is gone.
static int grow_key_arrays(sc_ctx* c, uint64_t M, uint32_t T_eff, bool want_list, bool* moved) {
  const bool spec = c->pass.form.spec;
  const uint64_t M_room = spec ? M : c->shape.room(M, ShapeHistory::KEYS, shape_continues(c));
  Caps key_arrays;
  key_arrays.add(c->wkey); key_arrays.add(c->kcol);
  ENSURE_ROOM(c, c->wkey, M * 4, M_room * 4);
  ENSURE_ROOM(c, c->kcol, M * 8, M_room * 8);
  *moved = key_arrays.moved();
  ENSURE(c, c->blk_minmax, 2 * 8192 * 4);
  SC_TRY(ensure_compaction(c, compact_blocks(M), compact_blocks(spec ? M : keys_of(c).cap), T_eff));
  if (want_list) ENSURE(c, c->tri, (size_t)T_eff * 12);
  return SC_OK;
}

// Ordinal-order compaction of the keys at or above the threshold the select found -> sel_ord / sel_key.
// Two launches (count per tile; write, every tile summing the counts before it by itself).  (The ONE-launch form — counts of the
// earlier tiles by decoupled look-back — was built as VERDICT r01 asked, bit-exact and slower: 16.4 us against 4.7 + 4.7 on C2;
// removed in r05.)  Tuning::compact_self_max == 0 (a test) takes the scanned three-launch form.
int run_compaction(sc_ctx* c, const KeyView& view, size_t nb, int rounds, uint64_t* host_short) {
  hipStream_t st = c->stream;
  SelectState* sel = &c->ctl.as<ControlBlock>()->sel;
  launch_compact_count(view, sel, rounds, c->blk_gt.as<uint32_t>(), c->blk_eq.as<uint32_t>(), host_short, st);
  // few tiles (and M < 2^32): compact_write adds up the tile counts itself, no scan launch in between
  const bool self_off = nb <= c->tn.compact_self_max && view.M < (1ull << 32);
  if (!self_off)
    launch_scan_u32_pair(ScanWork{c->scan_tmp.p, c->tn}, ScanJob{c->blk_gt.as<uint32_t>(), c->off_gt.as<uint64_t>()},
                         ScanJob{c->blk_eq.as<uint32_t>(), c->off_eq.as<uint64_t>()}, nb, st);
  launch_compact_write(view, sel, c->blk_gt.as<uint32_t>(), c->blk_eq.as<uint32_t>(),
                       self_off ? nullptr : c->off_gt.as<uint64_t>(), self_off ? nullptr : c->off_eq.as<uint64_t>(), selection_of(c), st);
  return SC_OK;
}

// A region overflowed (not: too many chunks of an ordered strong list — a larger event buffer would not help): the next call's
// event buffer is larger
static void grow_event_capacity(sc_ctx* c, uint64_t M) {
  if (chunk_overflow(c)) return;
  uint64_t want_cap = c->ev_capacity * 2;          // every event holds >= 1 triangle, so M bounds the need
  if (want_cap < M + M / 4) want_cap = M + M / 4;
  if (want_cap > (1ull << 28)) want_cap = 1ull << 28;
  c->ev_capacity = want_cap;
}

// Every key into wkey / kcol, now that the count is known and the arrays hold it: nothing where the speculative pass wrote them
// all, the key pass again, or — after an event overflow — the row-walking kernel.  SC_FLAG_TIMING brackets it (events 9, 10).
static int write_keys(sc_ctx* c, const sc_params* p, const SelectArgs& a) {
  const StageBForm& f = c->pass.form;
  if (c->pass.timing) HIPCHK(c, hipEventRecord(c->ev[9], c->stream));
  if (f.keys_done) {
    // nothing to do
  } else if (f.events_ok) {  // (ord_on: no overflow here, the lists of the counting pass stand)
    key_pass(c, p, a, f.fast_window ? (uint64_t)select_want(c, p) : (uint64_t)c->pass.T_eff, f.fast_window, nullptr);
  } else {
    launch_tri_keys(a.g, a.pr, a.el, a.cnt, p->rank_mode, keys_of(c), c->pass.T_eff, c->tn, c->stream);
  }
  if (c->pass.timing) HIPCHK(c, hipEventRecord(c->ev[10], c->stream));
  c->pass.timed_trikeys = c->pass.timing;
  return SC_OK;
}

// The exact threshold key, then the keys at or above it in ordinal order -> sel_ord / sel_key
static int select_and_compact(sc_ctx* c, uint64_t M, const SelectArgs& a) {
  const StageBForm& f = c->pass.form;
  const KeyArrays ka = keys_of(c);
  KeyView view = plain_view(ka.wkey, M);
  if (f.spec) view.M_dev = a.cnt.toff + a.el.E;
  // an estimated bound is verified by the first round over the a-priori window; any other path leaves it unverified
  if (f.est_active && !f.fast_window) c->pass.est_void = true;
  launch_select_rounds(view, ka.sel, select_rounds(f.fast_window), select_short_word(c), c->tn, c->stream);
  return run_compaction(c, view, compact_blocks(M), select_rounds(f.fast_window), select_short_word(c));
}

static bool hostfree_form_met(const sc_ctx* c, uint64_t M, uint32_t want_sel);

// Stage B, second half: prune with the (summed) sample histogram, enumerate, select.  On return c->pass.M, c->pass.T_eff are set
// and sel_ord / sel_key hold the selection.  want_list: also materialise the T x 3 triangle list (stage hook; the hot
// path reads triangles through TriSource).  hist == nullptr: the control block's own histogram — as run_edges was told.
int run_select(sc_ctx* c, const sc_params* p, const uint32_t* hist, bool want_list) {
  const uint64_t E = c->pass.E;  // (host-free call: the cover, the real count sits in edge_off[n] — see read_edge_count)
  if (E == 0) return SC_OK;
  SC_TRY(form_select(c, p, hist));
  const StageBForm& f = c->pass.form;
  SelectArgs a;
  a.g = graph_of(c); a.el = edges_of(c); a.cnt = counts_of(c);  // (run_edges grew them: they stay where they are — `held` below)
  Caps held;
  held.add(c->ei); held.add(c->ej); held.add(c->es); held.add(c->tcnt); held.add(c->toff);
  SC_TRY(prune(c, p, hist, a));
  SC_TRY(count_triangles(c, p, a));
  counts_range(c, a);
  // (ordered strong list: the count comes from the key kernel, which makes the ordinals without a scan)
  if (f.ord_on) arm_word(c, HW_TRIANGLES);
  else SC_TRY(scan_counts(c, a));
  // While the host polls for the count, the key kernel already runs into the key arrays this context holds from earlier
  // calls (it takes everything else from device memory); re-run below if the count outgrew the arrays or a region overflowed.
  while ((256 >> a.chunk_shift) > tri_count_events_lanes(a.g, c->tn)) a.chunk_shift++;
  if (f.spec_cap) {
    ENSURE(c, c->blk_minmax, 2 * 8192 * 4);
    key_pass(c, p, a, select_want(c, p), true, (f.ord_on && !f.spec) ? &c->pinned[HW_TRIANGLES] : nullptr);
  }
  SC_TRY(read_triangle_count(c, a));
  const uint64_t M = c->pass.M;
  if (M == 0) {
    // no triangle in the pruned graph: under a CERTIFIED bound (or none) the graph has none; an ESTIMATED bound has verified nothing
    // (the select that checks it never runs): the call is repeated with a certifying sample (finalize_wait)
    if (f.est_active) c->pass.est_void = true;
    return SC_OK;
  }
  const uint32_t want_sel = select_want(c, p);
  const uint32_t T_eff = c->pass.T_eff = (uint32_t)(M < want_sel ? M : want_sel);
  if (M * 12 > c->cap_bytes) { c->last_error = "triangle keys exceed the workspace cap"; return SC_ETOOMANY; }
  bool key_arrays_moved = false;
  SC_TRY(grow_key_arrays(c, M, T_eff, want_list, &key_arrays_moved));
  form_keys(c, p, M, key_arrays_moved);
  if (f.use_events && !f.events_ok) grow_event_capacity(c, M);
  if (held.moved()) { c->last_error = "internal: an edge array was re-allocated under run_select's views"; return SC_EHIP; }
  SC_TRY(write_keys(c, p, a));
  SC_TRY(select_and_compact(c, M, a));
  // the list stays in ordinal order: no sort on the hot path (the winner is found by (count, key, position))
  if (want_list) launch_tri_decode(a.el, keys_of(c), selection_of(c), T_eff, c->tri.as<uint32_t>(), c->stream);
  c->pass.regular = hostfree_form_met(c, M, want_sel);
  return SC_OK;
}

int run_triangles(sc_ctx* c, const sc_params* p, bool want_list) {
  SC_TRY(run_edges(c, p, nullptr, 0, 1));
  return run_select(c, p, nullptr, want_list);
}

// ---- what a host-free frame assumes --------------------------------------------------------------------------------------------
// A host-free frame (include/saccot.h; PassMode) is enqueued without looking at anything the GPU produces.  It assumes
//   (a) the parameters and knobs of the common form: events, the a-priori select window, pruning, no stage timing, no exact total,
//       and the last completed call's shape                                                              — hostfree_shape_ok
//   (b) counts that fit: a graph big enough to prune (E >= 4096), E and M within what the launches cover,
//       and T triangles found (M >= T)                                                                   — counts_fit (sc_frame_check.hpp)
//   (c) that the call it repeats took that form itself: waited, events that did not overflow, the a-priori window, the whole sample
//       in its own histogram, stages A and B whole on this GPU (one rank, or replicated ranks)           — hostfree_form_met, hostfree_next_ok
// Four places ask: fast_plan PREDICTS (a) and (b) from the last call's counts; run_select NOTES (c) for the call in hand; the frame's
// verdict (frame_end -> hostfree_valid, sc_frame_check.hpp; finalize_wait, sc_capi_frame.hip) VALIDATES (b) and the event list once
// the frame has run; note_completed (sc_capi_frame.hip) FILES all of it as sc_ctx::fast_ok and in sc_ctx::shape.

static bool hostfree_shape_ok(const sc_ctx* c, int64_t n, const sc_params* p) {
  if (c->tn.no_fast || c->tn.no_events || n != c->shape.n) return false;
  if (p->flags & (SC_FLAG_TIMING | SC_FLAG_EXACT_TOTAL | SC_FLAG_NO_PRUNE)) return false;
  if (!ShapeHistory::same_shape(p, &c->shape.p)) return false;
  return window_known(p);  // the a-priori select window (weight ranking with it)
}

// May this call be enqueued host-free?  Only a repetition of the last call's shape on this context, and only when that call
// was regular (note_completed); sets what the launches cover (ShapeHistory::cover), within what the arrays hold.
bool fast_plan(const sc_ctx* c, int64_t n, const sc_params* p, PassMode* mode) {
  if (!c->fast_ok || !hostfree_shape_ok(c, n, p)) return false;
  const uint64_t ecap = edge_capacity(c, edge_build_ok(c, p, n, true));  // (every entry point that comes here may estimate; the fused edge kernel writes no per-edge bases)
  const uint64_t kcap = keys_of(c).cap;
  const ShapeHistory& h = c->shape;
  uint64_t ecov = h.cover(h.E_last, h.E_hi), mcov = h.cover(h.M_last, h.M_hi);
  if (ecov > ecap) ecov = ecap;
  if (mcov > kcap) mcov = kcap;
  // The prediction: the last call's counts fit the covers.  (fast_ok says of those counts what counts_fit asks beside the covers —
  // E_last >= 4096, M_last >= T: hostfree_next_ok — so the covers are at least that large as well.)
  if (!counts_fit(h.E_last, h.M_last, ecov, mcov, p->max_triangles) || ecov >= (1ull << 32)) return false;
  mode->host_free = true; mode->E_cov = ecov; mode->M_cov = mcov;
  return true;
}

// run_select, of the waited call in hand: the shape a host-free repetition of it assumes.  (A host-free call notes nothing here:
// apply_verdict says "regular" once the frame is validated.)  Differs from (a) in looking at what the call DID, not at its parameters:
// events_ok and fast_window fold in use_events, pruning and window_known; have_total is SC_FLAG_EXACT_TOTAL on a pruned graph.
static bool hostfree_form_met(const sc_ctx* c, uint64_t M, uint32_t want_sel) {
  const StageBForm& f = c->pass.form;
  return !f.spec && f.events_ok && f.fast_window && !f.have_total && !c->pass.timing && M >= want_sel && f.own_sample;
}

// note_completed, of the call that just completed (regular: hostfree_form_met's answer, or a validated host-free frame): may the
// next call of its shape be enqueued host-free?  The counts are their own covers here: what is left of counts_fit is E >= 4096 and
// M >= T (T_eff == T says the same: T_eff = min(M, T) off the sharded path).  Not sharded: stages A and B whole on this GPU (one
// rank, or replicated ranks) — hostfree_form_met cannot say, sharded calls have a select_want below T
bool hostfree_next_ok(const sc_ctx* c, bool regular) {
  return regular && !c->pass.sharded_ab && counts_fit(c->pass.E, c->pass.M, c->pass.E, c->pass.M, c->pass.params.max_triangles);
}

}  // namespace sc
