// sc_capi_frame.hip — a frame's end on the host: the lane, the finalize step's two halves, the verdict on a frame that has run and
// what it leaves for the next call, the library's own repeat of a call, and the register, finalize and wait entries.  Host-only, on
// the context (sc_ctx.hpp); the stages themselves are sc_capi.hip's (hyp_begin, hyp_end) and sc_capi_tri.hip's.
//
// The rules are not here: how a frame may end and what each end does (FrameEnd, frame_end_row), the estimate's history and the
// shape's are sc_frame_check.hpp's, host-only and tested on the CPU.  This file reads the facts, asks, and applies:
//   finalize_wait = wait_winner -> frame_facts -> frame_end -> apply_verdict -> note_completed -> read_stats
// and apply_verdict is the only place where a verdict touches the context.
#include "sc_ctx.hpp"

using namespace sc;

namespace sc {

// ---- the lane (sc_ctx.hpp): a host-free frame of a direct sc_register_device_async call on a caller's stream runs beside that stream
// Fork: everything the caller enqueued before the call — producers of d_src / d_tgt, earlier readers of d_Rt / d_mask, this context's
// own earlier launches — is ordered before the frame; from here to the join the frame's launches go to the lane as c->stream.
static int lane_fork_caller(sc_ctx* c) {
  HIPCHK(c, hipEventRecord(c->lane_fork, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->own_stream, c->lane_fork, 0));
  c->lane_home = c->stream;
  c->stream = c->own_stream;
  c->on_lane = true;
  return SC_OK;
}
// Join (wait_winner; a no-op off the lane): the caller's stream waits for the event behind the frame's last launch, and is the
// context's stream again — the validation, a repeat, sc_peel / sc_polish* and the caller's own reads of d_Rt / d_mask follow the
// frame in stream order, as they do without a lane.
static int lane_join_caller(sc_ctx* c) {
  if (!c->on_lane) return SC_OK;
  c->on_lane = false;
  c->stream = c->lane_home;
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->lane_join, 0));
  return SC_OK;
}
// Behind the frame's last launch on the lane: what the join waits for
static int lane_mark_end(sc_ctx* c) {
  HIPCHK(c, hipEventRecord(c->lane_join, c->stream));
  return SC_OK;
}
// The enqueue failed half-way: what reached the lane runs out (no join was recorded), then the caller's stream is the context's again
static void lane_drain(sc_ctx* c) {
  if (!c->on_lane) return;
  (void)hipStreamSynchronize(c->own_stream);
  c->on_lane = false;
  c->stream = c->lane_home;
}

// phase 2, first half: the winner / mask kernel (and the optional refit) are enqueued; nothing is waited for
static int finalize_enqueue(sc_ctx* c, const uint64_t* d_keys, int n_pairs, float* d_Rt, uint8_t* d_mask) {
  SC_TRY(rec(c, 7));
  ControlBlock* ctl = c->ctl.as<ControlBlock>();
  arm_word(c, HW_WINNER);
  // a host-free call's kernels have published nothing yet: this one hands the counts and the coordinate statistics over with the winner
  DeferredPub dp{c->edge_off.as<uint64_t>() + c->pass.n, c->toff.as<uint64_t>() + c->pass.E, c->fx_mx.as<uint32_t>(),
                 reinterpret_cast<unsigned long long*>(c->pinned), (c->n_fast_ok & 63u) == 63u ? 1 : 0};
  if (d_keys == c->key.as<uint64_t>() && n_pairs == 1 && c->pass.amx_blocks) { d_keys = c->amx_pairs.as<uint64_t>(); n_pairs = (int)c->pass.amx_blocks; }
  launch_finalize(points_of(c), tri_source_of(c), hyps_of(c), WinnerIn{c->pass.T_eff ? c->sel_key.as<uint32_t>() : nullptr, c->pass.T_eff, d_keys, n_pairs},
                  WinnerOut{d_Rt, d_mask, &c->pinned[HW_WINNER]}, c->pass.dv.tau2, ctl->key2, &ctl->fin_word,
                  c->pass.mode.host_free ? &dp : nullptr, c->stream);
  if (c->pass.refine) {  // fp64 least-squares refit over the winner's inliers (mask unchanged)
    ENSURE(c, c->refine_tmp, refine_scratch_bytes(c->pass.n));
    launch_refine(points_of(c), d_mask, ctl->key2, c->refine_tmp.as<double>(), d_Rt, c->stream);
  }
  return rec(c, 8);
}

// ---- finalize_wait's steps, in its order ------------------------------------------------------------------------------------------

// The finalize kernel publishes key / position / rank.  On a caller-provided stream (sc_set_stream) d_Rt and d_mask are complete in
// stream order, like any other work the caller enqueues there; on the context's private stream — which the caller cannot order
// against — and when the per-stage events are read afterwards, wait for everything.  "Private" means that no caller's stream is set —
// a frame on its lane has the private stream as c->stream and is polled for.
static int wait_winner(sc_ctx* c) {
  if (c->pass.timing || !c->caller_stream) HIPCHK(c, hipStreamSynchronize(c->stream));
  else if (c->pass.timing_one == 6) HIPCHK(c, hipEventSynchronize(c->ev[8]));  // the mask bracket ends after the kernel polled below
  const int rc_winner = wait_word(c, HW_WINNER);  // (a lane frame: polled, or after 1 ms synchronised, on the lane)
  const int rc_join = lane_join_caller(c);        // ... and before anything else the caller's stream is behind the frame
  if (rc_winner || rc_join) { c->fast_ok = false; return rc_winner ? rc_winner : rc_join; }
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// The winner word is the last thing the stream writes: every kernel of the frame has finished, so the host words are final — the
// two counts of a host-free frame (one word: DeferredPub) and the flags of kernels earlier in the stream, whose system-scope stores
// are visible once the winner word is.  Each is read once, here.
static FrameFacts frame_facts(const sc_ctx* c, bool host_free) {
  FrameFacts f;
  f.host_free = host_free;
  f.bad_input = c->pinned[HW_BAD_INPUT]; f.counts = c->pinned[HW_EDGES]; f.ev_overflow = c->pinned[HW_EV_OVERFLOW];
  f.select_short = c->pinned[HW_SELECT_SHORT]; f.merge_short = c->pinned[HW_MERGE_SHORT]; f.cand_cut = c->pinned[HW_CAND_CUT];
  f.winner_pos = c->pinned[HW_WINNER_POS]; f.winner_key = c->pinned[HW_WINNER];
  f.est_active = c->pass.form.est_active; f.est_void = c->pass.est_void;
  f.sharded_ab = c->pass.sharded_ab; f.cand_all = c->pass.cand_all != nullptr;
  f.est_bound_flag = (c->pass.params.flags & SC_FLAG_EST_BOUND) != 0;
  f.E_cov = c->pass.mode.E_cov; f.M_cov = c->pass.mode.M_cov; f.T = c->pass.params.max_triangles;
  return f;
}

// what the next call on this context may assume (fast_plan): the call that just completed was a "regular" one
static void note_completed(sc_ctx* c, bool regular) {
  c->fast_ok = hostfree_next_ok(c, regular);
  c->shape.note(c->fast_ok, c->pass.E, c->pass.M, c->pass.n, c->pass.params);
  c->est.completed(c->frame.est_failed_call);
  // (the call is complete: its staging kernel's words have arrived — unless it was a host-free call, whose statistics travel with
  // the winner only now and then: DeferredPub; the last ones known stay)
  const CoordStats cs = read_coord_stats(c);
  if (cs.mx != ~0ull) {
    c->mx_last = cs.mx;
    for (int k = 0; k < 6; k++) c->box_last[k] = cs.box[k];
  }
  // room for the event list of a call like this one: an event holds >= 1 triangle, so 2 M records can only overflow a region
  // on a fill 2 x off the mean (the regions fill evenly: a wave moves to the next one with every flush)
  if (c->pass.form.use_events && c->ev_capacity < 2 * c->pass.M) c->ev_capacity = 2 * c->pass.M < (1ull << 28) ? 2 * c->pass.M : (1ull << 28);
}

// One row of frame_end_row, applied: the only place where a verdict changes the context.  A host-free frame whose outputs are void
// (HostfreeVoid, EstFailed) comes back as SC_ESPEC: the caller (sc_wait, register_waited) repeats the call the waiting way, which
// handles every one of these cases.
static int apply_verdict(sc_ctx* c, FrameEnd end, const FrameFacts& f) {
  const FrameEndRow& row = frame_end_row(end);
  if (row.validated) {
    if (f.host_free) {  // the covers give way to the real counts
      const Counts k = unpack_counts(f.counts);
      c->pass.E = k.E; c->pass.M = c->pass.M_total = k.M;
      c->frame.fast_state = 1;
      c->pass.regular = true;
    }
    c->pass.est_state = f.est_active ? 1 : 0;
  }
  const std::string text = frame_end_text(end, f);
  if (!text.empty()) c->last_error = text;
  if (row.clears_fast_ok) c->fast_ok = false;
  if (row.est_failed_call) c->frame.est_failed_call = true;
  if (row.est_fails) c->est.fail();  // this context certifies for a while (note_completed counts the hold-off down)
  if (row.repairs_overflow) {
    if (chunks_overflowed(f.ev_overflow)) c->ord_off = true;  // (the repeat, and the calls after it, scan the per-edge counts)
    else if (events_overflowed(f.ev_overflow) && c->ev_capacity < (1ull << 28)) c->ev_capacity *= 2;  // (the repeat must not overflow again)
  }
  if (row.completes) note_completed(c, c->pass.regular);
  return row.status;
}

// the caller's sc_stats of a completed call: the counts, the winner's, and the stage brackets the call recorded
static void read_stats(sc_ctx* c, sc_stats* stats, uint64_t key) {
  if (!stats || stats->size != sizeof(sc_stats)) return;
  fill_stats(c, stats);
  stats->best_count = (uint32_t)(key >> 32);
  stats->best_rank = key ? (uint32_t)(c->pinned[HW_WINNER_POS] >> 32) : 0u;  // (rank index << 32 | position: one word beside the key)
  if (c->pass.timing) {
    stats->us_stage = ev_us(c, 0, 1);
    stats->us_compat = ev_us(c, 1, 2);
    stats->us_triangles = ev_us(c, 2, 3);  // includes its two 8-byte read-backs
    stats->us_trikeys = c->pass.timed_trikeys ? ev_us(c, 9, 10) : 0.f;
    stats->us_kabsch = ev_us(c, 3, 4);
    stats->us_score = ev_us(c, 4, 5);
    stats->us_argmax = ev_us(c, 5, 6);
    stats->us_mask = ev_us(c, 7, 8);
    stats->us_total = stats->us_stage + stats->us_compat + stats->us_triangles + stats->us_kabsch +
                      stats->us_score + stats->us_argmax + stats->us_mask;
  } else if (c->pass.timing_hot) {
    stats->us_score = c->pass.hot_ext ? ev_us_raw(c, 4, 5) : ev_us(c, 4, 5);
  } else if (c->pass.timing_one >= 0) {  // one bracket, recorded on the hot path (speculative launches on)
    float* dst[7] = {&stats->us_stage, &stats->us_compat, &stats->us_triangles, &stats->us_kabsch, &stats->us_score,
                     &stats->us_argmax, &stats->us_mask};
    *dst[c->pass.timing_one] = ev_us(c, STAGE_EV[c->pass.timing_one][0], STAGE_EV[c->pass.timing_one][1]);
  }
}

// phase 2, second half: wait for the winner; the frame that has run gets its verdict here
static int finalize_wait(sc_ctx* c, sc_stats* stats) {
  const bool host_free = pass_end(c);
  SC_TRY(wait_winner(c));
  const FrameFacts f = frame_facts(c, host_free);
  const FrameEnd end = frame_end(f);
  const int rc = apply_verdict(c, end, f);
  if (frame_end_row(end).completes) read_stats(c, stats, f.winner_key);
  return rc;
}

// the whole path the waiting way (what sc_register_device always did): complete on return.  The only caller of the phases
// that may prune by an ESTIMATED bound (it can repeat the call): a failed estimate comes back as SC_ESPEC from finalize_wait
// and has switched estimating off for this context, so the second pass certifies.
static int register_waited(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p, float* d_Rt,
                    uint8_t* d_mask, sc_stats* stats) {
  int rc = SC_OK;
  for (int pass = 0; pass < 2; pass++) {
    rc = hyp_begin(c, d_src, d_tgt, n, p, nullptr, 0, 1, PassMode{true});  // (waited; may estimate)
    if (!rc) rc = hyp_end(c, nullptr, c->key.as<uint64_t>(), stats);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = finalize_enqueue(c, c->key.as<uint64_t>(), 1, d_Rt, d_mask);
    if (!rc) rc = finalize_wait(c, stats);
    if (rc != SC_ESPEC) return rc;
  }
  c->last_error = "internal: a call was asked to repeat twice";
  return SC_EHIP;
}

// one more frame (a call of sc_register_device(_async) / sc_register, or sc_hypothesize_device + its finalize call) has come to its
// end with status rc: the context's cumulative counters (sc_debug_last)
static void count_frame(sc_ctx* c, int rc) {
  c->n_frames++;
  if (c->frame.est_failed_call) c->n_est_fail++;
  else if (c->pass.est_state == 1 && (rc == SC_OK || rc == SC_ENOHYP)) c->n_est_ok++;
  if (c->frame.fast_state == 2 || (rc == SC_EBOUND && !c->frame.est_failed_call)) c->n_fast_repeat++;  // host-free, void: repeated (here, or by the caller)
  else if (c->frame.fast_state == 1) c->n_fast_ok++;
}

// the finalize call of a HOST-FREE sc_hypothesize_device: a failed validation is the caller's to repeat (every rank alike)
static int finalize_status(sc_ctx* c, int rc) {
  if (rc != SC_ESPEC) return rc;
  c->last_error += " — repeat sc_hypothesize_device and the finalize call without SC_FLAG_EST_BOUND";
  return SC_EBOUND;
}

// the finalize call's two forms: arguments, a free context, a hypothesize half to finalize; then the winner / mask kernel is enqueued
static int finalize_begin(sc_ctx* c, const uint64_t* d_keys, int n_pairs, float* d_Rt, uint8_t* d_mask) {
  if (!c || !d_keys || !d_Rt || !d_mask || n_pairs < 1 || n_pairs > 4096) return SC_EINVAL;
  SC_TRY(continue_pass(c, c->pass.have_hyp, "sc_finalize_device without a preceding sc_hypothesize_device"));
  return finalize_enqueue(c, d_keys, n_pairs, d_Rt, d_mask);
}

// ---- the outstanding call (Outstanding, sc_ctx.hpp) --------------------------------------------------------------------------------

// The library's own copy of a call's statistics, fresh and of the library's size (fill_stats and read_stats write into nothing else):
// before the first stage that fills it
static sc_stats* fresh_stats(sc_ctx* c) {
  c->frame.pend_stats = sc_stats{};
  c->frame.pend_stats.size = sizeof(sc_stats);
  return &c->frame.pend_stats;
}
// An entry returns with its call outstanding (held_rc: the status of one that is Complete); sc_wait takes it back
static int leave_outstanding(sc_ctx* c, Outstanding state, int held_rc = SC_OK) {
  c->frame.outstanding = state;
  c->frame.held_rc = held_rc;
  return SC_OK;
}

// sc_register_device_async.  `direct`: the caller gets the context back before the frame is waited for, so a host-free frame on a
// caller's stream takes the lane; sc_register_device (async + wait in one call) overlaps nothing and pays no fork and join.
static int register_async(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p,
                          float* d_Rt, uint8_t* d_mask, bool direct) {
  if (!c || !d_src || !d_tgt || !d_Rt || !d_mask) return SC_EINVAL;
  peel_end(c);
  if (c->frame.outstanding != Outstanding::None) { c->last_error = "sc_register_device_async: a call is already outstanding on this context (sc_wait first)"; return SC_EINVAL; }
  SC_TRY(entry_checks(c, p, PARAMS | ONE_RANK));  // (the frame ended above; "busy" has this entry's own text)
  HIPCHK(c, hipSetDevice(c->device));
  ENSURE(c, c->key, 64);
  SC_TRY(frame_begin(c));
  c->frame.call = PendingCall{d_src, d_tgt, n, *p, d_Rt, d_mask};
  sc_stats* stats = fresh_stats(c);
  PassMode mode{true};  // (sc_wait repeats a call whose estimated pruning bound fails, like any other failed assumption)
  if (fast_plan(c, n, p, &mode)) {
    // host-free: the whole chain is enqueued without looking at anything the GPU produces; sc_wait validates
    int rc = SC_OK;
    if (direct && c->caller_stream && !c->tn.no_lane) rc = lane_fork_caller(c);
    if (!rc) rc = hyp_begin(c, d_src, d_tgt, n, p, nullptr, 0, 1, mode);
    if (!rc) rc = hyp_end(c, nullptr, c->key.as<uint64_t>(), stats);
    if (!rc) rc = finalize_enqueue(c, c->key.as<uint64_t>(), 1, d_Rt, d_mask);
    if (!rc && c->on_lane) {
      rc = lane_mark_end(c);
      if (!rc) { c->frame.lane = true; c->n_lane++; }
    }
    if (!rc) return leave_outstanding(c, Outstanding::Enqueued);
    // The host-free enqueue failed (an allocation sized by the COVERS hit the workspace cap, a launch failed): the waited form of
    // the same call may well fit — "results are identical either way" (include/saccot.h) includes the status.  What was enqueued
    // so far runs out first: its kernels publish into the pinned words the waited call is about to arm.  
    // A frame on its lane: the lane is drained and the caller's stream is the context's again before the waited form starts.
    pass_end(c); c->fast_ok = false;
    if (c->on_lane) lane_drain(c);
    else (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
  }
  const int rc = register_waited(c, d_src, d_tgt, n, p, d_Rt, d_mask, stats);
  if (rc != SC_OK && rc != SC_ENOHYP) return rc;
  return leave_outstanding(c, Outstanding::Complete, rc);
}

}  // namespace sc

extern "C" {

int sc_finalize_gathered_device(sc_ctx* c, const uint64_t* d_keys, int n_pairs, float* d_Rt, uint8_t* d_mask,
                                sc_stats* stats) {
  SC_TRY(finalize_begin(c, d_keys, n_pairs, d_Rt, d_mask));
  const int rc = finalize_status(c, finalize_wait(c, stats));
  count_frame(c, rc);
  return rc;
}

int sc_finalize_device(sc_ctx* c, const uint64_t* d_key, float* d_Rt, uint8_t* d_mask, sc_stats* stats) {
  return sc_finalize_gathered_device(c, d_key, 1, d_Rt, d_mask, stats);
}

int sc_finalize_gathered_device_async(sc_ctx* c, const uint64_t* d_keys, int n_pairs, float* d_Rt, uint8_t* d_mask) {
  SC_TRY(finalize_begin(c, d_keys, n_pairs, d_Rt, d_mask));
  fresh_stats(c);
  return leave_outstanding(c, Outstanding::Finalize);
}

int sc_register_device_async(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p,
                             float* d_Rt, uint8_t* d_mask) {
  return register_async(c, d_src, d_tgt, n, p, d_Rt, d_mask, true);
}

int sc_wait(sc_ctx* c, sc_stats* stats) {
  if (!c) return SC_EINVAL;
  const Outstanding was = c->frame.outstanding;
  if (was == Outstanding::None) { c->last_error = "sc_wait without an outstanding sc_register_device_async / sc_finalize_gathered_device_async"; return SC_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  c->frame.outstanding = Outstanding::None;
  int rc = c->frame.held_rc;  // (Complete)
  if (was == Outstanding::Finalize) rc = finalize_status(c, finalize_wait(c, &c->frame.pend_stats));  // sc_finalize_gathered_device's second half
  if (was == Outstanding::Enqueued) {
    rc = finalize_wait(c, &c->frame.pend_stats);
    if (rc == SC_ESPEC) {  // a count outgrew what the launches covered (or another fallback was needed): the waiting way
      const PendingCall& call = c->frame.call;
      rc = register_waited(c, call.src, call.tgt, call.n, &call.p, call.Rt, call.mask, &c->frame.pend_stats);
      c->frame.fast_state = 2;
    }
  }
  count_frame(c, rc);
  copy_stats(stats, c->frame.pend_stats);
  if (rc == SC_OK && was != Outstanding::Finalize) peel_open(c);  // a frame: sc_peel may follow
  return rc;
}

int sc_register_device(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p,
                       float* d_Rt, uint8_t* d_mask, sc_stats* stats) {
  SC_TRY(register_async(c, d_src, d_tgt, n, p, d_Rt, d_mask, false));  // (waited for at once: no lane)
  return sc_wait(c, stats);
}

int sc_register(sc_ctx* c, const float* src, const float* tgt, int64_t n, const sc_params* p, float R[9],
                float t[3], uint8_t* mask, sc_stats* stats) {
  if (c) peel_end(c);
  if (!c || !src || !tgt || !R || !t || !mask || n < 3 || n > (1 << 24)) return SC_EINVAL;
  SC_TRY(entry_checks(c, p, PARAMS | ONE_RANK));  // (busy: sc_register_device_async's answer, below)
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  if (n <= (1 << 20)) {
    // Zero-copy form (up to 1 M correspondences = 24 MB in, 1 MB out over the host link): two memcpys on the host into a
    // pinned, device-mapped area; the staging kernel reads it, the finalize kernel writes (R, t) and the mask into the
    // other.  No hipMemcpy at all: a pageable-memory copy costs 10-20 us of driver time each (C2: 0.36 -> 0.31 ms).
    const size_t in_bytes = (size_t)n * 24, out_bytes = 64 + (size_t)n;
    auto grow = [&](void** p_, size_t* cap, size_t want) -> int {
      if (*cap >= want) return SC_OK;
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (*p_) { (void)hipHostFree(*p_); *p_ = nullptr; *cap = 0; }
      size_t sz = want + want / 4 + 4096;
      if (hipHostMalloc(p_, sz, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *p_ = nullptr; c->last_error = "hipHostMalloc failed"; return SC_ENOMEM; }
      *cap = sz;
      return SC_OK;
    };
    SC_TRY(grow(&c->h_in, &c->h_in_cap, in_bytes));
    SC_TRY(grow(&c->h_out, &c->h_out_cap, out_bytes));
    float* hs = static_cast<float*>(c->h_in);
    float* ht = hs + (size_t)n * 3;
    memcpy(hs, src, (size_t)n * 12);
    memcpy(ht, tgt, (size_t)n * 12);
    void *d_s = nullptr, *d_t = nullptr, *d_o = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&d_s, hs, 0));
    HIPCHK(c, hipHostGetDevicePointer(&d_t, ht, 0));
    HIPCHK(c, hipHostGetDevicePointer(&d_o, c->h_out, 0));
    const int rc = sc_register_device(c, static_cast<float*>(d_s), static_cast<float*>(d_t), n, p, static_cast<float*>(d_o),
                            static_cast<uint8_t*>(d_o) + 64, stats);
    if (rc != SC_OK && rc != SC_ENOHYP) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (idle already on the private stream; a caller's stream may hold the refit)
    const float* Rt = static_cast<const float*>(c->h_out);
    memcpy(R, Rt, 36);
    memcpy(t, Rt + 9, 12);
    memcpy(mask, static_cast<const uint8_t*>(c->h_out) + 64, (size_t)n);
    return rc;
  }
  ENSURE(c, c->rt12, 64);
  ENSURE(c, c->mask, (size_t)n);
  SC_TRY(points_to_device(c, src, tgt, n));
  const int rc = sc_register_device(c, c->in_src.as<float>(), c->in_tgt.as<float>(), n, p, c->rt12.as<float>(),
                          c->mask.as<uint8_t>(), stats);
  if (rc != SC_OK && rc != SC_ENOHYP) return rc;
  SC_TRY(outputs_to_host(c, (size_t)n, R, t, mask));
  return rc;
}

}  // extern "C"
