// sc_capi.hip — the core of the C ABI of include/saccot.h: the context's lifetime and its grow-only device workspace, sc_set_debug /
// sc_debug_last, pass and frame begin, the stage sequencer of stage C, and the hypothesize and shard entries.  Stage A's
// sequencer (stage_inputs, run_compat, run_row_stats) is sc_capi_compat.hip, stage B's
// (run_edges, run_select, the host-free plan) sc_capi_tri.hip; a frame's end (the lane, the finalize step, the verdict,
// the register, finalize and wait entries) is sc_capi_frame.hip.  The
// rest of the ABI sits in host-only files of its own, on sc_ctx.hpp (sc_ctx itself and the shared helpers): sc_capi_hooks.hip (the
// sc_*_host stage hooks), sc_capi_peel.hip (sc_peel*, sc_register_instances), sc_capi_match.hip (sc_match*, sc_register_features), sc_capi_polish.hip (sc_polish*),
// sc_capi_batch.hip (sc_register_batch*).
//
// There is no reference interface to mirror (the reference tree holds a two-line README.md and no code, which is why there is no
// oracle/_ref); the boundary is SURVEY.md §8(b).  Everything that computes runs on the GPU: these files only validate, allocate,
// enqueue kernels (sc_kernels.hpp) and copy.  Two small read-backs (edge count, triangle count) size the data-dependent buffers;
// there is no CPU fallback of any stage.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <new>
#include <utility>

#include "sc_ctx.hpp"
#include "sc_gramref.hpp"

using namespace sc;

namespace sc {

int fail_hip(sc_ctx* c, hipError_t e, const char* what) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  if (c) c->last_error = buf;
  return SC_EHIP;
}

int ensure(sc_ctx* c, Buf& b, size_t bytes) {
  if (bytes <= b.cap) return SC_OK;
  size_t want = bytes + bytes / 8 + 256;
  // a host-free call that has to grow a buffer stalls (the re-allocation below synchronises the stream): grow in big steps there,
  // so that a stream whose covers are still rising pays a few of these, not one per frame; and never allocate crumbs
  if (c->pass.mode.host_free) want = 2 * bytes + 256;
  if (want < 65536) want = 65536;
  if (c->held - b.cap + want > c->cap_bytes) {
    want = bytes;
    if (c->held - b.cap + want > c->cap_bytes) { c->last_error = "workspace cap exceeded"; return SC_ENOMEM; }
  }
  if (b.p) {
    if (c->pass.mode.host_free) c->n_spec_grow++;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(b.p));
    c->held -= b.cap;
    b.p = nullptr; b.cap = 0;
  }
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) { b.p = nullptr; (void)hipGetLastError(); c->last_error = "hipMalloc failed"; return SC_ENOMEM; }
  b.cap = want;
  c->held += want;
  return SC_OK;
}

// `need` bytes now, `room` bytes wanted (room for the counts of the NEXT calls of this shape: a host-free call's launches are
// sized by a cover of the recent counts and must fit the arrays it finds — fast_plan); under a tight workspace cap: just `need`
int ensure_room(sc_ctx* c, Buf& b, size_t need, size_t room) {
  if (room > need && room > b.cap) {
    const size_t want = room + room / 8 + 256;
    if (c->held - b.cap + want <= c->cap_bytes && ensure(c, b, room) == SC_OK) return SC_OK;
  }
  return ensure(c, b, need);
}
int check_params(const sc_params* p) {
  if (!p || p->size != sizeof(sc_params)) return SC_EINVAL;
  if (!(p->sigma > 0.f) || !(p->t_cmp > 0.f) || !(p->t_cmp < 1.f) || !(p->tau > 0.f) || !(p->min_len >= 0.f))
    return SC_EINVAL;
  if (!std::isfinite(p->sigma) || !std::isfinite(p->tau) || !std::isfinite(p->min_len)) return SC_EINVAL;
  if (p->max_triangles == 0 || p->max_triangles > 0xFFFFFF00u) return SC_EINVAL;  // padded to 256 in u32
  if (p->rank_mode != SC_RANK_WEIGHT && p->rank_mode != SC_RANK_DEGREE) return SC_EINVAL;
  if (p->layout != SC_AOS && p->layout != SC_SOA) return SC_EINVAL;
  if (p->shard_world < 1 || p->shard_rank < 0 || p->shard_rank >= p->shard_world) return SC_EINVAL;
  if (p->score_mode < SC_SCORE_COUNT || p->score_mode > SC_SCORE_MAE) return SC_EINVAL;
  if (p->shard_cand_level < -16 || p->shard_cand_level > 30) return SC_EINVAL;
  return SC_OK;
}

// thresholds precomputed on the host in fp64, rounded once to fp32
Derived derive(const sc_params* p) {
  Derived d;
  d.d_thr = (float)((double)p->sigma * std::sqrt(-2.0 * std::log((double)p->t_cmp)));
  d.neg_inv2sig2 = (float)(-1.0 / (2.0 * (double)p->sigma * (double)p->sigma));
  d.tau2 = (float)((double)p->tau * (double)p->tau);
  d.min_len = p->min_len;
  d.inv_tau2 = (float)(1.0 / ((double)p->tau * (double)p->tau));
  d.inv_tau = (float)(1.0 / (double)p->tau);
  return d;
}

// Look-back launches (single-pass scans, fused row kernel, fused compaction).  lb_state holds the tile descriptors and
// is written by look-back kernels only: zeroed when new, when it grew, and when the 12-bit epoch wraps.  The TICKET and
// error words live in a small buffer of their own (lb_ticket, zeroed once): a ticket inside the descriptor area would,
// after a launch with another layout, sit on an old descriptor and hand out garbage tile indices (that was a GPU
// memory fault at N = 20 000 sharded in development).  slot: which ticket (launches that may be in flight together on
// the stream's order use different ones); desc_off: byte offset of this launch's descriptors inside the area.
int lb_next(sc_ctx* c, size_t bytes, int slot, size_t desc_off, LbArgs* out) {
  ENSURE(c, c->lb_state, bytes);
  if (!c->lb_ticket.p) {
    ENSURE(c, c->lb_ticket, 256);
    HIPCHK(c, hipMemsetAsync(c->lb_ticket.p, 0, c->lb_ticket.cap, c->stream));
  }
  if (c->lb_state.p != c->lb_zeroed || c->lb_state.cap != c->lb_zeroed_cap || c->lb_epoch >= 4095u) {
    HIPCHK(c, hipMemsetAsync(c->lb_state.p, 0, c->lb_state.cap, c->stream));
    c->lb_zeroed = c->lb_state.p; c->lb_zeroed_cap = c->lb_state.cap; c->lb_epoch = 0;
  }
  out->epoch = ++c->lb_epoch;
  out->ticket = c->lb_ticket.as<uint32_t>() + 2 * slot;  // 8 bytes apart
  out->err = c->lb_ticket.as<uint32_t>() + 32 + slot;
  out->desc = reinterpret_cast<uint64_t*>(static_cast<char*>(c->lb_state.p) + desc_off);
  return SC_OK;
}

TriSource tri_source_of(const sc_ctx* c) {
  TriSource ts{c->sel_ord.as<uint64_t>(), c->kcol.as<uint2>(), c->ei.as<uint32_t>(), c->ej.as<uint32_t>(), nullptr, 0, 0, 0u, 0u, 0ull};
  if (c->pass.mode.host_free) { ts.lim_vertex = (uint32_t)c->pass.n; ts.lim_edge = (uint32_t)c->pass.mode.E_cov; ts.lim_ord = c->pass.mode.M_cov; }
  // an ESTIMATED pruning bound that turns out too high leaves a selection shorter than the T_eff the launches were sized for
  // (the call is then repeated): what lies beyond it in sel_ord must not be followed
  else if (c->pass.form.est_active) { ts.lim_vertex = (uint32_t)c->pass.n; ts.lim_edge = (uint32_t)c->pass.E; ts.lim_ord = c->pass.M; }
  if (c->pass.sharded_ab && c->pass.cand_all) {  // the selection indexes the gathered candidate blobs
    const size_t cap = cand_cap(c->pass.params.max_triangles, (uint32_t)c->pass.params.shard_world, c->pass.params.shard_cand_level);
    ts.cand_recs = cand_blob(const_cast<void*>(c->pass.cand_all), cap).recs;
    ts.cand_seg = cap;
    ts.cand_stride = c->pass.cand_bytes / 16;
  }
  return ts;
}

int rec(sc_ctx* c, int i) {
  const bool hot = i == 4 || i == 5;
  const bool one = c->pass.timing_one >= 0 && (i == STAGE_EV[c->pass.timing_one][0] || i == STAGE_EV[c->pass.timing_one][1]);
  if (c->pass.timing || (c->pass.timing_hot && hot) || one) HIPCHK(c, hipEventRecord(c->ev[i], c->stream));
  return SC_OK;
}

// A bracket of two event records contains the cost of one record (a barrier packet with a timestamp: ~4-5 us of
// stream time on this part) on top of what lies between them.  That cost is measured once per context — an empty
// bracket on the idle stream — and subtracted, so that a bracket around one kernel reads like the profiler's duration
// of that kernel (plus any genuine launch gap).
static int calibrate_events(sc_ctx* c) {
  if (c->ev_overhead_us >= 0.f) return SC_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float best = 1e9f;
  for (int rep = 0; rep < 5; rep++) {
    // a chain of back-to-back records: the first interval includes waking an idle queue, the later ones are the
    // steady cost of a record that follows other work — which is what sits inside a stage bracket
    for (int k = 0; k < 6; k++) HIPCHK(c, hipEventRecord(c->ev[k], c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 2; k < 5; k++) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, c->ev[k], c->ev[k + 1]) == hipSuccess && ms * 1000.f < best) best = ms * 1000.f;
    }
  }
  c->ev_overhead_us = best < 1e8f ? best : 0.f;
  return SC_OK;
}

// SC_FLAG_TIMING / _HOT / _ONE -> the context's timing state for this call
static int set_timing(sc_ctx* c, const sc_params* p) {
  c->pass.timing = (p->flags & SC_FLAG_TIMING) != 0;
  c->pass.timing_hot = !c->pass.timing && (p->flags & SC_FLAG_TIMING_HOT) != 0;
  c->pass.timing_one = -1;
  if (!c->pass.timing && !c->pass.timing_hot && (p->flags & SC_FLAG_TIMING_ONE)) {
    const int stage = (int)((p->flags >> 8) & 15u);
    if (stage > 6) return SC_EINVAL;
    c->pass.timing_one = stage;
  }
  if (c->pass.timing || c->pass.timing_hot || c->pass.timing_one >= 0) return calibrate_events(c);
  return SC_OK;
}

// Read-backs: the producing kernel stores its 8-byte result into host-pinned memory (publish_host) and the host
// polls that word instead of blocking in hipStreamSynchronize (whose wake-up alone costs ~10 us, twice per call).
// After ~1 ms of polling it falls back to the blocking wait (very long stages, or a failed launch).
static inline void cpu_relax() {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
  __builtin_ia32_pause();
#endif
}
int wait_word(sc_ctx* c, HostWord idx) {
  volatile uint64_t* w = &c->pinned[idx];
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t spins = 0;
  while (*w == PIN_PENDING) {
    cpu_relax();
    if ((++spins & 255u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(1000)) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      break;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  if (*w == PIN_PENDING) { c->last_error = "a kernel did not deliver its result"; return SC_EHIP; }
  return SC_OK;
}

void fill_stats(const sc_ctx* c, sc_stats* s) {
  if (!s || s->size != sizeof(sc_stats)) return;
  s->n = (uint32_t)c->pass.n;
  s->edges = c->pass.E;
  s->tri_total = c->pass.M_total;
  s->tri_kept = c->pass.T_eff;
  s->tri_scored = c->pass.sh.n_local;
  s->workspace_bytes = c->held;
  // algorithmic bytes of this call (include/saccot.h): SURVEY §8d's per-stage formulas with the call's own counts
  const uint64_t n = (uint64_t)c->pass.n, nn8 = n * n / 8;
  const bool dense = !(c->pass.params.flags & SC_FLAG_NO_DENSE_S);
  s->bytes_moved = (dense ? 4 * n * n : 0) + nn8 + 24 * n          // A: S, bit rows, the correspondences
                   + nn8 + 20 * c->pass.E + 12 * c->pass.M + 16 * (uint64_t)c->pass.T_eff  // B: bit rows once, edge records, keys + {vertex, edge}, selection
                   + 52 * (uint64_t)c->pass.sh.n_local + 24 * n + n;   // C: (R,t) out and in, counts, the correspondences, the mask
}

float ev_us_raw(sc_ctx* c, int a, int b) {  // start / stop of kernel dispatches: nothing to subtract
  float ms = 0.f;
  if (hipEventSynchronize(c->ev[b]) != hipSuccess || hipEventElapsedTime(&ms, c->ev[a], c->ev[b]) != hipSuccess) {
    (void)hipGetLastError();
    return 0.f;
  }
  return ms > 0.f ? ms * 1000.f : 0.f;
}

float ev_us(sc_ctx* c, int a, int b) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, c->ev[a], c->ev[b]) != hipSuccess) { (void)hipGetLastError(); return 0.f; }
  const float us = ms * 1000.f - (c->ev_overhead_us > 0.f ? c->ev_overhead_us : 0.f);
  return us > 0.f ? us : 0.f;
}

int entry_checks(sc_ctx* c, const sc_params* p, unsigned checks) {
  if (checks & ENDS_FRAME) peel_end(c);
  if (checks & NOT_BUSY) SC_TRY(busy(c));
  if (checks & PARAMS) SC_TRY(check_params(p));
  if ((checks & ONE_RANK) && p->shard_world != 1) return SC_EINVAL;
  return SC_OK;
}

int points_to_device(sc_ctx* c, const float* src, const float* tgt, int64_t n) {
  ENSURE(c, c->in_src, (size_t)n * 12);
  ENSURE(c, c->in_tgt, (size_t)n * 12);
  HIPCHK(c, hipMemcpyAsync(c->in_src.p, src, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->in_tgt.p, tgt, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
  return SC_OK;
}

int outputs_to_host(sc_ctx* c, size_t n, float R[9], float t[3], uint8_t* mask) {
  float Rt[12];
  HIPCHK(c, hipMemcpyAsync(Rt, c->rt12.p, 48, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(mask, c->mask.p, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(R, Rt, 36);
  memcpy(t, Rt + 9, 12);
  return SC_OK;
}

}  // namespace sc

extern "C" {

int sc_version(void) { return (SC_VERSION_MAJOR << 16) | SC_VERSION_MINOR; }

const char* sc_strerror(int status) {
  switch (status) {
    case SC_OK: return "ok";
    case SC_EINVAL: return "invalid argument";
    case SC_ENOMEM: return "out of memory or workspace cap exceeded";
    case SC_EHIP: return "HIP runtime error";
    case SC_ERCCL: return "collective error";
    case SC_ENOHYP: return "no hypothesis: the compatibility graph has no triangle with an inlier";
    case SC_ETOOMANY: return "too many triangles for the workspace cap";
    case SC_ERETRY: return "a candidate blob was too small: repeat with sc_params.shard_cand_level + 1";
    case SC_EBOUND: return "the estimated pruning bound was too high: repeat without SC_FLAG_EST_BOUND";
    default: return "unknown status";
  }
}

void sc_default_params(sc_params* p) {
  if (!p) return;
  memset(p, 0, sizeof *p);
  p->size = sizeof(sc_params);
  p->sigma = 0.1f; p->t_cmp = 0.9f; p->tau = 0.1f; p->min_len = 0.1f;
  p->max_triangles = 50000;
  p->rank_mode = SC_RANK_WEIGHT;
  p->layout = SC_AOS;
  p->shard_rank = 0; p->shard_world = 1; p->shard_block = 1024;
  p->flags = 0; p->max_workspace = 0;
  p->score_mode = SC_SCORE_COUNT; p->shard_cand_level = 0;
}

int sc_create(int device, sc_ctx** out) {
  if (!out) return SC_EINVAL;
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) { (void)hipGetLastError(); return SC_EHIP; }  // no GPU: fail loudly
  if (device < 0 || device >= count) return SC_EINVAL;
  sc_ctx* c = new (std::nothrow) sc_ctx();
  if (!c) return SC_ENOMEM;
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return SC_EHIP;
  }
  c->stream = c->own_stream;
  for (int i = 0; i < N_EVENTS; i++)
    if (hipEventCreateWithFlags(&c->ev[i], hipEventDisableSystemFence) != hipSuccess) { sc_destroy(c); return SC_EHIP; }
  // the lane's fork and join (sc_ctx.hpp): no timestamps; the default fence of a record stays (the join orders a frame's outputs
  // in front of whatever the caller's stream does with them)
  if (hipEventCreateWithFlags(&c->lane_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->lane_join, hipEventDisableTiming) != hipSuccess) { sc_destroy(c); return SC_EHIP; }
  if (hipHostMalloc((void**)&c->pinned, N_PINNED * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) {
    sc_destroy(c);
    return SC_EHIP;
  }
  *out = c;
  return SC_OK;
}

void sc_destroy(sc_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);  // nullptr = the default stream
  if (c->on_lane) (void)hipStreamSynchronize(c->lane_home);  // (a lane frame outstanding: `stream` above was the lane)
  else if (c->own_stream && c->stream != c->own_stream) (void)hipStreamSynchronize(c->own_stream);  // (the lane: idle once the caller's stream has passed the join)
  for (sc_ctx::WgMap& m : c->wg_maps) if (m.buf.p) (void)hipFree(m.buf.p);
  for (size_t k = 0; k < N_WORKSPACE_BUFS; k++) if (workspace_bufs(c)[k].p) (void)hipFree(workspace_bufs(c)[k].p);  // every Buf of sc::Workspace
  for (int i = 0; i < N_EVENTS; i++) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  if (c->pinned) (void)hipHostFree(c->pinned);
  if (c->h_in) (void)hipHostFree(c->h_in);
  if (c->h_out) (void)hipHostFree(c->h_out);
  if (c->h_batch_off) (void)hipHostFree(c->h_batch_off);
  if (c->batch_off_ev) (void)hipEventDestroy(c->batch_off_ev);
  if (c->lane_fork) (void)hipEventDestroy(c->lane_fork);
  if (c->lane_join) (void)hipEventDestroy(c->lane_join);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

int sc_set_stream(sc_ctx* c, void* hip_stream) {
  if (!c) return SC_EINVAL;
  SC_TRY(busy(c));
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (no call is outstanding: `stream` is not the lane ...
  if (c->stream != c->own_stream) HIPCHK(c, hipStreamSynchronize(c->own_stream));  // ... which is drained as well)
  c->ev_overhead_us = -1.f;  // event cost differs between streams: calibrate again on the next timed call
  if (hip_stream == SC_STREAM_DEFAULT) c->stream = nullptr;  // the null stream
  else c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
  c->caller_stream = hip_stream != nullptr;
  return SC_OK;
}

const char* sc_last_error(const sc_ctx* c) { return c ? c->last_error.c_str() : "null context"; }

// sc_set_debug: the next call waits (its launch geometry may differ from the last call's), estimates again and takes its ordinals from
// the ordered strong list again.  The shape's history stays: the counts are the knobs' in no way.
static void reset_history(sc_ctx* c) { c->fast_ok = false; c->est.reset(); c->ord_off = false; }

int sc_set_debug(sc_ctx* c, const sc_debug* d) {
  if (!c) return SC_EINVAL;
  SC_TRY(busy(c));
  if (!d) { c->tn = Tuning(); reset_history(c); return SC_OK; }
  if (d->size != sizeof(sc_debug)) return SC_EINVAL;
  auto tg_ok = [](uint32_t t) { return t == 0 || t == 4 || t == 8 || t == 16 || t == 32 || t == 64; };
  for (int k = 0; k < 4; k++) if (!tg_ok(d->lanes_per_edge[k])) return SC_EINVAL;
  if (d->lanes_per_edge[0] == 64) return SC_EINVAL;  // the plain counting kernel has no 64-lane form
  if (d->score_split > 256 || (d->compat_rows != 0 && d->compat_rows != 16 && d->compat_rows != 32 && d->compat_rows != 64)) return SC_EINVAL;
  if (d->event_cap != 0 && d->event_cap < 256) return SC_EINVAL;
  Tuning t;
  t.no_events = d->no_events != 0;
  t.event_cap = d->event_cap;
  if (d->compact_self_max >= 0) t.compact_self_max = (size_t)d->compact_self_max;
  if (d->scan_self_max >= 0) t.scan_self_max = (size_t)d->scan_self_max;
  t.cnt_blocks = d->grid_blocks[0]; t.keys_blocks = d->grid_blocks[1]; t.sel_blocks = d->grid_blocks[2]; t.sample_blocks = d->grid_blocks[3];
  if (d->lanes_per_edge[0]) t.tg_count = (int)d->lanes_per_edge[0];
  if (d->lanes_per_edge[1]) t.tg_keys = (int)d->lanes_per_edge[1];
  if (d->lanes_per_edge[2]) t.tg_sample = (int)d->lanes_per_edge[2];
  if (d->lanes_per_edge[3]) t.tg_events = (int)d->lanes_per_edge[3];
  t.sample_edges = d->sample_edges;
  t.score_split = d->score_split;
  t.compat_one_phase = d->compat_one_phase != 0;
  t.compat_rows = (int)d->compat_rows;  // 0 (by size), 16, 32, 64: checked above
  t.compat_store_mode = d->compat_store_mode & 7u;
  t.compat_linear_order = d->compat_linear_order != 0;
  t.sample_mode = d->sample_mode <= 2 ? d->sample_mode : 0u;  // (!= 0 also keeps the estimate off: a certifying form was asked for)
  t.rows_unfused = d->rows_unfused != 0;
  t.score_filter = d->score_filter <= 3 ? d->score_filter : 0u;
  t.filter_splits = d->filter_splits;
  t.filter_queue_cap = d->filter_queue_cap;
  t.filter_lds_queue = d->filter_lds_queue;
  t.filter_blind = d->filter_blind != 0;
  t.gram_kappa_q4 = d->gram_kappa_q4;
  t.gram_ref_late = d->gram_ref_late != 0;
  t.no_fast = d->no_fast != 0;
  t.no_lane = d->no_lane != 0;
  t.gram_guard_fail = d->gram_guard_fail != 0;
  t.no_estimate = d->no_estimate != 0;
  t.no_edge_build = d->no_edge_build != 0;
  t.scan_ordinals = d->scan_ordinals != 0;
  t.ord_chunk_max = d->ord_chunk_max;
#ifdef SC_ABLATIONS
  t.filter_variant = d->filter_variant;  // (lab builds only: most values are timing-only bodies that return WRONG counts)
#endif
  t.est_margin_pct = d->est_margin_pct;
  c->tn = t;
  reset_history(c);
  return SC_OK;
}

int sc_debug_last(sc_ctx* c, sc_debug_info* out) {
  if (!c || !out || out->size != sizeof(sc_debug_info)) return SC_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  out->c2_kernel = c->pass.filter_on ? (uint32_t)c->pass.filter_mode : 0u;
  out->filter_splits = c->pass.filter_on ? c->pass.fx_plan.splits : 0u;
  out->filter_undecided = 0; out->filter_recounts = 0;
  out->fast_path = (uint32_t)c->frame.fast_state;
  out->gram_guard = c->tn.gram_guard_fail && c->gram_guard != 0 ? 2u : (uint32_t)c->gram_guard; out->gram_guard_worst = c->gram_guard_worst;
  out->prune_bound = c->frame.est_failed_call ? 2u : (uint32_t)c->pass.est_state; out->lane = c->frame.lane ? 1u : 0u;
  out->gram_near_corr = out->gram_near_hyp = out->gram_rows = out->gram_ref_votes_q8 = 0u; out->gram_ref = 0xFFFFFFFFu;
  out->us_c2_filter = (c->pass.hot_ext && c->pass.filter_on) ? ev_us_raw(c, 4, 11) : 0.f;
  out->n_frames = c->n_frames; out->n_fast_ok = c->n_fast_ok; out->n_fast_repeat = c->n_fast_repeat;
  out->n_est_ok = c->n_est_ok; out->n_est_fail = c->n_est_fail;
  out->cover_edges = c->pass.mode.E_cov; out->cover_triangles = c->pass.mode.M_cov; out->n_hostfree_grow = c->n_spec_grow;
  out->n_lane = c->n_lane;
  out->ordinals = (uint32_t)c->pass.form.ord_state; out->strong_edges = 0;
  if (c->pass.form.ord_state != 0 && c->ctl.p) {  // (the control block of the last call: zeroed by the next one's staging kernel)
    HIPCHK(c, hipMemcpyAsync(&out->strong_edges, &c->ctl.as<ControlBlock>()->n_strong, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (c->pass.filter_on && c->fx_state.p)
    HIPCHK(c, filter_read_counters(c->fx_state.p, c->pass.fx_plan, c->stream, &out->filter_undecided, &out->filter_recounts));
  if (c->pass.filter_on && c->pass.filter_mode == 2 && c->fx_frame.p) {
    uint32_t fr[5];
    HIPCHK(c, filter_read_frame(c->fx_frame.p, c->stream, fr));
    out->gram_near_corr = fr[0]; out->gram_near_hyp = fr[1]; out->gram_rows = fr[2]; out->gram_ref = fr[3]; out->gram_ref_votes_q8 = fr[4];
  }
  return SC_OK;
}

}  // extern "C" (the two halves below are internal)

namespace sc {

// An entry that continues what an earlier one began (the _end, shard and finalize entries): frame over, context free, the earlier
// half there — `otherwise` is the refusal's text — then the device
int continue_pass(sc_ctx* c, bool in_order, const char* otherwise) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  if (!in_order) { c->last_error = otherwise; return SC_EINVAL; }
  HIPCHK(c, hipSetDevice(c->device));
  return SC_OK;
}

// A frame starts here and nowhere else: every entry point that begins a call of its own (not the library's repeat of one) comes
// through here, and finds nothing of the previous frame
int frame_begin(sc_ctx* c) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  c->frame = Frame{};
  return SC_OK;
}
// A pass starts here and nowhere else (hyp_begin, sc_shard_compat_device): afterwards it holds its mode, its parameters and what follows
// from them, and "no" for everything else — no stage may assume anything an earlier pass did
static int pass_begin(sc_ctx* c, const sc_params* p, const PassMode& mode) {
  SC_TRY(busy(c));
  HIPCHK(c, hipSetDevice(c->device));
  c->pass = Pass{};
  c->pass.mode = mode;
  SC_TRY(set_timing(c, p));
  c->pass.refine = (p->flags & SC_FLAG_REFINE) != 0;
  c->cap_bytes = workspace_cap(p);
  c->pass.dv = derive(p);
  c->pass.params = *p;
  return SC_OK;
}

// A pass ends when its finalize step starts to wait (or its enqueue fails): nothing more is enqueued host-free, whichever way
// finalize_wait is left — validated, void, failed, timed out.  ensure() and tri_source_of() read the flag, so an entry that starts no
// pass of its own (a stage hook, a second finalize call) must not find it set.  Returns whether the pass was host-free.
bool pass_end(sc_ctx* c) { return std::exchange(c->pass.mode.host_free, false); }

// phase 1, first half: staging, stage A, the edge list and this process's share of the pruning sample
int hyp_begin(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p, uint32_t* d_hist,
              uint32_t part, uint32_t parts, const PassMode& mode) {
  SC_TRY(check_params(p));
  SC_TRY(pass_begin(c, p, mode));
  // SC_FLAG_EST_BOUND outside the sc_shard_* phase API: sc_hypothesize_device only (stages A and B replicated, every rank takes the
  // whole estimating sample; a shared histogram — sc_hypothesize_begin / _end_device — is a certifying sample's)
  if ((p->flags & SC_FLAG_EST_BOUND) && !(d_hist == nullptr && parts == 1 && mode.may_estimate)) {
    c->last_error = "SC_FLAG_EST_BOUND belongs to the sc_shard_* phase API and to sc_hypothesize_device";
    return SC_EINVAL;
  }
  c->pass.form.build = d_hist == nullptr && parts == 1 && edge_build_ok(c, p, n, mode.may_estimate);  // (the whole sample, own histogram: run_edges checks that it is told the same)
  SC_TRY(rec(c, 0));
  SC_TRY(stage_inputs(c, d_src, d_tgt, n, p));
  SC_TRY(rec(c, 1));
  SC_TRY(run_compat(c, !(p->flags & SC_FLAG_NO_DENSE_S)));
  SC_TRY(rec(c, 2));
  SC_TRY(run_row_stats(c, may_prune(p), true));
  SC_TRY(run_edges(c, p, d_hist, part, parts));
  c->pass.begun = true;
  return SC_OK;
}

// The coordinate statistics as the host words hold them now (mx all ones: not arrived; the boxes then mean nothing).
// flag, THEN data: the staging kernel writes the six box words before the word of maxima, so the maxima are loaded with
// acquire semantics and the boxes only afterwards (the fence used to sit behind both loads, which only the
// load order of x86 made right)
CoordStats read_coord_stats(const sc_ctx* c) {
  CoordStats cs;
  cs.mx = __atomic_load_n(&c->pinned[HW_COORD_MAX], __ATOMIC_ACQUIRE);
  for (int k = 0; k < 6; k++) cs.box[k] = *const_cast<volatile uint64_t*>(&c->pinned[HW_BOX + k]);
  return cs;
}
// ... and what stage C2's kernel is picked by: nothing when blind, else those — or the last completed call's
static CoordStats filter_stats(const sc_ctx* c) {
  CoordStats cs = read_coord_stats(c);
  if (c->tn.filter_blind) { cs.mx = ~0ull; return cs; }
  // A host-free call enqueued while the previous frame still runs (sc_register_device_async on a second context of the stream)
  // gets here before its own staging kernel has started: it is a repetition of the last call's shape, so it decides by the last
  // call's words.  Any choice gives the same counts (see above); decided blind, every such call ran the linear filter — at C2 53 us
  // against 27 (tools/r4/b2b.py).
  if (cs.mx == ~0ull && c->pass.mode.host_free && c->mx_last != ~0ull) {
    cs.mx = c->mx_last;
    for (int k = 0; k < 6; k++) cs.box[k] = c->box_last[k];
  }
  return cs;
}
// C2 by filter?  By mode / size / knobs (score_uses_filter), and — unless forced — only when tau is on a scale the filter
// can bound (a tau below ~2.4e-4 of the scene's extent, or above 8 x, would send every wave to the exact recount, which
// is slower than the plain kernel): the staging kernel has told the host the coordinate maxima long before this point.
static int use_filter(const sc_ctx* c, const sc_params* p, const Shard& sh) {
  const CoordStats cs = filter_stats(c);
  return score_filter_mode(p->score_mode, c->tn, c->pass.n, sh.ld_local, cs.mx, cs.mx == ~0ull ? nullptr : cs.box, c->pass.dv.tau2);
}
// The Gram filter's bound rests on a measured model of the matrix pipe (sc_gram_guard.hip, gram_guard_kernel): probe the pipe this
// context runs on, once, the first time a call would choose that filter.  0 not run, 1 the model holds, 2 violated.
static int run_gram_guard(sc_ctx* c) {
  if (c->gram_guard != 0) return SC_OK;
  ENSURE(c, c->guard_tmp, 64);
  float worst = 0.f; bool sub_ok = false; uint32_t compared = 0;
  const hipError_t e = gram_guard_probe(c->guard_tmp.p, c->stream, &worst, &sub_ok, &compared);
  if (e != hipSuccess) return fail_hip(c, e, "gram_guard_probe");
  c->gram_guard_worst = worst;
  c->gram_guard = (sub_ok && compared != 0 && worst <= gram_guard_limit()) ? 1 : 2;
  return SC_OK;
}
// Evaluated ONCE per call (decide_filter stores the answer in the context): the word it reads is written by the GPU, so
// two evaluations could disagree.  On the path the maxima have always arrived by then (the host has polled results of
// later kernels of the same stream); the stage hook waits for the word.  Not known (sc_debug.filter_blind forces that
// case) means "assume in range": the filter itself hands whatever it cannot bound to the exact recount, so the counts
// are the same either way, only slower.
int decide_filter(sc_ctx* c, const sc_params* p, const Shard& sh) {
  c->pass.filter_mode = use_filter(c, p, sh);
  if (c->pass.filter_mode == 2) {
    SC_TRY(run_gram_guard(c));
    if (c->gram_guard == 2 || c->tn.gram_guard_fail) {
      // this pipe does not add the way the Gram bound assumes (or a test says so): the linear filter, whose bound allows a
      // truncating accumulation, where tau is on its scale; the plain kernel otherwise
      // (the words as they are, where use_filter went by filter_stats: a host-free call whose own staging kernel has not run yet reads
      // "not known" here — ADVICE r05 #2.  The fix is filter_stats(c).mx in this line; it changes which kernel this branch picks)
      const uint64_t mx = c->tn.filter_blind ? ~0ull : read_coord_stats(c).mx;
      c->pass.filter_mode = filter_in_range(mx, c->pass.dv.tau2) ? 1 : 0;
    }
  }
  c->pass.filter_on = c->pass.filter_mode != 0;
  if (c->pass.filter_on) c->pass.fx_plan = filter_plan(c->pass.n, sh.ld_local, c->tn, (uint32_t)c->pass.filter_mode);
  return SC_OK;
}

// the filter's buffers for this pass's plan; filter_of(c) is taken behind it
static int ensure_filter(sc_ctx* c) {
  const FilterPlan& fp = c->pass.fx_plan;
  ENSURE(c, c->fx_tile, fp.tile_bytes);
  ENSURE(c, c->fx_state, fp.state_bytes);
  if (fp.coef_bytes) ENSURE(c, c->fx_coef, fp.coef_bytes);
  if (fp.mode == 2) SC_TRY(ensure_frame(c));
  return SC_OK;
}
// the views of the context's stage-C arrays (sc_kernels.hpp): the one place each Buf becomes a typed pointer.
// hyps_of: behind the ENSUREs of rt and rt_aos and behind decide_filter (aos: only where the exact pass will read it); t_eff_dev: a
// host-free call, or one with an estimated bound — the selection may turn out shorter than the T its launches were sized for (then the
// call is repeated); its real length is what the select left in sel.want
Hyps hyps_of(const sc_ctx* c) {
  return Hyps{c->pass.sh, c->pass.sh.n_local ? c->rt.as<float>() : nullptr, c->pass.filter_on ? c->rt_aos.as<float>() : nullptr,
              (c->pass.mode.host_free || c->pass.form.est_active) ? &c->ctl.as<ControlBlock>()->sel.want : nullptr};
}
FilterBufs filter_of(const sc_ctx* c) {
  return FilterBufs{c->pass.fx_plan, c->fx_tile.p, c->fx_state.p, c->fx_coef.p, c->fx_frame.p, c->fx_mx.as<uint32_t>()};
}

// C2: the counts of the hypotheses h into c->partial; *out: that array and the rows of it the arg-max has to add up.
// SC_SCORE_COUNT runs the matrix-pipe filter + the exact fix-up (sc_filter.hip); the truncated scores, and
// sc_debug.score_filter = 1, the plain fp32 kernel.
int run_score(sc_ctx* c, const sc_params* p, const Hyps& h, Partial* out, bool tile_done, const Stamps& ev) {
  if (c->pass.filter_on) {  // decide_filter() ran earlier in this call
    const FilterPlan& fp = c->pass.fx_plan;
    ENSURE(c, c->partial, (size_t)fp.splits * h.sh.ld_local * 4);
    *out = Partial{c->partial.as<uint32_t>(), fp.splits};
    if (!tile_done) SC_TRY(ensure_filter(c));  // (the stage hook; the path builds the tile inside the Kabsch launch)
    const FilterBufs fb = filter_of(c);
    if (!tile_done) {
      const FilterTileJob job = filter_tile_job(fb, h.sh.ld_local, c->pass.dv.tau2);
      if (fp.mode == 2)  // the frame first: tile and coefficients are made in it (the hypotheses exist already: it votes among them)
        launch_gram_ref(points_of(c), nullptr, h, fb, c->pass.dv.tau2, c->tn, c->stream);
      launch_filter_tile(points_of(c), job, c->stream);
      if (fp.mode == 2) launch_gram_coef(h, c->pass.dv.tau2, job.coef, c->stream);
    }
    launch_score_filter(points_of(c), h, fb, *out, ev, c->pass.dv, c->tn, c->stream);
    return SC_OK;
  }
  const uint32_t rows = score_chunks(c->pass.n, h.sh.ld_local);
  if (h.sh.ld_local) ENSURE(c, c->partial, (size_t)rows * h.sh.ld_local * 4);
  *out = Partial{c->partial.as<uint32_t>(), rows};
  launch_score(points_of(c), h, *out, ev, c->pass.dv, p->score_mode, c->tn, c->stream);
  return SC_OK;
}

// stage C on this rank's blocks of the (replicated) selection: C1, C2, arg-max key pair -> d_key
static int run_stage_c(sc_ctx* c, uint64_t* d_key, sc_stats* stats) {
  const sc_params* p = &c->pass.params;
  SC_TRY(rec(c, 3));
  Shard sh;
  sh.T_eff = c->pass.T_eff;
  sh.block = p->shard_block ? p->shard_block : 1024u;
  sh.rank = (uint32_t)p->shard_rank;
  sh.world = (uint32_t)p->shard_world;
  sh.n_local = shard_local_count(sh.T_eff, sh.block, sh.rank, sh.world);
  sh.ld_local = (uint32_t)(((uint64_t)sh.n_local + 255u) / 256u * 256u);  // T <= 2^32 - 256 (check_params)
  c->pass.sh = sh;
  c->pass.filter_on = false; c->pass.filter_mode = 0;  // (nothing to score: no filter; else decide_filter says)
  if (sh.n_local) {
    ENSURE(c, c->rt, (size_t)12 * sh.ld_local * 4);
    ENSURE(c, c->cnt, (size_t)sh.ld_local * 4);
    SC_TRY(decide_filter(c, p, sh));
    if (c->pass.filter_on) { ENSURE(c, c->rt_aos, (size_t)12 * sh.ld_local * 4); SC_TRY(ensure_filter(c)); }  // (rt_aos: the exact pass reads 12 consecutive floats per hypothesis)
  }
  const Hyps h = hyps_of(c);  // once, behind the ENSUREs of rt, cnt and rt_aos: every launch of the stage takes this one
  if (sh.n_local) {
    const TriSource ts = tri_source_of(c);
    FilterTileJob job;
    if (c->pass.filter_on) {
      const FilterBufs fb = filter_of(c);
      job = filter_tile_job(fb, sh.ld_local, c->pass.dv.tau2);
      if (fb.plan.mode == 2 && !c->pass.ref_done)  // the Gram filter's reference frame, where the counting pass did not carry the vote: among 64 hypotheses of the selection
        launch_gram_ref(points_of(c), &ts, h, fb, c->pass.dv.tau2, c->tn, c->stream);
    }
    launch_kabsch(points_of(c), ts, h, c->pass.filter_on ? &job : nullptr, c->stream);
  }
  // SC_FLAG_TIMING_HOT: the score stage's duration from the dispatch packets of its own kernels (no record on the stream:
  // the two records of a bracket opened ~4.5 us gaps before and after the stage — 3 % of a C2 step)
  const bool hot_ext = c->pass.timing_hot && sh.n_local != 0;
  c->pass.hot_ext = hot_ext;
  if (!hot_ext) SC_TRY(rec(c, 4));
  Partial partial{};
  SC_TRY(run_score(c, p, h, &partial, true, hot_ext ? Stamps{c->ev[4], c->ev[5], c->ev[11]} : Stamps{}));
  if (!hot_ext) SC_TRY(rec(c, 5));
  ENSURE(c, c->amx_pairs, argmax_scratch_bytes(sh.ld_local));
  // the winner pair: reduced by the launch for a caller that gathers it; left as one pair per workgroup for this context's own
  // finalize step (sc_register*: d_key is the context's own word), whose workgroups reduce them themselves
  const bool own_pairs = d_key == c->key.as<uint64_t>() && sh.n_local != 0;
  c->pass.amx_blocks = own_pairs ? argmax_blocks(sh.ld_local) : 0u;
  launch_argmax(sh, partial, ArgmaxOut{c->pass.T_eff ? c->sel_key.as<uint32_t>() : nullptr, c->cnt.as<uint32_t>(), c->amx_pairs.as<uint64_t>(),
                                       &c->ctl.as<ControlBlock>()->amx_ticket, own_pairs ? nullptr : d_key}, c->stream);
  SC_TRY(rec(c, 6));
  HIPCHK(c, hipGetLastError());
  c->pass.have_hyp = true;
  fill_stats(c, stats);  // counts only: the event times are read by sc_finalize_device, after ITS synchronisation
  return SC_OK;
}

// phase 1, second half: prune with the (summed) histogram, enumerate, select, then stage C on this rank's share
int hyp_end(sc_ctx* c, const uint32_t* d_hist, uint64_t* d_key, sc_stats* stats) {
  const sc_params* p = &c->pass.params;
  c->pass.begun = false;
  SC_TRY(run_select(c, p, d_hist, false));
  return run_stage_c(c, d_key, stats);
}

}  // namespace sc

extern "C" {

int sc_hypothesize_device(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p,
                          uint64_t* d_key, sc_stats* stats) {
  if (!c || !d_src || !d_tgt || !d_key) return SC_EINVAL;
  // SC_FLAG_EST_BOUND (r04b): stage B pruned by an estimated bound, like sc_register_device's — the select verifies it and
  // sc_finalize(_gathered)_device returns SC_EBOUND when it was too high (on every rank of a job alike: stages A and B are
  // replicated and deterministic): the caller repeats both calls without the flag
  const bool est = p && p->size == sizeof(sc_params) && (p->flags & SC_FLAG_EST_BOUND) != 0;
  SC_TRY(frame_begin(c));
  // r04c: with the flag, a call that repeats the last call's shape on this context is enqueued HOST-FREE, as sc_register_device's
  // is (fast_plan): no wait for stage B's two counts — the rank's host thread is free to enqueue the job's next frame.  The
  // finalize call validates; a count that outgrew what the launches covered comes back as SC_EBOUND too ("repeat both calls
  // without the flag" — the waiting, certifying way handles every case), on every rank alike: stages A and B are replicated.
  PassMode mode{est};
  if (est && check_params(p) == SC_OK) fast_plan(c, n, p, &mode);
  if (est) c->est.caller_decides();  // (the CALLER decides when to stop estimating on this entry; fast_plan above still went by the context's own verdict)
  int rc = hyp_begin(c, d_src, d_tgt, n, p, nullptr, 0, 1, mode);  // the whole sample, into the context's histogram
  if (rc == SC_OK) rc = hyp_end(c, nullptr, d_key, stats);
  if (rc != SC_OK && mode.host_free) c->fast_ok = false;
  if (rc != SC_OK) pass_end(c);  // (what was enqueued is void: no covers for whatever comes next)
  return rc;
}

int sc_hypothesize_begin_device(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p,
                                uint32_t* d_hist, sc_stats* stats) {
  if (!c || !d_src || !d_tgt || !d_hist || !p || p->size != sizeof(sc_params)) return SC_EINVAL;
  SC_TRY(frame_begin(c));
  const int rc = hyp_begin(c, d_src, d_tgt, n, p, d_hist, (uint32_t)p->shard_rank, (uint32_t)p->shard_world, PassMode{});
  if (rc == SC_OK) fill_stats(c, stats);
  return rc;
}

int sc_hypothesize_end_device(sc_ctx* c, const uint32_t* d_hist, uint64_t* d_key, sc_stats* stats) {
  if (!c || !d_hist || !d_key) return SC_EINVAL;
  SC_TRY(continue_pass(c, c->pass.begun, "sc_hypothesize_end_device without a preceding sc_hypothesize_begin_device"));
  return hyp_end(c, d_hist, d_key, stats);
}

// ---- sharded A + B ------------------------------------------------------------------------

int sc_shard_plan_query(const sc_params* p, int64_t n, sc_shard_plan* out) {
  if (!out || out->size != sizeof(sc_shard_plan)) return SC_EINVAL;
  SC_TRY(check_params(p));
  if (n < 3 || n > (1 << 24) || p->shard_world > 64) return SC_EINVAL;
  const uint64_t ld = (uint64_t)round_up((int)n, 64), W = ld >> 6, G = (uint64_t)p->shard_world;
  const uint64_t R = (((uint64_t)n + G - 1) / G + 63) / 64 * 64;  // rows per rank, a multiple of the tile block
  out->rows_per_rank = (uint32_t)R;
  out->words_per_row = (uint32_t)W;
  out->bits_bytes_per_rank = R * W * 8;
  out->bits_bytes_total = G * R * W * 8;
  out->cand_bytes_per_rank = cand_blob_bytes(cand_cap(p->max_triangles, (uint32_t)p->shard_world, p->shard_cand_level));
  return SC_OK;
}

int sc_shard_compat_device(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p,
                           void* d_bits_all) {
  if (!c || !d_src || !d_tgt || !d_bits_all) return SC_EINVAL;
  SC_TRY(check_params(p));
  if (p->shard_world > 64) return SC_EINVAL;
  SC_TRY(frame_begin(c));
  SC_TRY(pass_begin(c, p, PassMode{}));  // (waited, certified bounds, the separate kernels)
  SC_TRY(rec(c, 0));
  SC_TRY(stage_inputs(c, d_src, d_tgt, n, p));
  SC_TRY(rec(c, 1));
  sc_shard_plan plan; plan.size = sizeof plan;
  SC_TRY(sc_shard_plan_query(p, n, &plan));
  const int R = (int)plan.rows_per_rank;
  const int r0 = p->shard_rank * R < c->pass.n ? p->shard_rank * R : c->pass.n, r1 = r0 + R < c->pass.n ? r0 + R : c->pass.n;
  const size_t W = (size_t)c->pass.ld >> 6;
  const bool dense = !(p->flags & SC_FLAG_NO_DENSE_S);
  if (dense && r1 > r0) ENSURE(c, c->S, (size_t)(r1 - r0) * c->pass.ld * sizeof(float));  // this rank's rows of S only
  ENSURE(c, c->deg, (size_t)c->pass.n * sizeof(uint32_t));
  ENSURE(c, c->degp, (size_t)c->pass.n * sizeof(uint32_t));
  ENSURE(c, c->wpre, (size_t)c->pass.n * W * sizeof(uint32_t));
  c->pass.bits_cur = static_cast<uint64_t*>(d_bits_all);
  c->pass.sharded_ab = true;
  // world == 1: [0, n) -> the symmetric tiles; else the one-sided row-block form, bit rows at their global index
  launch_compat(points_of(c), CompatOpts{}, c->pass.dv, dense ? c->S.as<float>() : nullptr, c->pass.bits_cur, r0, r1, c->tn, c->stream);
  SC_TRY(rec(c, 2));
  HIPCHK(c, hipGetLastError());
  c->pass.shard_phase = 1;
  return SC_OK;
}

int sc_shard_edges_device(sc_ctx* c, uint32_t* d_hist) {
  if (!c || !d_hist) return SC_EINVAL;
  SC_TRY(continue_pass(c, c->pass.sharded_ab && c->pass.shard_phase == 1, "sc_shard_edges_device: call sc_shard_compat_device first"));
  const sc_params* p = &c->pass.params;
  c->pass.shard_phase = 0;
  SC_TRY(run_row_stats(c, may_prune(p), true));
  SC_TRY(run_edges(c, p, d_hist, (uint32_t)p->shard_rank, (uint32_t)p->shard_world));
  c->pass.shard_phase = 2;
  return SC_OK;
}

int sc_shard_select_device(sc_ctx* c, const uint32_t* d_hist, void* d_cand_mine) {
  if (!c || !d_hist || !d_cand_mine) return SC_EINVAL;
  SC_TRY(continue_pass(c, c->pass.sharded_ab && c->pass.shard_phase == 2, "sc_shard_select_device: call sc_shard_edges_device first"));
  const sc_params* p = &c->pass.params;
  c->pass.shard_phase = 0;
  SC_TRY(run_select(c, p, d_hist, false));   // this rank's own top-T, in (i,j,k) order
  const CandBlob b = cand_blob(d_cand_mine, cand_cap(p->max_triangles, (uint32_t)p->shard_world, p->shard_cand_level));
  if (c->pass.M == 0) {  // nothing enumerated here (also E == 0): an empty blob
    HIPCHK(c, hipMemsetAsync(b.hdr, 0, CAND_HDR_WORDS * 8, c->stream));
  } else {
    launch_cand_emit(selection_of(c), keys_of(c), edges_of(c), counts_of(c), c->pass.T_eff,
                     // a full-length list (T entries) is never "cut": the global top-T takes at most T from one rank
                     select_want(c, p) < p->max_triangles ? (uint64_t)c->pass.T_eff : ~0ull, b, c->stream);
  }
  HIPCHK(c, hipGetLastError());
  c->pass.shard_phase = 3;
  return SC_OK;
}

int sc_shard_score_device(sc_ctx* c, const void* d_cand_all, uint64_t* d_key, sc_stats* stats) {
  if (!c || !d_cand_all || !d_key) return SC_EINVAL;
  SC_TRY(continue_pass(c, c->pass.sharded_ab && c->pass.shard_phase == 3, "sc_shard_score_device: call sc_shard_select_device first"));
  const sc_params* p = &c->pass.params;
  c->pass.shard_phase = 0;
  hipStream_t st = c->stream;
  const uint32_t T = p->max_triangles, G = (uint32_t)p->shard_world;
  const size_t cap = cand_cap(T, G, p->shard_cand_level);
  const size_t blob_bytes = cand_blob_bytes(cap);
  c->pass.cand_all = d_cand_all; c->pass.cand_bytes = blob_bytes;
  // Merge: the same exact select + (i,j,k)-order compaction as on one GPU, over the concatenated candidate keys.
  ControlBlock* ctl = c->ctl.as<ControlBlock>();
  SelectState* sel = &ctl->sel;
  const KeyView view = cand_view(d_cand_all, blob_bytes, G, cap);
  const size_t nb = compact_blocks(view.M);
  SC_TRY(ensure_compaction(c, nb, nb, T));  // (no room beyond the need: no host-free call comes here)
  arm_word(c, HW_MERGED_T);
  c->pinned[HW_MERGE_SHORT] = 0;  // "an estimated bound promised T keys above it and the merged candidates hold fewer" (merge_prepare_kernel)
  launch_merge_prepare(d_cand_all, blob_bytes, G, T, window_known(p), &ctl->klb, sel, &c->pinned[HW_MERGED_T],
                       c->pass.form.est_active ? &c->pinned[HW_MERGE_SHORT] : nullptr, st);
  launch_select_rounds(view, sel, select_rounds(window_known(p)), nullptr, c->tn, st);
  c->pinned[HW_CAND_CUT] = 0;  // "a cut candidate list could have mattered": read by the finalize call (SC_ERETRY)
  SC_TRY(run_compaction(c, view, nb, select_rounds(window_known(p)), nullptr));
  launch_merge_check(d_cand_all, blob_bytes, G, sel, &c->pinned[HW_CAND_CUT], st);  // (behind the compaction: its counting kernel is what resolves the last round into k*)
  // the merged length, published by merge_prepare long before the compaction ends: the poll costs no GPU time
  SC_TRY(wait_word(c, HW_MERGED_T));
  c->pass.T_eff = (uint32_t)c->pinned[HW_MERGED_T];
  c->pass.M = c->pass.M_total = c->pinned[HW_MERGED_M];
  return run_stage_c(c, d_key, stats);
}

}  // extern "C"
