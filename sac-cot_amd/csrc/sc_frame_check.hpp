// sc_frame_check.hpp — the host-only rules of a frame's end (sc_capi_frame.hip) and of what a completed call leaves for the next one:
// how finalize_wait is left once the winner word has arrived (FrameEnd, frame_end) and what each way of leaving does (frame_end_row),
// the estimate's history (EstHistory) and the shape's (ShapeHistory: the last counts and the window of maxima the covers are sized
// by).  All of it is a function of a few host words and flags, said here without a context.  No HIP: sc_ctx.hpp includes it, and so
// does tests/native/frame_check_main.cpp, which runs these rules under the sanitizers on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "../../include/saccot.h"

#pragma GCC visibility push(hidden)  // (inline functions of the library's own: no part of its dynamic symbol table)
namespace sc {

constexpr int SC_ESPEC = -100;           // internal: the library repeats the call the waiting way (never leaves the library)
constexpr uint64_t PIN_PENDING = ~0ull;  // a host word whose kernel has not delivered yet (wait_word polls it)

// ---- the counts of a host-free frame ---------------------------------------------------------------------------------------------

// (b) of "what a host-free frame assumes" (sc_capi_tri.hip): a graph big enough to prune, E and M within what the launches cover,
// and T triangles found
inline bool counts_fit(uint64_t E, uint64_t M, uint64_t E_cov, uint64_t M_cov, uint32_t T) {
  return E >= 4096 && E <= E_cov && M <= M_cov && M >= (uint64_t)T;
}
// The finalize kernel hands both counts over in one word (DeferredPub): the low half the edges, the high half the triangles; a word
// that never arrived leaves both pending
struct Counts { uint64_t E, M; };
inline Counts unpack_counts(uint64_t word) {
  return word == PIN_PENDING ? Counts{PIN_PENDING, PIN_PENDING} : Counts{word & 0xFFFFFFFFull, word >> 32};
}
// HW_EV_OVERFLOW: the low half counts what overflowed; the high half says that it was the ordered strong list's chunk count, not —
// or not only — an event region
inline bool events_overflowed(uint64_t ev_overflow) { return (uint32_t)ev_overflow != 0; }
inline bool chunks_overflowed(uint64_t ev_overflow) { return (ev_overflow >> 32) != 0; }

// ---- the verdict -----------------------------------------------------------------------------------------------------------------

// What finalize_wait knows once the winner word has arrived: the pass's flags and the host words, each read once (frame_facts)
struct FrameFacts {
  bool host_free = false;       // the pass was enqueued host-free (pass_end's answer)
  uint64_t bad_input = 0;       // HW_BAD_INPUT
  uint64_t counts = 0;          // HW_EDGES as the finalize kernel of a host-free frame leaves it: both counts, packed
  uint64_t ev_overflow = 0;     // HW_EV_OVERFLOW
  uint64_t select_short = 0;    // HW_SELECT_SHORT
  uint64_t merge_short = 0;     // HW_MERGE_SHORT
  uint64_t cand_cut = 0;        // HW_CAND_CUT
  uint64_t winner_pos = 0;      // HW_WINNER_POS
  uint64_t winner_key = 0;      // HW_WINNER
  bool est_active = false;      // StageBForm::est_active
  bool est_void = false;        // Pass::est_void
  bool sharded_ab = false;      // Pass::sharded_ab
  bool cand_all = false;        // Pass::cand_all != nullptr: the selection indexes gathered candidate blobs
  bool est_bound_flag = false;  // SC_FLAG_EST_BOUND: the caller repeats, not the library
  uint64_t E_cov = 0, M_cov = 0;  // what the launches of a host-free frame covered
  uint32_t T = 0;               // sc_params::max_triangles
};

// a host-free frame that has run: the launches covered E_cov edges and M_cov keys and assumed T triangles exist, an event list that
// did not overflow and a graph big enough to prune
inline bool hostfree_valid(const FrameFacts& f) {
  const Counts k = unpack_counts(f.counts);
  return k.E != PIN_PENDING && k.M != PIN_PENDING && counts_fit(k.E, k.M, f.E_cov, f.M_cov, f.T) && !events_overflowed(f.ev_overflow);
}

// The ways finalize_wait is left behind the winner word, in the order in which they are asked: the first that applies wins.
enum class FrameEnd {
  BadInput,      // host-free: a coordinate was not finite
  HostfreeVoid,  // host-free: a count outgrew its cover, fewer than T triangles, a small graph, an overflow
  ShardBound,    // sharded stage B estimated, and the merge found the bound too high (or it went unverified)
  CertShort,     // the select came up short under a CERTIFIED bound: a defect
  CallerBound,   // the estimate failed and the caller repeats (SC_FLAG_EST_BOUND)
  EstFailed,     // the estimate failed and the library repeats
  CandCut,       // sharded: a cut candidate list could have mattered
  BadPair,       // the winner pair points outside the selection
  Found,         // a winner
  NoHypothesis,  // a complete call without one
};
constexpr int N_FRAME_ENDS = (int)FrameEnd::NoHypothesis + 1;

inline FrameEnd frame_end(const FrameFacts& f) {
  if (f.host_free && (uint32_t)f.bad_input != 0) return FrameEnd::BadInput;
  if (f.host_free && !hostfree_valid(f)) return FrameEnd::HostfreeVoid;
  if (f.sharded_ab && f.est_active && (f.merge_short != 0 || f.est_void)) return FrameEnd::ShardBound;
  if (f.select_short != 0 || (f.est_active && f.est_void)) {
    // select_round_kernel: fewer keys at or above the pruning bound than it promised (or the bound went unverified).  A CERTIFIED
    // bound holds by construction: that would be a defect, not an input
    if (!f.est_active) return FrameEnd::CertShort;
    return f.est_bound_flag ? FrameEnd::CallerBound : FrameEnd::EstFailed;
  }
  if (f.sharded_ab && f.cand_all && f.cand_cut != 0) return FrameEnd::CandCut;
  if (f.winner_pos == ~0ull) return FrameEnd::BadPair;
  return f.winner_key != 0 ? FrameEnd::Found : FrameEnd::NoHypothesis;
}

// What each way of leaving does — apply_verdict (sc_capi_frame.hip) is the only reader.
struct FrameEndRow {
  int status;               // what finalize_wait returns
  const char* text;         // last_error (nullptr: untouched; HostfreeVoid: formatted, frame_end_text)
  bool validated;           // the frame got past the host-free validation: a host-free frame's real counts are taken over, est_state is set
  bool clears_fast_ok;      // the next call waits
  bool est_failed_call;     // Frame::est_failed_call: a pass of this frame saw its estimate fail
  bool est_fails;           // EstHistory::fail: the context certifies for a while
  bool repairs_overflow;    // an overflow sets ord_off (chunks) or doubles the event capacity (events): the repeat must not overflow again
  bool completes;           // note_completed runs: the call is complete and files its history
};

namespace frame_text {
// SC_EBOUND: the caller repeats the call without the flag (include/saccot.h), on every rank alike
constexpr const char* BOUND_TOO_HIGH = "the estimated pruning bound was too high for this input: repeat the call without SC_FLAG_EST_BOUND";
constexpr const char* BAD_INPUT = "non-finite input coordinate";
constexpr const char* CERT_SHORT = "internal: the select found fewer keys above a certified pruning bound than the certificate counted";
constexpr const char* EST_FAILED = "estimated pruning bound too high: call repeated with a certifying sample";
constexpr const char* CAND_CUT = "a candidate blob was too small for this input: repeat the call with sc_params.shard_cand_level raised by one";
constexpr const char* BAD_PAIR = "a winner key pair points outside the selected list (stale / uninitialised pair, or ranks that disagree on T or the parameters)";
}  // namespace frame_text

inline const FrameEndRow& frame_end_row(FrameEnd e) {
  using namespace frame_text;
  static const FrameEndRow rows[N_FRAME_ENDS] = {
      //                 status      text            validated fast_ok est_call est_fails overflow completes
      /* BadInput     */ {SC_EINVAL, BAD_INPUT,      false,    true,   false,   false,    false,   false},
      /* HostfreeVoid */ {SC_ESPEC,  nullptr,        false,    true,   false,   false,    true,    false},
      // (every rank holds the same gathered blobs, so every rank ends here together)
      /* ShardBound   */ {SC_EBOUND, BOUND_TOO_HIGH, true,     false,  false,   false,    false,   false},
      /* CertShort    */ {SC_EHIP,   CERT_SHORT,     true,     false,  false,   false,    false,   false},
      // (sc_hypothesize_device + sc_finalize*_device)
      /* CallerBound  */ {SC_EBOUND, BOUND_TOO_HIGH, true,     false,  true,    false,    false,   false},
      /* EstFailed    */ {SC_ESPEC,  EST_FAILED,     true,     true,   true,    true,     false,   false},
      // (merge_check_kernel: some rank's candidate list was cut at a key the merged threshold does not clear)
      /* CandCut      */ {SC_ERETRY, CAND_CUT,       true,     false,  false,   false,    false,   false},
      // (finalize_kernel: a pair decodes to a position outside the selection; outputs: identity, zero mask)
      /* BadPair      */ {SC_EINVAL, BAD_PAIR,       true,     false,  false,   false,    false,   false},
      /* Found        */ {SC_OK,     nullptr,        true,     false,  false,   false,    false,   true},
      /* NoHypothesis */ {SC_ENOHYP, nullptr,        true,     false,  false,   false,    false,   true},
  };
  return rows[(int)e];
}

// last_error of a verdict ("": the verdict leaves it alone).  HostfreeVoid says why, for sc_last_error: the repeat itself is silent.
inline std::string frame_end_text(FrameEnd e, const FrameFacts& f) {
  if (e == FrameEnd::HostfreeVoid) {
    const Counts k = unpack_counts(f.counts);
    char buf[256];
    snprintf(buf, sizeof buf, "host-free call repeated: edges %llu (covered %llu), triangles %llu (covered %llu, T %u), event overflow %u",
             (unsigned long long)k.E, (unsigned long long)f.E_cov, (unsigned long long)k.M, (unsigned long long)f.M_cov, f.T,
             (uint32_t)f.ev_overflow);
    return buf;
  }
  const char* text = frame_end_row(e).text;
  return text ? text : "";
}

// ---- the estimate's history ------------------------------------------------------------------------------------------------------

// An estimate that failed on this context: it certifies for the next `holdoff` completed calls — and not for ever.  One frame whose
// estimate fails — a change of scene — used to cost the context its estimating sample (25 us per C2 call) for the rest of its life;
// now the k-th failure costs 64 << min(k - 1, 6) certifying calls, then the context estimates again: a stream whose estimates always
// fail wastes one repeated call in 4096.
struct EstHistory {
  bool failed = false;  // the context certifies (edge_build_ok, form_begin)
  uint32_t holdoff = 0, failures = 0;
  void reset() { *this = EstHistory{}; }  // (sc_set_debug)
  void fail() {
    failed = true;
    failures++;
    holdoff = 64u << (failures - 1 < 6 ? failures - 1 : 6);
  }
  // a call completed (note_completed); this_frame_failed: it is the repeat of the frame whose estimate failed, which does not count
  void completed(bool this_frame_failed) {
    if (failed && !this_frame_failed && holdoff != 0 && --holdoff == 0) failed = false;
  }
  // sc_hypothesize_device with SC_FLAG_EST_BOUND: the CALLER decides when to stop estimating on that entry
  void caller_decides() { failed = false; }
};

// ---- the shape's history ---------------------------------------------------------------------------------------------------------

// The last completed call's counts and shape, and what the covers of a host-free repetition are sized by.  A stream of DIFFERENT
// frames of one shape (bench.py's: 32 scenes whose inlier ratio moves the edge count by 1.6 x and the triangle count by 4 x) outgrew
// "the last call's counts plus half" in a frame out of six; the covers follow the largest counts of the last HI_WINDOW .. 2 HI_WINDOW
// regular calls of the shape (two buckets: the current one and the one before it), so a stream pays for the spread of its frames
// once.  A change of shape empties the window.
struct ShapeHistory {
  static constexpr uint32_t HI_WINDOW = 64, HI_YOUNG = 8;
  enum Which { EDGES, KEYS };
  uint64_t E_last = 0, M_last = 0;
  int n = 0;
  sc_params p{};
  uint64_t E_hi[2] = {0, 0}, M_hi[2] = {0, 0};
  uint32_t hi_n = 0, hi_seen = 0;  // calls in the current bucket; regular calls of this shape seen so far (saturating)

  // the parameters that make two calls "the same shape" (a host-free call repeats the last call's; timing flags aside)
  static bool same_shape(const sc_params* p, const sc_params* q) {
    constexpr uint32_t TIMING_BITS = SC_FLAG_TIMING | SC_FLAG_TIMING_HOT | SC_FLAG_TIMING_ONE | (15u << 8);
    return p->sigma == q->sigma && p->t_cmp == q->t_cmp && p->tau == q->tau && p->min_len == q->min_len &&
           p->max_triangles == q->max_triangles && p->rank_mode == q->rank_mode && p->layout == q->layout &&
           p->shard_world == q->shard_world && p->shard_rank == q->shard_rank && p->shard_block == q->shard_block &&
           p->score_mode == q->score_mode && (p->flags & ~TIMING_BITS) == (q->flags & ~TIMING_BITS);
  }
  // a call of n_ correspondences with p_ continues the shape of the last completed call
  bool continues(int64_t n_, const sc_params* p_) const { return n_ == n && same_shape(p_, &p); }
  void forget_window() { E_hi[0] = E_hi[1] = M_hi[0] = M_hi[1] = 0; hi_n = 0; hi_seen = 0; }
  // A call completed (note_completed).  regular: a host-free repetition may follow it (sc_ctx::fast_ok) — its counts are what such a
  // repetition has to cover
  void note(bool regular, uint64_t E, uint64_t M, int n_, const sc_params& p_) {
    if (!continues(n_, &p_)) forget_window();
    if (regular) {
      if (hi_seen < 0xFFFFFFFFu) hi_seen++;
      if (E > E_hi[0]) E_hi[0] = E;
      if (M > M_hi[0]) M_hi[0] = M;
      if (++hi_n >= HI_WINDOW) { E_hi[1] = E_hi[0]; M_hi[1] = M_hi[0]; E_hi[0] = M_hi[0] = 0; hi_n = 0; }
    }
    E_last = E; M_last = M; n = n_; p = p_;
  }
  // While the shape is young on this context the last count is doubled (cover_of): the first frames of a stream say little about the
  // spread of the frames to come, and a miss costs a whole repeated call (bench.py's stream, frames of 386 k .. 697 k edges: with
  // "plus half" from the first frame on, one of the first twenty was repeated).
  bool young() const { return hi_seen < HI_YOUNG; }
  // what a host-free repetition of the shape is sized to cover (fast_plan): cover(E_last, E_hi), cover(M_last, M_hi)
  uint64_t cover(uint64_t last, const uint64_t hi[2]) const { return cover_of(last, hi, young()); }
  // entries a waited call leaves in an array indexed by one of stage B's two counts: what the host-free repetitions of its shape
  // will want to cover (the window's maxima only while the shape continues: note() empties it after a change)
  uint64_t room(uint64_t count, Which which, bool continues_) const {
    static const uint64_t none[2] = {0, 0};
    return cover_of(count, !continues_ ? none : which == EDGES ? E_hi : M_hi, !continues_ || young());
  }

 private:
  static uint64_t cover_of(uint64_t last, const uint64_t hi[2], bool young_) {
    const uint64_t h = hi[0] > hi[1] ? hi[0] : hi[1];
    const uint64_t b = h + h / 4;
    // young: twice the last count (or the window's maximum plus a quarter, if larger); later the window alone decides — the last
    // count is in it — so that a stream's covers stay put from frame to frame instead of following every large frame by half
    // (a cover beyond 2^20 edges takes the scan's two-launch form, and every launch sized by it grows with it)
    const uint64_t a = young_ ? 2 * last : (h ? 0 : last + last / 2);
    return (a > b ? a : b) + 4096;
  }
};

}  // namespace sc
#pragma GCC visibility pop
