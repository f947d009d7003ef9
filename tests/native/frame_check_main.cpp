// Stand-alone program for the host-only rules of a frame's end (sac-cot_amd/csrc/sc_frame_check.hpp): the verdict on a frame that has
// run — every way of leaving, the priority between them, the packed word of a host-free frame's counts —, the table of what each
// verdict does, the estimate's hold-off arithmetic and the covers of the shape's history.  Every expected value is written out here
// by hand; none is computed by the header.  tests/test_frame_check.py builds it with -fsanitize=address,undefined and runs it on the
// CPU: no GPU, no Python in the process.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../sac-cot_amd/csrc/sc_frame_check.hpp"

using sc::EstHistory;
using sc::FrameEnd;
using sc::FrameFacts;
using sc::ShapeHistory;

static int failures = 0;

static void check(const char* what, bool ok) {
  if (!ok) { printf("FAIL %s\n", what); failures++; }
}
static void same_u64(const char* what, uint64_t got, uint64_t want) {
  if (got != want) { printf("FAIL %s: got %llu, want %llu\n", what, (unsigned long long)got, (unsigned long long)want); failures++; }
}

static const char* const END_NAME[] = {"BadInput", "HostfreeVoid", "ShardBound", "CertShort", "CallerBound", "EstFailed", "CandCut", "BadPair",
                                       "Found", "NoHypothesis"};
static void verdict(const char* what, const FrameFacts& f, FrameEnd want) {
  FrameFacts* heap = new FrameFacts(f);  // (an exactly sized heap copy: the sanitizer sees a read past it)
  const FrameEnd got = sc::frame_end(*heap);
  delete heap;
  if (got != want) { printf("FAIL %s: got %s, want %s\n", what, END_NAME[(int)got], END_NAME[(int)want]); failures++; }
}

// a waited frame that found a winner: count 100, key 5; rank 2 at position 7
static FrameFacts waited() {
  FrameFacts f;
  f.winner_key = (100ull << 32) | 5u;
  f.winner_pos = (2ull << 32) | 7u;
  f.T = 1000;
  return f;
}
static uint64_t pack(uint64_t E, uint64_t M) { return (M << 32) | E; }
// ... and a host-free one: 5000 edges under a cover of 6000, 2000 triangles under a cover of 3000, T = 1000
static FrameFacts hostfree(uint64_t E = 5000, uint64_t M = 2000) {
  FrameFacts f = waited();
  f.host_free = true;
  f.counts = pack(E, M);
  f.E_cov = 6000; f.M_cov = 3000;
  return f;
}

static void test_verdict() {
  // ---- every value is reached
  verdict("a waited frame with a winner", waited(), FrameEnd::Found);
  verdict("a host-free frame with a winner", hostfree(), FrameEnd::Found);
  { FrameFacts f = waited(); f.winner_key = 0; verdict("no hypothesis", f, FrameEnd::NoHypothesis); }
  { FrameFacts f = hostfree(); f.winner_key = 0; verdict("host-free, no hypothesis", f, FrameEnd::NoHypothesis); }
  { FrameFacts f = hostfree(); f.bad_input = 1; verdict("host-free, bad input", f, FrameEnd::BadInput); }
  { FrameFacts f = waited(); f.bad_input = 1; verdict("waited: the staging step's wait has answered bad input, not this one", f, FrameEnd::Found); }
  { FrameFacts f = hostfree(); f.bad_input = 1ull << 32; verdict("bad input: the low half is the flag", f, FrameEnd::Found); }
  verdict("host-free, edges past the cover", hostfree(6001), FrameEnd::HostfreeVoid);
  { FrameFacts f = waited(); f.sharded_ab = true; f.est_active = true; f.merge_short = 1; verdict("sharded, merge short", f, FrameEnd::ShardBound); }
  { FrameFacts f = waited(); f.sharded_ab = true; f.est_active = true; f.est_void = true; verdict("sharded, estimate unverified", f, FrameEnd::ShardBound); }
  { FrameFacts f = waited(); f.sharded_ab = true; f.merge_short = 1; verdict("sharded, merge short, certified: the word is not the merge's to write", f, FrameEnd::Found); }
  { FrameFacts f = waited(); f.select_short = 1; verdict("select short under a certified bound", f, FrameEnd::CertShort); }
  { FrameFacts f = waited(); f.select_short = 1; f.est_bound_flag = true; verdict("... the flag does not matter there", f, FrameEnd::CertShort); }
  { FrameFacts f = waited(); f.select_short = 1; f.est_active = true; f.est_bound_flag = true; verdict("select short, the caller's estimate", f, FrameEnd::CallerBound); }
  { FrameFacts f = waited(); f.est_void = true; f.est_active = true; f.est_bound_flag = true; verdict("unverified, the caller's estimate", f, FrameEnd::CallerBound); }
  { FrameFacts f = waited(); f.select_short = 1; f.est_active = true; verdict("select short, the library's estimate", f, FrameEnd::EstFailed); }
  { FrameFacts f = hostfree(); f.est_void = true; f.est_active = true; verdict("unverified, the library's estimate, host-free", f, FrameEnd::EstFailed); }
  { FrameFacts f = waited(); f.est_void = true; verdict("est_void without an estimate says nothing", f, FrameEnd::Found); }
  { FrameFacts f = waited(); f.sharded_ab = true; f.cand_all = true; f.cand_cut = 1; verdict("candidate cut", f, FrameEnd::CandCut); }
  { FrameFacts f = waited(); f.sharded_ab = true; f.cand_cut = 1; verdict("candidate cut without gathered blobs", f, FrameEnd::Found); }
  { FrameFacts f = waited(); f.cand_all = true; f.cand_cut = 1; verdict("candidate cut, not sharded", f, FrameEnd::Found); }
  { FrameFacts f = waited(); f.winner_pos = ~0ull; verdict("bad pair", f, FrameEnd::BadPair); }

  // ---- priority: of two that hold the earlier one wins, for every adjacent pair of the list
  { FrameFacts f = hostfree(6001); f.bad_input = 1; verdict("1 before 2: bad input, void counts", f, FrameEnd::BadInput); }
  { FrameFacts f = hostfree(6001); f.sharded_ab = true; f.est_active = true; f.merge_short = 1; verdict("2 before 3: void counts, sharded bound", f, FrameEnd::HostfreeVoid); }
  { FrameFacts f = waited(); f.sharded_ab = true; f.est_active = true; f.merge_short = 1; f.select_short = 1;
    verdict("3 before 4: sharded bound, select short", f, FrameEnd::ShardBound);
    f.est_bound_flag = true; verdict("3 before 4, with the flag", f, FrameEnd::ShardBound); }
  { FrameFacts f = waited(); f.select_short = 1; f.sharded_ab = true; f.cand_all = true; f.cand_cut = 1;
    verdict("4 before 5: select short (certified), candidate cut", f, FrameEnd::CertShort);
    f.est_active = true; f.merge_short = 0; f.sharded_ab = false; f.est_void = true;
    verdict("4 before 5 asks sharded: off the sharded path the estimate fails", f, FrameEnd::EstFailed); }
  { FrameFacts f = waited(); f.select_short = 1; f.est_active = true; f.winner_pos = ~0ull; f.winner_key = 0; verdict("4 before 6 and 7", f, FrameEnd::EstFailed); }
  { FrameFacts f = waited(); f.sharded_ab = true; f.cand_all = true; f.cand_cut = 1; f.winner_pos = ~0ull; verdict("5 before 6: candidate cut, bad pair", f, FrameEnd::CandCut); }
  { FrameFacts f = waited(); f.winner_pos = ~0ull; f.winner_key = 0; verdict("6 before 7: bad pair, no key", f, FrameEnd::BadPair); }

  // ---- the packed word of a host-free frame
  {
    const sc::Counts k = sc::unpack_counts(0x000007D000001388ull);
    same_u64("unpack: the low half is the edges", k.E, 5000);
    same_u64("unpack: the high half is the triangles", k.M, 2000);
    const sc::Counts pend = sc::unpack_counts(~0ull);
    same_u64("unpack: pending stays pending, E", pend.E, 0xFFFFFFFFFFFFFFFFull);
    same_u64("unpack: pending stays pending, M", pend.M, 0xFFFFFFFFFFFFFFFFull);
  }
  { FrameFacts f = hostfree(); f.counts = ~0ull; verdict("the word never arrived", f, FrameEnd::HostfreeVoid); }
  { FrameFacts f = hostfree(); f.counts = ~0ull; f.E_cov = ~0ull; f.M_cov = ~0ull; verdict("... whatever the covers", f, FrameEnd::HostfreeVoid); }
  verdict("E at the cover", hostfree(6000), FrameEnd::Found);
  verdict("E just above the cover", hostfree(6001), FrameEnd::HostfreeVoid);
  verdict("M at the cover", hostfree(5000, 3000), FrameEnd::Found);
  verdict("M just above the cover", hostfree(5000, 3001), FrameEnd::HostfreeVoid);
  verdict("M = T", hostfree(5000, 1000), FrameEnd::Found);
  verdict("M = T - 1", hostfree(5000, 999), FrameEnd::HostfreeVoid);
  verdict("E = 4096", hostfree(4096), FrameEnd::Found);
  verdict("E = 4095", hostfree(4095), FrameEnd::HostfreeVoid);
  { FrameFacts f = hostfree(); f.ev_overflow = 3; verdict("event overflow, an event region", f, FrameEnd::HostfreeVoid);
    check("... it is the events'", sc::events_overflowed(f.ev_overflow) && !sc::chunks_overflowed(f.ev_overflow)); }
  { FrameFacts f = hostfree(); f.ev_overflow = (1ull << 32) | 3u; verdict("event overflow, the chunk count", f, FrameEnd::HostfreeVoid);
    check("... it is the chunks'", sc::events_overflowed(f.ev_overflow) && sc::chunks_overflowed(f.ev_overflow)); }
  { FrameFacts f = hostfree(); f.ev_overflow = 1ull << 32; verdict("the high half alone is no overflow (the low half counts)", f, FrameEnd::Found); }
  { FrameFacts f = waited(); f.ev_overflow = 3; f.counts = ~0ull; verdict("a waited frame's overflow was handled by run_select", f, FrameEnd::Found); }
  check("counts_fit, all four", sc::counts_fit(4096, 1000, 4096, 1000, 1000) && !sc::counts_fit(4095, 1000, 4096, 1000, 1000) &&
                                    !sc::counts_fit(4097, 1000, 4096, 1000, 1000) && !sc::counts_fit(4096, 1001, 4096, 1000, 1000) &&
                                    !sc::counts_fit(4096, 999, 4096, 1000, 1000));
}

struct WantRow { FrameEnd end; int status; const char* text; bool validated, fast_ok, est_call, est_fails, overflow, completes; };

static void test_table() {
  static_assert(sc::N_FRAME_ENDS == 10, "ten ways of leaving");
  static_assert(sc::SC_ESPEC == -100, "the internal status");
  static const char* const BOUND = "the estimated pruning bound was too high for this input: repeat the call without SC_FLAG_EST_BOUND";
  const WantRow want[] = {
      {FrameEnd::BadInput, SC_EINVAL, "non-finite input coordinate", false, true, false, false, false, false},
      {FrameEnd::HostfreeVoid, -100, nullptr, false, true, false, false, true, false},
      {FrameEnd::ShardBound, SC_EBOUND, BOUND, true, false, false, false, false, false},
      {FrameEnd::CertShort, SC_EHIP, "internal: the select found fewer keys above a certified pruning bound than the certificate counted", true, false,
       false, false, false, false},
      {FrameEnd::CallerBound, SC_EBOUND, BOUND, true, false, true, false, false, false},
      {FrameEnd::EstFailed, -100, "estimated pruning bound too high: call repeated with a certifying sample", true, true, true, true, false, false},
      {FrameEnd::CandCut, SC_ERETRY, "a candidate blob was too small for this input: repeat the call with sc_params.shard_cand_level raised by one", true,
       false, false, false, false, false},
      {FrameEnd::BadPair, SC_EINVAL,
       "a winner key pair points outside the selected list (stale / uninitialised pair, or ranks that disagree on T or the parameters)", true, false, false,
       false, false, false},
      {FrameEnd::Found, SC_OK, nullptr, true, false, false, false, false, true},
      {FrameEnd::NoHypothesis, SC_ENOHYP, nullptr, true, false, false, false, false, true},
  };
  int rows = 0;
  for (const WantRow& w : want) {
    const sc::FrameEndRow& r = sc::frame_end_row(w.end);
    const char* name = END_NAME[(int)w.end];
    rows++;
    if (r.status != w.status) { printf("FAIL row %s: status %d\n", name, r.status); failures++; }
    if (w.text ? (!r.text || strcmp(r.text, w.text) != 0) : r.text != nullptr) { printf("FAIL row %s: text %s\n", name, r.text ? r.text : "(none)"); failures++; }
    if (r.validated != w.validated || r.clears_fast_ok != w.fast_ok || r.est_failed_call != w.est_call || r.est_fails != w.est_fails ||
        r.repairs_overflow != w.overflow || r.completes != w.completes) {
      printf("FAIL row %s: flags %d %d %d %d %d %d\n", name, r.validated, r.clears_fast_ok, r.est_failed_call, r.est_fails, r.repairs_overflow, r.completes);
      failures++;
    }
    // the text as last_error gets it: the row's own, or nothing
    if (w.end != FrameEnd::HostfreeVoid && sc::frame_end_text(w.end, waited()) != std::string(w.text ? w.text : "")) { printf("FAIL text of %s\n", name); failures++; }
  }
  check("every row was walked", rows == sc::N_FRAME_ENDS);
  check("the statuses are the library's", SC_OK == 0 && SC_EINVAL == -1 && SC_EHIP == -3 && SC_ENOHYP == -5 && SC_ERETRY == -7 && SC_EBOUND == -8);

  FrameFacts f = hostfree(7000, 2000);
  const std::string got = sc::frame_end_text(FrameEnd::HostfreeVoid, f);
  const char* want_text = "host-free call repeated: edges 7000 (covered 6000), triangles 2000 (covered 3000, T 1000), event overflow 0";
  if (got != want_text) { printf("FAIL the repeat's text: %s\n", got.c_str()); failures++; }
  f.counts = ~0ull; f.ev_overflow = (1ull << 32) | 17u;
  const std::string got2 = sc::frame_end_text(FrameEnd::HostfreeVoid, f);
  const char* want2 =
      "host-free call repeated: edges 18446744073709551615 (covered 6000), triangles 18446744073709551615 (covered 3000, T 1000), event overflow 17";
  if (got2 != want2) { printf("FAIL the repeat's text, pending: %s\n", got2.c_str()); failures++; }
}

static void test_est_history() {
  EstHistory h;
  check("est: starts clear", !h.failed && h.holdoff == 0 && h.failures == 0);
  h.completed(false);
  check("est: a completed call without a failure counts nothing", !h.failed && h.holdoff == 0 && h.failures == 0);
  const uint32_t want[9] = {64, 128, 256, 512, 1024, 2048, 4096, 4096, 4096};
  for (uint32_t k = 0; k < 9; k++) {
    h.fail();
    if (!h.failed || h.failures != k + 1 || h.holdoff != want[k]) { printf("FAIL est: failure %u: hold-off %u\n", k + 1, h.holdoff); failures++; }
    h.completed(true);  // the failing frame's own repeat
    if (!h.failed || h.holdoff != want[k]) { printf("FAIL est: the repeat of failure %u was counted\n", k + 1); failures++; }
    uint32_t calls = 0;
    while (h.failed && calls < 100000) { h.completed(false); calls++; }
    if (calls != want[k] || h.holdoff != 0 || h.failures != k + 1) { printf("FAIL est: failure %u certified for %u calls\n", k + 1, calls); failures++; }
  }
  // one call short of the hold-off it still certifies
  h.reset();
  check("est: reset clears all three", !h.failed && h.holdoff == 0 && h.failures == 0);
  h.fail();
  for (int k = 0; k < 63; k++) h.completed(false);
  check("est: 63 of 64", h.failed && h.holdoff == 1);
  h.completed(false);
  check("est: 64 of 64", !h.failed && h.holdoff == 0 && h.failures == 1);
  // the caller decides: `failed` only
  h.fail();
  check("est: the second failure", h.failed && h.holdoff == 128 && h.failures == 2);
  h.caller_decides();
  check("est: caller_decides leaves the hold-off and the count", !h.failed && h.holdoff == 128 && h.failures == 2);
  h.completed(false);
  check("est: ... and nothing counts down while the context estimates", !h.failed && h.holdoff == 128);
  h.fail();
  check("est: the third failure", h.failed && h.holdoff == 256 && h.failures == 3);
  h.reset();
  check("est: reset after failures", !h.failed && h.holdoff == 0 && h.failures == 0);
}

static sc_params shape_params() {
  sc_params p;
  memset(&p, 0, sizeof p);
  p.size = sizeof p;
  p.sigma = 0.1f; p.t_cmp = 0.9f; p.tau = 0.1f; p.min_len = 0.1f;
  p.max_triangles = 1000; p.rank_mode = SC_RANK_WEIGHT; p.layout = SC_AOS;
  p.shard_rank = 0; p.shard_world = 1; p.shard_block = 1024; p.score_mode = SC_SCORE_COUNT;
  return p;
}

static void test_shape_history() {
  static_assert(ShapeHistory::HI_WINDOW == 64 && ShapeHistory::HI_YOUNG == 8, "the window and the young age");
  const sc_params p = shape_params();
  // ---- the cover's three rules, on fields set by hand
  {
    ShapeHistory s;
    s.hi_seen = 7;
    check("young at 7", s.young());
    same_u64("young, empty window: 2 x last + 4096", s.cover(10000, s.E_hi), 24096);
    s.M_hi[0] = 12000;
    same_u64("young, a small window: doubling wins", s.cover(10000, s.M_hi), 24096);
    s.M_hi[0] = 0; s.M_hi[1] = 30000;
    same_u64("young, a large window: h + h / 4 wins", s.cover(10000, s.M_hi), 41596);
    s.hi_seen = 8;
    check("not young at 8", !s.young());
    same_u64("not young, empty window: last + last / 2 + 4096", s.cover(10000, s.E_hi), 19096);
    s.E_hi[1] = 20000;
    same_u64("not young, window maximum 20000", s.cover(10000, s.E_hi), 29096);
    same_u64("... whatever the last count", s.cover(50000, s.E_hi), 29096);
    s.E_hi[0] = 20003;
    same_u64("the larger bucket, the quarter rounded down", s.cover(10000, s.E_hi), 20003 + 5000 + 4096);
    // room: the window only while the shape continues, young when it does not
    same_u64("room, continuing, not young", s.room(10000, ShapeHistory::EDGES, true), 20003 + 5000 + 4096);
    same_u64("room, keys take the keys' window", s.room(10000, ShapeHistory::KEYS, true), 41596);
    same_u64("room, not continuing: 2 x count + 4096", s.room(10000, ShapeHistory::EDGES, false), 24096);
    s.hi_seen = 3;
    same_u64("room, continuing and young", s.room(30000, ShapeHistory::EDGES, true), 64096);
    same_u64("room, nothing counted", s.room(0, ShapeHistory::KEYS, false), 4096);
  }
  // ---- note(): the first calls of a shape
  {
    ShapeHistory s;
    check("nothing continues an empty history of another size", !s.continues(500, &p));
    s.note(true, 10000, 5000, 500, p);
    check("the first regular call", s.E_last == 10000 && s.M_last == 5000 && s.n == 500 && s.hi_seen == 1 && s.hi_n == 1 && s.E_hi[0] == 10000 &&
                                        s.M_hi[0] == 5000 && s.E_hi[1] == 0 && s.M_hi[1] == 0);
    check("it continues itself", s.continues(500, &p) && !s.continues(501, &p));
    same_u64("cover of the edges after one call", s.cover(s.E_last, s.E_hi), 24096);
    same_u64("cover of the keys after one call", s.cover(s.M_last, s.M_hi), 14096);
    for (int k = 2; k <= 7; k++) s.note(true, 10000, 5000, 500, p);
    same_u64("the 7th call: still doubled", s.cover(s.E_last, s.E_hi), 24096);
    s.note(true, 10000, 5000, 500, p);
    check("the 8th call", s.hi_seen == 8 && s.hi_n == 8);
    same_u64("from the 8th: h + h / 4 + 4096", s.cover(s.E_last, s.E_hi), 16596);
    same_u64("... the keys", s.cover(s.M_last, s.M_hi), 10346);
  }
  // ---- the two buckets
  {
    ShapeHistory s;
    s.note(true, 50000, 40000, 500, p);  // the stream's largest frame comes first
    for (int k = 2; k <= 63; k++) s.note(true, 10000, 5000, 500, p);
    check("63 calls: one bucket", s.hi_n == 63 && s.E_hi[0] == 50000 && s.E_hi[1] == 0 && s.M_hi[0] == 40000);
    s.note(true, 10000, 5000, 500, p);
    check("the 64th call moves the bucket", s.hi_n == 0 && s.hi_seen == 64 && s.E_hi[0] == 0 && s.E_hi[1] == 50000 && s.M_hi[0] == 0 && s.M_hi[1] == 40000);
    same_u64("... and the cover still sees its maximum", s.cover(s.E_last, s.E_hi), 66596);
    same_u64("... the keys'", s.cover(s.M_last, s.M_hi), 54096);
    for (int k = 65; k <= 127; k++) s.note(true, 10000, 5000, 500, p);
    check("127 calls", s.hi_n == 63 && s.E_hi[0] == 10000 && s.E_hi[1] == 50000);
    same_u64("the 127th call: the maximum is still in the window", s.cover(s.E_last, s.E_hi), 66596);
    s.note(true, 10000, 5000, 500, p);
    check("the 128th call moves the bucket again", s.hi_n == 0 && s.hi_seen == 128 && s.E_hi[0] == 0 && s.E_hi[1] == 10000 && s.M_hi[1] == 5000);
    same_u64("after 128 the first frame's maximum is gone", s.cover(s.E_last, s.E_hi), 16596);
    // an irregular call: the last counts, not the window
    s.note(false, 99999, 88888, 500, p);
    check("an irregular call updates the last counts only", s.E_last == 99999 && s.M_last == 88888 && s.hi_n == 0 && s.hi_seen == 128 && s.E_hi[0] == 0 &&
                                                                s.E_hi[1] == 10000 && s.M_hi[0] == 0 && s.M_hi[1] == 5000);
    same_u64("... so the cover stays", s.cover(s.E_last, s.E_hi), 16596);
  }
  // ---- a change of shape empties the window; timing flags are no change
  {
    auto filled = [&]() {
      ShapeHistory s;
      for (int k = 0; k < 10; k++) s.note(true, 10000, 5000, 500, p);
      return s;
    };
    auto emptied = [](const ShapeHistory& s) { return s.E_hi[0] == 0 && s.E_hi[1] == 0 && s.M_hi[0] == 0 && s.M_hi[1] == 0 && s.hi_n == 0 && s.hi_seen == 0; };
    auto kept = [](const ShapeHistory& s) { return s.E_hi[0] == 10000 && s.M_hi[0] == 5000 && s.hi_n == 10 && s.hi_seen == 10; };
    { ShapeHistory s = filled(); check("ten calls fill it", kept(s)); }
    { ShapeHistory s = filled(); s.note(false, 10000, 5000, 501, p); check("a change of n", emptied(s) && s.n == 501); }
    { ShapeHistory s = filled(); s.note(true, 20000, 6000, 501, p);
      check("a change of n, regular: the new shape's first call", s.hi_seen == 1 && s.hi_n == 1 && s.E_hi[0] == 20000 && s.M_hi[0] == 6000 && s.E_hi[1] == 0);
      same_u64("... and it is young again", s.cover(s.E_last, s.E_hi), 44096); }
    struct Change { const char* what; void (*apply)(sc_params*); };
    const Change changes[] = {
        {"sigma", [](sc_params* q) { q->sigma = 0.2f; }},
        {"t_cmp", [](sc_params* q) { q->t_cmp = 0.8f; }},
        {"tau", [](sc_params* q) { q->tau = 0.2f; }},
        {"min_len", [](sc_params* q) { q->min_len = 0.2f; }},
        {"max_triangles", [](sc_params* q) { q->max_triangles = 1001; }},
        {"rank_mode", [](sc_params* q) { q->rank_mode = SC_RANK_DEGREE; }},
        {"layout", [](sc_params* q) { q->layout = SC_SOA; }},
        {"shard_world", [](sc_params* q) { q->shard_world = 2; }},
        {"shard_rank", [](sc_params* q) { q->shard_rank = 1; }},
        {"shard_block", [](sc_params* q) { q->shard_block = 512; }},
        {"score_mode", [](sc_params* q) { q->score_mode = SC_SCORE_MSE; }},
        {"a flag that is no timing flag", [](sc_params* q) { q->flags |= SC_FLAG_NO_DENSE_S; }},
    };
    for (const Change& ch : changes) {
      sc_params q = p;
      ch.apply(&q);
      ShapeHistory s = filled();
      if (s.continues(500, &q) || ShapeHistory::same_shape(&p, &q)) { printf("FAIL shape: a change of %s continues\n", ch.what); failures++; }
      s.note(false, 10000, 5000, 500, q);
      if (!emptied(s)) { printf("FAIL shape: a change of %s kept the window\n", ch.what); failures++; }
    }
    const uint32_t timing[] = {SC_FLAG_TIMING, SC_FLAG_TIMING_HOT, SC_FLAG_TIMING_ONE | (5u << 8), SC_FLAG_TIMING | SC_FLAG_TIMING_HOT | SC_FLAG_TIMING_ONE | (15u << 8)};
    for (uint32_t bits : timing) {
      sc_params q = p;
      q.flags |= bits;
      ShapeHistory s = filled();
      check("timing flags continue the shape", s.continues(500, &q));
      s.note(false, 10000, 5000, 500, q);
      check("timing flags keep the window", kept(s));
    }
  }
  // ---- hi_seen saturates
  {
    ShapeHistory s;
    s.note(true, 10000, 5000, 500, p);
    s.hi_seen = 0xFFFFFFFEu;
    s.note(true, 10000, 5000, 500, p);
    check("hi_seen reaches all ones", s.hi_seen == 0xFFFFFFFFu);
    s.note(true, 10000, 5000, 500, p);
    check("... and stays", s.hi_seen == 0xFFFFFFFFu && !s.young());
  }
}

int main() {
  test_verdict();
  test_table();
  test_est_history();
  test_shape_history();
  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
