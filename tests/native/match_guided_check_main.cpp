// Stand-alone program for the host-only checks of sc_match_guided (sac-cot_amd/csrc/sc_match_guided_check.hpp): every refusal of
// sc_guide_params, the boundary values of the gate, and the threshold derived from it.  The block is a heap copy of its exact size, so
// that a read past it ends the run when this is built with -fsanitize=address,undefined (tests/test_match_guided_abi.py builds and
// runs it that way; no GPU, no Python in the process).
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../sac-cot_amd/csrc/sc_match_guided_check.hpp"

static int failures = 0;

static sc_guide_params params(float gate, uint32_t layout = SC_AOS, uint32_t flags = 0) {
  sc_guide_params gp;
  memset(&gp, 0, sizeof(gp));
  gp.size = sizeof(gp); gp.layout = layout; gp.gate = gate; gp.flags = flags;
  return gp;
}

static void expect(const char* what, const sc_guide_params& gp, const char* want) {
  sc_guide_params* p = new sc_guide_params(gp);
  const char* got = sc::guide_params_error(p);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
  delete p;
}

static void check(const char* what, bool ok) {
  if (!ok) { printf("FAIL %s\n", what); failures++; }
}

int main() {
  static_assert(sizeof(sc_guide_params) == 32, "sc_guide_params is 32 bytes");
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float sub = std::numeric_limits<float>::denorm_min();
  expect("good, AoS", params(0.15f), nullptr);
  expect("good, SoA", params(0.15f, SC_SOA), nullptr);
  expect("layout 2", params(0.15f, 2), "layout");
  expect("layout all ones", params(0.15f, 0xFFFFFFFFu), "layout");
  expect("flag 1", params(0.15f, SC_AOS, 1), "flags");
  expect("flag 2^31", params(0.15f, SC_AOS, 0x80000000u), "flags");
  // the gate: finite and > 0
  expect("gate 0 (the default: the caller must set it)", params(0.f), "gate");
  expect("gate -0", params(-0.f), "gate");
  expect("gate negative", params(-0.15f), "gate");
  expect("gate -subnormal", params(-sub), "gate");
  expect("gate NaN", params(nan), "gate");
  expect("gate -NaN", params(-nan), "gate");
  expect("gate +inf", params(inf), "gate");
  expect("gate -inf", params(-inf), "gate");
  expect("gate the smallest subnormal", params(sub), nullptr);
  expect("gate FLT_MIN", params(FLT_MIN), nullptr);
  expect("gate FLT_MAX", params(FLT_MAX), nullptr);
  {
    sc_guide_params bad = params(0.15f);
    bad.size = 28; expect("size 28", bad, "size");
    bad.size = 36; expect("size 36", bad, "size");
    bad.size = 0; expect("size 0", bad, "size");
    for (int r = 0; r < 4; r++) {
      sc_guide_params res = params(0.15f);
      res.reserved[r] = 1;
      expect("reserved", res, "reserved");
    }
    // the order of the rules: the size is looked at before anything it would place
    sc_guide_params two = params(nan, 7, 9); two.size = 4;
    expect("size first", two, "size");
  }
  // the threshold, as tau^2 is derived: squared in fp64, rounded once
  check("gate2 of 0.5", sc::guide_gate2(0.5f) == 0.25f);
  check("gate2 of 0.15f", sc::guide_gate2(0.15f) == (float)((double)0.15f * (double)0.15f));
  check("gate2 of the smallest subnormal is 0: nothing is admissible", sc::guide_gate2(sub) == 0.f);
  check("gate2 of FLT_MAX is +inf: an infinite residual still is not below it", std::isinf(sc::guide_gate2(FLT_MAX)) && !(inf < sc::guide_gate2(FLT_MAX)));
  check("gate2 of 1e18f is finite", std::isfinite(sc::guide_gate2(1e18f)));
  check("a NaN residual is never admissible", !(nan < sc::guide_gate2(0.5f)));
  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
