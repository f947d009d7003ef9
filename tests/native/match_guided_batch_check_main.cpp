// Stand-alone program for the host-only checks of sc_match_guided_batch (sac-cot_amd/csrc/sc_match_guided_batch_check.hpp): the
// guide block with the one flag those entries know — every refusal of sc_guide_params still holds, SC_GUIDE_POSE_STATUS is accepted,
// any other bit is not — and the rule of the pose stride.  The block is a heap copy of its exact size, so that a read past it ends the
// run when this is built with -fsanitize=address,undefined (tests/test_match_guided_batch_abi.py builds and runs it that way; no GPU,
// no Python in the process).
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../sac-cot_amd/csrc/sc_match_guided_batch_check.hpp"

static int failures = 0;

static sc_guide_params params(float gate, uint32_t layout = SC_AOS, uint32_t flags = 0) {
  sc_guide_params gp;
  memset(&gp, 0, sizeof(gp));
  gp.size = sizeof(gp); gp.layout = layout; gp.gate = gate; gp.flags = flags;
  return gp;
}

static void expect(const char* what, const sc_guide_params& gp, const char* want) {
  sc_guide_params* p = new sc_guide_params(gp);
  const char* got = sc::guide_batch_params_error(p);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
  if (memcmp(p, &gp, sizeof(gp)) != 0) { printf("FAIL %s: the block was written\n", what); failures++; }
  delete p;
}

static void stride(uint32_t flags, uint32_t s, const char* want) {
  const char* got = sc::guide_pose_stride_error(flags, s);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL stride %u flags %u: got %s\n", s, flags, got ? got : "(accepted)"); failures++; }
}

int main() {
  static_assert(SC_GUIDE_POSE_STATUS == 1u, "the flag is bit 0");
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float sub = std::numeric_limits<float>::denorm_min();
  expect("good, AoS", params(0.15f), nullptr);
  expect("good, SoA", params(0.15f, SC_SOA), nullptr);
  expect("good, the status flag", params(0.15f, SC_AOS, SC_GUIDE_POSE_STATUS), nullptr);
  expect("good, SoA and the status flag", params(0.15f, SC_SOA, 1), nullptr);
  expect("flag 2", params(0.15f, SC_AOS, 2), "flags");
  expect("flags 3", params(0.15f, SC_AOS, 3), "flags");
  expect("flag 2^31", params(0.15f, SC_AOS, 0x80000000u), "flags");
  expect("layout 2", params(0.15f, 2), "layout");
  expect("layout 2 with the flag", params(0.15f, 2, 1), "layout");
  expect("layout all ones", params(0.15f, 0xFFFFFFFFu), "layout");
  // the gate: finite and > 0, with and without the flag
  for (uint32_t f = 0; f < 2; f++) {
    expect("gate 0", params(0.f, SC_AOS, f), "gate");
    expect("gate -0", params(-0.f, SC_AOS, f), "gate");
    expect("gate negative", params(-0.15f, SC_AOS, f), "gate");
    expect("gate NaN", params(nan, SC_AOS, f), "gate");
    expect("gate +inf", params(inf, SC_AOS, f), "gate");
    expect("gate -inf", params(-inf, SC_AOS, f), "gate");
    expect("gate the smallest subnormal", params(sub, SC_AOS, f), nullptr);
    expect("gate FLT_MAX", params(FLT_MAX, SC_AOS, f), nullptr);
  }
  {
    sc_guide_params bad = params(0.15f, SC_AOS, 1);
    bad.size = 28; expect("size 28", bad, "size");
    bad.size = 36; expect("size 36", bad, "size");
    bad.size = 0; expect("size 0", bad, "size");
    for (int r = 0; r < 4; r++) {
      sc_guide_params res = params(0.15f, SC_AOS, 1);
      res.reserved[r] = 1;
      expect("reserved", res, "reserved");
    }
    // the order of the rules: the size is looked at before anything it would place
    sc_guide_params two = params(nan, 7, 9); two.size = 4;
    expect("size first", two, "size");
  }
  // sc_match_guided's own rule is what it was: any flag is refused there
  {
    sc_guide_params one = params(0.15f, SC_AOS, 1);
    const char* got = sc::guide_params_error(&one);
    if (!got || !strstr(got, "flags")) { printf("FAIL guide_params_error accepts a flag\n"); failures++; }
  }
  // the pose stride: a multiple of 4, >= 48, >= 52 with the flag
  stride(0, 44, "pose_stride"); stride(1, 44, "pose_stride");
  stride(0, 48, nullptr);       stride(1, 48, "pose_stride");
  stride(0, 50, "pose_stride"); stride(1, 50, "pose_stride");
  stride(0, 52, nullptr);       stride(1, 52, nullptr);
  stride(0, 64, nullptr);       stride(1, 64, nullptr);
  stride(0, 80, nullptr);       stride(1, 80, nullptr);
  stride(0, 0, "pose_stride");  stride(1, 0, "pose_stride");
  stride(0, 49, "pose_stride"); stride(1, 54, "pose_stride");
  stride(0, 0xFFFFFFFCu, nullptr); stride(1, 0xFFFFFFFFu, "pose_stride");
  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
