// Stand-alone program for the host-only checks of sc_match_guided_poses (sac-cot_amd/csrc/sc_match_guided_poses_check.hpp): the
// guide block with SC_GUIDE_POSE_STATUS accepted and any other bit refused, the stride of the pose records, the number of records,
// and the order of the three rules.  The block is a heap copy of its exact size, so that a read past it ends the run when this is
// built with -fsanitize=address,undefined (tests/test_match_guided_poses_abi.py builds and runs it that way; no GPU, no Python in
// the process).
#include <cfloat>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../sac-cot_amd/csrc/sc_match_guided_poses_check.hpp"

static int failures = 0;

static sc_guide_params params(float gate, uint32_t layout = SC_AOS, uint32_t flags = 0) {
  sc_guide_params gp;
  memset(&gp, 0, sizeof(gp));
  gp.size = sizeof(gp); gp.layout = layout; gp.gate = gate; gp.flags = flags;
  return gp;
}

static void expect(const char* what, const sc_guide_params& gp, uint32_t stride, uint32_t n_poses, const char* want) {
  sc_guide_params* p = new sc_guide_params(gp);
  const char* got = sc::guide_poses_error(p, stride, n_poses);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s (stride %u, n_poses %u): got %s\n", what, stride, n_poses, got ? got : "(accepted)"); failures++; }
  if (memcmp(p, &gp, sizeof(gp)) != 0) { printf("FAIL %s: the block was written\n", what); failures++; }
  delete p;
}

int main() {
  static_assert(SC_GUIDE_MAX_POSES == 64u, "sixty-four records at most");
  static_assert(SC_GUIDE_POSE_STATUS == 1u, "the flag is bit 0");
  static_assert(SC_HAS_MATCH_GUIDED_POSES == 1, "the feature macro");
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const sc_guide_params plain = params(0.15f), flagged = params(0.15f, SC_SOA, SC_GUIDE_POSE_STATUS);
  // what is accepted
  expect("plain, stride 48, one record", plain, 48, 1, nullptr);
  expect("plain, stride 48, 64 records", plain, 48, 64, nullptr);
  expect("plain, stride 64", plain, 64, 3, nullptr);
  expect("flagged, stride 52", flagged, 52, 1, nullptr);
  expect("flagged, stride 80", flagged, 80, 64, nullptr);
  expect("flagged, stride 64", flagged, 64, 16, nullptr);
  // the stride: a multiple of 4, >= 48, >= 52 with the flag
  expect("stride 44", plain, 44, 1, "pose_stride");
  expect("stride 44, flagged", flagged, 44, 1, "pose_stride");
  expect("stride 46", plain, 46, 1, "pose_stride");
  expect("stride 50", plain, 50, 1, "pose_stride");
  expect("stride 50, flagged", flagged, 50, 1, "pose_stride");
  expect("stride 0", plain, 0, 1, "pose_stride");
  expect("stride 48 with the flag", flagged, 48, 1, "52");
  expect("stride 48 with the flag, 64 records", flagged, 48, 64, "pose_stride");
  expect("stride 0xFFFFFFFC", plain, 0xFFFFFFFCu, 1, nullptr);
  expect("stride 0xFFFFFFFF", flagged, 0xFFFFFFFFu, 1, "pose_stride");
  // the number of records: 1 .. 64
  expect("n_poses 0", plain, 48, 0, "n_poses");
  expect("n_poses 0, flagged", flagged, 80, 0, "n_poses");
  expect("n_poses 65", plain, 48, 65, "n_poses");
  expect("n_poses 65, flagged", flagged, 80, 65, "n_poses");
  expect("n_poses all ones", plain, 48, 0xFFFFFFFFu, "n_poses");
  // the flags: SC_GUIDE_POSE_STATUS is the only one
  expect("flag 2", params(0.15f, SC_AOS, 2), 80, 1, "flags");
  expect("flags 3", params(0.15f, SC_AOS, 3), 80, 1, "flags");
  expect("flag 2^31", params(0.15f, SC_AOS, 0x80000000u), 80, 1, "flags");
  // every rule of sc_guide_params still holds, with and without the flag
  for (uint32_t f = 0; f < 2; f++) {
    expect("layout 2", params(0.15f, 2, f), 80, 1, "layout");
    expect("gate 0", params(0.f, SC_AOS, f), 80, 1, "gate");
    expect("gate negative", params(-0.15f, SC_AOS, f), 80, 1, "gate");
    expect("gate NaN", params(nan, SC_AOS, f), 80, 1, "gate");
    expect("gate inf", params(inf, SC_AOS, f), 80, 1, "gate");
    expect("gate the smallest subnormal", params(std::numeric_limits<float>::denorm_min(), SC_AOS, f), 80, 1, nullptr);
    expect("gate FLT_MAX", params(FLT_MAX, SC_AOS, f), 80, 1, nullptr);
    sc_guide_params res = params(0.15f, SC_AOS, f);
    res.reserved[3] = 1;
    expect("reserved", res, 80, 1, "reserved");
    sc_guide_params size = params(0.15f, SC_AOS, f);
    size.size = 28; expect("size 28", size, 80, 1, "size");
    size.size = 36; expect("size 36", size, 80, 1, "size");
  }
  // the order: the block, then the stride, then the count; the size before anything it would place
  expect("block before stride", params(nan), 44, 0, "gate");
  expect("stride before count", plain, 44, 0, "pose_stride");
  {
    sc_guide_params two = params(nan, 7, 9); two.size = 4;
    expect("size first", two, 44, 0, "size");
  }
  // sc_match_guided's own rule is what it was: any flag is refused there
  {
    sc_guide_params one = params(0.15f, SC_AOS, 1);
    const char* got = sc::guide_params_error(&one);
    if (!got || !strstr(got, "flags")) { printf("FAIL guide_params_error accepts a flag\n"); failures++; }
  }
  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
