// Stand-alone program for the host-only checks of sc_assign_poses (sac-cot_amd/csrc/sc_assign_check.hpp): what is refused of the
// parameter block, the stride and n_poses in either form, the motion-major offsets, and the bytes a call reads of the pose array —
// walked on an exactly sized heap array, so that a read past it ends the run when this is built with -fsanitize=address,undefined
// (tests/test_assign_abi.py builds and runs it that way; no GPU, no Python in the process).
#include <cstdio>
#include <cstring>

#include "../../sac-cot_amd/csrc/sc_assign_check.hpp"

static int failures = 0;

static sc_assign_params params(uint32_t mode = SC_ASSIGN_BEST, uint32_t sel_mode = SC_ASSIGN_SEL_NONE, uint32_t flags = 0) {
  sc_assign_params ap;
  memset(&ap, 0, sizeof(ap));
  ap.size = sizeof(ap); ap.mode = mode; ap.sel_mode = sel_mode; ap.flags = flags;
  return ap;
}

static void expect(const char* what, const sc_assign_params& ap, uint32_t stride, uint32_t n_poses, bool batch, bool has_sel, const char* want) {
  // a heap copy of the exact size: the sanitizer sees every read past the block
  sc_assign_params* p = new sc_assign_params(ap);
  const char* got = sc::assign_params_error(p, stride, n_poses, batch, has_sel);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
  delete p;
}

// every word a call reads of an accepted pose array lies inside pose_bytes_read, and the last one ends exactly there
static void walk(const char* what, uint32_t n_poses, uint32_t n_problems, uint32_t stride, bool reads_status) {
  const uint64_t records = (uint64_t)n_poses * n_problems, bytes = sc::pose_bytes_read(records, stride, reads_status);
  unsigned char* pose = new unsigned char[bytes];
  memset(pose, 0, bytes);
  const uint32_t read = reads_status ? sc::POSE_STATUS_BYTES : sc::POSE_RT_BYTES;
  uint64_t last = 0, seen = 0;
  unsigned sum = 0;
  for (uint32_t k = 0; k < n_poses; k++)
    for (uint32_t b = 0; b < n_problems; b++) {
      const uint64_t at = sc::pose_record_offset(k, b, n_problems, stride);
      if (at != sc::pose_record_index(k, b, n_problems) * stride || sc::pose_record_index(k, b, n_problems) != seen) {
        printf("FAIL %s: record (%u, %u)\n", what, k, b);
        failures++;
      }
      seen++;
      for (uint32_t x = 0; x < read; x++) sum += pose[at + x];
      if (at + read > last) last = at + read;
    }
  if (last != bytes || sum != 0) { printf("FAIL %s: %llu bytes read, %llu counted\n", what, (unsigned long long)last, (unsigned long long)bytes); failures++; }
  delete[] pose;
}

int main() {
  const sc_assign_params ok = params();
  expect("frame, good", ok, 48, 1, false, false, nullptr);
  expect("frame, 1024 poses, stride 80, the flag", params(SC_ASSIGN_FIRST, SC_ASSIGN_SEL_MASK, SC_ASSIGN_STATUS), 80, 1024, false, true, nullptr);
  expect("frame, 1025 poses", ok, 48, 1025, false, false, "n_poses");
  expect("frame, no pose", ok, 48, 0, false, false, "n_poses");
  expect("frame, stride 44", ok, 44, 1, false, false, "pose_stride");
  expect("frame, stride 50", ok, 50, 1, false, false, "pose_stride");
  expect("frame, stride 48 with the flag", params(0, 0, SC_ASSIGN_STATUS), 48, 1, false, false, "pose_stride");
  expect("frame, stride 52 with the flag", params(0, 0, SC_ASSIGN_STATUS), 52, 1, false, false, nullptr);
  expect("frame, mode 2", params(2), 48, 1, false, false, "mode");
  expect("frame, sel_mode 2", params(0, 2), 48, 1, false, true, "sel_mode");
  expect("frame, a mask without sel", params(0, SC_ASSIGN_SEL_MASK), 48, 1, false, false, "sel is NULL");
  expect("frame, flag 2", params(0, 0, 2), 48, 1, false, false, "flag");
  {
    sc_assign_params bad = ok; bad.size = 28;
    expect("frame, size", bad, 48, 1, false, false, "size");
    for (int r = 0; r < 4; r++) {
      sc_assign_params res = ok; res.reserved[r] = 1;
      expect("frame, reserved", res, 48, 1, false, false, "reserved");
      expect("batch, reserved", res, 80, 1, true, false, "reserved");
    }
  }
  expect("batch, good", ok, 80, 64, true, false, nullptr);
  expect("batch, the flag is allowed", params(SC_ASSIGN_FIRST, 0, SC_ASSIGN_STATUS), 52, 1, true, false, nullptr);
  expect("batch, 65 poses", ok, 80, 65, true, false, "n_poses");
  expect("batch, no pose", ok, 80, 0, true, false, "n_poses");
  expect("batch, stride 48", ok, 48, 1, true, false, "pose_stride");
  expect("batch, stride 54", ok, 54, 1, true, false, "pose_stride");
  expect("batch, a mask", params(0, SC_ASSIGN_SEL_MASK), 80, 1, true, true, "sel_mode");
  expect("batch, mode 2", params(2), 80, 1, true, false, "mode");

  walk("frame, stride 48", 1024, 1, 48, false);
  walk("frame, stride 64 with the status", 65, 1, 64, true);
  walk("frame, one pose", 1, 1, 48, false);
  walk("batch, 64 x 7, stride 80", 64, 7, 80, true);
  walk("batch, 1 x 1, stride 52", 1, 1, 52, true);
  // the offsets are 64-bit: 64 planes of 2^26 problems at the largest stride pass 2^32 bytes by far
  if (sc::pose_record_offset(63, (1u << 26) - 1, 1u << 26, 0xFFFFFFFCu) != ((uint64_t)63 * (1u << 26) + (1u << 26) - 1) * 0xFFFFFFFCull) {
    printf("FAIL the 64-bit offset\n");
    failures++;
  }
  if (sc::pose_bytes_read(0, 48, false) != 0) { printf("FAIL no record, no byte\n"); failures++; }
  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
