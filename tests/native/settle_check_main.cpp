// Stand-alone program for the host-only checks of sc_settle_poses (sac-cot_amd/csrc/sc_settle_check.hpp): every refusal rule of the
// parameter block, the stride and n_poses in either form, and the bytes a call reads of the pose array — walked on an exactly sized
// heap array, so that a read past it ends the run when this is built with -fsanitize=address,undefined (tests/test_settle_abi.py
// builds and runs it that way; no GPU, no Python in the process).
#include <cstdio>
#include <cstring>

#include "../../sac-cot_amd/csrc/sc_settle_check.hpp"

static int failures = 0;

static sc_settle_params params(uint32_t max_iter = 16, uint32_t sel_mode = SC_ASSIGN_SEL_NONE, uint32_t flags = 0) {
  sc_settle_params sp;
  memset(&sp, 0, sizeof(sp));
  sp.size = sizeof(sp); sp.max_iter = max_iter; sp.sel_mode = sel_mode; sp.flags = flags;
  return sp;
}

static void expect(const char* what, const sc_settle_params& sp, uint32_t stride, uint32_t n_poses, bool batch, bool has_sel, const char* want) {
  // a heap copy of the exact size: the sanitizer sees every read past the block
  sc_settle_params* p = new sc_settle_params(sp);
  const char* got = sc::settle_params_error(p, stride, n_poses, batch, has_sel);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
  delete p;
}

// every word a call reads of an accepted pose array lies inside pose_bytes_read, and the last one ends exactly there
static void walk(const char* what, uint32_t n_poses, uint32_t n_problems, uint32_t stride, const sc_settle_params& sp, bool batch) {
  const uint64_t records = (uint64_t)n_poses * n_problems, bytes = sc::pose_bytes_read(records, stride, sc::settle_reads_status(&sp, batch));
  unsigned char* pose = new unsigned char[bytes];
  memset(pose, 0, bytes);
  const uint32_t read = sc::settle_reads_status(&sp, batch) ? sc::POSE_STATUS_BYTES : sc::POSE_RT_BYTES;
  uint64_t last = 0;
  unsigned sum = 0;
  for (uint32_t k = 0; k < n_poses; k++)
    for (uint32_t b = 0; b < n_problems; b++) {
      const uint64_t at = sc::pose_record_offset(k, b, n_problems, stride);
      for (uint32_t x = 0; x < read; x++) sum += pose[at + x];
      if (at + read > last) last = at + read;
    }
  if (last != bytes || sum != 0) { printf("FAIL %s: %llu bytes read, %llu counted\n", what, (unsigned long long)last, (unsigned long long)bytes); failures++; }
  delete[] pose;
}

int main() {
  const sc_settle_params ok = params();
  const sc_settle_params flag = params(16, SC_ASSIGN_SEL_NONE, SC_SETTLE_STATUS);
  expect("frame, good", ok, 48, 1, false, false, nullptr);
  expect("frame, 64 poses, stride 80, a mask, the flag", params(64, SC_ASSIGN_SEL_MASK, SC_SETTLE_STATUS), 80, 64, false, true, nullptr);
  expect("frame, one round", params(1), 48, 2, false, false, nullptr);
  expect("frame, max_iter 0", params(0), 48, 1, false, false, "max_iter");
  expect("frame, max_iter 65", params(65), 48, 1, false, false, "max_iter");
  expect("frame, 65 poses", ok, 48, 65, false, false, "n_poses");
  expect("frame, no pose", ok, 48, 0, false, false, "n_poses");
  expect("frame, stride 0", ok, 0, 1, false, false, "pose_stride");
  expect("frame, stride 44", ok, 44, 1, false, false, "pose_stride");
  expect("frame, stride 50", ok, 50, 1, false, false, "pose_stride");
  expect("frame, stride 48 with the flag", flag, 48, 1, false, false, "pose_stride");
  expect("frame, stride 52 with the flag", flag, 52, 1, false, false, nullptr);
  expect("frame, sel_mode 2", params(16, 2), 48, 1, false, true, "sel_mode");
  expect("frame, a mask without sel", params(16, SC_ASSIGN_SEL_MASK), 48, 1, false, false, "sel is NULL");
  expect("frame, flag 2", params(16, 0, 2), 48, 1, false, false, "flag");
  expect("frame, flag 3", params(16, 0, 3), 52, 1, false, false, "flag");
  {
    sc_settle_params bad = ok; bad.size = 28;
    expect("frame, size", bad, 48, 1, false, false, "size");
    expect("batch, size", bad, 80, 1, true, false, "size");
    for (int r = 0; r < 4; r++) {
      sc_settle_params res = ok; res.reserved[r] = 1;
      expect("frame, reserved", res, 48, 1, false, false, "reserved");
      expect("batch, reserved", res, 80, 1, true, false, "reserved");
    }
  }
  expect("batch, good", ok, 80, 16, true, false, nullptr);
  expect("batch, the flag is allowed", flag, 52, 1, true, false, nullptr);
  expect("batch, 17 poses", ok, 80, 17, true, false, "n_poses");
  expect("batch, no pose", ok, 80, 0, true, false, "n_poses");
  expect("batch, stride 48", ok, 48, 1, true, false, "pose_stride");
  expect("batch, stride 54", ok, 54, 1, true, false, "pose_stride");
  expect("batch, a mask", params(16, SC_ASSIGN_SEL_MASK), 80, 1, true, true, "sel_mode");
  expect("batch, max_iter 0", params(0), 80, 1, true, false, "max_iter");
  expect("batch, max_iter 65", params(65), 80, 1, true, false, "max_iter");

  walk("frame, stride 48", 64, 1, 48, ok, false);
  walk("frame, stride 64 with the status", 64, 1, 64, flag, false);
  walk("frame, one pose", 1, 1, 48, ok, false);
  walk("batch, 16 x 7, stride 80", 16, 7, 80, ok, true);
  walk("batch, 1 x 1, stride 52", 1, 1, 52, ok, true);
  if (sc::pose_bytes_read(0, 48, sc::settle_reads_status(&ok, false)) != 0) { printf("FAIL no record, no byte\n"); failures++; }
  if (sc::settle_reads_status(&ok, false) || !sc::settle_reads_status(&ok, true) || !sc::settle_reads_status(&flag, false)) {
    printf("FAIL who reads the status\n");
    failures++;
  }
  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
