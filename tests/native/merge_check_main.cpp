// Stand-alone program for the host-only checks of sc_merge_poses (sac-cot_amd/csrc/sc_merge_check.hpp): every refusal rule of the
// parameter block, the stride and n_poses in either form, the bytes a call reads of the pose array — walked on an exactly sized heap
// array, so that a read past it ends the run when this is built with -fsanitize=address,undefined (tests/test_merge_abi.py builds
// and runs it that way; no GPU, no Python in the process) — and the sizes of the frame form's scratch at the ends of their ranges.
#include <cstdio>
#include <cstring>

#include "../../sac-cot_amd/csrc/sc_merge_check.hpp"

static int failures = 0;

static sc_merge_params params(uint32_t measure = SC_MERGE_OVER_MIN, uint32_t num = 1, uint32_t den = 2, uint32_t min_count = 0,
                              uint32_t sel_mode = SC_ASSIGN_SEL_NONE, uint32_t flags = 0) {
  sc_merge_params mp;
  memset(&mp, 0, sizeof(mp));
  mp.size = sizeof(mp); mp.measure = measure; mp.num = num; mp.den = den; mp.min_count = min_count; mp.sel_mode = sel_mode; mp.flags = flags;
  return mp;
}

static void expect(const char* what, const sc_merge_params& mp, uint32_t stride, uint32_t n_poses, bool batch, bool has_sel, const char* want) {
  // a heap copy of the exact size: the sanitizer sees every read past the block
  sc_merge_params* p = new sc_merge_params(mp);
  const char* got = sc::merge_params_error(p, stride, n_poses, batch, has_sel);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
  delete p;
}

// every word a call reads of an accepted pose array lies inside pose_bytes_read, and the last one ends exactly there
static void walk(const char* what, uint32_t n_poses, uint32_t n_problems, uint32_t stride, const sc_merge_params& mp, bool batch) {
  const uint64_t records = (uint64_t)n_poses * n_problems, bytes = sc::pose_bytes_read(records, stride, sc::merge_reads_status(&mp, batch));
  unsigned char* pose = new unsigned char[bytes];
  memset(pose, 0, bytes);
  const uint32_t read = sc::merge_reads_status(&mp, batch) ? sc::POSE_STATUS_BYTES : sc::POSE_RT_BYTES;
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

static void size_is(const char* what, uint64_t got, uint64_t want) {
  if (got != want) { printf("FAIL %s: %llu, expected %llu\n", what, (unsigned long long)got, (unsigned long long)want); failures++; }
}

int main() {
  const sc_merge_params ok = params();
  const sc_merge_params flag = params(0, 1, 2, 0, SC_ASSIGN_SEL_NONE, SC_MERGE_STATUS);
  const uint32_t NONE = SC_ASSIGN_SEL_NONE, MASK = SC_ASSIGN_SEL_MASK;
  expect("frame, good", ok, 48, 1, false, false, nullptr);
  expect("frame, 1024 poses, stride 80, a mask, both flags, Jaccard", params(SC_MERGE_OVER_UNION, 3, 4, 5, MASK, SC_MERGE_STATUS | SC_MERGE_COMPACT), 80, 1024,
         false, true, nullptr);
  expect("frame, num == den", params(0, 7, 7), 48, 2, false, false, nullptr);
  expect("frame, 65536 / 65536", params(0, 65536, 65536), 48, 2, false, false, nullptr);
  expect("frame, 1 / 65536", params(1, 1, 65536), 48, 2, false, false, nullptr);
  expect("frame, a huge min_count", params(0, 1, 2, 0xFFFFFFFFu), 48, 2, false, false, nullptr);
  expect("frame, compact alone", params(0, 1, 2, 0, NONE, SC_MERGE_COMPACT), 48, 2, false, false, nullptr);
  expect("frame, measure 2", params(2), 48, 1, false, false, "measure");
  expect("frame, num 0", params(0, 0, 2), 48, 1, false, false, "num");
  expect("frame, num above den", params(0, 3, 2), 48, 1, false, false, "num");
  expect("frame, den 0", params(0, 0, 0), 48, 1, false, false, "den");
  expect("frame, den 65537", params(0, 1, 65537), 48, 1, false, false, "den");
  expect("frame, num and den all ones", params(0, 0xFFFFFFFFu, 0xFFFFFFFFu), 48, 1, false, false, "den");
  expect("frame, 1025 poses", ok, 48, 1025, false, false, "n_poses");
  expect("frame, no pose", ok, 48, 0, false, false, "n_poses");
  expect("frame, stride 0", ok, 0, 1, false, false, "pose_stride");
  expect("frame, stride 44", ok, 44, 1, false, false, "pose_stride");
  expect("frame, stride 50", ok, 50, 1, false, false, "pose_stride");
  expect("frame, stride 48 with the flag", flag, 48, 1, false, false, "pose_stride");
  expect("frame, stride 52 with the flag", flag, 52, 1, false, false, nullptr);
  expect("frame, sel_mode 2", params(0, 1, 2, 0, 2), 48, 1, false, true, "sel_mode");
  expect("frame, a mask without sel", params(0, 1, 2, 0, MASK), 48, 1, false, false, "sel is NULL");
  expect("frame, flag 4", params(0, 1, 2, 0, NONE, 4), 48, 1, false, false, "flag");
  expect("frame, flag 7", params(0, 1, 2, 0, NONE, 7), 52, 1, false, false, "flag");
  {
    sc_merge_params bad = ok; bad.size = 28;
    expect("frame, size", bad, 48, 1, false, false, "size");
    expect("batch, size", bad, 80, 1, true, false, "size");
    sc_merge_params res = ok; res.reserved[0] = 1;
    expect("frame, reserved", res, 48, 1, false, false, "reserved");
    expect("batch, reserved", res, 80, 1, true, false, "reserved");
  }
  expect("batch, good", ok, 80, 64, true, false, nullptr);
  expect("batch, both flags are allowed", params(0, 1, 2, 0, NONE, SC_MERGE_STATUS | SC_MERGE_COMPACT), 52, 1, true, false, nullptr);
  expect("batch, 65 poses", ok, 80, 65, true, false, "n_poses");
  expect("batch, no pose", ok, 80, 0, true, false, "n_poses");
  expect("batch, stride 48", ok, 48, 1, true, false, "pose_stride");
  expect("batch, stride 54", ok, 54, 1, true, false, "pose_stride");
  expect("batch, a mask", params(0, 1, 2, 0, MASK), 80, 1, true, true, "sel_mode");
  expect("batch, measure 2", params(2), 80, 1, true, false, "measure");
  expect("batch, num above den", params(0, 2, 1), 80, 1, true, false, "num");

  walk("frame, stride 48", 64, 1, 48, ok, false);
  walk("frame, stride 64 with the status", 1024, 1, 64, flag, false);
  walk("frame, one pose", 1, 1, 48, ok, false);
  walk("batch, 64 x 7, stride 80", 64, 7, 80, ok, true);
  walk("batch, 1 x 1, stride 52", 1, 1, 52, ok, true);
  if (sc::pose_bytes_read(0, 48, sc::merge_reads_status(&ok, false)) != 0) { printf("FAIL no record, no byte\n"); failures++; }
  if (sc::merge_reads_status(&ok, false) || !sc::merge_reads_status(&ok, true) || !sc::merge_reads_status(&flag, false)) {
    printf("FAIL who reads the status\n");
    failures++;
  }

  size_is("words, n = 1", sc::merge_row_words_of(1), 1);
  size_is("words, n = 64", sc::merge_row_words_of(64), 1);
  size_is("words, n = 65", sc::merge_row_words_of(65), 2);
  size_is("rows, n = 129, 3 poses", sc::merge_rows_bytes(129, 3), 3 * 3 * 8);
  size_is("scratch, n = 129, 3 poses", sc::merge_scratch_bytes(129, 3), 3 * 3 * 8 + 3 * 8);
  size_is("scratch, n = 2^31 - 1, 1024 poses", sc::merge_scratch_bytes(0x7FFFFFFFull, 1024), 1024ull * 33554432ull * 8 + 1024 * 8);  // (64 bits)
  size_is("table, 1024 poses", sc::merge_table_bytes(1024), 4ull << 20);
  size_is("table, one pose", sc::merge_table_bytes(1), 4);
  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
