// Stand-alone program for the host-only rules of the caller's pose records (sac-cot_amd/csrc/sc_pose_check.hpp): every refusal rule of
// sc_polish_poses and of sc_pose_info_frame with its full message, the order of the rules, the bytes a call reads of the pose array —
// walked on an exactly sized heap array, so that a read past it ends the run when this is built with -fsanitize=address,undefined —
// and the three messages of the guides' stride rule (tests/test_pose_check_abi.py builds and runs it that way; no GPU, no Python in
// the process).
#include <cstdio>
#include <cstring>

#include "../../sac-cot_amd/csrc/sc_match_guided_batch_check.hpp"
#include "../../sac-cot_amd/csrc/sc_pose_check.hpp"

static int failures = 0;

// the messages, as sc_last_error has carried them behind the entry's name since the entries exist
static const char* const Q_SIZE = "params->size is not sizeof(sc_polish_poses_params)";
static const char* const Q_ITER = "max_iter must be 1 .. 64";
static const char* const Q_MODE = "sel_mode must be SC_POLISH_POSES_SEL_NONE, _MASK, _LABEL or _ALIVE";
static const char* const Q_LABEL0 = "label0 must be 0 unless sel_mode is SC_POLISH_POSES_SEL_LABEL or _ALIVE";
static const char* const Q_POSES = "n_poses must be 1 .. SC_POLISH_POSES_MAX";
static const char* const Q_STRIDE = "pose_stride must be a multiple of 4 and at least 48 (52 with SC_POLISH_POSES_STATUS)";
static const char* const I_SIZE = "params->size is not sizeof(sc_pose_info_params)";
static const char* const I_MODE = "sel_mode must be SC_POSE_INFO_SEL_NONE, _MASK or _LABEL";
static const char* const I_LABEL0 = "label0 must be 0 unless sel_mode is SC_POSE_INFO_SEL_LABEL";
static const char* const I_POSES = "n_poses must be 1 .. SC_POSE_INFO_MAX_POSES";
static const char* const I_STRIDE = "pose_stride must be a multiple of 4 and at least 48 (52 with SC_POSE_INFO_STATUS)";
static const char* const NO_SEL = "sel is NULL with a sel_mode that reads it";
static const char* const FLAGS = "an unknown flag, or a reserved field that is not 0";

static sc_polish_poses_params polish(uint32_t max_iter = 16, uint32_t sel_mode = 0, int32_t label0 = 0, uint32_t flags = 0) {
  sc_polish_poses_params qp;
  memset(&qp, 0, sizeof(qp));
  qp.size = sizeof(qp); qp.max_iter = max_iter; qp.sel_mode = sel_mode; qp.label0 = label0; qp.flags = flags;
  return qp;
}
static sc_pose_info_params info(uint32_t sel_mode = 0, int32_t label0 = 0, uint32_t flags = 0) {
  sc_pose_info_params ip;
  memset(&ip, 0, sizeof(ip));
  ip.size = sizeof(ip); ip.sel_mode = sel_mode; ip.label0 = label0; ip.flags = flags;
  return ip;
}

static void same(const char* what, const char* got, const char* want) {
  const bool ok = want ? (got && strcmp(got, want) == 0) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
}
// a heap copy of the exact size: the sanitizer sees every read past the block
static void expect(const char* what, const sc_polish_poses_params& qp, uint32_t stride, uint32_t n_poses, bool has_sel, const char* want) {
  sc_polish_poses_params* p = new sc_polish_poses_params(qp);
  same(what, sc::polish_poses_params_error(p, stride, n_poses, has_sel), want);
  delete p;
}
static void expect(const char* what, const sc_pose_info_params& ip, uint32_t stride, uint32_t n_poses, bool has_sel, const char* want) {
  sc_pose_info_params* p = new sc_pose_info_params(ip);
  same(what, sc::pose_info_params_error(p, stride, n_poses, has_sel), want);
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
      if (at != seen * stride || sc::pose_record_index(k, b, n_problems) != seen) { printf("FAIL %s: record (%u, %u)\n", what, k, b); failures++; }
      seen++;
      for (uint32_t x = 0; x < read; x++) sum += pose[at + x];
      if (at + read > last) last = at + read;
    }
  if (last != bytes || sum != 0) { printf("FAIL %s: %llu bytes read, %llu counted\n", what, (unsigned long long)last, (unsigned long long)bytes); failures++; }
  delete[] pose;
}

int main() {
  static_assert(sc::POSE_RT_BYTES == 12 * sizeof(float) && sc::POSE_STATUS_BYTES == sc::POSE_RT_BYTES + sizeof(int32_t), "Rt[12], then the status");
  static_assert(SC_POLISH_POSES_SEL_ALIVE == 3u && SC_POSE_INFO_SEL_LABEL == 2u, "the families' last sel_mode");
  const uint32_t QS = SC_POLISH_POSES_STATUS, IS = SC_POSE_INFO_STATUS;

  // ---- sc_polish_poses
  expect("polish, good", polish(), 48, 1, false, nullptr);
  expect("polish, 1024 poses, stride 80, alive, the flag", polish(64, SC_POLISH_POSES_SEL_ALIVE, -7, QS), 80, SC_POLISH_POSES_MAX, true, nullptr);
  expect("polish, one refit", polish(1), 48, 2, false, nullptr);
  {
    sc_polish_poses_params bad = polish(); bad.size = 28;
    expect("polish, size", bad, 48, 1, false, Q_SIZE);
    bad.size = 36;
    expect("polish, size 36", bad, 48, 1, false, Q_SIZE);
  }
  expect("polish, max_iter 0", polish(0), 48, 1, false, Q_ITER);
  expect("polish, max_iter 65", polish(65), 48, 1, false, Q_ITER);
  expect("polish, sel_mode 4", polish(16, 4), 48, 1, true, Q_MODE);
  expect("polish, sel_mode all ones", polish(16, 0xFFFFFFFFu), 48, 1, true, Q_MODE);
  for (uint32_t mode = SC_POLISH_POSES_SEL_MASK; mode <= SC_POLISH_POSES_SEL_ALIVE; mode++) {
    expect("polish, a reading sel_mode without sel", polish(16, mode), 48, 1, false, NO_SEL);
    expect("polish, a reading sel_mode with sel", polish(16, mode), 48, 1, true, nullptr);
  }
  expect("polish, label0 without a selection", polish(16, SC_POLISH_POSES_SEL_NONE, 1), 48, 1, false, Q_LABEL0);
  expect("polish, label0 with a mask", polish(16, SC_POLISH_POSES_SEL_MASK, -1), 48, 1, true, Q_LABEL0);
  expect("polish, label0 with labels", polish(16, SC_POLISH_POSES_SEL_LABEL, 5), 48, 1, true, nullptr);
  expect("polish, flag 2", polish(16, 0, 0, 2), 48, 1, false, FLAGS);
  expect("polish, flags 3", polish(16, 0, 0, 3), 52, 1, false, FLAGS);
  for (int r = 0; r < 3; r++) {
    sc_polish_poses_params res = polish(); res.reserved[r] = 1;
    expect("polish, reserved", res, 48, 1, false, FLAGS);
  }
  expect("polish, no pose", polish(), 48, 0, false, Q_POSES);
  expect("polish, 1025 poses", polish(), 48, SC_POLISH_POSES_MAX + 1, false, Q_POSES);
  expect("polish, stride 0", polish(), 0, 1, false, Q_STRIDE);
  expect("polish, stride 44", polish(), 44, 1, false, Q_STRIDE);
  expect("polish, stride 50", polish(), 50, 1, false, Q_STRIDE);
  expect("polish, stride 48 with the flag", polish(16, 0, 0, QS), 48, 1, false, Q_STRIDE);
  expect("polish, stride 52 with the flag", polish(16, 0, 0, QS), 52, 1, false, nullptr);
  // the order of the rules: of two that are broken the earlier one is reported
  {
    sc_polish_poses_params two = polish(0, 9, 3, 2); two.size = 4;
    expect("polish, size before max_iter", two, 0, 0, false, Q_SIZE);
    two.size = sizeof(two);
    expect("polish, max_iter before sel_mode", two, 0, 0, false, Q_ITER);
    two.max_iter = 16;
    expect("polish, sel_mode before sel", two, 0, 0, false, Q_MODE);
    two.sel_mode = SC_POLISH_POSES_SEL_MASK;
    expect("polish, sel before label0", two, 0, 0, false, NO_SEL);
    expect("polish, label0 before the flags", two, 0, 0, true, Q_LABEL0);
    two.label0 = 0;
    expect("polish, the flags before n_poses", two, 0, 0, true, FLAGS);
    two.flags = 0;
    expect("polish, n_poses before the stride", two, 0, 0, true, Q_POSES);
    expect("polish, the stride last", two, 0, 1, true, Q_STRIDE);
  }

  // ---- sc_pose_info_frame
  expect("info, good", info(), 48, 1, false, nullptr);
  expect("info, 1024 poses, stride 80, labels, the flag", info(SC_POSE_INFO_SEL_LABEL, -7, IS), 80, SC_POSE_INFO_MAX_POSES, true, nullptr);
  {
    sc_pose_info_params bad = info(); bad.size = 28;
    expect("info, size", bad, 48, 1, false, I_SIZE);
    bad.size = 36;
    expect("info, size 36", bad, 48, 1, false, I_SIZE);
  }
  expect("info, sel_mode 3", info(3), 48, 1, true, I_MODE);
  expect("info, sel_mode all ones", info(0xFFFFFFFFu), 48, 1, true, I_MODE);
  for (uint32_t mode = SC_POSE_INFO_SEL_MASK; mode <= SC_POSE_INFO_SEL_LABEL; mode++) {
    expect("info, a reading sel_mode without sel", info(mode), 48, 1, false, NO_SEL);
    expect("info, a reading sel_mode with sel", info(mode), 48, 1, true, nullptr);
  }
  expect("info, label0 without a selection", info(SC_POSE_INFO_SEL_NONE, 1), 48, 1, false, I_LABEL0);
  expect("info, label0 with a mask", info(SC_POSE_INFO_SEL_MASK, -1), 48, 1, true, I_LABEL0);
  expect("info, flag 2", info(0, 0, 2), 48, 1, false, FLAGS);
  expect("info, flags 3", info(0, 0, 3), 52, 1, false, FLAGS);
  for (int r = 0; r < 4; r++) {
    sc_pose_info_params res = info(); res.reserved[r] = 1;
    expect("info, reserved", res, 48, 1, false, FLAGS);
  }
  expect("info, no pose", info(), 48, 0, false, I_POSES);
  expect("info, 1025 poses", info(), 48, SC_POSE_INFO_MAX_POSES + 1, false, I_POSES);
  expect("info, stride 0", info(), 0, 1, false, I_STRIDE);
  expect("info, stride 44", info(), 44, 1, false, I_STRIDE);
  expect("info, stride 50", info(), 50, 1, false, I_STRIDE);
  expect("info, stride 48 with the flag", info(0, 0, IS), 48, 1, false, I_STRIDE);
  expect("info, stride 52 with the flag", info(0, 0, IS), 52, 1, false, nullptr);
  {
    sc_pose_info_params two = info(9, 3, 2); two.size = 4;
    expect("info, size before sel_mode", two, 0, 0, false, I_SIZE);
    two.size = sizeof(two);
    expect("info, sel_mode before sel", two, 0, 0, false, I_MODE);
    two.sel_mode = SC_POSE_INFO_SEL_MASK;
    expect("info, sel before label0", two, 0, 0, false, NO_SEL);
    expect("info, label0 before the flags", two, 0, 0, true, I_LABEL0);
    two.label0 = 0;
    expect("info, the flags before n_poses", two, 0, 0, true, FLAGS);
    two.flags = 0;
    expect("info, n_poses before the stride", two, 0, 0, true, I_POSES);
    expect("info, the stride last", two, 0, 1, true, I_STRIDE);
  }

  // ---- the record rule itself
  if (sc::pose_stride_ok(0, false) || sc::pose_stride_ok(44, false) || sc::pose_stride_ok(50, false) || !sc::pose_stride_ok(48, false) ||
      sc::pose_stride_ok(48, true) || !sc::pose_stride_ok(52, true) || sc::pose_stride_ok(54, true) || !sc::pose_stride_ok(0xFFFFFFFCu, true)) {
    printf("FAIL pose_stride_ok\n");
    failures++;
  }
  walk("one record", 1, 1, 48, false);
  walk("one record with the status", 1, 1, 52, true);
  walk("64 records, stride 48", 64, 1, 48, false);
  walk("64 records, stride 64 with the status", 64, 1, 64, true);
  walk("16 x 7 motion-major, stride 80", 16, 7, 80, true);
  if (sc::pose_bytes_read(0, 48, false) != 0 || sc::pose_bytes_read(0, 80, true) != 0) { printf("FAIL no record, no byte\n"); failures++; }
  // the offsets are 64-bit: 64 planes of 2^26 problems at the largest stride pass 2^32 bytes by far
  if (sc::pose_record_offset(63, (1u << 26) - 1, 1u << 26, 0xFFFFFFFCu) != ((uint64_t)63 * (1u << 26) + (1u << 26) - 1) * 0xFFFFFFFCull) {
    printf("FAIL the 64-bit offset\n");
    failures++;
  }

  // ---- the guides' stride rule keeps its three messages
  same("guide, stride 50", sc::guide_pose_stride_error(0, 50), "pose_stride must be a multiple of 4");
  same("guide, stride 44", sc::guide_pose_stride_error(0, 44), "pose_stride must be at least 48 (float Rt[12])");
  same("guide, stride 48 with the flag", sc::guide_pose_stride_error(SC_GUIDE_POSE_STATUS, 48),
       "pose_stride must be at least 52 with SC_GUIDE_POSE_STATUS (the status at byte 48)");
  same("guide, stride 48", sc::guide_pose_stride_error(0, 48), nullptr);
  same("guide, stride 52 with the flag", sc::guide_pose_stride_error(SC_GUIDE_POSE_STATUS, 52), nullptr);
  same("guide, stride 50 with the flag: the multiple first", sc::guide_pose_stride_error(SC_GUIDE_POSE_STATUS, 50), "pose_stride must be a multiple of 4");

  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
