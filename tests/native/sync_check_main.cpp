// Stand-alone program for the host-only rules of sc_pairs_sync (sac-cot_amd/csrc/sc_sync_check.hpp): every refusal of the parameter
// block, of the two strides and of the anchor with its text, the two thresholds, the bytes of a strided use array that a call
// reads, and where the staged words and the workspace areas lie — on exactly sized heap copies, so that a read past one ends the run
// when this is built with -fsanitize=address,undefined (tests/test_sync_abi.py builds and runs it that way; no GPU, no Python in the
// process).  The list's rules and the adjacency are sc_cycles_check.hpp's and have a program of their own (cycles_check_main.cpp);
// here the staged image of a call is written by the function that every entry stages it with (sc_cycles_check.hpp: pairs_image),
// into a buffer of exactly sync_meta_bytes — and of exactly cycles_meta_bytes without the list starts —, and read back.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sac-cot_amd/csrc/sc_sync_check.hpp"

static int failures = 0;

static void check(const char* what, bool ok) {
  if (!ok) { printf("FAIL %s\n", what); failures++; }
}

static sc_sync_params params(float rot_tol = 1e-4f, float trans_tol = 1e-4f, uint32_t anchor = 0, uint32_t max_rounds = 32, uint32_t flags = 0) {
  sc_sync_params sp;
  memset(&sp, 0, sizeof(sp));
  sp.size = sizeof(sp); sp.anchor = anchor; sp.max_rounds = max_rounds; sp.flags = flags; sp.rot_tol = rot_tol; sp.trans_tol = trans_tol;
  return sp;
}

// the first rule that refuses (params, then the strides, then the anchor), as sc_capi_sync.hip asks them
static void expect(const char* what, const sc_sync_params& sp, uint32_t pose_stride, bool has_use, uint32_t use_stride, uint32_t n_sets, const char* want) {
  sc_sync_params* p = new sc_sync_params(sp);  // a heap copy of the exact size
  const char* got = sc::sync_params_error(p);
  if (!got) got = sc::sync_stride_error(p, pose_stride, has_use, use_stride);
  if (!got) got = sc::sync_anchor_error(p, n_sets);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
  delete p;
}

int main() {
  // ---- the parameter block
  expect("defaults", params(), 48, false, 0, 3, nullptr);
  { sc_sync_params sp = params(); sp.size = 28; expect("size", sp, 48, false, 0, 3, "params->size is not sizeof(sc_sync_params)"); }
  expect("max_rounds 0", params(1e-4f, 1e-4f, 0, 0), 48, false, 0, 3, "max_rounds must be 1 .. 256");
  expect("max_rounds 257", params(1e-4f, 1e-4f, 0, 257), 48, false, 0, 3, "max_rounds must be 1 .. 256");
  expect("max_rounds 256", params(1e-4f, 1e-4f, 0, 256), 48, false, 0, 3, nullptr);
  expect("max_rounds 1", params(1e-4f, 1e-4f, 0, 1), 48, false, 0, 3, nullptr);
  expect("rot_tol negative", params(-1e-9f), 48, false, 0, 3, "rot_tol must be finite and in [0, pi]");
  expect("rot_tol NaN", params(NAN), 48, false, 0, 3, "rot_tol");
  expect("rot_tol inf", params(INFINITY), 48, false, 0, 3, "rot_tol");
  expect("rot_tol past pi", params(3.1415930f), 48, false, 0, 3, "rot_tol");
  expect("rot_tol pi", params(sc::CYCLES_ROT_TOL_MAX), 48, false, 0, 3, nullptr);
  expect("tolerances 0", params(0.f, 0.f), 48, false, 0, 3, nullptr);
  expect("trans_tol negative", params(1e-4f, -1e-9f), 48, false, 0, 3, "trans_tol must be finite and >= 0");
  expect("trans_tol NaN", params(1e-4f, NAN), 48, false, 0, 3, "trans_tol");
  expect("trans_tol inf", params(1e-4f, INFINITY), 48, false, 0, 3, "trans_tol");
  expect("unknown flag", params(1e-4f, 1e-4f, 0, 32, 2), 52, false, 0, 3, "an unknown flag");
  { sc_sync_params sp = params(); sp.reserved[0] = 1; expect("reserved 0", sp, 48, false, 0, 3, "a reserved field"); }
  { sc_sync_params sp = params(); sp.reserved[1] = 1; expect("reserved 1", sp, 48, false, 0, 3, "a reserved field"); }
  // ---- the strides
  expect("pose_stride 44", params(), 44, false, 0, 3, "pose_stride must be a multiple of 4 and at least 48 (52 with SC_SYNC_STATUS)");
  expect("pose_stride 50", params(), 50, false, 0, 3, "pose_stride");
  expect("pose_stride 48 with the status", params(1e-4f, 1e-4f, 0, 32, SC_SYNC_STATUS), 48, false, 0, 3, "pose_stride");
  expect("pose_stride 52 with the status", params(1e-4f, 1e-4f, 0, 32, SC_SYNC_STATUS), 52, false, 0, 3, nullptr);
  expect("pose_stride 160 with the status", params(1e-4f, 1e-4f, 0, 32, SC_SYNC_STATUS), 160, false, 0, 3, nullptr);
  expect("use_stride 0", params(), 48, true, 0, 3, "use_stride must be a multiple of 4 and at least 4");
  expect("use_stride 2", params(), 48, true, 2, 3, "use_stride");
  expect("use_stride 6", params(), 48, true, 6, 3, "use_stride");
  expect("use_stride 4", params(), 48, true, 4, 3, nullptr);
  expect("use_stride 48", params(), 48, true, 48, 3, nullptr);
  expect("use_stride 6 without use", params(), 48, false, 6, 3, nullptr);  // ignored with NULL
  // ---- the anchor
  expect("anchor == n_sets", params(1e-4f, 1e-4f, 3), 48, false, 0, 3, "anchor must be less than n_sets");
  expect("anchor all ones", params(1e-4f, 1e-4f, 0xFFFFFFFFu), 48, false, 0, 3, "anchor");
  expect("anchor n_sets - 1", params(1e-4f, 1e-4f, 2), 48, false, 0, 3, nullptr);

  // ---- the thresholds: on the squared Frobenius distance, and not zero where a trace's would be
  {
    double out[2];
    const sc_sync_params sp = params(0.25f, 0.5f);
    sc::sync_thresholds(&sp, out);
    check("thresholds", out[0] == 0.125 && out[1] == 0.25);
    const sc_sync_params zero = params(0.f, 0.f);
    sc::sync_thresholds(&zero, out);
    check("thresholds at 0", out[0] == 0.0 && out[1] == 0.0);
    const sc_sync_params tiny = params(1e-8f, 1e-20f);
    sc::sync_thresholds(&tiny, out);
    check("thresholds of tiny tolerances", out[0] == 2.0 * (double)1e-8f * (double)1e-8f && out[0] > 0.0 && out[1] == (double)1e-20f * (double)1e-20f && out[1] > 0.0 &&
                                               1.0 + 2.0 * cos((double)1e-8f) == 3.0);
  }

  // ---- the offsets
  check("use bytes", sc::sync_use_bytes_read(0, 48) == 0 && sc::sync_use_bytes_read(1, 48) == 4 && sc::sync_use_bytes_read(276, 48) == 275 * 48 + 4 &&
                         sc::sync_use_bytes_read(276, 4) == 276 * 4 && sc::sync_use_bytes_read(1u << 22, 0xFFFFFFFCu) == ((1ull << 22) - 1) * 0xFFFFFFFCull + 4);
  check("workspace", sc::sync_wide_bytes(10) == 10 * 200 && sc::sync_weight_at(10) == 1920 && sc::sync_info_at(7) == 2048 + 2 * 104 * 7 &&
                         sc::sync_state_bytes(7) == 2048 + 224 * 7 && sc::sync_state_bytes(0xFFFFFFFFu) == 2048 + 224ull * 0xFFFFFFFFull);
  {
    // the staged image of a list with a self pair, a repeat and an unreferenced set, in a buffer of exactly its size
    const std::vector<uint32_t> pairs = {4, 1, 0, 0, 1, 4, 4, 1, 0, 1, 5, 4, 1, 5};
    const uint32_t n_sets = 7, n_pairs = (uint32_t)(pairs.size() / 2);
    uint32_t* off = new uint32_t[n_sets + 1];
    check("the list is accepted", sc::cycles_list_error(n_sets, pairs.data(), n_pairs, off) == nullptr);
    const uint64_t n_entries = sc::cycles_entry_count(pairs.data(), n_pairs);
    const uint64_t bytes = sc::sync_meta_bytes(n_sets, n_pairs, n_entries), off_at = sc::sync_off_at(n_pairs, n_entries);
    check("meta bytes", n_entries == 12 && off_at == 32 * 7 + 8 * 12 && bytes == off_at + 4 * 8 && off_at % 8 == 0);
    const sc::PairsImageAt at = sc::pairs_image_at(n_pairs, n_entries);
    check("the image's parts", at.rec == 0 && at.entries == 32 * n_pairs && at.starts == off_at);
    char* h = new char[bytes];
    sc::pairs_image(n_sets, pairs.data(), n_pairs, n_entries, off, true, h);
    const uint32_t* staged = reinterpret_cast<const uint32_t*>(h + at.starts);
    const uint64_t* entries = reinterpret_cast<const uint64_t*>(h + at.entries);
    bool ok = staged[0] == 0 && staged[n_sets] == n_entries;
    for (uint32_t s = 0; s < n_sets && ok; s++) {
      ok = staged[s] <= staged[s + 1];
      for (uint32_t i = staged[s]; i < staged[s + 1] && ok; i++) {
        const uint32_t p = sc::cycles_entry_pair(entries[i]), nb = sc::cycles_entry_set(entries[i]);
        ok = p < n_pairs && nb < n_sets && nb != s && (pairs[2 * p] == s || pairs[2 * p + 1] == s) && (pairs[2 * p] == nb || pairs[2 * p + 1] == nb) &&
             (i == staged[s] || entries[i - 1] < entries[i]);
      }
    }
    check("the staged list starts", ok && staged[2] == staged[3] && staged[6] == staged[7]);  // sets 2, 3 and 6 are named by no pair
    // the image without the starts: the same records and entries in a buffer that ends where the starts would begin
    char* g = new char[at.starts];
    sc::pairs_image(n_sets, pairs.data(), n_pairs, n_entries, off, false, g);
    check("the image without the starts", sc::cycles_meta_bytes(n_pairs, n_entries) == at.starts && memcmp(g, h, at.starts) == 0);
    delete[] g;
    delete[] h;
    delete[] off;
  }

  if (failures) { printf("%d failed\n", failures); return 1; }
  printf("all passed\n");
  return 0;
}
