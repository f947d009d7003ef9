// Stand-alone program for the host-only rules of sc_pairs_cycles (sac-cot_amd/csrc/sc_cycles_check.hpp): every refusal of the
// parameter block, the stride and the list, the two thresholds, and the adjacency build — on exactly sized heap arrays, so that a
// read or write past one ends the run when this is built with -fsanitize=address,undefined (tests/test_cycles_abi.py builds and
// runs it that way; no GPU, no Python in the process).  The adjacency of every list is checked against its definition, restated
// here the slow way: set s's entries are the pairs that name s and another set, ordered by (that set, pair index), each flagged
// with its stored direction; a pair's record names its two sets in ascending order and the two lists' ranges.  The adjacency is
// read out of the image that a call stages (pairs_image, without the list starts), written into a buffer of exactly
// cycles_meta_bytes; the 7-set list is written with the starts as well.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sac-cot_amd/csrc/sc_cycles_check.hpp"

static int failures = 0;

static void check(const char* what, bool ok) {
  if (!ok) { printf("FAIL %s\n", what); failures++; }
}

static sc_cycle_params params(float rot_tol = 0.01f, float trans_tol = 0.01f, uint32_t min_ok = 1, uint32_t max_rounds = 16, uint32_t flags = 0) {
  sc_cycle_params cp;
  memset(&cp, 0, sizeof(cp));
  cp.size = sizeof(cp); cp.min_ok = min_ok; cp.max_rounds = max_rounds; cp.flags = flags; cp.rot_tol = rot_tol; cp.trans_tol = trans_tol;
  return cp;
}

static void expect_params(const char* what, const sc_cycle_params& cp, uint32_t stride, const char* want) {
  sc_cycle_params* p = new sc_cycle_params(cp);  // a heap copy of the exact size
  const char* got = sc::cycles_params_error(p);
  if (!got) got = sc::cycles_stride_error(p, stride);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
  delete p;
}

static const char* list_error(uint32_t n_sets, const std::vector<uint32_t>& pairs, std::vector<uint32_t>* deg_out = nullptr) {
  const uint32_t n_pairs = (uint32_t)(pairs.size() / 2);
  uint32_t* list = new uint32_t[pairs.size()];
  if (!pairs.empty()) memcpy(list, pairs.data(), pairs.size() * 4);
  uint32_t* deg = new uint32_t[n_sets];
  const char* got = sc::cycles_list_error(n_sets, list, n_pairs, deg);
  if (deg_out) deg_out->assign(deg, deg + n_sets);
  delete[] deg;
  delete[] list;
  return got;
}

static void expect_list(const char* what, uint32_t n_sets, const std::vector<uint32_t>& pairs, const char* want) {
  const char* got = list_error(n_sets, pairs);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
}

// the adjacency of an accepted list against its definition
static void adjacency(const char* what, uint32_t n_sets, const std::vector<uint32_t>& pairs) {
  const uint32_t n_pairs = (uint32_t)(pairs.size() / 2);
  if (list_error(n_sets, pairs)) { printf("FAIL %s: the list is refused\n", what); failures++; return; }
  const uint64_t n_entries = sc::cycles_entry_count(pairs.data(), n_pairs);
  uint32_t* off = new uint32_t[(size_t)n_sets + 1];
  const sc::PairsImageAt at = sc::pairs_image_at(n_pairs, n_entries);
  char* image = new char[sc::cycles_meta_bytes(n_pairs, n_entries)];
  sc::pairs_image(n_sets, pairs.data(), n_pairs, n_entries, off, false, image);
  const uint64_t* entries = reinterpret_cast<const uint64_t*>(image + at.entries);
  const uint32_t* rec = reinterpret_cast<const uint32_t*>(image + at.rec);
  bool ok = off[0] == 0 && off[n_sets] == n_entries && sc::cycles_meta_bytes(n_pairs, n_entries) == 32ull * n_pairs + 8 * n_entries;
  // every list: ascending (strictly: an entry is unique), only pairs that name s and another set, with the right direction
  std::vector<uint32_t> seen(n_pairs, 0);
  for (uint32_t s = 0; s < n_sets && ok; s++) {
    ok = ok && off[s] <= off[s + 1];
    for (uint32_t i = off[s]; i < off[s + 1] && ok; i++) {
      const uint64_t e = entries[i];
      const uint32_t nb = sc::cycles_entry_set(e), p = sc::cycles_entry_pair(e);
      ok = ok && p < n_pairs && nb != s;
      if (!ok) break;
      const uint32_t a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
      ok = ok && (sc::cycles_entry_forward(e) ? (a == s && b == nb) : (b == s && a == nb));
      if (i > off[s]) {
        const uint64_t before = entries[i - 1];
        const uint32_t nb0 = sc::cycles_entry_set(before), p0 = sc::cycles_entry_pair(before);
        ok = ok && (nb0 < nb || (nb0 == nb && p0 < p));  // by (neighbour, pair)
      }
      seen[p]++;
    }
  }
  for (uint32_t p = 0; p < n_pairs && ok; p++) {
    const uint32_t a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1], lo = a < b ? a : b, hi = a < b ? b : a;
    const uint32_t* r = rec + (size_t)sc::CYCLES_REC_WORDS * p;
    ok = ok && seen[p] == (a == b ? 0u : 2u) && r[sc::CW_LO] == lo && r[sc::CW_HI] == hi && r[sc::CW_FWD] == (a < b ? 1u : 0u) && r[3] == 0;
    if (a == b) ok = ok && r[sc::CW_LO_BEGIN] == r[sc::CW_LO_END] && r[sc::CW_HI_BEGIN] == r[sc::CW_HI_END];
    else ok = ok && r[sc::CW_LO_BEGIN] == off[lo] && r[sc::CW_LO_END] == off[lo + 1] && r[sc::CW_HI_BEGIN] == off[hi] && r[sc::CW_HI_END] == off[hi + 1];
  }
  if (!ok) { printf("FAIL %s: the adjacency is not what the list says\n", what); failures++; }
  delete[] image;
  delete[] off;
}

// the image with the list starts against the one without: the same records and entries, then the n_sets + 1 offsets
static void image_with_starts(const char* what, uint32_t n_sets, const std::vector<uint32_t>& pairs) {
  const uint32_t n_pairs = (uint32_t)(pairs.size() / 2);
  const uint64_t n_entries = sc::cycles_entry_count(pairs.data(), n_pairs);
  const sc::PairsImageAt at = sc::pairs_image_at(n_pairs, n_entries);
  const uint64_t bytes = sc::sync_meta_bytes(n_sets, n_pairs, n_entries);
  uint32_t* off = new uint32_t[(size_t)n_sets + 1];
  char* without = new char[at.starts];
  char* with = new char[bytes];
  sc::pairs_image(n_sets, pairs.data(), n_pairs, n_entries, off, false, without);
  sc::pairs_image(n_sets, pairs.data(), n_pairs, n_entries, off, true, with);
  check(what, at.rec == 0 && at.entries == 32ull * n_pairs && at.starts == at.entries + 8 * n_entries && bytes == at.starts + 4 * ((uint64_t)n_sets + 1) &&
                  memcmp(with, without, at.starts) == 0 && memcmp(with + at.starts, off, ((size_t)n_sets + 1) * 4) == 0 && off[n_sets] == n_entries);
  delete[] with;
  delete[] without;
  delete[] off;
}

int main() {
  // ---- the parameter block and the stride
  expect_params("defaults", params(), 48, nullptr);
  { sc_cycle_params cp = params(); cp.size = 28; expect_params("size", cp, 48, "params->size"); }
  expect_params("max_rounds 0", params(0.01f, 0.01f, 1, 0), 48, "max_rounds");
  expect_params("max_rounds 65", params(0.01f, 0.01f, 1, 65), 48, "max_rounds");
  expect_params("max_rounds 64", params(0.01f, 0.01f, 1, 64), 48, nullptr);
  expect_params("min_ok 0", params(0.01f, 0.01f, 0), 48, nullptr);
  expect_params("min_ok all ones", params(0.01f, 0.01f, 0xFFFFFFFFu), 48, nullptr);
  expect_params("rot_tol negative", params(-1e-9f), 48, "rot_tol");
  expect_params("rot_tol NaN", params(NAN), 48, "rot_tol");
  expect_params("rot_tol inf", params(INFINITY), 48, "rot_tol");
  expect_params("rot_tol past pi", params(3.1415930f), 48, "rot_tol");
  expect_params("rot_tol pi", params(sc::CYCLES_ROT_TOL_MAX), 48, nullptr);
  expect_params("rot_tol 0", params(0.f, 0.f), 48, nullptr);
  expect_params("trans_tol negative", params(0.01f, -1e-9f), 48, "trans_tol");
  expect_params("trans_tol NaN", params(0.01f, NAN), 48, "trans_tol");
  expect_params("trans_tol inf", params(0.01f, INFINITY), 48, "trans_tol");
  expect_params("unknown flag", params(0.01f, 0.01f, 1, 16, 2), 52, "unknown flag");
  { sc_cycle_params cp = params(); cp.reserved[1] = 1; expect_params("reserved", cp, 48, "reserved"); }
  expect_params("stride 44", params(), 44, "pose_stride");
  expect_params("stride 50", params(), 50, "pose_stride");
  expect_params("stride 48 with the status", params(0.01f, 0.01f, 1, 16, SC_CYCLES_STATUS), 48, "pose_stride");
  expect_params("stride 52 with the status", params(0.01f, 0.01f, 1, 16, SC_CYCLES_STATUS), 52, nullptr);
  expect_params("stride 80", params(0.01f, 0.01f, 1, 16, SC_CYCLES_STATUS), 80, nullptr);

  // ---- the thresholds
  {
    const sc_cycle_params cp = params(0.25f, 0.5f);
    double out[2];
    sc::cycles_thresholds(&cp, out);
    check("thresholds", out[0] == 1.0 + 2.0 * cos((double)0.25f) && out[1] == 0.25);
    const sc_cycle_params zero = params(0.f, 0.f);
    sc::cycles_thresholds(&zero, out);
    check("thresholds at 0", out[0] == 3.0 && out[1] == 0.0);
  }

  // ---- the list
  expect_list("n_sets 0", 0, {}, "n_sets == 0");
  expect_list("n_pairs 0", 3, {}, "n_pairs == 0");
  expect_list("an index past the sets", 3, {0, 1, 1, 3}, "set index");
  expect_list("self pairs, repeats, both directions", 4, {0, 0, 0, 1, 1, 0, 0, 1, 2, 2}, nullptr);
  {
    std::vector<uint32_t> many((size_t)2 * (SC_CYCLES_MAX_PAIRS + 1), 0);
    for (size_t p = 0; p < many.size() / 2; p++) { many[2 * p] = (uint32_t)(p % 1000); many[2 * p + 1] = 1000 + (uint32_t)(p / 1000 % 5000); }
    expect_list("one pair too many", 6000, many, "SC_CYCLES_MAX_PAIRS");
    many.resize((size_t)2 * SC_CYCLES_MAX_PAIRS);
    expect_list("2^22 pairs", 6000, many, nullptr);
  }
  // a degree of exactly 65 535 and of 65 536: set 0 against the others, then one pair more; a self pair names its set once
  {
    std::vector<uint32_t> star;
    for (uint32_t i = 1; i <= SC_CYCLES_MAX_DEGREE; i++) { star.push_back(i % 2 ? 0 : i); star.push_back(i % 2 ? i : 0); }
    std::vector<uint32_t> deg;
    check("degree 65 535 is accepted", list_error(SC_CYCLES_MAX_DEGREE + 2, star, &deg) == nullptr && deg[0] == SC_CYCLES_MAX_DEGREE && deg[1] == 1 &&
                                           deg[SC_CYCLES_MAX_DEGREE + 1] == 0);
    adjacency("the star of 65 535", SC_CYCLES_MAX_DEGREE + 2, star);
    std::vector<uint32_t> more = star;
    more.push_back(0); more.push_back(0);
    expect_list("degree 65 536 by a self pair", SC_CYCLES_MAX_DEGREE + 2, more, "SC_CYCLES_MAX_DEGREE");
    more = star;
    more.push_back(SC_CYCLES_MAX_DEGREE + 1); more.push_back(0);
    expect_list("degree 65 536", SC_CYCLES_MAX_DEGREE + 2, more, "SC_CYCLES_MAX_DEGREE");
  }

  // ---- the adjacency
  adjacency("one pair", 2, {1, 0});
  adjacency("only self pairs", 2, {0, 0, 1, 1});
  adjacency("self pairs, repeats, both directions, an unreferenced set", 6, {4, 1, 0, 0, 1, 4, 4, 1, 0, 1, 5, 4, 1, 5, 4, 4, 0, 4, 1, 4});
  adjacency("seven sets: a self pair, a repeat, unreferenced sets", 7, {4, 1, 0, 0, 1, 4, 4, 1, 0, 1, 5, 4, 1, 5});
  image_with_starts("seven sets: the image with its list starts", 7, {4, 1, 0, 0, 1, 4, 4, 1, 0, 1, 5, 4, 1, 5});
  {
    std::vector<uint32_t> all;  // every pair of 40 sets in a scrambled order and direction, every third one twice
    for (uint32_t k = 0; k < 40 * 39 / 2; k++) {
      const uint32_t j = (k * 577) % (40 * 39 / 2);
      uint32_t a = 0, left = j;
      while (left >= 39 - a) { left -= 39 - a; a++; }
      const uint32_t b = a + 1 + left;
      for (int rep = 0; rep < (k % 3 == 0 ? 2 : 1); rep++) { all.push_back((k + rep) % 2 ? b : a); all.push_back((k + rep) % 2 ? a : b); }
    }
    adjacency("all pairs of 40 sets", 41, all);
  }
  {
    std::vector<uint32_t> all;  // every pair of 130 sets, scrambled: 8385 pairs, more than a round's waves; every list 129 entries, longer than two waves
    const uint32_t n = 130, np = n * (n - 1) / 2;
    for (uint32_t k = 0; k < np; k++) {
      const uint32_t j = (uint32_t)(((uint64_t)k * 2579) % np);  // (2579 is prime and does not divide 8385)
      uint32_t a = 0, left = j;
      while (left >= n - 1 - a) { left -= n - 1 - a; a++; }
      const uint32_t b = a + 1 + left;
      all.push_back(k % 2 ? b : a); all.push_back(k % 2 ? a : b);
    }
    std::vector<uint32_t> deg;
    bool ok = list_error(n, all, &deg) == nullptr && all.size() == 2 * 8385u;
    for (uint32_t s = 0; s < n && ok; s++) ok = deg[s] == 129;
    check("all pairs of 130 sets: every degree is 129", ok);
    adjacency("all pairs of 130 sets", n, all);
  }

  if (failures) { printf("%d failed\n", failures); return 1; }
  printf("all passed\n");
  return 0;
}
