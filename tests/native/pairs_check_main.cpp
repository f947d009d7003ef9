// Stand-alone program for the host-only checks of sc_match_pairs (sac-cot_amd/csrc/sc_pairs_check.hpp): the rules of the table and
// the list, the slot starts, the pairs' records and the tile map, on exactly sized heap arrays, so that a read or write past an
// array ends the run when it is built with -fsanitize=address,undefined (tests/test_pairs_abi.py builds and runs it that way; no
// GPU, no Python in the process).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sac-cot_amd/csrc/sc_pairs_check.hpp"

static int failures = 0;

static void fail(const char* what, const char* why, unsigned long long at) {
  printf("FAIL %s: %s %llu\n", what, why, at);
  failures++;
}

static void expect(const char* what, std::vector<uint32_t> off, std::vector<uint32_t> prs, uint32_t knn, bool features, const char* want) {
  const uint32_t n_sets = (uint32_t)off.size() - 1, np = (uint32_t)prs.size() / 2;
  // heap copies of the exact size: the sanitizer sees every index past the arrays
  uint32_t* so = new uint32_t[off.size()];
  uint32_t* pr = new uint32_t[prs.size() ? prs.size() : 1];
  memcpy(so, off.data(), off.size() * 4);
  if (!prs.empty()) memcpy(pr, prs.data(), prs.size() * 4);
  const char* got = sc::pairs_error(so, n_sets, pr, np, knn, features);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
  if (!got) {
    // accepted: the bases of a pair are the sums over the pairs BEFORE it — never a function of its sets' rows in the table, so two
    // pairs that share a set share nothing; the tile map covers every source row of every pair once, in order, inside the pair
    const sc::PairsTotals tot = sc::pairs_totals(so, pr, np, 64);
    // the three as the device copy holds them: one array of exactly pairs_meta_layout's words, filled by pairs_meta_fill
    const sc::BatchMetaLayout at = sc::pairs_meta_layout(np, (uint32_t)tot.tiles);
    if (at.slot_at != (size_t)sc::PAIRS_REC_WORDS * np || at.map_at != at.slot_at + np + 1 || at.words != at.map_at + 2 * tot.tiles)
      fail(what, "the metadata's layout", at.words);
    uint32_t* meta = new uint32_t[at.words];
    sc::pairs_meta_fill(so, pr, np, knn, 64, at, meta);
    const uint32_t *rec = meta, *slot = meta + at.slot_at, *map = meta + at.map_at;
    uint64_t rows_s = 0, rows_t = 0, t = 0;
    for (uint32_t p = 0; p < np; p++) {
      const uint32_t a = pr[2 * p], b = pr[2 * p + 1], ns = so[a + 1] - so[a], nt = so[b + 1] - so[b];
      const uint32_t* r = rec + (size_t)sc::PAIRS_REC_WORDS * p;
      if (r[0] != so[a] || r[1] != ns || r[2] != so[b] || r[3] != nt) fail(what, "the sets of pair", p);
      if (r[4] != rows_s || r[5] != rows_s * knn || slot[p] != r[5]) fail(what, "the list base / slot of pair", p);
      if (((uint64_t)r[7] << 32 | r[6]) != rows_t) fail(what, "the column base of pair", p);
      for (uint32_t row = 0; row < ns; row += 64, t++)
        if (t >= tot.tiles || map[2 * t] != p || map[2 * t + 1] != row) fail(what, "tile", t);
      rows_s += ns; rows_t += nt;
    }
    if (slot[np] != rows_s * knn || tot.total_s != rows_s || tot.total_t != rows_t) fail(what, "the totals", rows_s);
    if (t != tot.tiles) fail(what, "tiles mapped", t);
    delete[] meta;
  }
  delete[] so;
  delete[] pr;
}

int main() {
  //   sets: 0: 1 row, 1: 64, 2: 65, 3: 0 rows, 4: 4096, 5: 4097, 6: 257, 7: 256
  const std::vector<uint32_t> off = {0, 1, 65, 130, 130, 4226, 8323, 8580, 8836};
  expect("good: shared, self, repeated, descending", off, {2, 1, 1, 1, 2, 1, 2, 1, 4, 0, 0, 4, 1, 0}, 4, false, nullptr);
  expect("good: one row tile either side", off, {1, 2, 2, 1, 0, 0}, 1, true, nullptr);
  expect("an unreferenced empty set and an unreferenced set of 4097", off, {0, 1}, 1, false, nullptr);
  expect("n_sets == 0", {0}, {0, 0}, 1, false, "n_sets == 0");
  expect("n_pairs == 0", off, {}, 1, false, "n_pairs == 0");
  expect("knn == 0", off, {0, 1}, 0, false, "knn");
  expect("knn == 5", off, {0, 1}, 5, false, "knn");
  expect("set_off decreases (an unreferenced set)", {0, 8, 4, 12}, {2, 2}, 1, false, "decreases");
  expect("a source index == n_sets", off, {8, 0}, 1, false, ">= n_sets");
  expect("a target index == n_sets", off, {0, 1, 1, 8}, 1, false, ">= n_sets");
  expect("an index of all ones", off, {0, 0xFFFFFFFFu}, 1, false, ">= n_sets");
  expect("a referenced empty source", off, {3, 1}, 1, false, "no rows");
  expect("a referenced empty target", off, {1, 3}, 1, false, "no rows");
  expect("4097 source rows", off, {5, 1}, 1, false, "SC_MATCH_BATCH_MAX_N");
  expect("4097 target rows", off, {1, 5}, 1, false, "SC_MATCH_BATCH_MAX_N");
  expect("features: 257 x 2 entries", off, {6, 1}, 2, true, "SC_BATCH_MAX_N");
  expect("features: 256 x 2 entries", off, {7, 6}, 2, true, nullptr);
  expect("features: a TARGET of 257 at knn 2", off, {7, 6}, 2, true, nullptr);
  expect("match alone: 257 x 2 entries", off, {6, 1}, 2, false, nullptr);
  {  // the entries in all: 2^31 are accepted, one pair more is not (2^19 pairs of a 4096-row source at knn 1; 2^17 at knn 4) — a
     // total that no set_off can express for packed problems of a table this small: one set, referenced by every pair
    for (uint32_t knn : {1u, 4u}) {
      const uint32_t np = (1u << 19) / knn;
      std::vector<uint32_t> prs(2 * ((size_t)np + 1));
      for (size_t p = 0; p <= np; p++) { prs[2 * p] = 4; prs[2 * p + 1] = 0; }
      expect("2^31 entries", off, std::vector<uint32_t>(prs.begin(), prs.end() - 2), knn, false, nullptr);
      expect("2^31 + 4096 knn entries", off, prs, knn, false, "2^31");
    }
  }
  {  // the column base passes 2^32: 2^20 + 1 pairs whose target holds 4096 rows (their source holds one)
    const uint32_t np = (1u << 20) + 1;
    std::vector<uint32_t> prs(2 * (size_t)np);
    for (size_t p = 0; p < np; p++) { prs[2 * p] = 0; prs[2 * p + 1] = 4; }
    expect("2^32 target rows before the last pair", off, prs, 1, false, nullptr);
  }
  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
