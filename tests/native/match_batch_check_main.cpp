// Stand-alone program for the host-only checks of sc_match_batch (sac-cot_amd/csrc/sc_match_batch_check.hpp): the offset rules and
// the tile map, on exactly sized heap arrays, so that a read or write past an array ends the run when it is built with
// -fsanitize=address,undefined (tests/test_match_batch_abi.py builds and runs it that way; no GPU, no Python in the process).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sac-cot_amd/csrc/sc_match_batch_check.hpp"

static int failures = 0;

static void expect(const char* what, std::vector<uint32_t> so, std::vector<uint32_t> to, uint32_t knn, bool features, const char* want) {
  const uint32_t nb = (uint32_t)so.size() - 1;
  // heap copies of the exact size: the sanitizer sees every index past n_problems
  uint32_t* a = new uint32_t[so.size()];
  uint32_t* b = new uint32_t[to.size()];
  memcpy(a, so.data(), so.size() * 4);
  memcpy(b, to.data(), to.size() * 4);
  const char* got = sc::match_batch_offsets_error(a, b, nb, knn, features);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
  if (!got) {  // accepted: the tile map covers every row once, in order, and never crosses a problem
    const uint64_t tiles = sc::match_batch_tile_count(a, nb, 64);
    // ... inside the metadata as the device copy holds it: one array of exactly match_batch_meta_layout's words, both offset arrays
    // and the slot starts in front of the map
    const sc::BatchMetaLayout at = sc::match_batch_meta_layout(nb, (uint32_t)tiles);
    uint32_t* meta = new uint32_t[at.words];
    sc::match_batch_meta_fill(a, b, nb, knn, 64, at, meta);
    const uint32_t* map = meta + at.map_at;
    const size_t nb1 = (size_t)nb + 1;
    if (at.slot_at != 2 * nb1 || at.map_at != 3 * nb1 || at.words != at.map_at + 2 * tiles) { printf("FAIL %s: the layout\n", what); failures++; }
    for (uint32_t p = 0; p <= nb; p++)
      if (meta[p] != a[p] || meta[nb1 + p] != b[p] || meta[at.slot_at + p] != (uint32_t)((uint64_t)a[p] * knn)) {
        printf("FAIL %s: offsets / slot %u\n", what, p);
        failures++;
      }
    uint64_t t = 0;
    for (uint32_t p = 0; p < nb; p++)
      for (uint32_t r = 0; r < a[p + 1] - a[p]; r += 64, t++)
        if (t >= tiles || map[2 * t] != p || map[2 * t + 1] != r) { printf("FAIL %s: tile %llu\n", what, (unsigned long long)t); failures++; }
    if (t != tiles) { printf("FAIL %s: %llu tiles counted, %llu mapped\n", what, (unsigned long long)tiles, (unsigned long long)t); failures++; }
    delete[] meta;
  }
  delete[] a;
  delete[] b;
}

int main() {
  expect("good", {0, 1, 65, 129, 4225}, {0, 4096, 4097, 4100, 4101}, 4, false, nullptr);
  expect("one row tile either side", {0, 63, 127, 192}, {0, 1, 2, 3}, 1, true, nullptr);
  expect("n_problems == 0", {0}, {0}, 1, false, "n_problems == 0");
  expect("source offsets decrease", {0, 64, 60, 128}, {0, 10, 20, 30}, 1, false, "decrease");
  expect("target offsets decrease", {0, 10, 20, 30}, {0, 64, 60, 128}, 1, false, "decrease");
  expect("empty source side", {0, 5, 5}, {0, 5, 10}, 1, false, "no rows");
  expect("empty target side", {0, 5, 10}, {0, 5, 5}, 1, false, "no rows");
  expect("4097 source rows", {0, 4097}, {0, 5}, 1, false, "SC_MATCH_BATCH_MAX_N");
  expect("4097 target rows", {0, 5}, {0, 4097}, 1, false, "SC_MATCH_BATCH_MAX_N");
  expect("features: 257 x 2 entries", {0, 257}, {0, 300}, 2, true, "SC_BATCH_MAX_N");
  expect("features: 256 x 2 entries", {0, 256}, {0, 300}, 2, true, nullptr);
  expect("match alone: 257 x 2 entries", {0, 257}, {0, 300}, 2, false, nullptr);
  {  // total_s * knn: 2^31 entries are accepted, one problem more is not (2^19 problems of 4096 rows at knn 1; 2^17 at knn 4)
    for (uint32_t knn : {1u, 4u}) {
      const uint32_t nb = (1u << 19) / knn;
      std::vector<uint32_t> so(nb + 2), to(nb + 2);
      for (uint32_t b = 0; b < nb + 2; b++) { so[b] = b * 4096u; to[b] = b; }
      expect("2^31 entries", std::vector<uint32_t>(so.begin(), so.end() - 1), std::vector<uint32_t>(to.begin(), to.end() - 1), knn, false, nullptr);
      expect("2^31 + 4096 knn entries", so, to, knn, false, "2^31");
    }
  }
  printf(failures ? "%d FAILED\n" : "all passed\n", failures);
  return failures ? 1 : 0;
}
