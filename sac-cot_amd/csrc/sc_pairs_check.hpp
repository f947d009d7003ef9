// sc_pairs_check.hpp — what sc_match_pairs* decides about the caller's table of sets and list of pairs on the host, before anything
// is enqueued, and what it derives from them for the device: the slot starts, a record per pair, the tile map.  Plain C++ on host
// memory, no HIP: sc_capi_pairs.hip includes it, and so does the stand-alone program tests/native/pairs_check_main.cpp, which runs
// it under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/saccot.h"
#include "sc_match_batch_check.hpp"

namespace sc {

// the words of a pair's record as the kernels read them (sc_kernels.hpp, PairWord: the same order, asserted in sc_capi_pairs.hip)
constexpr int PAIRS_REC_WORDS = 8;

// set_off holds n_sets + 1 words, pairs 2 * n_pairs.  Nothing of set_off decreasing; every index below n_sets; a REFERENCED set
// holds 1 .. SC_MATCH_BATCH_MAX_N rows (an unreferenced one may hold any number); knn 1 .. 4; at most 2^31 output entries
// (the sum of ns_p * knn); `features`: a slot (ns_p * knn entries) must fit one workgroup of sc_register_batch.
// nullptr: they are fine.
inline const char* pairs_error(const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, uint32_t knn,
                               bool features) {
  if (n_sets == 0) return "sc_match_pairs: n_sets == 0";
  if (n_pairs == 0) return "sc_match_pairs: n_pairs == 0";
  if (knn < 1 || knn > 4) return "sc_match_pairs: knn must be 1 .. 4";
  for (uint32_t s = 0; s < n_sets; s++)
    if (set_off[s + 1] < set_off[s]) return "sc_match_pairs: set_off decreases";
  uint64_t entries = 0;
  for (uint32_t p = 0; p < n_pairs; p++) {
    const uint32_t a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    if (a >= n_sets || b >= n_sets) return "sc_match_pairs: a pair names a set index >= n_sets";
    const uint32_t ns = set_off[a + 1] - set_off[a], nt = set_off[b + 1] - set_off[b];
    if (ns < 1 || nt < 1 || ns > SC_MATCH_BATCH_MAX_N || nt > SC_MATCH_BATCH_MAX_N)
      return "sc_match_pairs: a referenced set has no rows or more than SC_MATCH_BATCH_MAX_N";
    if (features && (uint64_t)ns * knn > SC_BATCH_MAX_N) return "sc_register_pairs_features: a pair's ns * knn exceeds SC_BATCH_MAX_N";
    entries += (uint64_t)ns * knn;
    if (entries > (1ull << 31)) return "sc_match_pairs: more than 2^31 output entries (the sum of ns * knn)";
  }
  return nullptr;
}

// What a list that pairs_error accepts adds up to: source rows, target rows and row tiles of all pairs (tiles of `rows` source
// rows, none across two pairs).
struct PairsTotals { uint64_t total_s, total_t, tiles; };
inline PairsTotals pairs_totals(const uint32_t* set_off, const uint32_t* pairs, uint32_t n_pairs, uint32_t rows) {
  PairsTotals t{0, 0, 0};
  for (uint32_t p = 0; p < n_pairs; p++) {
    const uint32_t a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    const uint64_t ns = set_off[a + 1] - set_off[a];
    t.total_s += ns;
    t.total_t += set_off[b + 1] - set_off[b];
    t.tiles += (ns + rows - 1) / rows;
  }
  return t;
}

// slot: n_pairs + 1 words, slot[p] = knn x the source rows of the pairs before p (at most 2^31: checked above)
inline void pairs_slots(const uint32_t* set_off, const uint32_t* pairs, uint32_t n_pairs, uint32_t knn, uint32_t* slot) {
  uint64_t at = 0;
  for (uint32_t p = 0; p < n_pairs; p++) {
    slot[p] = (uint32_t)at;
    const uint32_t a = pairs[2 * (size_t)p];
    at += (uint64_t)(set_off[a + 1] - set_off[a]) * knn;
  }
  slot[n_pairs] = (uint32_t)at;
}

// rec: PAIRS_REC_WORDS words per pair — first row and rows of the source set, of the target set, then the bases that are the
// pair's own: its first row of lists (the source rows of the pairs before it), its slot, its first column minimum (the target
// rows of the pairs before it, 64 bits: low word, high word).  Two pairs never share a base, whatever sets they share.
inline void pairs_records(const uint32_t* set_off, const uint32_t* pairs, uint32_t n_pairs, uint32_t knn, uint32_t* rec) {
  uint64_t rows_s = 0, rows_t = 0;
  for (uint32_t p = 0; p < n_pairs; p++) {
    const uint32_t a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    const uint32_t ns = set_off[a + 1] - set_off[a], nt = set_off[b + 1] - set_off[b];
    uint32_t* r = rec + (size_t)PAIRS_REC_WORDS * p;
    r[0] = set_off[a]; r[1] = ns; r[2] = set_off[b]; r[3] = nt;
    r[4] = (uint32_t)rows_s; r[5] = (uint32_t)(rows_s * knn);
    r[6] = (uint32_t)rows_t; r[7] = (uint32_t)(rows_t >> 32);
    rows_s += ns; rows_t += nt;
  }
}

// map: pairs_totals().tiles pairs (pair, first row of the tile inside its source set)
inline void pairs_tile_map(const uint32_t* set_off, const uint32_t* pairs, uint32_t n_pairs, uint32_t rows, uint32_t* map) {
  size_t t = 0;
  for (uint32_t p = 0; p < n_pairs; p++) {
    const uint32_t a = pairs[2 * (size_t)p], ns = set_off[a + 1] - set_off[a];
    for (uint32_t r = 0; r < ns; r += rows) { map[2 * t] = p; map[2 * t + 1] = r; t++; }
  }
}

// the pairs form's metadata (BatchMetaLayout, sc_match_batch_check.hpp): the records | slot starts | tile map
inline BatchMetaLayout pairs_meta_layout(uint32_t n_pairs, uint32_t n_tiles) {
  const size_t recs = (size_t)PAIRS_REC_WORDS * n_pairs;
  return BatchMetaLayout{recs + n_pairs + 1 + 2 * (size_t)n_tiles, recs, recs + n_pairs + 1};
}
inline void pairs_meta_fill(const uint32_t* set_off, const uint32_t* pairs, uint32_t n_pairs, uint32_t knn, uint32_t rows,
                            const BatchMetaLayout& at, uint32_t* meta) {
  pairs_records(set_off, pairs, n_pairs, knn, meta);
  pairs_slots(set_off, pairs, n_pairs, knn, meta + at.slot_at);
  pairs_tile_map(set_off, pairs, n_pairs, rows, meta + at.map_at);
}

}  // namespace sc
