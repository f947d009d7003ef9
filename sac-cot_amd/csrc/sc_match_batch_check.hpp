// sc_match_batch_check.hpp — what sc_match_batch* decides about the caller's offset arrays on the host, before anything is enqueued,
// and the metadata it derives from them for the device.  Plain C++ on host memory, no HIP: the host files include it (through
// sc_ctx.hpp), and so does the stand-alone program tests/native/match_batch_check_main.cpp, which runs it under the address and
// undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/saccot.h"

namespace sc {

// Both offset arrays hold n_problems + 1 words.  Sizes 1 .. SC_MATCH_BATCH_MAX_N on both sides, nothing decreasing, at most 2^31
// output entries (total_s * knn); `features`: a slot (ns_b * knn entries) must fit one workgroup of sc_register_batch.
// nullptr: they are fine.
inline const char* match_batch_offsets_error(const uint32_t* src_off, const uint32_t* tgt_off, uint32_t n_problems, uint32_t knn,
                                             bool features) {
  if (n_problems == 0) return "sc_match_batch: n_problems == 0";
  for (uint32_t b = 0; b < n_problems; b++) {
    if (src_off[b + 1] < src_off[b] || tgt_off[b + 1] < tgt_off[b]) return "sc_match_batch: offsets decrease";
    const uint32_t ns = src_off[b + 1] - src_off[b], nt = tgt_off[b + 1] - tgt_off[b];
    if (ns < 1 || nt < 1 || ns > SC_MATCH_BATCH_MAX_N || nt > SC_MATCH_BATCH_MAX_N)
      return "sc_match_batch: a problem has no rows or more than SC_MATCH_BATCH_MAX_N on one side";
    if (features && (uint64_t)ns * knn > SC_BATCH_MAX_N)
      return "sc_register_batch_features: a problem's ns * knn exceeds SC_BATCH_MAX_N";
  }
  if ((uint64_t)src_off[n_problems] * knn > (1ull << 31)) return "sc_match_batch: more than 2^31 output entries (total_s * knn)";
  return nullptr;
}

// The slot metadata of n_problems problems, 3 (n_problems + 1) words into meta: src_off | tgt_off | the slot starts src_off * knn
// (at most 2^31: checked above).
inline void batch_slot_meta(const uint32_t* src_off, const uint32_t* tgt_off, uint32_t n_problems, uint32_t knn, uint32_t* meta) {
  const size_t nb1 = (size_t)n_problems + 1;
  memcpy(meta, src_off, nb1 * 4);
  memcpy(meta + nb1, tgt_off, nb1 * 4);
  for (size_t b = 0; b < nb1; b++) meta[2 * nb1 + b] = (uint32_t)((uint64_t)src_off[b] * knn);
}

// tiles of `rows` source rows, none across two problems (offsets as checked above: every problem has a row)
inline uint64_t match_batch_tile_count(const uint32_t* src_off, uint32_t n_problems, uint32_t rows) {
  uint64_t tiles = 0;
  for (uint32_t b = 0; b < n_problems; b++) tiles += ((uint64_t)(src_off[b + 1] - src_off[b]) + rows - 1) / rows;
  return tiles;
}
// map: match_batch_tile_count pairs (problem, first row of the tile inside the problem)
inline void match_batch_tile_map(const uint32_t* src_off, uint32_t n_problems, uint32_t rows, uint32_t* map) {
  size_t t = 0;
  for (uint32_t b = 0; b < n_problems; b++)
    for (uint32_t r = 0; r < src_off[b + 1] - src_off[b]; r += rows) { map[2 * t] = b; map[2 * t + 1] = r; t++; }
}

// The metadata of a batched match as one device copy holds it: `words` 32-bit words, the slot starts (n_problems + 1 words,
// sc_batch.hip's offset array) from word slot_at, the tile map (two words a tile) from word map_at.
struct BatchMetaLayout { size_t words, slot_at, map_at; };
// the packed form's: src_off | tgt_off | slot starts (batch_slot_meta) | tile map
inline BatchMetaLayout match_batch_meta_layout(uint32_t n_problems, uint32_t n_tiles) {
  const size_t nb1 = (size_t)n_problems + 1;
  return BatchMetaLayout{3 * nb1 + 2 * (size_t)n_tiles, 2 * nb1, 3 * nb1};
}
inline void match_batch_meta_fill(const uint32_t* src_off, const uint32_t* tgt_off, uint32_t n_problems, uint32_t knn, uint32_t rows,
                                  const BatchMetaLayout& at, uint32_t* meta) {
  batch_slot_meta(src_off, tgt_off, n_problems, knn, meta);
  match_batch_tile_map(src_off, n_problems, rows, meta + at.map_at);
}

}  // namespace sc
