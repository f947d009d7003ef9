// sc_cycles_check.hpp — the host-only rules of sc_pairs_cycles (include/saccot.h), and what every entry on a pair list shares with
// it (sc_pairs_sync, sc_pairs_solve), said once: the rules of the two tolerances, of use_stride and of the anchor with their
// thresholds; what is refused of sc_cycle_params, of the stride and of the list; the ADJACENCY a call builds from the list alone —
// every set's neighbour entries, sorted by (neighbour set, pair index), as offsets plus entries — with the record a pair's wave
// finds its two lists through; and the IMAGE a call stages for the device (pairs_image).  The pose records are every pose entry's
// (sc_pose_check.hpp).  No HIP: sc_capi_graph.hpp includes it, and so do tests/native/cycles_check_main.cpp and
// sync_check_main.cpp, programs of their own that run these functions under the sanitizers on the CPU.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>

#include "sc_pose_check.hpp"

namespace sc {

constexpr float CYCLES_ROT_TOL_MAX = 3.14159274f;  // the float nearest pi
constexpr uint32_t CYCLES_ROUNDS_MAX = 64;

// ---- what the pair-list entries ask alike of their parameters — the rule that is broken; nullptr: it is kept — and the thresholds
// they derive alike.  r2_max is on the squared Frobenius distance of two rotations, 2 theta^2 to first order — not on a trace:
// 1 + 2 cos(rot_tol) is exactly 3.0 below 2e-8.
inline const char* pairs_tol_error(float rot_tol, float trans_tol) {
  if (!(rot_tol >= 0.f && rot_tol <= CYCLES_ROT_TOL_MAX)) return "rot_tol must be finite and in [0, pi]";
  if (!(trans_tol >= 0.f && trans_tol < INFINITY)) return "trans_tol must be finite and >= 0";
  return nullptr;
}
inline const char* pairs_use_stride_error(bool has_use, uint32_t use_stride) {
  return has_use && (use_stride < 4 || use_stride % 4 != 0) ? "use_stride must be a multiple of 4 and at least 4" : nullptr;
}
inline const char* pairs_anchor_error(uint32_t anchor, uint32_t n_sets) { return anchor >= n_sets ? "anchor must be less than n_sets" : nullptr; }
inline double pairs_r2_max(float rot_tol) { return 2.0 * (double)rot_tol * (double)rot_tol; }
inline double pairs_e2_max(float trans_tol) { return (double)trans_tol * (double)trans_tol; }

inline bool cycles_reads_status(const sc_cycle_params* cp) { return (cp->flags & SC_CYCLES_STATUS) != 0; }

// What a call refuses of its parameter block and of the stride — the rule that is broken, for the caller to put its name in front
// of; nullptr: they are fine.
inline const char* cycles_params_error(const sc_cycle_params* cp) {
  if (cp->size != sizeof(sc_cycle_params)) return "params->size is not sizeof(sc_cycle_params)";
  if (cp->max_rounds < 1 || cp->max_rounds > CYCLES_ROUNDS_MAX) return "max_rounds must be 1 .. 64";
  if (const char* what = pairs_tol_error(cp->rot_tol, cp->trans_tol)) return what;
  if ((cp->flags & ~SC_CYCLES_STATUS) || cp->reserved[0] || cp->reserved[1]) return "an unknown flag, or a reserved field that is not 0";
  return nullptr;
}
inline const char* cycles_stride_error(const sc_cycle_params* cp, uint32_t pose_stride) {
  if (!pose_stride_ok(pose_stride, cycles_reads_status(cp))) return "pose_stride must be a multiple of 4 and at least 48 (52 with SC_CYCLES_STATUS)";
  return nullptr;
}

// The two thresholds a call uses (of parameters that cycles_params_error accepts): tr_min, e2_max.
inline void cycles_thresholds(const sc_cycle_params* cp, double out[2]) {
  out[0] = 1.0 + 2.0 * cos((double)cp->rot_tol);
  out[1] = pairs_e2_max(cp->trans_tol);
}

// What a call refuses of the list.  deg: scratch of n_sets words, left holding every set's degree — the listed pairs that name it, a
// self pair once.  nullptr: the list is fine.
inline const char* cycles_counts_error(uint32_t n_sets, uint32_t n_pairs) {  // (what needs no look at the list, nor any scratch)
  if (n_sets == 0) return "n_sets == 0";
  if (n_pairs == 0) return "n_pairs == 0";
  if (n_pairs > SC_CYCLES_MAX_PAIRS) return "n_pairs exceeds SC_CYCLES_MAX_PAIRS";
  return nullptr;
}
inline const char* cycles_list_error(uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, uint32_t* deg) {
  if (const char* what = cycles_counts_error(n_sets, n_pairs)) return what;
  for (uint32_t s = 0; s < n_sets; s++) deg[s] = 0;
  for (uint32_t p = 0; p < n_pairs; p++) {
    const uint32_t a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    if (a >= n_sets || b >= n_sets) return "a pair names a set index >= n_sets";
    deg[a]++;
    if (b != a) deg[b]++;
  }
  for (uint32_t s = 0; s < n_sets; s++)
    if (deg[s] > SC_CYCLES_MAX_DEGREE) return "a set is named by more than SC_CYCLES_MAX_DEGREE listed pairs";
  return nullptr;
}

// ---- the adjacency.  Set s owns entries [off[s], off[s + 1]).  An entry is one u64: the neighbour set in the high half; below it
// the pair's index shifted up by one, and bit 0 raised when the pair is stored as (s, neighbour) — so the order of the u64 is the
// order by (neighbour, pair).  A self pair has no entry; every other listed pair has two, one in either set's list: whether its
// pose turns out valid is the device's to find.
// (constexpr: the kernels read an entry with the same three functions)
constexpr uint64_t cycles_entry(uint32_t neighbour, uint32_t pair, bool forward) { return (uint64_t)neighbour << 32 | (uint64_t)pair << 1 | (forward ? 1u : 0u); }
constexpr uint32_t cycles_entry_set(uint64_t e) { return (uint32_t)(e >> 32); }
constexpr uint32_t cycles_entry_pair(uint64_t e) { return ((uint32_t)e) >> 1; }
constexpr bool cycles_entry_forward(uint64_t e) { return (e & 1) != 0; }
// A pair's record, CYCLES_REC_WORDS words: its lower set, its higher set, 1 if it is stored (lower, higher), a zero; then the entry
// range of the lower set's list and of the higher set's, [begin, end) each.  A self pair: lo == hi, both ranges empty.
constexpr int CYCLES_REC_WORDS = 8;
enum CyclesWord { CW_LO = 0, CW_HI = 1, CW_FWD = 2, CW_LO_BEGIN = 4, CW_LO_END = 5, CW_HI_BEGIN = 6, CW_HI_END = 7 };

// entries of a list: two per pair that is no self pair
inline uint64_t cycles_entry_count(const uint32_t* pairs, uint32_t n_pairs) {
  uint64_t n = 0;
  for (uint32_t p = 0; p < n_pairs; p++) n += pairs[2 * (size_t)p] != pairs[2 * (size_t)p + 1] ? 2 : 0;
  return n;
}

// The build, on a list that cycles_list_error accepts.  off: n_sets + 1 words; entries: cycles_entry_count of them; rec:
// CYCLES_REC_WORDS x n_pairs words — all three written whole.  A counting sort by set, then every list sorted.
inline void cycles_adjacency(uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, uint32_t* off, uint64_t* entries, uint32_t* rec) {
  for (uint32_t s = 0; s <= n_sets; s++) off[s] = 0;
  for (uint32_t p = 0; p < n_pairs; p++) {
    const uint32_t a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    if (a != b) { off[a + 1]++; off[b + 1]++; }
  }
  for (uint32_t s = 0; s < n_sets; s++) off[s + 1] += off[s];
  for (uint32_t p = 0; p < n_pairs; p++) {  // off[s] runs from its list's start to its end ...
    const uint32_t a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    if (a == b) continue;
    entries[off[a]++] = cycles_entry(b, p, true);
    entries[off[b]++] = cycles_entry(a, p, false);
  }
  for (uint32_t s = n_sets; s > 0; s--) off[s] = off[s - 1];  // ... and is put back
  off[0] = 0;
  for (uint32_t s = 0; s < n_sets; s++) std::sort(entries + off[s], entries + off[s + 1]);
  for (uint32_t p = 0; p < n_pairs; p++) {
    const uint32_t a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    const bool self = a == b;
    uint32_t* r = rec + (size_t)CYCLES_REC_WORDS * p;
    r[CW_LO] = lo; r[CW_HI] = hi; r[CW_FWD] = a < b ? 1u : 0u; r[3] = 0;
    r[CW_LO_BEGIN] = self ? 0 : off[lo]; r[CW_LO_END] = self ? 0 : off[lo + 1];
    r[CW_HI_BEGIN] = self ? 0 : off[hi]; r[CW_HI_END] = self ? 0 : off[hi + 1];
  }
}

// ---- the image: what a call stages for the device.  The pairs' records, then the entries, then — for an entry whose waves own a
// set, not a pair — the n_sets + 1 list starts (the records and the entries are multiples of 8 bytes: each part is aligned).
struct PairsImageAt { uint64_t rec, entries, starts; };  // where a reader finds the three parts, in bytes
inline PairsImageAt pairs_image_at(uint32_t n_pairs, uint64_t n_entries) {
  return PairsImageAt{0, (uint64_t)CYCLES_REC_WORDS * 4 * n_pairs, (uint64_t)CYCLES_REC_WORDS * 4 * n_pairs + 8 * n_entries};
}
inline uint64_t cycles_meta_bytes(uint32_t n_pairs, uint64_t n_entries) { return pairs_image_at(n_pairs, n_entries).starts; }  // without the starts
inline uint64_t sync_off_at(uint32_t n_pairs, uint64_t n_entries) { return pairs_image_at(n_pairs, n_entries).starts; }
inline uint64_t sync_meta_bytes(uint32_t n_sets, uint32_t n_pairs, uint64_t n_entries) { return sync_off_at(n_pairs, n_entries) + 4 * ((uint64_t)n_sets + 1); }
// The image of a list that cycles_list_error accepts, written whole into `image`: sync_meta_bytes of them with the starts,
// cycles_meta_bytes without.  off: n_sets + 1 words of scratch, left holding the list starts; n_entries: cycles_entry_count's.
inline void pairs_image(uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, uint64_t n_entries, uint32_t* off, bool starts, void* image) {
  const PairsImageAt at = pairs_image_at(n_pairs, n_entries);
  char* const h = static_cast<char*>(image);
  cycles_adjacency(n_sets, pairs, n_pairs, off, reinterpret_cast<uint64_t*>(h + at.entries), reinterpret_cast<uint32_t*>(h + at.rec));
  if (starts) memcpy(h + at.starts, off, ((size_t)n_sets + 1) * 4);
}

// ---- the device workspace behind the staged words: the oriented fp64 poses, two records of 12 doubles a pair (lower -> higher
// set, then higher -> lower); and the state: the round words (CyclesCtl, sc_kernels.hpp) with the two buffers of alive bytes,
// n_pairs each, behind them.
constexpr uint32_t CYCLES_POSE_BYTES = 192;
constexpr uint32_t CYCLES_CTL_BYTES = 512;
inline uint64_t cycles_pose_bytes(uint32_t n_pairs) { return (uint64_t)n_pairs * CYCLES_POSE_BYTES; }
inline uint64_t cycles_state_bytes(uint32_t n_pairs) { return CYCLES_CTL_BYTES + 2 * (uint64_t)n_pairs; }

}  // namespace sc
