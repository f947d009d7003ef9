// sc_capi_graph.hpp — the host steps the entries on a pair list share (sc_pairs_cycles, sc_pairs_sync, sc_pairs_solve), said once:
// the order of their refusals and the staging of the list.  The host knows the graph: it builds the adjacency once per call from
// the list alone (sc_cycles_check.hpp: pairs_image) and reads nothing from the device.  The image -> pinned staging (the area and
// event every batch entry shares) -> ONE device copy (enqueued); behind it the entry's own memset and launches, and no wait in the
// device form.  Each entry brings what is its own: its rules (the check headers), its room, its job, its launch.  A host form's
// sequence is HostArrays::run (sc_ctx.hpp).  Everything that can refuse a call is decided before anything is enqueued.
#pragma once
#include <new>
#include <vector>

#include "sc_ctx.hpp"
#include "sc_cycles_check.hpp"

namespace sc {

// What the check leaves of an accepted list.  off: n_sets + 1 words — scratch of the list check, and then the adjacency's offsets.
struct PairGraph {
  const uint32_t* pairs;
  uint32_t n_sets, n_pairs;
  uint64_t n_entries;
  std::vector<uint32_t> off;
};
// The refusals, in this order: the frame ends, a call outstanding, the entry's parameter block and then its strides (`broken`: what
// its *_params_error returned, or else its *_stride_error), the counts, SC_ENOMEM for the scratch, the list, the anchor (nullptr: the
// entry has none); then the context's device.  `who` opens the message.
inline int pair_graph_check(sc_ctx* c, const char* who, const char* broken, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs,
                            const uint32_t* anchor, PairGraph* g) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  if (broken) return refuse(c, who, broken);
  if (const char* what = cycles_counts_error(n_sets, n_pairs)) return refuse(c, who, what);
  try {
    g->off.assign((size_t)n_sets + 1, 0u);
  } catch (const std::bad_alloc&) {
    c->last_error = std::string(who) + ": no host memory for n_sets + 1 words";
    return SC_ENOMEM;
  }
  if (const char* what = cycles_list_error(n_sets, pairs, n_pairs, g->off.data())) return refuse(c, who, what);
  if (anchor)
    if (const char* what = pairs_anchor_error(*anchor, n_sets)) return refuse(c, who, what);
  HIPCHK(c, hipSetDevice(c->device));
  g->pairs = pairs; g->n_sets = n_sets; g->n_pairs = n_pairs;
  g->n_entries = cycles_entry_count(pairs, n_pairs);
  return SC_OK;
}
inline size_t pair_graph_meta_bytes(const PairGraph& g, bool starts) {  // of the image, in the entry's *_meta buffer
  return (size_t)(starts ? sync_meta_bytes(g.n_sets, g.n_pairs, g.n_entries) : cycles_meta_bytes(g.n_pairs, g.n_entries));
}

// The staged image on the device (starts: nullptr where the entry stages none).
struct PairGraphStaged { const uint32_t* rec; const uint64_t* entries; const uint32_t* starts; };
// `meta` has its room: the image into the staging area and its copy into `meta` (enqueued).
inline int pair_graph_stage(sc_ctx* c, PairGraph& g, Buf& meta, bool starts, PairGraphStaged* d) {
  const size_t bytes = pair_graph_meta_bytes(g, starts);
  SC_TRY(batch_staging_begin(c, bytes));
  pairs_image(g.n_sets, g.pairs, g.n_pairs, g.n_entries, g.off.data(), starts, c->h_batch_off);
  SC_TRY(batch_staging_send(c, meta, bytes));
  const PairsImageAt at = pairs_image_at(g.n_pairs, g.n_entries);
  const char* const m = static_cast<const char*>(meta.p);
  d->rec = reinterpret_cast<const uint32_t*>(m + at.rec);
  d->entries = reinterpret_cast<const uint64_t*>(m + at.entries);
  d->starts = starts ? reinterpret_cast<const uint32_t*>(m + at.starts) : nullptr;
  return SC_OK;
}

}  // namespace sc
