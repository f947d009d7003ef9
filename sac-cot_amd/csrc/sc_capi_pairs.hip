// sc_capi_pairs.hip — the C ABI's matching and registration of listed pairs of shared keypoint sets (include/saccot.h,
// sc_match_pairs): sc_pairs_layout, sc_match_pairs_device, sc_match_pairs, sc_register_pairs_features_device,
// sc_register_pairs_features and sc_polish_pairs_slots_device.  Host-only, on the context and the helpers of sc_ctx.hpp; the kernels
// are the pairs forms of sc_match_batch.hip and sc_polish_batch.hip, and sc_batch.hip's kernel on the slots.
//
// the pairs' records, the slot starts and the tile map (sc_pairs_check.hpp) -> pinned staging (the area and event every batch entry
// shares) -> ONE device copy (enqueued) -> memset (a "clean" word per pair and, for SC_MATCH_MUTUAL, every pair's own column
// minima: all ones) -> distance + select -> finish [-> sc_batch.hip's kernel on the slots]: the packed form's four or five stream
// operations, whatever the list, and nothing is read back.  Everything that can refuse the call is decided on the host before
// anything is enqueued.  The workspace is the packed entries' (the mbatch / pbatch buffers): a pair is a problem of theirs whose rows
// are found through a record.
#include "sc_ctx.hpp"
#include "sc_pairs_check.hpp"

using namespace sc;

static_assert(PAIR_WORDS == PAIRS_REC_WORDS && PW_SRC == 0 && PW_NS == 1 && PW_TGT == 2 && PW_NT == 3 && PW_TOP == 4 && PW_SLOT == 5 &&
              PW_COL_LO == 6 && PW_COL_HI == 7, "pairs_records (sc_pairs_check.hpp) writes the words the kernels read (sc_kernels.hpp)");

namespace {

using Sizes = MatchBatchSizes;  // n_problems: the pairs; total_s / total_t: the source / target rows of all pairs

// device words of the metadata: the records, the slot starts (n_pairs + 1: sc_batch.hip's offset array), the tile map
size_t meta_words(const Sizes& sz) { return (size_t)PAIR_WORDS * sz.n_problems + sz.n_problems + 1 + 2 * (size_t)sz.n_tiles; }

// every refusal of the entries; `p` only for the features entries, whose name for the messages is `features`.  Fills *job (but its
// pointers) and *sz.
int pairs_check(sc_ctx* c, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp,
                const sc_params* p, const char* features, MatchJob* job, Sizes* sz) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(match_check(c, mp, 1, 1, job));  // the parameter rules; the sizes are the table's business
  if (features) SC_TRY(batch_params_check(c, p, features));
  if (const char* what = pairs_error(set_off, n_sets, pairs, n_pairs, job->knn, features != nullptr)) { c->last_error = what; return SC_EINVAL; }
  const PairsTotals t = pairs_totals(set_off, pairs, n_pairs, MATCH_BATCH_ROWS);
  if (t.tiles > 0x7FFFFFFFull) { c->last_error = "sc_match_pairs: more than 2^31 - 1 row tiles"; return SC_EINVAL; }
  sz->n_problems = n_pairs; sz->n_tiles = (uint32_t)t.tiles;
  sz->total_s = t.total_s; sz->total_t = t.total_t; sz->slots = sz->total_s * job->knn;
  return SC_OK;
}

// the workspace of the match itself (gather: and of the gathered points)
int pairs_room(sc_ctx* c, const MatchJob& mj, const Sizes& sz, bool gather) {
  const uint32_t kp = mj.r2 > 0.f ? 2u : mj.knn;
  ENSURE(c, c->mbatch_meta, meta_words(sz) * 4);
  ENSURE(c, c->mbatch_top, sz.total_s * kp * 8);
  ENSURE(c, c->mbatch_words, (((size_t)sz.n_problems + 1) / 2 + (mj.mutual ? sz.total_t : 0)) * 8);
  if (gather) {
    ENSURE(c, c->mbatch_gsrc, sz.slots * 12);
    ENSURE(c, c->mbatch_gtgt, sz.slots * 12);
  }
  return SC_OK;
}

const uint32_t* slot_starts(const sc_ctx* c, const Sizes& sz) { return c->mbatch_meta.as<uint32_t>() + (size_t)PAIR_WORDS * sz.n_problems; }

// the staging copy, the memset and the two launches (pairs_room has been called).  d_pts: the table's points for the gather
// (nullptr: the match alone), `total` rows in `layout`.
int pairs_enqueue(sc_ctx* c, const MatchJob& mj, const Sizes& sz, const float* d_feat, const uint32_t* set_off, const uint32_t* pairs,
                  int32_t* d_corr, float* d_d2, uint32_t* d_count, const float* d_pts, uint32_t total, int layout) {
  const size_t np = sz.n_problems, bytes = meta_words(sz) * 4;
  SC_TRY(batch_staging_begin(c, bytes));
  uint32_t* h = static_cast<uint32_t*>(c->h_batch_off);
  pairs_records(set_off, pairs, sz.n_problems, mj.knn, h);
  pairs_slots(set_off, pairs, sz.n_problems, mj.knn, h + PAIR_WORDS * np);
  pairs_tile_map(set_off, pairs, sz.n_problems, MATCH_BATCH_ROWS, h + PAIR_WORDS * np + np + 1);
  SC_TRY(batch_staging_send(c, c->mbatch_meta, bytes));
  const size_t clean_bytes = ((np + 1) / 2) * 8, words_bytes = clean_bytes + (mj.mutual ? sz.total_t * 8 : 0);
  HIPCHK(c, hipMemsetAsync(c->mbatch_words.p, 0xFF, words_bytes, c->stream));
  const uint32_t* meta = c->mbatch_meta.as<uint32_t>();
  MatchPairsJob job{};
  job.feat = d_feat;
  job.rec = meta; job.tile_map = meta + PAIR_WORDS * np + np + 1;
  job.n_problems = sz.n_problems; job.n_tiles = sz.n_tiles; job.dim = mj.dim; job.knn = mj.knn; job.kp = mj.r2 > 0.f ? 2u : mj.knn;
  job.mutual = mj.mutual; job.r2 = mj.r2;
  job.top = c->mbatch_top.as<uint64_t>();
  job.colmin = mj.mutual ? reinterpret_cast<uint64_t*>(static_cast<char*>(c->mbatch_words.p) + clean_bytes) : nullptr;
  job.clean = c->mbatch_words.as<uint32_t>();
  job.corr = d_corr; job.d2 = d_d2; job.count = d_count;
  if (d_pts) {  // both sides of a pair are rows of the one table
    const bool soa = layout == SC_SOA;
    job.g = MatchGather{d_pts, d_pts, soa ? 1u : 3u, soa ? total : 1u, soa ? 1u : 3u, soa ? total : 1u, c->mbatch_gsrc.as<float>(),
                        c->mbatch_gtgt.as<float>()};
  }
  launch_match_pairs_dist(job, c->stream);
  launch_match_pairs_finish(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// sc_batch.hip's kernel on the slots the match filled: launch_batch_register_slots, with the slot starts as its offset array
int pairs_register(sc_ctx* c, const Sizes& sz, const sc_params* p, const uint32_t* d_count, sc_batch_result* d_res, uint8_t* d_mask) {
  BatchSlotJob slots{};
  slots.count = d_count;
  BatchJob& job = slots.job;
  job.src = c->mbatch_gsrc.as<float>(); job.tgt = c->mbatch_gtgt.as<float>();  // n x 3 whatever the caller's layout
  job.offset = slot_starts(c, sz);
  job.n_problems = sz.n_problems; job.total = (uint32_t)sz.slots;
  job.soa = 0; job.T = p->max_triangles; job.rank_mode = p->rank_mode; job.score_mode = p->score_mode;
  job.dv = derive(p);
  job.res = reinterpret_cast<BatchRecord*>(d_res); job.mask = d_mask;
  launch_batch_register_slots(slots, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_pairs_layout(const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, uint32_t knn, uint32_t* slot) {
  if (!set_off || !pairs || !slot) return SC_EINVAL;
  if (pairs_error(set_off, n_sets, pairs, n_pairs, knn, false)) return SC_EINVAL;
  pairs_slots(set_off, pairs, n_pairs, knn, slot);
  return SC_OK;
}

int sc_match_pairs_device(sc_ctx* c, const float* d_feat, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs,
                          const sc_match_params* mp, int32_t* d_corr, float* d_d2, uint32_t* d_count) {
  if (!c) return SC_EINVAL;
  if (!d_feat || !set_off || !pairs || !mp || !d_corr || !d_d2 || !d_count) return refuse(c, "sc_match_pairs_device", "a NULL argument");
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(pairs_check(c, set_off, n_sets, pairs, n_pairs, mp, nullptr, nullptr, &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  SC_TRY(pairs_room(c, mj, sz, false));
  return pairs_enqueue(c, mj, sz, d_feat, set_off, pairs, d_corr, d_d2, d_count, nullptr, 0, SC_AOS);
}

int sc_match_pairs(sc_ctx* c, const float* feat, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs,
                   const sc_match_params* mp, int32_t* corr, float* d2, uint32_t* count) {
  if (!c) return SC_EINVAL;
  if (!feat || !set_off || !pairs || !mp || !corr || !d2 || !count) return refuse(c, "sc_match_pairs", "a NULL argument");
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(pairs_check(c, set_off, n_sets, pairs, n_pairs, mp, nullptr, nullptr, &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t fb = (size_t)set_off[n_sets] * mj.dim * 4, cb = (size_t)n_pairs * 8;
  SC_TRY(pairs_room(c, mj, sz, false));
  ENSURE(c, c->mbatch_fsrc, fb);  // the table: one copy serves both sides
  ENSURE(c, c->mbatch_corr, sz.slots * 8);
  ENSURE(c, c->mbatch_d2, sz.slots * 4);
  ENSURE(c, c->mbatch_count, cb);
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->mbatch_fsrc.p, feat, fb, hipMemcpyHostToDevice, st));
  SC_TRY(pairs_enqueue(c, mj, sz, c->mbatch_fsrc.as<float>(), set_off, pairs, c->mbatch_corr.as<int32_t>(), c->mbatch_d2.as<float>(),
                       c->mbatch_count.as<uint32_t>(), nullptr, 0, SC_AOS));
  HIPCHK(c, hipMemcpyAsync(corr, c->mbatch_corr.p, sz.slots * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(d2, c->mbatch_d2.p, sz.slots * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(count, c->mbatch_count.p, cb, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return SC_OK;
}

int sc_register_pairs_features_device(sc_ctx* c, const float* d_pts, const float* d_feat, const uint32_t* set_off, uint32_t n_sets,
                                      const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp, const sc_params* p,
                                      sc_batch_result* d_res, int32_t* d_corr, float* d_d2, uint32_t* d_count, uint8_t* d_mask) {
  if (!c) return SC_EINVAL;
  if (!d_pts || !d_feat || !set_off || !pairs || !mp || !p || !d_res || !d_corr || !d_d2 || !d_count || !d_mask)
    return refuse(c, "sc_register_pairs_features_device", "a NULL argument");
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(pairs_check(c, set_off, n_sets, pairs, n_pairs, mp, p, "sc_register_pairs_features", &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  SC_TRY(pairs_room(c, mj, sz, true));
  SC_TRY(pairs_enqueue(c, mj, sz, d_feat, set_off, pairs, d_corr, d_d2, d_count, d_pts, set_off[n_sets], p->layout));
  return pairs_register(c, sz, p, d_count, d_res, d_mask);
}

int sc_register_pairs_features(sc_ctx* c, const float* pts, const float* feat, const uint32_t* set_off, uint32_t n_sets,
                               const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp, const sc_params* p,
                               sc_batch_result* res, int32_t* corr, float* d2, uint32_t* count, uint8_t* mask) {
  if (!c) return SC_EINVAL;
  if (!pts || !feat || !set_off || !pairs || !mp || !p || !res || !corr || !d2 || !count || !mask)
    return refuse(c, "sc_register_pairs_features", "a NULL argument");
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(pairs_check(c, set_off, n_sets, pairs, n_pairs, mp, p, "sc_register_pairs_features", &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  const size_t total = set_off[n_sets], fb = total * mj.dim * 4, cb = (size_t)n_pairs * 8;
  const size_t recs = (size_t)n_pairs * sizeof(sc_batch_result);
  SC_TRY(pairs_room(c, mj, sz, true));
  ENSURE(c, c->mbatch_fsrc, fb);  // the table, descriptors and points: one copy of each serves both sides
  ENSURE(c, c->mbatch_psrc, total * 12);
  ENSURE(c, c->mbatch_corr, sz.slots * 8);
  ENSURE(c, c->mbatch_d2, sz.slots * 4);
  ENSURE(c, c->mbatch_count, cb);
  ENSURE(c, c->mbatch_res, recs);
  ENSURE(c, c->mbatch_mask, sz.slots);
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->mbatch_fsrc.p, feat, fb, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->mbatch_psrc.p, pts, total * 12, hipMemcpyHostToDevice, st));
  uint32_t* d_count = c->mbatch_count.as<uint32_t>();
  SC_TRY(pairs_enqueue(c, mj, sz, c->mbatch_fsrc.as<float>(), set_off, pairs, c->mbatch_corr.as<int32_t>(), c->mbatch_d2.as<float>(), d_count,
                       c->mbatch_psrc.as<float>(), (uint32_t)total, p->layout));
  SC_TRY(pairs_register(c, sz, p, d_count, c->mbatch_res.as<sc_batch_result>(), c->mbatch_mask.as<uint8_t>()));
  HIPCHK(c, hipMemcpyAsync(res, c->mbatch_res.p, recs, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(corr, c->mbatch_corr.p, sz.slots * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(d2, c->mbatch_d2.p, sz.slots * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(count, c->mbatch_count.p, cb, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(mask, c->mbatch_mask.p, sz.slots, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return SC_OK;
}

int sc_polish_pairs_slots_device(sc_ctx* c, const float* d_pts, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs,
                                 uint32_t n_pairs, uint32_t knn, const sc_params* p, const sc_polish_params* pp, const int32_t* d_corr,
                                 const uint32_t* d_count, const sc_batch_result* d_res, sc_polish_batch_result* d_pol, uint8_t* d_mask) {
  static const char* const who = "sc_polish_pairs_slots_device";
  if (!c) return SC_EINVAL;
  if (!d_pts || !set_off || !pairs || !p || !pp || !d_corr || !d_count || !d_res || !d_pol || !d_mask) return refuse(c, who, "a NULL argument");
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(batch_params_check(c, p, who));
  SC_TRY(pbatch_pparams_check(c, pp, who));
  if (const char* what = pairs_error(set_off, n_sets, pairs, n_pairs, knn, true)) return refuse(c, who, what);
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  // the pairs' records, one copy
  const size_t bytes = (size_t)PAIR_WORDS * n_pairs * 4;
  ENSURE(c, c->pbatch_off, bytes);
  SC_TRY(batch_staging_begin(c, bytes));
  pairs_records(set_off, pairs, n_pairs, knn, static_cast<uint32_t*>(c->h_batch_off));
  SC_TRY(batch_staging_send(c, c->pbatch_off, bytes));
  PolishBatchPairsJob arg{};
  arg.job = pbatch_job(p, pp);
  PolishBatchJob& job = arg.job;
  job.src = d_pts; job.tgt = d_pts; job.offset = nullptr;  // both sides are rows of the one table; the records say which
  job.n_problems = n_pairs; job.total = set_off[n_sets];
  job.in = reinterpret_cast<const BatchRecord*>(d_res); job.out = reinterpret_cast<PolishBatchRecord*>(d_pol); job.mask = d_mask;
  arg.rec = c->pbatch_off.as<uint32_t>();
  arg.corr = d_corr; arg.count = d_count; arg.knn = knn;
  launch_polish_batch_pairs(arg, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // extern "C"
