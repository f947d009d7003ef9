// sc_capi_pairs.hip — the C ABI's matching and registration of listed pairs of shared keypoint sets (include/saccot.h,
// sc_match_pairs): sc_pairs_layout, sc_match_pairs_device, sc_match_pairs, sc_register_pairs_features_device,
// sc_register_pairs_features and sc_polish_pairs_slots_device.  Host-only, on the context and the helpers of sc_ctx.hpp; the kernels
// are the pairs forms of sc_match_batch.hip and sc_polish_batch.hip, and sc_batch.hip's kernel on the slots.
//
// the pairs' records, the slot starts and the tile map (sc_pairs_check.hpp) -> pinned staging (the area and event every batch entry
// shares) -> ONE device copy (enqueued) -> memset (a "clean" word per pair and, for SC_MATCH_MUTUAL, every pair's own column
// minima: all ones) -> distance + select -> finish [-> sc_batch.hip's kernel on the slots]: the packed form's four or five stream
// operations, whatever the list, and nothing is read back.  Everything that can refuse the call is decided on the host before
// anything is enqueued.  The workspace is the packed entries' (the mbatch / pbatch buffers), and so is the sequence (mbatch_room,
// mbatch_enqueue, mbatch_register: sc_ctx.hpp, sc_capi_match_batch.hip): a pair is a problem of theirs whose rows are found through a
// record.  What is the pairs' own is here: the checks, the staging-area fill and the job's head (pairs_match), the entry points.
#include "sc_ctx.hpp"
#include "sc_pairs_check.hpp"

using namespace sc;

static_assert(PAIR_WORDS == PAIRS_REC_WORDS && PW_SRC == 0 && PW_NS == 1 && PW_TGT == 2 && PW_NT == 3 && PW_TOP == 4 && PW_SLOT == 5 &&
              PW_COL_LO == 6 && PW_COL_HI == 7, "pairs_records (sc_pairs_check.hpp) writes the words the kernels read (sc_kernels.hpp)");

using Sizes = MatchBatchSizes;  // n_problems: the pairs; total_s / total_t: the source / target rows of all pairs

// every refusal of the entries (declared in sc_ctx.hpp: sc_capi_match_guided_batch.hip's pairs entries share it)
int sc::pairs_check(sc_ctx* c, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp,
                const sc_params* p, const char* features, MatchJob* job, Sizes* sz) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(match_check(c, mp, 1, 1, job));  // the parameter rules; the sizes are the table's business
  if (features) SC_TRY(batch_params_check(c, p, features));
  if (const char* what = pairs_error(set_off, n_sets, pairs, n_pairs, job->knn, features != nullptr)) { c->last_error = what; return SC_EINVAL; }
  const PairsTotals t = pairs_totals(set_off, pairs, n_pairs, MATCH_BATCH_ROWS);
  if (t.tiles > 0x7FFFFFFFull) { c->last_error = "sc_match_pairs: more than 2^31 - 1 row tiles"; return SC_EINVAL; }
  sz->n_problems = n_pairs; sz->n_tiles = (uint32_t)t.tiles;
  sz->total_s = t.total_s; sz->total_t = t.total_t; sz->slots = sz->total_s * job->knn;
  sz->meta = pairs_meta_layout(n_pairs, sz->n_tiles);
  return SC_OK;
}

namespace {

// the match on the list (mbatch_room has been called): the records, the slot starts and the tile map into the staging area,
// MatchPairsJob and its launches.  p, d_pts: a features entry's sc_params and the table's points (`total` rows), for the gather
// (p == nullptr: the match alone).
int pairs_match(sc_ctx* c, const MatchJob& mj, const Sizes& sz, const float* d_feat, const uint32_t* set_off, const uint32_t* pairs,
                int32_t* d_corr, float* d_d2, uint32_t* d_count, const sc_params* p = nullptr, const float* d_pts = nullptr, uint32_t total = 0) {
  MatchPairsJob job{};
  job.feat = d_feat;
  job.rec = c->mbatch_meta.as<uint32_t>();
  // both sides of a pair are rows of the one table
  const MatchGather g = p ? gather_of(d_pts, total, d_pts, total, p->layout, c->mbatch_gsrc.as<float>(), c->mbatch_gtgt.as<float>()) : MatchGather{};
  return mbatch_enqueue(
      c, mj, sz, job, [&](uint32_t* h) { pairs_meta_fill(set_off, pairs, sz.n_problems, mj.knn, MATCH_BATCH_ROWS, sz.meta, h); },
      d_corr, d_d2, d_count, g);
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
  SC_TRY(mbatch_room(c, mj, sz, false));
  return pairs_match(c, mj, sz, d_feat, set_off, pairs, d_corr, d_d2, d_count);
}

int sc_match_pairs(sc_ctx* c, const float* feat, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs,
                   const sc_match_params* mp, int32_t* corr, float* d2, uint32_t* count) {
  if (!c) return SC_EINVAL;
  if (!feat || !set_off || !pairs || !mp || !corr || !d2 || !count) return refuse(c, "sc_match_pairs", "a NULL argument");
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(pairs_check(c, set_off, n_sets, pairs, n_pairs, mp, nullptr, nullptr, &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  SC_TRY(mbatch_room(c, mj, sz, false));
  HostArrays h(c);
  // the table: one copy serves both sides
  const MatchBatchArrays a = mbatch_arrays(h, sz, mj.dim, feat, set_off[n_sets], nullptr, 0, nullptr, nullptr, corr, d2, count);
  return h.run([&] {
    return pairs_match(c, mj, sz, h.at<float>(a.fsrc), set_off, pairs, h.at<int32_t>(a.corr), h.at<float>(a.d2), h.at<uint32_t>(a.count));
  });
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
  SC_TRY(mbatch_room(c, mj, sz, true));
  SC_TRY(pairs_match(c, mj, sz, d_feat, set_off, pairs, d_corr, d_d2, d_count, p, d_pts, set_off[n_sets]));
  return mbatch_register(c, sz, p, d_count, d_res, d_mask);
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
  const size_t total = set_off[n_sets];
  SC_TRY(mbatch_room(c, mj, sz, true));
  HostArrays h(c);
  // the table, descriptors and points: one copy of each serves both sides
  const MatchBatchArrays a = mbatch_arrays(h, sz, mj.dim, feat, total, nullptr, 0, pts, nullptr, corr, d2, count);
  const int a_res = h.out(res, (size_t)n_pairs * sizeof(sc_batch_result), true);  // the records are fetched first
  const int a_mask = h.out(mask, sz.slots);
  return h.run([&] {
    uint32_t* d_count = h.at<uint32_t>(a.count);
    SC_TRY(pairs_match(c, mj, sz, h.at<float>(a.fsrc), set_off, pairs, h.at<int32_t>(a.corr), h.at<float>(a.d2), d_count, p, h.at<float>(a.psrc),
                       (uint32_t)total));
    return mbatch_register(c, sz, p, d_count, h.at<sc_batch_result>(a_res), h.at<uint8_t>(a_mask));
  });
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
