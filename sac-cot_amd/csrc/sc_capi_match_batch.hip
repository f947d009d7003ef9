// sc_capi_match_batch.hip — the C ABI's batched descriptor matching (include/saccot.h, sc_match_batch): sc_match_batch_device,
// sc_match_batch, sc_register_batch_features_device and sc_register_batch_features.  Host-only, on the context and the helpers of
// sc_ctx.hpp; the kernels are sc_match_batch.hip's and sc_batch.hip's.
//
// both offset arrays and the slot starts (batch_slot_meta, shared with sc_polish_batch_slots_device), then the tile map -> pinned
// staging -> ONE device copy (enqueued) -> memset (a "clean" word per problem and, for SC_MATCH_MUTUAL, the column minima: all
// ones) -> distance + select -> finish [-> sc_batch.hip's kernel on the slots]: four or five stream operations whatever the batch,
// and nothing is read back — a problem's count, its non-finite flag and its status are words in device memory.  Everything that can
// refuse the call is decided on the host before anything is enqueued.  The sequence is said once, for this packed form and for the
// pairs form (sc_capi_pairs.hip): mbatch_room, mbatch_enqueue (a template over the form's job type, sc_ctx.hpp), mbatch_slots_job
// and mbatch_register take what differs — the metadata's layout and fill, the job's own fields — from the caller; the launch pair
// follows from the job's type (launch_match_batch_dist / _finish, sc_kernels.hpp).
#include "sc_ctx.hpp"

using namespace sc;

static_assert(MATCH_BATCH_MAX_N == SC_MATCH_BATCH_MAX_N, "sc_kernels.hpp and saccot.h agree");

using Sizes = MatchBatchSizes;

// The match sequence — what is refused, the workspace, the enqueue, the registration on the slots — is namespace sc's: the entries
// here, sc_register_instances_batch_features_device (sc_capi_instances_batch.hip) and the pairs entries (sc_capi_pairs.hip) share it
// (declared in sc_ctx.hpp).
namespace sc {

int mbatch_check(sc_ctx* c, const uint32_t* src_off, const uint32_t* tgt_off, uint32_t n_problems, const sc_match_params* mp,
                 const sc_params* p, const char* features, MatchJob* job, Sizes* sz) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(match_check(c, mp, 1, 1, job));  // the parameter rules; the sizes are the offsets' business
  if (features) SC_TRY(batch_params_check(c, p, features));
  if (const char* what = match_batch_offsets_error(src_off, tgt_off, n_problems, job->knn, features != nullptr)) { c->last_error = what; return SC_EINVAL; }
  const uint64_t tiles = match_batch_tile_count(src_off, n_problems, MATCH_BATCH_ROWS);
  if (tiles > 0x7FFFFFFFull) { c->last_error = "sc_match_batch: more than 2^31 - 1 row tiles"; return SC_EINVAL; }
  sz->n_problems = n_problems; sz->n_tiles = (uint32_t)tiles;
  sz->total_s = src_off[n_problems]; sz->total_t = tgt_off[n_problems]; sz->slots = sz->total_s * job->knn;
  sz->meta = match_batch_meta_layout(n_problems, sz->n_tiles);
  return SC_OK;
}

int mbatch_room(sc_ctx* c, const MatchJob& mj, const Sizes& sz, bool gather) {
  const uint32_t kp = mj.r2 > 0.f ? 2u : mj.knn;
  ENSURE(c, c->mbatch_meta, sz.meta.words * 4);
  ENSURE(c, c->mbatch_top, sz.total_s * kp * 8);
  ENSURE(c, c->mbatch_words, mbatch_clean_bytes(sz) + (mj.mutual ? sz.total_t * 8 : 0));
  if (gather) {
    ENSURE(c, c->mbatch_gsrc, sz.slots * 12);
    ENSURE(c, c->mbatch_gtgt, sz.slots * 12);
  }
  return SC_OK;
}

int mbatch_enqueue_packed(sc_ctx* c, const MatchJob& mj, const Sizes& sz, const float* d_fsrc, const float* d_ftgt, const uint32_t* src_off,
                          const uint32_t* tgt_off, int32_t* d_corr, float* d_d2, uint32_t* d_count, const sc_params* p, const float* d_src_pts,
                          const float* d_tgt_pts) {
  const uint32_t* meta = c->mbatch_meta.as<uint32_t>();
  const size_t nb1 = (size_t)sz.n_problems + 1;
  MatchBatchJob job{};
  job.fsrc = d_fsrc; job.ftgt = d_ftgt;
  job.src_off = meta; job.tgt_off = meta + nb1; job.slot = meta + sz.meta.slot_at;
  const MatchGather g = p ? gather_of(d_src_pts, (uint32_t)sz.total_s, d_tgt_pts, (uint32_t)sz.total_t, p->layout, c->mbatch_gsrc.as<float>(),
                                      c->mbatch_gtgt.as<float>())
                          : MatchGather{};
  return mbatch_enqueue(
      c, mj, sz, job, [&](uint32_t* h) { match_batch_meta_fill(src_off, tgt_off, sz.n_problems, mj.knn, MATCH_BATCH_ROWS, sz.meta, h); },
      d_corr, d_d2, d_count, g);
}

BatchJob mbatch_slots_job(const sc_ctx* c, const Sizes& sz, const sc_params* p) {
  BatchJob job = batch_job_of(p);
  job.src = c->mbatch_gsrc.as<float>(); job.tgt = c->mbatch_gtgt.as<float>(); job.soa = 0;  // n x 3 whatever the caller's layout
  job.offset = c->mbatch_meta.as<uint32_t>() + sz.meta.slot_at;
  job.n_problems = sz.n_problems; job.total = (uint32_t)sz.slots;
  return job;
}

int mbatch_register(sc_ctx* c, const Sizes& sz, const sc_params* p, const uint32_t* d_count, sc_batch_result* d_res, uint8_t* d_mask) {
  BatchSlotJob slots{};
  slots.count = d_count;
  slots.job = mbatch_slots_job(c, sz, p);
  slots.job.res = reinterpret_cast<BatchRecord*>(d_res); slots.job.mask = d_mask;
  launch_batch_register_slots(slots, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace sc

namespace {

// match, gather, registration on the slots: what both features entries enqueue (mbatch_room has been called)
int features_enqueue(sc_ctx* c, const MatchJob& mj, const Sizes& sz, const float* d_src_pts, const float* d_fsrc, const uint32_t* src_off,
                     const float* d_tgt_pts, const float* d_ftgt, const uint32_t* tgt_off, const sc_params* p, sc_batch_result* d_res,
                     int32_t* d_corr, float* d_d2, uint32_t* d_count, uint8_t* d_mask) {
  SC_TRY(mbatch_enqueue_packed(c, mj, sz, d_fsrc, d_ftgt, src_off, tgt_off, d_corr, d_d2, d_count, p, d_src_pts, d_tgt_pts));
  return mbatch_register(c, sz, p, d_count, d_res, d_mask);
}

}  // namespace

extern "C" {

int sc_match_batch_device(sc_ctx* c, const float* d_fsrc, const uint32_t* src_off, const float* d_ftgt, const uint32_t* tgt_off,
                          uint32_t n_problems, const sc_match_params* mp, int32_t* d_corr, float* d_d2, uint32_t* d_count) {
  if (!c) return SC_EINVAL;
  if (!d_fsrc || !src_off || !d_ftgt || !tgt_off || !mp || !d_corr || !d_d2 || !d_count) return refuse(c, "sc_match_batch_device", "a NULL argument");
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(mbatch_check(c, src_off, tgt_off, n_problems, mp, nullptr, nullptr, &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  SC_TRY(mbatch_room(c, mj, sz, false));
  return mbatch_enqueue_packed(c, mj, sz, d_fsrc, d_ftgt, src_off, tgt_off, d_corr, d_d2, d_count);
}

int sc_match_batch(sc_ctx* c, const float* fsrc, const uint32_t* src_off, const float* ftgt, const uint32_t* tgt_off, uint32_t n_problems,
                   const sc_match_params* mp, int32_t* corr, float* d2, uint32_t* count) {
  if (!c) return SC_EINVAL;
  if (!fsrc || !src_off || !ftgt || !tgt_off || !mp || !corr || !d2 || !count) return refuse(c, "sc_match_batch", "a NULL argument");
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(mbatch_check(c, src_off, tgt_off, n_problems, mp, nullptr, nullptr, &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  SC_TRY(mbatch_room(c, mj, sz, false));
  HostArrays h(c);
  const MatchBatchArrays a = mbatch_arrays(h, sz, mj.dim, fsrc, sz.total_s, ftgt, sz.total_t, nullptr, nullptr, corr, d2, count);
  return h.run([&] {
    return mbatch_enqueue_packed(c, mj, sz, h.at<float>(a.fsrc), h.at<float>(a.ftgt), src_off, tgt_off, h.at<int32_t>(a.corr), h.at<float>(a.d2),
                                 h.at<uint32_t>(a.count));
  });
}

int sc_register_batch_features_device(sc_ctx* c, const float* d_src_pts, const float* d_fsrc, const uint32_t* src_off,
                                      const float* d_tgt_pts, const float* d_ftgt, const uint32_t* tgt_off, uint32_t n_problems,
                                      const sc_match_params* mp, const sc_params* p, sc_batch_result* d_res, int32_t* d_corr, float* d_d2,
                                      uint32_t* d_count, uint8_t* d_mask) {
  if (!c) return SC_EINVAL;
  if (!d_src_pts || !d_fsrc || !src_off || !d_tgt_pts || !d_ftgt || !tgt_off || !mp || !p || !d_res || !d_corr || !d_d2 || !d_count || !d_mask)
    return refuse(c, "sc_register_batch_features_device", "a NULL argument");
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(mbatch_check(c, src_off, tgt_off, n_problems, mp, p, "sc_register_batch_features", &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  SC_TRY(mbatch_room(c, mj, sz, true));
  return features_enqueue(c, mj, sz, d_src_pts, d_fsrc, src_off, d_tgt_pts, d_ftgt, tgt_off, p, d_res, d_corr, d_d2, d_count, d_mask);
}

int sc_register_batch_features(sc_ctx* c, const float* src_pts, const float* fsrc, const uint32_t* src_off, const float* tgt_pts,
                               const float* ftgt, const uint32_t* tgt_off, uint32_t n_problems, const sc_match_params* mp,
                               const sc_params* p, sc_batch_result* res, int32_t* corr, float* d2, uint32_t* count, uint8_t* mask) {
  if (!c) return SC_EINVAL;
  if (!src_pts || !fsrc || !src_off || !tgt_pts || !ftgt || !tgt_off || !mp || !p || !res || !corr || !d2 || !count || !mask)
    return refuse(c, "sc_register_batch_features", "a NULL argument");
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(mbatch_check(c, src_off, tgt_off, n_problems, mp, p, "sc_register_batch_features", &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  SC_TRY(mbatch_room(c, mj, sz, true));
  HostArrays h(c);
  const MatchBatchArrays a = mbatch_arrays(h, sz, mj.dim, fsrc, sz.total_s, ftgt, sz.total_t, src_pts, tgt_pts, corr, d2, count);
  const int a_res = h.out(res, (size_t)n_problems * sizeof(sc_batch_result), true);  // the records are fetched first
  const int a_mask = h.out(mask, sz.slots);
  return h.run([&] {
    return features_enqueue(c, mj, sz, h.at<float>(a.psrc), h.at<float>(a.fsrc), src_off, h.at<float>(a.ptgt), h.at<float>(a.ftgt), tgt_off, p,
                            h.at<sc_batch_result>(a_res), h.at<int32_t>(a.corr), h.at<float>(a.d2), h.at<uint32_t>(a.count), h.at<uint8_t>(a_mask));
  });
}

}  // extern "C"
