// sc_capi_match_batch.hip — the C ABI's batched descriptor matching (include/saccot.h, sc_match_batch): sc_match_batch_device,
// sc_match_batch, sc_register_batch_features_device and sc_register_batch_features.  Host-only, on the context and the helpers of
// sc_ctx.hpp; the kernels are sc_match_batch.hip's and sc_batch.hip's.
//
// both offset arrays and the slot starts (batch_slot_meta, shared with sc_polish_batch_slots_device), then the tile map -> pinned
// staging -> ONE device copy (enqueued) -> memset (a "clean" word per problem and, for SC_MATCH_MUTUAL, the column minima: all
// ones) -> distance + select -> finish [-> sc_batch.hip's kernel on the slots]: four or five stream operations whatever the batch,
// and nothing is read back — a problem's count, its non-finite flag and its status are words in device memory.  Everything that can
// refuse the call is decided on the host before anything is enqueued.
#include "sc_ctx.hpp"
#include "sc_match_batch_check.hpp"

using namespace sc;

static_assert(MATCH_BATCH_MAX_N == SC_MATCH_BATCH_MAX_N, "sc_kernels.hpp and saccot.h agree");

using Sizes = MatchBatchSizes;

// The match sequence — what is refused, the workspace, the enqueue, the gather's description — is namespace sc's: the entries here
// and sc_register_instances_batch_features_device (sc_capi_instances_batch.hip) share it (declared in sc_ctx.hpp).
namespace sc {

// every refusal of the entries; `p` only for the features entries, whose name for the messages is `features`.  Fills *job (but its
// pointers) and *sz.
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
  return SC_OK;
}

// the workspace of the match itself
int mbatch_room(sc_ctx* c, const MatchJob& mj, const Sizes& sz, bool gather) {
  const uint32_t kp = mj.r2 > 0.f ? 2u : mj.knn;
  ENSURE(c, c->mbatch_meta, (3 * ((size_t)sz.n_problems + 1) + 2 * (size_t)sz.n_tiles) * 4);
  ENSURE(c, c->mbatch_top, sz.total_s * kp * 8);
  ENSURE(c, c->mbatch_words, (((size_t)sz.n_problems + 1) / 2 + (mj.mutual ? sz.total_t : 0)) * 8);
  if (gather) {
    ENSURE(c, c->mbatch_gsrc, sz.slots * 12);
    ENSURE(c, c->mbatch_gtgt, sz.slots * 12);
  }
  return SC_OK;
}

// the staging copy, the memset and the two launches (mbatch_room has been called)
int mbatch_enqueue(sc_ctx* c, const MatchJob& mj, const Sizes& sz, const float* d_fsrc, const float* d_ftgt, const uint32_t* src_off,
                   const uint32_t* tgt_off, int32_t* d_corr, float* d_d2, uint32_t* d_count, const MatchGather& g) {
  const size_t nb1 = (size_t)sz.n_problems + 1, meta_bytes = (3 * nb1 + 2 * (size_t)sz.n_tiles) * 4;
  SC_TRY(batch_staging_begin(c, meta_bytes));
  uint32_t* h = static_cast<uint32_t*>(c->h_batch_off);
  batch_slot_meta(src_off, tgt_off, sz.n_problems, mj.knn, h);
  match_batch_tile_map(src_off, sz.n_problems, MATCH_BATCH_ROWS, h + 3 * nb1);
  SC_TRY(batch_staging_send(c, c->mbatch_meta, meta_bytes));
  const size_t clean_bytes = (nb1 / 2) * 8, words_bytes = clean_bytes + (mj.mutual ? sz.total_t * 8 : 0);
  HIPCHK(c, hipMemsetAsync(c->mbatch_words.p, 0xFF, words_bytes, c->stream));
  const uint32_t* meta = c->mbatch_meta.as<uint32_t>();
  MatchBatchJob job{};
  job.fsrc = d_fsrc; job.ftgt = d_ftgt;
  job.src_off = meta; job.tgt_off = meta + nb1; job.slot = meta + 2 * nb1; job.tile_map = meta + 3 * nb1;
  job.n_problems = sz.n_problems; job.n_tiles = sz.n_tiles; job.dim = mj.dim; job.knn = mj.knn; job.kp = mj.r2 > 0.f ? 2u : mj.knn;
  job.mutual = mj.mutual; job.r2 = mj.r2;
  job.top = c->mbatch_top.as<uint64_t>();
  job.colmin = mj.mutual ? reinterpret_cast<uint64_t*>(static_cast<char*>(c->mbatch_words.p) + clean_bytes) : nullptr;
  job.clean = c->mbatch_words.as<uint32_t>();
  job.corr = d_corr; job.d2 = d_d2; job.count = d_count; job.g = g;
  launch_match_batch_dist(job, c->stream);
  launch_match_batch_finish(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

MatchGather gather_of(const sc_ctx* c, const sc_params* p, const Sizes& sz, const float* d_src_pts, const float* d_tgt_pts) {
  const bool soa = p->layout == SC_SOA;
  return MatchGather{d_src_pts, d_tgt_pts, soa ? 1u : 3u, soa ? (uint32_t)sz.total_s : 1u, soa ? 1u : 3u, soa ? (uint32_t)sz.total_t : 1u,
                     c->mbatch_gsrc.as<float>(), c->mbatch_gtgt.as<float>()};
}

// sc_batch.hip's kernel argument on the slots the match filled: the gathered points, the slot starts (the count pairs are the caller's)
BatchJob mbatch_slots_job(const sc_ctx* c, const Sizes& sz, const sc_params* p) {
  BatchJob job{};
  job.src = c->mbatch_gsrc.as<float>(); job.tgt = c->mbatch_gtgt.as<float>();  // n x 3 whatever the caller's layout
  job.offset = c->mbatch_meta.as<uint32_t>() + 2 * ((size_t)sz.n_problems + 1);
  job.n_problems = sz.n_problems; job.total = (uint32_t)sz.slots;
  job.soa = 0; job.T = p->max_triangles; job.rank_mode = p->rank_mode; job.score_mode = p->score_mode;
  job.dv = derive(p);
  return job;
}

}  // namespace sc

namespace {

// sc_batch.hip's kernel on the slots the match filled
int mbatch_register(sc_ctx* c, const Sizes& sz, const sc_params* p, const uint32_t* d_count, sc_batch_result* d_res, uint8_t* d_mask) {
  BatchSlotJob slots{};
  slots.count = d_count;
  slots.job = mbatch_slots_job(c, sz, p);
  slots.job.res = reinterpret_cast<BatchRecord*>(d_res); slots.job.mask = d_mask;
  launch_batch_register_slots(slots, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
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
  return mbatch_enqueue(c, mj, sz, d_fsrc, d_ftgt, src_off, tgt_off, d_corr, d_d2, d_count, MatchGather{});
}

int sc_match_batch(sc_ctx* c, const float* fsrc, const uint32_t* src_off, const float* ftgt, const uint32_t* tgt_off, uint32_t n_problems,
                   const sc_match_params* mp, int32_t* corr, float* d2, uint32_t* count) {
  if (!c) return SC_EINVAL;
  if (!fsrc || !src_off || !ftgt || !tgt_off || !mp || !corr || !d2 || !count) return refuse(c, "sc_match_batch", "a NULL argument");
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(mbatch_check(c, src_off, tgt_off, n_problems, mp, nullptr, nullptr, &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t sb = sz.total_s * mj.dim * 4, tb = sz.total_t * mj.dim * 4, cb = (size_t)n_problems * 8;
  SC_TRY(mbatch_room(c, mj, sz, false));
  ENSURE(c, c->mbatch_fsrc, sb);
  ENSURE(c, c->mbatch_ftgt, tb);
  ENSURE(c, c->mbatch_corr, sz.slots * 8);
  ENSURE(c, c->mbatch_d2, sz.slots * 4);
  ENSURE(c, c->mbatch_count, cb);
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->mbatch_fsrc.p, fsrc, sb, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->mbatch_ftgt.p, ftgt, tb, hipMemcpyHostToDevice, st));
  SC_TRY(mbatch_enqueue(c, mj, sz, c->mbatch_fsrc.as<float>(), c->mbatch_ftgt.as<float>(), src_off, tgt_off, c->mbatch_corr.as<int32_t>(),
                        c->mbatch_d2.as<float>(), c->mbatch_count.as<uint32_t>(), MatchGather{}));
  HIPCHK(c, hipMemcpyAsync(corr, c->mbatch_corr.p, sz.slots * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(d2, c->mbatch_d2.p, sz.slots * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(count, c->mbatch_count.p, cb, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return SC_OK;
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
  SC_TRY(mbatch_enqueue(c, mj, sz, d_fsrc, d_ftgt, src_off, tgt_off, d_corr, d_d2, d_count, gather_of(c, p, sz, d_src_pts, d_tgt_pts)));
  return mbatch_register(c, sz, p, d_count, d_res, d_mask);
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
  const size_t sb = sz.total_s * mj.dim * 4, tb = sz.total_t * mj.dim * 4, cb = (size_t)n_problems * 8;
  const size_t recs = (size_t)n_problems * sizeof(sc_batch_result);
  SC_TRY(mbatch_room(c, mj, sz, true));
  ENSURE(c, c->mbatch_fsrc, sb);
  ENSURE(c, c->mbatch_ftgt, tb);
  ENSURE(c, c->mbatch_psrc, sz.total_s * 12);
  ENSURE(c, c->mbatch_ptgt, sz.total_t * 12);
  ENSURE(c, c->mbatch_corr, sz.slots * 8);
  ENSURE(c, c->mbatch_d2, sz.slots * 4);
  ENSURE(c, c->mbatch_count, cb);
  ENSURE(c, c->mbatch_res, recs);
  ENSURE(c, c->mbatch_mask, sz.slots);
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->mbatch_fsrc.p, fsrc, sb, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->mbatch_ftgt.p, ftgt, tb, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->mbatch_psrc.p, src_pts, sz.total_s * 12, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->mbatch_ptgt.p, tgt_pts, sz.total_t * 12, hipMemcpyHostToDevice, st));
  uint32_t* d_count = c->mbatch_count.as<uint32_t>();
  SC_TRY(mbatch_enqueue(c, mj, sz, c->mbatch_fsrc.as<float>(), c->mbatch_ftgt.as<float>(), src_off, tgt_off, c->mbatch_corr.as<int32_t>(),
                        c->mbatch_d2.as<float>(), d_count, gather_of(c, p, sz, c->mbatch_psrc.as<float>(), c->mbatch_ptgt.as<float>())));
  SC_TRY(mbatch_register(c, sz, p, d_count, c->mbatch_res.as<sc_batch_result>(), c->mbatch_mask.as<uint8_t>()));
  HIPCHK(c, hipMemcpyAsync(res, c->mbatch_res.p, recs, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(corr, c->mbatch_corr.p, sz.slots * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(d2, c->mbatch_d2.p, sz.slots * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(count, c->mbatch_count.p, cb, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(mask, c->mbatch_mask.p, sz.slots, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return SC_OK;
}

}  // extern "C"
