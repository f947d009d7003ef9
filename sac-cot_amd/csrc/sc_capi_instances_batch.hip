// sc_capi_instances_batch.hip — the C ABI's several motions per batch problem (include/saccot.h, sc_register_instances_batch):
// sc_register_instances_batch_device, sc_register_instances_batch and sc_register_instances_batch_features_device.  Host-only, on the
// context and the helpers of sc_ctx.hpp; the kernel is sc_batch.hip's, instantiated with rounds.
//
// offsets -> pinned staging (the area and event every batch entry shares: batch_offsets_to_device) -> device copy (enqueued) -> ONE
// launch, a workgroup per problem, the rounds inside it.  The features entry runs sc_capi_match_batch.hip's match sequence
// (mbatch_check / _room / _enqueue_packed) in front of the launch; the host entry is a HostArrays (sc_ctx.hpp).  Nothing is read back: a problem's status is a field of its records, its
// number of motions a word in device memory.  Everything that can refuse the call is decided on the host before anything is enqueued.
#include "sc_ctx.hpp"

using namespace sc;

static_assert(INSTANCES_BATCH_MAX == SC_INSTANCES_BATCH_MAX, "sc_kernels.hpp and saccot.h agree");

namespace {

int ibatch_instances_check(sc_ctx* c, uint32_t max_instances, const char* who) {
  if (max_instances < 1 || max_instances > SC_INSTANCES_BATCH_MAX) return refuse(c, who, "max_instances must be 1 .. SC_INSTANCES_BATCH_MAX");
  return SC_OK;
}

int ibatch_check(sc_ctx* c, const uint32_t* offset, uint32_t n_problems, const sc_params* p, uint32_t max_instances) {
  static const char* const who = "sc_register_instances_batch";
  SC_TRY(ibatch_instances_check(c, max_instances, who));  // (first: it touches nothing of the context but the message)
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(batch_params_check(c, p, who));
  if (const char* what = batch_offsets_error(offset, n_problems)) return refuse(c, who, what);
  return SC_OK;
}

BatchRounds rounds_of(uint32_t max_instances, uint32_t min_score, int32_t* d_label, uint32_t* d_nfound) {
  return BatchRounds{max_instances, min_score, d_label, d_nfound};
}

int ibatch_enqueue(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                   uint32_t max_instances, uint32_t min_score, sc_batch_result* d_res, int32_t* d_label, uint32_t* d_nfound) {
  SC_TRY(batch_offsets_to_device(c, offset, n_problems, c->ibatch_off));
  InstBatchJob inst{};
  inst.job = batch_job_of(p);
  BatchJob& job = inst.job;
  job.src = d_src; job.tgt = d_tgt; job.offset = c->ibatch_off.as<uint32_t>();
  job.n_problems = n_problems; job.total = offset[n_problems];
  job.res = reinterpret_cast<BatchRecord*>(d_res); job.mask = nullptr;
  inst.rounds = rounds_of(max_instances, min_score, d_label, d_nfound);
  launch_instances_batch(inst, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_register_instances_batch_device(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                                       const sc_params* p, uint32_t max_instances, uint32_t min_score, sc_batch_result* d_res,
                                       int32_t* d_label, uint32_t* d_nfound) {
  if (!c) return SC_EINVAL;
  if (!d_src || !d_tgt || !offset || !p || !d_res || !d_label || !d_nfound)
    return refuse(c, "sc_register_instances_batch_device", "a NULL argument");
  SC_TRY(ibatch_check(c, offset, n_problems, p, max_instances));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  return ibatch_enqueue(c, d_src, d_tgt, offset, n_problems, p, max_instances, min_score, d_res, d_label, d_nfound);
}

int sc_register_instances_batch(sc_ctx* c, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems,
                                const sc_params* p, uint32_t max_instances, uint32_t min_score, sc_batch_result* res, int32_t* label,
                                uint32_t* nfound) {
  if (!c) return SC_EINVAL;
  if (!src || !tgt || !offset || !p || !res || !label || !nfound) return refuse(c, "sc_register_instances_batch", "a NULL argument");
  SC_TRY(ibatch_check(c, offset, n_problems, p, max_instances));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  const size_t total = offset[n_problems], pts = total * 12;
  HostArrays h(c);
  const int a_src = h.in(src, pts), a_tgt = h.in(tgt, pts);
  const int a_res = h.out(res, (size_t)max_instances * n_problems * sizeof(sc_batch_result));
  const int a_label = h.out(label, total * 4), a_nfound = h.out(nfound, (size_t)n_problems * 4);
  h.also(c->ibatch_off, batch_offsets_bytes(n_problems));
  return h.run([&] {
    return ibatch_enqueue(c, h.at<float>(a_src), h.at<float>(a_tgt), offset, n_problems, p, max_instances, min_score,
                          h.at<sc_batch_result>(a_res), h.at<int32_t>(a_label), h.at<uint32_t>(a_nfound));
  });
}

int sc_register_instances_batch_features_device(sc_ctx* c, const float* d_src_pts, const float* d_fsrc, const uint32_t* src_off,
                                                const float* d_tgt_pts, const float* d_ftgt, const uint32_t* tgt_off, uint32_t n_problems,
                                                const sc_match_params* mp, const sc_params* p, uint32_t max_instances, uint32_t min_score,
                                                sc_batch_result* d_res, int32_t* d_corr, float* d_d2, uint32_t* d_count, int32_t* d_label,
                                                uint32_t* d_nfound) {
  static const char* const who = "sc_register_instances_batch_features_device";
  if (!c) return SC_EINVAL;
  if (!d_src_pts || !d_fsrc || !src_off || !d_tgt_pts || !d_ftgt || !tgt_off || !mp || !p || !d_res || !d_corr || !d_d2 || !d_count ||
      !d_label || !d_nfound)
    return refuse(c, who, "a NULL argument");
  MatchJob mj{};
  MatchBatchSizes sz{};
  SC_TRY(ibatch_instances_check(c, max_instances, who));
  SC_TRY(mbatch_check(c, src_off, tgt_off, n_problems, mp, p, who, &mj, &sz));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  SC_TRY(mbatch_room(c, mj, sz, true));
  SC_TRY(mbatch_enqueue_packed(c, mj, sz, d_fsrc, d_ftgt, src_off, tgt_off, d_corr, d_d2, d_count, p, d_src_pts, d_tgt_pts));
  InstBatchSlotJob slots{};
  slots.job = mbatch_slots_job(c, sz, p);
  slots.job.res = reinterpret_cast<BatchRecord*>(d_res); slots.job.mask = nullptr;
  slots.rounds = rounds_of(max_instances, min_score, d_label, d_nfound);
  slots.count = d_count;
  launch_instances_batch_slots(slots, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // extern "C"
