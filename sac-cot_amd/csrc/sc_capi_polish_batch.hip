// sc_capi_polish_batch.hip — the C ABI's iterated refits for a batch's winners (include/saccot.h, sc_polish_batch):
// sc_polish_batch_device, sc_polish_batch and sc_polish_batch_slots_device.  Host-only, on the context and the helpers of sc_ctx.hpp;
// the kernel is sc_polish_batch.hip's.
//
// offsets -> pinned staging (the area and event every batch entry shares: batch_offsets_to_device; the slot form's three arrays:
// batch_slot_meta, as sc_capi_match_batch.hip writes them) -> device copy (enqueued) -> ONE launch, a workgroup per problem.
// Nothing is read back: a problem's status is a field of its record.  Everything that can refuse the call is decided on the host
// before anything is enqueued.
#include "sc_ctx.hpp"

using namespace sc;

// What sc_polish_pairs_slots_device (sc_capi_pairs.hip) shares with the entries here (declared in sc_ctx.hpp, next to batch_job_of).
namespace sc {

// sc_polish_params as a batch takes them: one candidate per problem
int pbatch_pparams_check(sc_ctx* c, const sc_polish_params* pp, const char* who) {
  if (pp->size != sizeof(sc_polish_params)) return refuse(c, who, "pp->size is not sizeof(sc_polish_params)");
  if (pp->candidates != 1) return refuse(c, who, "candidates must be 1 (a batch member keeps only its winner)");
  if (pp->max_iter < 1 || pp->max_iter > 64) return refuse(c, who, "max_iter must be 1 .. 64");
  if (pp->flags || pp->reserved[0] || pp->reserved[1] || pp->reserved[2] || pp->reserved[3]) return refuse(c, who, "flags and reserved fields must be 0");
  return SC_OK;
}

// what the kernel reads of the two parameter blocks (the pointers are the caller's)
PolishBatchJob pbatch_job(const sc_params* p, const sc_polish_params* pp) {
  const Derived dv = derive(p);
  PolishBatchJob job{};
  job.soa = p->layout == SC_SOA; job.score_mode = p->score_mode; job.max_iter = pp->max_iter;
  job.tau2 = dv.tau2;
  job.thr = score_thr(dv, p->score_mode);
  return job;
}

}  // namespace sc

namespace {

int pbatch_check(sc_ctx* c, const uint32_t* offset, uint32_t n_problems, const sc_params* p, const sc_polish_params* pp) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(batch_params_check(c, p, "sc_polish_batch"));
  SC_TRY(pbatch_pparams_check(c, pp, "sc_polish_batch"));
  if (const char* what = batch_offsets_error(offset, n_problems)) return refuse(c, "sc_polish_batch", what);
  return SC_OK;
}

int pbatch_enqueue(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                   const sc_polish_params* pp, const sc_batch_result* d_res, sc_polish_batch_result* d_pol, uint8_t* d_mask) {
  SC_TRY(batch_offsets_to_device(c, offset, n_problems, c->pbatch_off));
  PolishBatchJob job = pbatch_job(p, pp);
  job.src = d_src; job.tgt = d_tgt; job.offset = c->pbatch_off.as<uint32_t>();
  job.n_problems = n_problems; job.total = offset[n_problems];
  job.in = reinterpret_cast<const BatchRecord*>(d_res); job.out = reinterpret_cast<PolishBatchRecord*>(d_pol); job.mask = d_mask;
  launch_polish_batch(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_polish_batch_device(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                           const sc_params* p, const sc_polish_params* pp, const sc_batch_result* d_res, sc_polish_batch_result* d_pol,
                           uint8_t* d_mask) {
  if (!c) return SC_EINVAL;
  if (!d_src || !d_tgt || !offset || !p || !pp || !d_res || !d_pol || !d_mask) return refuse(c, "sc_polish_batch_device", "a NULL argument");
  SC_TRY(pbatch_check(c, offset, n_problems, p, pp));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  return pbatch_enqueue(c, d_src, d_tgt, offset, n_problems, p, pp, d_res, d_pol, d_mask);
}

int sc_polish_batch(sc_ctx* c, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                    const sc_polish_params* pp, const sc_batch_result* res, sc_polish_batch_result* pol, uint8_t* mask) {
  if (!c) return SC_EINVAL;
  if (!src || !tgt || !offset || !p || !pp || !res || !pol || !mask) return refuse(c, "sc_polish_batch", "a NULL argument");
  SC_TRY(pbatch_check(c, offset, n_problems, p, pp));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  const size_t total = offset[n_problems], pts = total * 12;
  HostArrays h(c);
  const int a_src = h.in(src, pts), a_tgt = h.in(tgt, pts);
  const int a_res = h.in(res, (size_t)n_problems * sizeof(sc_batch_result));
  const int a_pol = h.out(pol, (size_t)n_problems * sizeof(sc_polish_batch_result)), a_mask = h.out(mask, total);
  h.also(c->pbatch_off, batch_offsets_bytes(n_problems));
  return h.run([&] {
    return pbatch_enqueue(c, h.at<float>(a_src), h.at<float>(a_tgt), offset, n_problems, p, pp, h.at<sc_batch_result>(a_res),
                          h.at<sc_polish_batch_result>(a_pol), h.at<uint8_t>(a_mask));
  });
}

int sc_polish_batch_slots_device(sc_ctx* c, const float* d_src_pts, const uint32_t* src_off, const float* d_tgt_pts, const uint32_t* tgt_off,
                                 uint32_t n_problems, uint32_t knn, const sc_params* p, const sc_polish_params* pp, const int32_t* d_corr,
                                 const uint32_t* d_count, const sc_batch_result* d_res, sc_polish_batch_result* d_pol, uint8_t* d_mask) {
  static const char* const who = "sc_polish_batch_slots_device";
  if (!c) return SC_EINVAL;
  if (!d_src_pts || !src_off || !d_tgt_pts || !tgt_off || !p || !pp || !d_corr || !d_count || !d_res || !d_pol || !d_mask)
    return refuse(c, who, "a NULL argument");
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(batch_params_check(c, p, who));
  SC_TRY(pbatch_pparams_check(c, pp, who));
  if (knn < 1 || knn > 4) return refuse(c, who, "knn must be 1 .. 4");
  if (const char* what = match_batch_offsets_error(src_off, tgt_off, n_problems, knn, true)) return refuse(c, who, what);
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  // both offset arrays and the slot starts, one copy
  const size_t nb1 = (size_t)n_problems + 1, bytes = 3 * nb1 * 4;
  ENSURE(c, c->pbatch_off, bytes);
  SC_TRY(batch_staging_begin(c, bytes));
  batch_slot_meta(src_off, tgt_off, n_problems, knn, static_cast<uint32_t*>(c->h_batch_off));
  SC_TRY(batch_staging_send(c, c->pbatch_off, bytes));
  const uint32_t* meta = c->pbatch_off.as<uint32_t>();
  PolishBatchSlotJob slots{};
  slots.job = pbatch_job(p, pp);
  PolishBatchJob& job = slots.job;
  job.src = d_src_pts; job.tgt = d_tgt_pts; job.offset = meta;
  job.n_problems = n_problems; job.total = src_off[n_problems];
  job.in = reinterpret_cast<const BatchRecord*>(d_res); job.out = reinterpret_cast<PolishBatchRecord*>(d_pol); job.mask = d_mask;
  slots.tgt_off = meta + nb1; slots.slot = meta + 2 * nb1;
  slots.corr = d_corr; slots.count = d_count;
  slots.knn = knn; slots.total_t = tgt_off[n_problems];
  launch_polish_batch_slots(slots, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // extern "C"
