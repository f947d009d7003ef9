// sc_capi_info_batch.hip — the C ABI's fp64 information matrix of a batch's poses (include/saccot.h, sc_pose_info_batch):
// sc_pose_info_batch_device, sc_pose_info_batch, sc_pose_info_batch_slots_device and sc_pose_info_pairs_slots_device.  Host-only, on
// the context and the helpers of sc_ctx.hpp; the kernel is sc_info_batch.hip's.
//
// offsets -> pinned staging (the area and event every batch entry shares: batch_offsets_to_device; the slot form's three arrays:
// batch_slot_meta; the pairs form's records: pairs_records) -> device copy (enqueued) -> ONE launch, a workgroup per problem.
// Nothing is read back: a problem's status is a field of its record.  Everything that can refuse the call is decided on the host
// before anything is enqueued.
#include "sc_capi_pose.hpp"
#include "sc_pairs_check.hpp"

using namespace sc;

namespace {

// the rule of the stride: the status of a record is always read (sc_pose_check.hpp)
const char* pinfo_stride_error(uint32_t pose_stride) {
  return pose_stride_ok(pose_stride, true) ? nullptr : "pose_stride must be a multiple of 4 and at least 52";
}

// the refusals the slot and the pairs form share: the context, sc_params, the stride of the pose records
int pinfo_common_check(sc_ctx* c, const sc_params* p, uint32_t pose_stride, const char* who) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(batch_params_check(c, p, who));
  if (const char* what = pinfo_stride_error(pose_stride)) return refuse(c, who, what);
  return SC_OK;
}

// what the kernel reads of sc_params and of the caller's records (the other pointers are the form's)
PoseInfoJob pinfo_job(const sc_params* p, uint32_t n_problems, const void* d_pose, uint32_t pose_stride, sc_pose_info_result* d_info) {
  PoseInfoJob job{};
  job.soa = p->layout == SC_SOA;
  job.tau2 = derive(p).tau2;
  job.n_problems = n_problems;
  job.pose = d_pose; job.pose_stride = pose_stride;
  job.out = reinterpret_cast<PoseInfoRecord*>(d_info);
  return job;
}

int pinfo_enqueue(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                  const void* d_pose, uint32_t pose_stride, sc_pose_info_result* d_info) {
  SC_TRY(batch_offsets_to_device(c, offset, n_problems, c->pinfo_off));
  PoseInfoJob job = pinfo_job(p, n_problems, d_pose, pose_stride, d_info);
  job.src = d_src; job.tgt = d_tgt; job.offset = c->pinfo_off.as<uint32_t>();
  job.total = offset[n_problems];
  launch_pose_info_batch(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_pose_info_batch_device(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                              const sc_params* p, const void* d_pose, uint32_t pose_stride, sc_pose_info_result* d_info) {
  if (!c) return SC_EINVAL;
  if (!d_src || !d_tgt || !offset || !p || !d_pose || !d_info) return refuse(c, "sc_pose_info_batch_device", "a NULL argument");
  SC_TRY(pose_batch_check(c, "sc_pose_info_batch", p, pinfo_stride_error(pose_stride), offset, n_problems));
  return pinfo_enqueue(c, d_src, d_tgt, offset, n_problems, p, d_pose, pose_stride, d_info);
}

int sc_pose_info_batch(sc_ctx* c, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                       const void* pose, uint32_t pose_stride, sc_pose_info_result* info) {
  if (!c) return SC_EINVAL;
  if (!src || !tgt || !offset || !p || !pose || !info) return refuse(c, "sc_pose_info_batch", "a NULL argument");
  SC_TRY(pose_batch_check(c, "sc_pose_info_batch", p, pinfo_stride_error(pose_stride), offset, n_problems));
  const size_t total = offset[n_problems], pts = total * 12;
  HostArrays h(c);
  const int a_src = h.in(src, pts), a_tgt = h.in(tgt, pts);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(n_problems, pose_stride, true));
  const int a_info = h.out(info, (size_t)n_problems * sizeof(sc_pose_info_result));
  h.also(c->pinfo_off, batch_offsets_bytes(n_problems));
  return h.run([&] {
    return pinfo_enqueue(c, h.at<float>(a_src), h.at<float>(a_tgt), offset, n_problems, p, h.at<void>(a_pose), pose_stride,
                         h.at<sc_pose_info_result>(a_info));
  });
}

int sc_pose_info_batch_slots_device(sc_ctx* c, const float* d_src_pts, const uint32_t* src_off, const float* d_tgt_pts,
                                    const uint32_t* tgt_off, uint32_t n_problems, uint32_t knn, const sc_params* p, const int32_t* d_corr,
                                    const uint32_t* d_count, const void* d_pose, uint32_t pose_stride, sc_pose_info_result* d_info) {
  static const char* const who = "sc_pose_info_batch_slots_device";
  if (!c) return SC_EINVAL;
  if (!d_src_pts || !src_off || !d_tgt_pts || !tgt_off || !p || !d_corr || !d_count || !d_pose || !d_info)
    return refuse(c, who, "a NULL argument");
  SC_TRY(pinfo_common_check(c, p, pose_stride, who));
  if (knn < 1 || knn > 4) return refuse(c, who, "knn must be 1 .. 4");
  if (const char* what = match_batch_offsets_error(src_off, tgt_off, n_problems, knn, true)) return refuse(c, who, what);
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  // both offset arrays and the slot starts, one copy
  const size_t nb1 = (size_t)n_problems + 1, bytes = 3 * nb1 * 4;
  ENSURE(c, c->pinfo_off, bytes);
  SC_TRY(batch_staging_begin(c, bytes));
  batch_slot_meta(src_off, tgt_off, n_problems, knn, static_cast<uint32_t*>(c->h_batch_off));
  SC_TRY(batch_staging_send(c, c->pinfo_off, bytes));
  const uint32_t* meta = c->pinfo_off.as<uint32_t>();
  PoseInfoSlotJob slots{};
  slots.job = pinfo_job(p, n_problems, d_pose, pose_stride, d_info);
  PoseInfoJob& job = slots.job;
  job.src = d_src_pts; job.tgt = d_tgt_pts; job.offset = meta;
  job.total = src_off[n_problems];
  slots.tgt_off = meta + nb1; slots.slot = meta + 2 * nb1;
  slots.corr = d_corr; slots.count = d_count;
  slots.knn = knn; slots.total_t = tgt_off[n_problems];
  launch_pose_info_batch_slots(slots, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

int sc_pose_info_pairs_slots_device(sc_ctx* c, const float* d_pts, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs,
                                    uint32_t n_pairs, uint32_t knn, const sc_params* p, const int32_t* d_corr, const uint32_t* d_count,
                                    const void* d_pose, uint32_t pose_stride, sc_pose_info_result* d_info) {
  static const char* const who = "sc_pose_info_pairs_slots_device";
  if (!c) return SC_EINVAL;
  if (!d_pts || !set_off || !pairs || !p || !d_corr || !d_count || !d_pose || !d_info) return refuse(c, who, "a NULL argument");
  SC_TRY(pinfo_common_check(c, p, pose_stride, who));
  if (const char* what = pairs_error(set_off, n_sets, pairs, n_pairs, knn, true)) return refuse(c, who, what);
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  // the pairs' records, one copy
  const size_t bytes = (size_t)PAIR_WORDS * n_pairs * 4;
  ENSURE(c, c->pinfo_off, bytes);
  SC_TRY(batch_staging_begin(c, bytes));
  pairs_records(set_off, pairs, n_pairs, knn, static_cast<uint32_t*>(c->h_batch_off));
  SC_TRY(batch_staging_send(c, c->pinfo_off, bytes));
  PoseInfoPairsJob arg{};
  arg.job = pinfo_job(p, n_pairs, d_pose, pose_stride, d_info);
  PoseInfoJob& job = arg.job;
  job.src = d_pts; job.tgt = d_pts; job.offset = nullptr;  // both sides are rows of the one table; the records say which
  job.total = set_off[n_sets];
  arg.rec = c->pinfo_off.as<uint32_t>();
  arg.corr = d_corr; arg.count = d_count; arg.knn = knn;
  launch_pose_info_batch_pairs(arg, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // extern "C"
