// sc_capi_assign.hip — the C ABI's labelling of correspondences by the pose that fits best (include/saccot.h, sc_assign_poses):
// sc_assign_default_params, sc_assign_poses_frame_device, sc_assign_poses_frame, sc_assign_poses_batch_device and
// sc_assign_poses_batch.  Host-only, on the context and the helpers of sc_ctx.hpp; the kernels are sc_assign_frame.hip's and
// sc_assign_batch.hip's, the rules of the parameters sc_assign_check.hpp's.
//
// The frame form: a memset of the caller's records, then ONE launch, a workgroup per tile — two stream operations whatever n and
// n_poses are — and no wait in the device form: the tallies are added into the records themselves, so there is no scratch, and
// nothing of the frame is written.  The batch form: offsets -> pinned staging (the area and event every batch entry shares) -> device
// copy (enqueued) -> ONE launch, a workgroup per problem.  Nothing is read back by either.  Everything that can refuse a call is
// decided on the host before anything is enqueued.
#include "sc_assign_check.hpp"
#include "sc_ctx.hpp"

using namespace sc;

static_assert(sizeof(sc_assign_params) == 32 && sizeof(sc_assign_result) == 32, "sc_assign_params and sc_assign_result are 32 bytes");

namespace {

// ---- the frame form: the refusals both entries share, then "is there a frame"; `who` opens the message
int asg_frame_check(sc_ctx* c, const sc_assign_params* ap, uint32_t pose_stride, uint32_t n_poses, const void* sel, const char* who) {
  SC_TRY(busy(c));
  if (const char* what = assign_params_error(ap, pose_stride, n_poses, false, sel != nullptr)) return refuse(c, who, what);
  return scored_frame_begin(c, who);
}

int asg_frame_enqueue(sc_ctx* c, const sc_assign_params* ap, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                      const uint8_t* d_sel, int32_t* d_label, float* d_d2, sc_assign_result* d_asg) {
  const Pass& ps = c->pass;
  AssignFrameJob job{};
  job.pts = points_of(c);
  job.tau2 = ps.dv.tau2;
  job.thr = score_thr(ps.dv, ps.params.score_mode);
  job.score_mode = ps.params.score_mode;
  job.mode = ap->mode; job.n_poses = n_poses;
  job.pose = d_pose; job.pose_stride = pose_stride;
  job.status = assign_reads_status(ap, false);
  job.sel = ap->sel_mode == SC_ASSIGN_SEL_MASK ? d_sel : nullptr;
  job.label = d_label; job.d2 = d_d2;
  job.out = reinterpret_cast<AssignRecord*>(d_asg);
  HIPCHK(c, hipMemsetAsync(d_asg, 0, (size_t)n_poses * sizeof(sc_assign_result), c->stream));  // the tallies are added into it
  launch_assign_frame(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// ---- the batch form: the refusals both entries share
int asg_batch_check(sc_ctx* c, const uint32_t* offset, uint32_t n_problems, const sc_params* p, const sc_assign_params* ap,
                    uint32_t pose_stride, uint32_t n_poses, const char* who) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(batch_params_check(c, p, who));
  if (const char* what = assign_params_error(ap, pose_stride, n_poses, true, false)) return refuse(c, who, what);
  if (const char* what = batch_offsets_error(offset, n_problems)) return refuse(c, who, what);
  return SC_OK;
}

int asg_batch_enqueue(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                      const sc_assign_params* ap, const void* d_pose, uint32_t pose_stride, uint32_t n_poses, int32_t* d_label,
                      sc_assign_result* d_asg) {
  SC_TRY(batch_offsets_to_device(c, offset, n_problems, c->asg_off));
  const Derived dv = derive(p);
  AssignBatchJob job{};
  job.src = d_src; job.tgt = d_tgt; job.offset = c->asg_off.as<uint32_t>();
  job.n_problems = n_problems; job.total = offset[n_problems];
  job.soa = p->layout == SC_SOA; job.score_mode = p->score_mode;
  job.tau2 = dv.tau2; job.thr = score_thr(dv, p->score_mode);
  job.mode = ap->mode; job.n_poses = n_poses;
  job.pose = d_pose; job.pose_stride = pose_stride;
  job.label = d_label;
  job.out = reinterpret_cast<AssignRecord*>(d_asg);
  launch_assign_batch(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_assign_default_params(sc_assign_params* ap) {
  if (!ap) return SC_EINVAL;
  memset(ap, 0, sizeof(*ap));
  ap->size = sizeof(sc_assign_params);
  return SC_OK;
}

int sc_assign_poses_frame_device(sc_ctx* c, const sc_assign_params* ap, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                                 const uint8_t* d_sel, int32_t* d_label, float* d_d2, sc_assign_result* d_asg) {
  static const char* const who = "sc_assign_poses_frame_device";
  if (!c) return SC_EINVAL;
  if (!ap || !d_pose || !d_label || !d_asg) return refuse(c, who, "a NULL argument");
  SC_TRY(asg_frame_check(c, ap, pose_stride, n_poses, d_sel, who));
  return asg_frame_enqueue(c, ap, d_pose, pose_stride, n_poses, d_sel, d_label, d_d2, d_asg);  // (no wait: the outputs are complete in stream order)
}

int sc_assign_poses_frame(sc_ctx* c, const sc_assign_params* ap, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                          const uint8_t* sel, int32_t* label, float* d2, sc_assign_result* asg) {
  static const char* const who = "sc_assign_poses_frame";
  if (!c) return SC_EINVAL;
  if (!ap || !pose || !label || !asg) return refuse(c, who, "a NULL argument");
  SC_TRY(asg_frame_check(c, ap, pose_stride, n_poses, sel, who));
  const size_t n = (size_t)c->pass.n;
  const bool masked = ap->sel_mode == SC_ASSIGN_SEL_MASK;
  HostArrays h(c);
  h.in(c->asg_pose, pose, (size_t)assign_pose_bytes(n_poses, pose_stride, assign_reads_status(ap, false)));
  if (masked) h.in(c->asg_sel, sel, n);
  h.out(c->asg_label, label, n * 4);
  if (d2) h.out(c->asg_d2, d2, n * 4);
  h.out(c->asg_out, asg, (size_t)n_poses * sizeof(sc_assign_result));
  SC_TRY(h.room());
  SC_TRY(h.send());
  SC_TRY(asg_frame_enqueue(c, ap, c->asg_pose.p, pose_stride, n_poses, masked ? c->asg_sel.as<uint8_t>() : nullptr,
                           c->asg_label.as<int32_t>(), d2 ? c->asg_d2.as<float>() : nullptr, c->asg_out.as<sc_assign_result>()));
  SC_TRY(h.fetch());
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

int sc_assign_poses_batch_device(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                                 const sc_params* p, const sc_assign_params* ap, const void* d_pose, uint32_t pose_stride,
                                 uint32_t n_poses, int32_t* d_label, sc_assign_result* d_asg) {
  static const char* const who = "sc_assign_poses_batch_device";
  if (!c) return SC_EINVAL;
  if (!d_src || !d_tgt || !offset || !p || !ap || !d_pose || !d_label || !d_asg) return refuse(c, who, "a NULL argument");
  SC_TRY(asg_batch_check(c, offset, n_problems, p, ap, pose_stride, n_poses, who));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  return asg_batch_enqueue(c, d_src, d_tgt, offset, n_problems, p, ap, d_pose, pose_stride, n_poses, d_label, d_asg);
}

int sc_assign_poses_batch(sc_ctx* c, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                          const sc_assign_params* ap, const void* pose, uint32_t pose_stride, uint32_t n_poses, int32_t* label,
                          sc_assign_result* asg) {
  static const char* const who = "sc_assign_poses_batch";
  if (!c) return SC_EINVAL;
  if (!src || !tgt || !offset || !p || !ap || !pose || !label || !asg) return refuse(c, who, "a NULL argument");
  SC_TRY(asg_batch_check(c, offset, n_problems, p, ap, pose_stride, n_poses, who));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  const size_t total = offset[n_problems], pts = total * 12, records = (size_t)n_poses * n_problems;
  HostArrays h(c);
  h.in(c->asg_src, src, pts);
  h.in(c->asg_tgt, tgt, pts);
  h.in(c->asg_pose, pose, (size_t)assign_pose_bytes(records, pose_stride, true));
  h.out(c->asg_label, label, total * 4);
  h.out(c->asg_out, asg, records * sizeof(sc_assign_result));
  SC_TRY(h.room());
  SC_TRY(h.send());
  SC_TRY(asg_batch_enqueue(c, c->asg_src.as<float>(), c->asg_tgt.as<float>(), offset, n_problems, p, ap, c->asg_pose.p, pose_stride, n_poses,
                           c->asg_label.as<int32_t>(), c->asg_out.as<sc_assign_result>()));
  return h.fetch();
}

}  // extern "C"
