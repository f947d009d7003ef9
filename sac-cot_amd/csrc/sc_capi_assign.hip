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
#include "sc_capi_pose.hpp"

using namespace sc;

static_assert(sizeof(sc_assign_params) == 32 && sizeof(sc_assign_result) == 32, "sc_assign_params and sc_assign_result are 32 bytes");

namespace {

// ---- the frame form
int asg_frame_enqueue(sc_ctx* c, const sc_assign_params* ap, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                      const uint8_t* d_sel, int32_t* d_label, float* d_d2, sc_assign_result* d_asg) {
  AssignFrameJob job{};
  pose_frame_head(c, &job, d_pose, pose_stride, n_poses, assign_reads_status(ap, false));
  job.mode = ap->mode;
  job.sel = ap->sel_mode == SC_ASSIGN_SEL_MASK ? d_sel : nullptr;
  job.label = d_label; job.d2 = d_d2;
  job.out = reinterpret_cast<AssignRecord*>(d_asg);
  HIPCHK(c, hipMemsetAsync(d_asg, 0, (size_t)n_poses * sizeof(sc_assign_result), c->stream));  // the tallies are added into it
  launch_assign_frame(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// ---- the batch form
int asg_batch_enqueue(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                      const sc_assign_params* ap, const void* d_pose, uint32_t pose_stride, uint32_t n_poses, int32_t* d_label,
                      sc_assign_result* d_asg) {
  AssignBatchJob job{};
  SC_TRY(pose_batch_head(c, &job, c->asg_off, d_src, d_tgt, offset, n_problems, p, d_pose, pose_stride, n_poses));
  job.mode = ap->mode;
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
  SC_TRY(pose_frame_check(c, who, assign_params_error(ap, pose_stride, n_poses, false, d_sel != nullptr)));
  return asg_frame_enqueue(c, ap, d_pose, pose_stride, n_poses, d_sel, d_label, d_d2, d_asg);  // (no wait: the outputs are complete in stream order)
}

int sc_assign_poses_frame(sc_ctx* c, const sc_assign_params* ap, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                          const uint8_t* sel, int32_t* label, float* d2, sc_assign_result* asg) {
  static const char* const who = "sc_assign_poses_frame";
  if (!c) return SC_EINVAL;
  if (!ap || !pose || !label || !asg) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_frame_check(c, who, assign_params_error(ap, pose_stride, n_poses, false, sel != nullptr)));
  const size_t n = (size_t)c->pass.n;
  const bool masked = ap->sel_mode == SC_ASSIGN_SEL_MASK;
  HostArrays h(c);  // the family's list: src, tgt, pose, sel, label, d2, asg
  h.absent(2);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(n_poses, pose_stride, assign_reads_status(ap, false)));
  const int a_sel = h.in(masked ? sel : nullptr, n);
  const int a_label = h.out(label, n * 4), a_d2 = h.out(d2, n * 4);
  const int a_asg = h.out(asg, (size_t)n_poses * sizeof(sc_assign_result));
  return h.run([&] {  // (no scratch: the tallies are added into the records)
    return asg_frame_enqueue(c, ap, h.at<void>(a_pose), pose_stride, n_poses, h.at<uint8_t>(a_sel), h.at<int32_t>(a_label), h.at<float>(a_d2),
                             h.at<sc_assign_result>(a_asg));
  });
}

int sc_assign_poses_batch_device(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                                 const sc_params* p, const sc_assign_params* ap, const void* d_pose, uint32_t pose_stride,
                                 uint32_t n_poses, int32_t* d_label, sc_assign_result* d_asg) {
  static const char* const who = "sc_assign_poses_batch_device";
  if (!c) return SC_EINVAL;
  if (!d_src || !d_tgt || !offset || !p || !ap || !d_pose || !d_label || !d_asg) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_batch_check(c, who, p, assign_params_error(ap, pose_stride, n_poses, true, false), offset, n_problems));
  return asg_batch_enqueue(c, d_src, d_tgt, offset, n_problems, p, ap, d_pose, pose_stride, n_poses, d_label, d_asg);
}

int sc_assign_poses_batch(sc_ctx* c, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                          const sc_assign_params* ap, const void* pose, uint32_t pose_stride, uint32_t n_poses, int32_t* label,
                          sc_assign_result* asg) {
  static const char* const who = "sc_assign_poses_batch";
  if (!c) return SC_EINVAL;
  if (!src || !tgt || !offset || !p || !ap || !pose || !label || !asg) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_batch_check(c, who, p, assign_params_error(ap, pose_stride, n_poses, true, false), offset, n_problems));
  const size_t total = offset[n_problems], pts = total * 12, records = (size_t)n_poses * n_problems;
  HostArrays h(c);  // the family's list: src, tgt, pose, sel, label, d2, asg
  const int a_src = h.in(src, pts), a_tgt = h.in(tgt, pts);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(records, pose_stride, true));
  h.absent();
  const int a_label = h.out(label, total * 4);
  h.absent();
  const int a_asg = h.out(asg, records * sizeof(sc_assign_result));
  h.also(c->asg_off, batch_offsets_bytes(n_problems));
  return h.run([&] {
    return asg_batch_enqueue(c, h.at<float>(a_src), h.at<float>(a_tgt), offset, n_problems, p, ap, h.at<void>(a_pose), pose_stride, n_poses,
                             h.at<int32_t>(a_label), h.at<sc_assign_result>(a_asg));
  });
}

}  // extern "C"
