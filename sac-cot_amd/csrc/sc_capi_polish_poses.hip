// sc_capi_polish_poses.hip — the C ABI's refit of caller-supplied poses on a scored frame (include/saccot.h, sc_polish_poses):
// sc_polish_poses_default_params, sc_polish_poses_device and sc_polish_poses.  Host-only, on the context and the helpers of
// sc_ctx.hpp and sc_capi_pose.hpp; the kernel is sc_polish_poses.hip's, the rules of the parameters sc_pose_check.hpp's.
//
// ONE launch, a workgroup per pose, and no wait in the device form: a pose's status is a field of its record, so no word of the GPU's
// is needed on the host.  Everything is read from what the frame left — the staged planes, n, tau, score_mode — and nothing of it is
// written: the chunk sums live in a buffer of this entry's own (ppose_tmp), not in polish_tmp or pinfo_frame_tmp, so a polish or an
// information matrix enqueued behind this call on the same stream shares nothing with it.  Everything that can refuse the call is
// decided on the host before anything is enqueued.
#include "sc_capi_pose.hpp"

using namespace sc;

static_assert(sizeof(sc_polish_poses_params) == 32, "sc_polish_poses_params is 32 bytes");

namespace {


// the scratch has its room (the caller's last ENSURE): the launch
int ppose_enqueue(sc_ctx* c, const sc_polish_poses_params* qp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                  const void* d_sel, sc_polish_batch_result* d_pol, uint8_t* d_mask) {
  PolishPosesJob job{};
  pose_frame_head(c, &job, d_pose, pose_stride, n_poses, polish_poses_reads_status(qp));
  job.max_iter = qp->max_iter;
  job.sel = polish_poses_reads_sel(qp->sel_mode) ? d_sel : nullptr;
  job.sel_mode = qp->sel_mode; job.label0 = qp->label0;
  job.scratch = c->ppose_tmp.as<double>();
  job.out = reinterpret_cast<PolishBatchRecord*>(d_pol);
  job.mask = d_mask;
  launch_polish_poses(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_polish_poses_default_params(sc_polish_poses_params* qp) {
  if (!qp) return SC_EINVAL;
  memset(qp, 0, sizeof(*qp));
  qp->size = sizeof(sc_polish_poses_params);
  qp->max_iter = 16;
  return SC_OK;
}

int sc_polish_poses_device(sc_ctx* c, const sc_polish_poses_params* qp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                           const void* d_sel, sc_polish_batch_result* d_pol, uint8_t* d_mask) {
  static const char* const who = "sc_polish_poses_device";
  if (!c) return SC_EINVAL;
  if (!qp || !d_pose || !d_pol) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_frame_check(c, who, polish_poses_params_error(qp, pose_stride, n_poses, d_sel != nullptr)));
  ENSURE(c, c->ppose_tmp, pose_frame_scratch_bytes(c, n_poses));
  return ppose_enqueue(c, qp, d_pose, pose_stride, n_poses, d_sel, d_pol, d_mask);  // (no wait: the outputs are complete in stream order)
}

int sc_polish_poses(sc_ctx* c, const sc_polish_poses_params* qp, const void* pose, uint32_t pose_stride, uint32_t n_poses, const void* sel,
                    sc_polish_batch_result* pol, uint8_t* mask) {
  static const char* const who = "sc_polish_poses";
  if (!c) return SC_EINVAL;
  if (!qp || !pose || !pol) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_frame_check(c, who, polish_poses_params_error(qp, pose_stride, n_poses, sel != nullptr)));
  const size_t n = (size_t)c->pass.n;
  HostArrays h(c);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(n_poses, pose_stride, polish_poses_reads_status(qp)));
  const int a_sel = h.in(polish_poses_reads_sel(qp->sel_mode) ? sel : nullptr, polish_poses_sel_is_label(qp->sel_mode) ? n * 4 : n);
  const int a_pol = h.out(pol, (size_t)n_poses * sizeof(sc_polish_batch_result)), a_mask = h.out(mask, (size_t)n_poses * n);
  h.also(c->ppose_tmp, pose_frame_scratch_bytes(c, n_poses));
  return h.run([&] {
    return ppose_enqueue(c, qp, h.at<void>(a_pose), pose_stride, n_poses, h.at<void>(a_sel), h.at<sc_polish_batch_result>(a_pol),
                         h.at<uint8_t>(a_mask));
  });
}

}  // extern "C"
