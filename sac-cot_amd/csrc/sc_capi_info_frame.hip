// sc_capi_info_frame.hip — the C ABI's fp64 information matrix on a scored frame (include/saccot.h, sc_pose_info_frame):
// sc_pose_info_default_params, sc_pose_info_frame_device and sc_pose_info_frame.  Host-only, on the context and the helpers of
// sc_ctx.hpp and sc_capi_pose.hpp; the kernel is sc_info_frame.hip's, the rules of the parameters sc_pose_check.hpp's.
//
// ONE launch, a workgroup per pose, and no wait in the device form: a pose's status is a field of its record, so no word of the GPU's
// is needed on the host.  Everything is read from what the frame left — the staged planes, n, tau — and nothing of it is written:
// the chunk sums live in a buffer of this entry's own (pinfo_frame_tmp), not in polish_tmp, so a polish enqueued behind this call on
// the same stream shares nothing with it.  Everything that can refuse the call is decided on the host before anything is enqueued.
#include "sc_capi_pose.hpp"

using namespace sc;

static_assert(sizeof(sc_pose_info_params) == 32, "sc_pose_info_params is 32 bytes");

namespace {


// the scratch has its room (the caller's last ENSURE): the launch
int pinfo_frame_enqueue(sc_ctx* c, const sc_pose_info_params* ip, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                        const void* d_sel, sc_pose_info_result* d_info) {
  PoseInfoFrameJob job{};
  pose_frame_head(c, &job, d_pose, pose_stride, n_poses, pose_info_reads_status(ip));
  job.sel = ip->sel_mode == SC_POSE_INFO_SEL_NONE ? nullptr : d_sel;
  job.sel_mode = ip->sel_mode; job.label0 = ip->label0;
  job.scratch = c->pinfo_frame_tmp.as<double>();
  job.out = reinterpret_cast<PoseInfoRecord*>(d_info);
  launch_pose_info_frame(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_pose_info_default_params(sc_pose_info_params* ip) {
  if (!ip) return SC_EINVAL;
  memset(ip, 0, sizeof(*ip));
  ip->size = sizeof(sc_pose_info_params);
  return SC_OK;
}

int sc_pose_info_frame_device(sc_ctx* c, const sc_pose_info_params* ip, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                              const void* d_sel, sc_pose_info_result* d_info) {
  static const char* const who = "sc_pose_info_frame_device";
  if (!c) return SC_EINVAL;
  if (!ip || !d_pose || !d_info) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_frame_check(c, who, pose_info_params_error(ip, pose_stride, n_poses, d_sel != nullptr)));
  ENSURE(c, c->pinfo_frame_tmp, pose_frame_scratch_bytes(c, n_poses));
  return pinfo_frame_enqueue(c, ip, d_pose, pose_stride, n_poses, d_sel, d_info);  // (no wait: d_info is complete in stream order)
}

int sc_pose_info_frame(sc_ctx* c, const sc_pose_info_params* ip, const void* pose, uint32_t pose_stride, uint32_t n_poses, const void* sel,
                       sc_pose_info_result* info) {
  static const char* const who = "sc_pose_info_frame";
  if (!c) return SC_EINVAL;
  if (!ip || !pose || !info) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_frame_check(c, who, pose_info_params_error(ip, pose_stride, n_poses, sel != nullptr)));
  const size_t n = (size_t)c->pass.n;
  HostArrays h(c);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(n_poses, pose_stride, pose_info_reads_status(ip)));
  const int a_sel = h.in(ip->sel_mode != SC_POSE_INFO_SEL_NONE ? sel : nullptr, ip->sel_mode == SC_POSE_INFO_SEL_MASK ? n : n * 4);
  const int a_info = h.out(info, (size_t)n_poses * sizeof(sc_pose_info_result));
  h.also(c->pinfo_frame_tmp, pose_frame_scratch_bytes(c, n_poses));
  return h.run([&] {
    return pinfo_frame_enqueue(c, ip, h.at<void>(a_pose), pose_stride, n_poses, h.at<void>(a_sel), h.at<sc_pose_info_result>(a_info));
  });
}

}  // extern "C"
