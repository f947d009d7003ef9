// sc_capi_info_frame.hip — the C ABI's fp64 information matrix on a scored frame (include/saccot.h, sc_pose_info_frame):
// sc_pose_info_default_params, sc_pose_info_frame_device and sc_pose_info_frame.  Host-only, on the context and the helpers of
// sc_ctx.hpp; the kernel is sc_info_frame.hip's.
//
// ONE launch, a workgroup per pose, and no wait in the device form: a pose's status is a field of its record, so no word of the GPU's
// is needed on the host.  Everything is read from what the frame left — the staged planes, n, tau — and nothing of it is written:
// the chunk sums live in a buffer of this entry's own (pinfo_frame_tmp), not in polish_tmp, so a polish enqueued behind this call on
// the same stream shares nothing with it.  Everything that can refuse the call is decided on the host before anything is enqueued.
#include "sc_ctx.hpp"

using namespace sc;

static_assert(sizeof(sc_pose_info_params) == 32, "sc_pose_info_params is 32 bytes");

namespace {

// the refusals both forms share, then "is there a frame"; `who` opens the message
int pinfo_frame_check(sc_ctx* c, const sc_pose_info_params* ip, uint32_t pose_stride, uint32_t n_poses, const void* sel, const char* who) {
  SC_TRY(busy(c));
  if (ip->size != sizeof(sc_pose_info_params)) return refuse(c, who, "params->size is not sizeof(sc_pose_info_params)");
  if (ip->sel_mode > SC_POSE_INFO_SEL_LABEL) return refuse(c, who, "sel_mode must be SC_POSE_INFO_SEL_NONE, _MASK or _LABEL");
  if (ip->sel_mode != SC_POSE_INFO_SEL_NONE && !sel) return refuse(c, who, "sel is NULL with a sel_mode that reads it");
  if (ip->label0 != 0 && ip->sel_mode != SC_POSE_INFO_SEL_LABEL) return refuse(c, who, "label0 must be 0 unless sel_mode is SC_POSE_INFO_SEL_LABEL");
  if ((ip->flags & ~SC_POSE_INFO_STATUS) || ip->reserved[0] || ip->reserved[1] || ip->reserved[2] || ip->reserved[3])
    return refuse(c, who, "an unknown flag, or a reserved field that is not 0");
  if (n_poses < 1 || n_poses > SC_POSE_INFO_MAX_POSES) return refuse(c, who, "n_poses must be 1 .. SC_POSE_INFO_MAX_POSES");
  const uint32_t least = (ip->flags & SC_POSE_INFO_STATUS) ? 52u : 48u;
  if (pose_stride < least || pose_stride % 4 != 0)
    return refuse(c, who, "pose_stride must be a multiple of 4 and at least 48 (52 with SC_POSE_INFO_STATUS)");
  return scored_frame_begin(c, who);
}

// the scratch has its room (the caller's last ENSURE): the launch
int pinfo_frame_enqueue(sc_ctx* c, const sc_pose_info_params* ip, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                        const void* d_sel, sc_pose_info_result* d_info) {
  const Pass& ps = c->pass;
  PoseInfoFrameJob job{};
  job.pts = points_of(c);
  job.tau2 = ps.dv.tau2;
  job.n_poses = n_poses;
  job.pose = d_pose; job.pose_stride = pose_stride;
  job.status = (ip->flags & SC_POSE_INFO_STATUS) != 0;
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
  SC_TRY(pinfo_frame_check(c, ip, pose_stride, n_poses, d_sel, who));
  ENSURE(c, c->pinfo_frame_tmp, (size_t)n_poses * pose_info_frame_scratch_bytes(c->pass.n));
  return pinfo_frame_enqueue(c, ip, d_pose, pose_stride, n_poses, d_sel, d_info);  // (no wait: d_info is complete in stream order)
}

int sc_pose_info_frame(sc_ctx* c, const sc_pose_info_params* ip, const void* pose, uint32_t pose_stride, uint32_t n_poses, const void* sel,
                       sc_pose_info_result* info) {
  static const char* const who = "sc_pose_info_frame";
  if (!c) return SC_EINVAL;
  if (!ip || !pose || !info) return refuse(c, who, "a NULL argument");
  SC_TRY(pinfo_frame_check(c, ip, pose_stride, n_poses, sel, who));
  const size_t n = (size_t)c->pass.n;
  const size_t read = (ip->flags & SC_POSE_INFO_STATUS) ? 52 : 48;  // (nothing is read behind the last record's last word)
  HostArrays h(c);
  h.in(c->pinfo_frame_pose, pose, (size_t)(n_poses - 1) * pose_stride + read);
  if (ip->sel_mode != SC_POSE_INFO_SEL_NONE) h.in(c->pinfo_frame_sel, sel, ip->sel_mode == SC_POSE_INFO_SEL_MASK ? n : n * 4);
  h.out(c->pinfo_frame_out, info, (size_t)n_poses * sizeof(sc_pose_info_result));
  SC_TRY(h.room());
  ENSURE(c, c->pinfo_frame_tmp, (size_t)n_poses * pose_info_frame_scratch_bytes(c->pass.n));
  SC_TRY(h.send());
  SC_TRY(pinfo_frame_enqueue(c, ip, c->pinfo_frame_pose.p, pose_stride, n_poses, c->pinfo_frame_sel.p, c->pinfo_frame_out.as<sc_pose_info_result>()));
  SC_TRY(h.fetch());
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // extern "C"
