// sc_capi_polish_poses.hip — the C ABI's refit of caller-supplied poses on a scored frame (include/saccot.h, sc_polish_poses):
// sc_polish_poses_default_params, sc_polish_poses_device and sc_polish_poses.  Host-only, on the context and the helpers of
// sc_ctx.hpp; the kernel is sc_polish_poses.hip's.
//
// ONE launch, a workgroup per pose, and no wait in the device form: a pose's status is a field of its record, so no word of the GPU's
// is needed on the host.  Everything is read from what the frame left — the staged planes, n, tau, score_mode — and nothing of it is
// written: the chunk sums live in a buffer of this entry's own (ppose_tmp), not in polish_tmp or pinfo_frame_tmp, so a polish or an
// information matrix enqueued behind this call on the same stream shares nothing with it.  Everything that can refuse the call is
// decided on the host before anything is enqueued.
#include "sc_ctx.hpp"

using namespace sc;

static_assert(sizeof(sc_polish_poses_params) == 32, "sc_polish_poses_params is 32 bytes");

namespace {

inline bool reads_sel(uint32_t sel_mode) { return sel_mode != SC_POLISH_POSES_SEL_NONE; }
inline bool sel_is_label(uint32_t sel_mode) { return sel_mode == SC_POLISH_POSES_SEL_LABEL || sel_mode == SC_POLISH_POSES_SEL_ALIVE; }

// the refusals both forms share, then "is there a frame"; `who` opens the message
int ppose_check(sc_ctx* c, const sc_polish_poses_params* qp, uint32_t pose_stride, uint32_t n_poses, const void* sel, const char* who) {
  SC_TRY(busy(c));
  if (qp->size != sizeof(sc_polish_poses_params)) return refuse(c, who, "params->size is not sizeof(sc_polish_poses_params)");
  if (qp->max_iter < 1 || qp->max_iter > 64) return refuse(c, who, "max_iter must be 1 .. 64");
  if (qp->sel_mode > SC_POLISH_POSES_SEL_ALIVE) return refuse(c, who, "sel_mode must be SC_POLISH_POSES_SEL_NONE, _MASK, _LABEL or _ALIVE");
  if (reads_sel(qp->sel_mode) && !sel) return refuse(c, who, "sel is NULL with a sel_mode that reads it");
  if (qp->label0 != 0 && !sel_is_label(qp->sel_mode))
    return refuse(c, who, "label0 must be 0 unless sel_mode is SC_POLISH_POSES_SEL_LABEL or _ALIVE");
  if ((qp->flags & ~SC_POLISH_POSES_STATUS) || qp->reserved[0] || qp->reserved[1] || qp->reserved[2])
    return refuse(c, who, "an unknown flag, or a reserved field that is not 0");
  if (n_poses < 1 || n_poses > SC_POLISH_POSES_MAX) return refuse(c, who, "n_poses must be 1 .. SC_POLISH_POSES_MAX");
  const uint32_t least = (qp->flags & SC_POLISH_POSES_STATUS) ? 52u : 48u;
  if (pose_stride < least || pose_stride % 4 != 0)
    return refuse(c, who, "pose_stride must be a multiple of 4 and at least 48 (52 with SC_POLISH_POSES_STATUS)");
  return scored_frame_begin(c, who);
}

// the scratch has its room (the caller's last ENSURE): the launch
int ppose_enqueue(sc_ctx* c, const sc_polish_poses_params* qp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                  const void* d_sel, sc_polish_batch_result* d_pol, uint8_t* d_mask) {
  const Pass& ps = c->pass;
  PolishPosesJob job{};
  job.pts = points_of(c);
  job.tau2 = ps.dv.tau2;
  job.thr = score_thr(ps.dv, ps.params.score_mode);
  job.score_mode = ps.params.score_mode;
  job.max_iter = qp->max_iter;
  job.n_poses = n_poses;
  job.pose = d_pose; job.pose_stride = pose_stride;
  job.status = (qp->flags & SC_POLISH_POSES_STATUS) != 0;
  job.sel = reads_sel(qp->sel_mode) ? d_sel : nullptr;
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
  SC_TRY(ppose_check(c, qp, pose_stride, n_poses, d_sel, who));
  ENSURE(c, c->ppose_tmp, (size_t)n_poses * polish_poses_scratch_bytes(c->pass.n));
  return ppose_enqueue(c, qp, d_pose, pose_stride, n_poses, d_sel, d_pol, d_mask);  // (no wait: the outputs are complete in stream order)
}

int sc_polish_poses(sc_ctx* c, const sc_polish_poses_params* qp, const void* pose, uint32_t pose_stride, uint32_t n_poses, const void* sel,
                    sc_polish_batch_result* pol, uint8_t* mask) {
  static const char* const who = "sc_polish_poses";
  if (!c) return SC_EINVAL;
  if (!qp || !pose || !pol) return refuse(c, who, "a NULL argument");
  SC_TRY(ppose_check(c, qp, pose_stride, n_poses, sel, who));
  const size_t n = (size_t)c->pass.n;
  const size_t read = (qp->flags & SC_POLISH_POSES_STATUS) ? 52 : 48;  // (nothing is read behind the last record's last word)
  HostArrays h(c);
  h.in(c->ppose_pose, pose, (size_t)(n_poses - 1) * pose_stride + read);
  if (reads_sel(qp->sel_mode)) h.in(c->ppose_sel, sel, sel_is_label(qp->sel_mode) ? n * 4 : n);
  h.out(c->ppose_out, pol, (size_t)n_poses * sizeof(sc_polish_batch_result));
  if (mask) h.out(c->ppose_mask, mask, (size_t)n_poses * n);
  SC_TRY(h.room());
  ENSURE(c, c->ppose_tmp, (size_t)n_poses * polish_poses_scratch_bytes(c->pass.n));
  SC_TRY(h.send());
  SC_TRY(ppose_enqueue(c, qp, c->ppose_pose.p, pose_stride, n_poses, c->ppose_sel.p, c->ppose_out.as<sc_polish_batch_result>(),
                       mask ? c->ppose_mask.as<uint8_t>() : nullptr));
  SC_TRY(h.fetch());
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // extern "C"
