// sc_capi_pose.hpp — the host steps the entries on a caller's pose records share (sc_pose_info_frame, sc_polish_poses,
// sc_assign_poses, sc_settle_poses; the batch check also sc_pose_info_batch's), said once: the heads of their jobs (PoseFrameHead,
// PoseBatchHead: sc_kernels.hpp) and the order of a frame form's and of a batch form's refusals.  A host form's sequence is
// HostArrays::run (sc_ctx.hpp).  Each entry brings what is its own: its rule (sc_pose_check.hpp and the check headers beside it), its scratch, its launch.
// Everything that can refuse a call is decided before anything is enqueued.
#pragma once
#include "sc_ctx.hpp"
#include "sc_pose_check.hpp"

namespace sc {

// ---- a frame form
// The refusals, in this order: a call outstanding, the family's rule (`broken`: what its *_params_error returned), "is there a
// frame"; `who` opens the message.
inline int pose_frame_check(sc_ctx* c, const char* who, const char* broken) {
  SC_TRY(busy(c));
  if (broken) return refuse(c, who, broken);
  return scored_frame_begin(c, who);
}
// What every frame job opens with, from what the frame left in the context.
inline void pose_frame_head(const sc_ctx* c, PoseFrameHead* h, const void* d_pose, uint32_t pose_stride, uint32_t n_poses, bool reads_status) {
  const Pass& ps = c->pass;
  h->pts = points_of(c);
  h->tau2 = ps.dv.tau2;
  h->thr = score_thr(ps.dv, ps.params.score_mode);
  h->score_mode = ps.params.score_mode;
  h->n_poses = n_poses;
  h->pose = d_pose; h->pose_stride = pose_stride;
  h->status = reads_status;
}
// the chunk scratch of an entry that keeps one: a block per pose (sc_chunks.hpp); a host form names it with HostArrays::also
inline size_t pose_frame_scratch_bytes(const sc_ctx* c, uint32_t n_poses) { return (size_t)n_poses * chunk_scratch_bytes(c->pass.n); }

// ---- a batch form
// The refusals, in this order: the context, sc_params, the family's rule (`broken`), the offsets; then the context's device and cap.
inline int pose_batch_check(sc_ctx* c, const char* who, const sc_params* p, const char* broken, const uint32_t* offset, uint32_t n_problems) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(batch_params_check(c, p, who));
  if (broken) return refuse(c, who, broken);
  if (const char* what = batch_offsets_error(offset, n_problems)) return refuse(c, who, what);
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  return SC_OK;
}
// What every motion-major batch job opens with: the offsets on their way to `off` (enqueued), the rest from sc_params.
inline int pose_batch_head(sc_ctx* c, PoseBatchHead* h, Buf& off, const float* d_src, const float* d_tgt, const uint32_t* offset,
                           uint32_t n_problems, const sc_params* p, const void* d_pose, uint32_t pose_stride, uint32_t n_poses) {
  SC_TRY(batch_offsets_to_device(c, offset, n_problems, off));
  const Derived dv = derive(p);
  h->src = d_src; h->tgt = d_tgt; h->offset = off.as<uint32_t>();
  h->n_problems = n_problems; h->total = offset[n_problems];
  h->soa = p->layout == SC_SOA; h->score_mode = p->score_mode;
  h->tau2 = dv.tau2; h->thr = score_thr(dv, p->score_mode);
  h->n_poses = n_poses;
  h->pose = d_pose; h->pose_stride = pose_stride;
  return SC_OK;
}

}  // namespace sc
