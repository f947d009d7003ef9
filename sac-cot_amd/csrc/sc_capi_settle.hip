// sc_capi_settle.hip — the C ABI's relabel-and-refit loop (include/saccot.h, sc_settle_poses): sc_settle_default_params,
// sc_settle_poses_frame_device, sc_settle_poses_frame, sc_settle_poses_batch_device and sc_settle_poses_batch.  Host-only, on the
// context and the helpers of sc_ctx.hpp; the kernels are sc_settle_frame.hip's and sc_settle_batch.hip's, the rules of the
// parameters sc_settle_check.hpp's.
//
// The frame form: ONE launch of one workgroup — one stream operation whatever n, n_poses and max_iter are — and no wait in the
// device form: the stop is decided on the device and is a word of the output.  The round's member bits and chunk sums live in
// ppose_tmp, the scratch of sc_polish_poses (the same layout, stream-ordered use).  The batch form: offsets -> pinned staging (the
// area and event every batch entry shares) -> device copy (enqueued) -> ONE launch, a workgroup per problem.  Nothing is read back
// by either.  Everything that can refuse a call is decided on the host before anything is enqueued.
#include "sc_ctx.hpp"
#include "sc_settle_check.hpp"

using namespace sc;

static_assert(sizeof(sc_settle_params) == 32, "sc_settle_params is 32 bytes");

namespace {

// ---- the frame form: the refusals both entries share, then "is there a frame"; `who` opens the message
int stl_frame_check(sc_ctx* c, const sc_settle_params* sp, uint32_t pose_stride, uint32_t n_poses, const void* sel, const char* who) {
  SC_TRY(busy(c));
  if (const char* what = settle_params_error(sp, pose_stride, n_poses, false, sel != nullptr)) return refuse(c, who, what);
  return scored_frame_begin(c, who);
}

// the scratch has its room (the caller's last ENSURE): the launch
int stl_frame_enqueue(sc_ctx* c, const sc_settle_params* sp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                      const uint8_t* d_sel, sc_polish_batch_result* d_pol, int32_t* d_label, float* d_d2, uint32_t* d_rounds) {
  const Pass& ps = c->pass;
  SettleFrameJob job{};
  job.pts = points_of(c);
  job.tau2 = ps.dv.tau2;
  job.thr = score_thr(ps.dv, ps.params.score_mode);
  job.score_mode = ps.params.score_mode;
  job.max_iter = sp->max_iter; job.n_poses = n_poses;
  job.pose = d_pose; job.pose_stride = pose_stride;
  job.status = settle_reads_status(sp, false);
  job.sel = sp->sel_mode == SC_ASSIGN_SEL_MASK ? d_sel : nullptr;
  job.scratch = c->ppose_tmp.as<double>();
  job.out = reinterpret_cast<PolishBatchRecord*>(d_pol);
  job.label = d_label; job.d2 = d_d2; job.rounds = d_rounds;
  launch_settle_frame(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// ---- the batch form: the refusals both entries share
int stl_batch_check(sc_ctx* c, const uint32_t* offset, uint32_t n_problems, const sc_params* p, const sc_settle_params* sp,
                    uint32_t pose_stride, uint32_t n_poses, const char* who) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(batch_params_check(c, p, who));
  if (const char* what = settle_params_error(sp, pose_stride, n_poses, true, false)) return refuse(c, who, what);
  if (const char* what = batch_offsets_error(offset, n_problems)) return refuse(c, who, what);
  return SC_OK;
}

int stl_batch_enqueue(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                      const sc_settle_params* sp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                      sc_polish_batch_result* d_pol, int32_t* d_label, uint32_t* d_rounds) {
  SC_TRY(batch_offsets_to_device(c, offset, n_problems, c->stl_off));
  const Derived dv = derive(p);
  SettleBatchJob job{};
  job.src = d_src; job.tgt = d_tgt; job.offset = c->stl_off.as<uint32_t>();
  job.n_problems = n_problems; job.total = offset[n_problems];
  job.soa = p->layout == SC_SOA; job.score_mode = p->score_mode;
  job.tau2 = dv.tau2; job.thr = score_thr(dv, p->score_mode);
  job.max_iter = sp->max_iter; job.n_poses = n_poses;
  job.pose = d_pose; job.pose_stride = pose_stride;
  job.out = reinterpret_cast<PolishBatchRecord*>(d_pol);
  job.label = d_label; job.rounds = d_rounds;
  launch_settle_batch(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_settle_default_params(sc_settle_params* sp) {
  if (!sp) return SC_EINVAL;
  memset(sp, 0, sizeof(*sp));
  sp->size = sizeof(sc_settle_params);
  sp->max_iter = 16;
  return SC_OK;
}

int sc_settle_poses_frame_device(sc_ctx* c, const sc_settle_params* sp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                                 const uint8_t* d_sel, sc_polish_batch_result* d_pol, int32_t* d_label, float* d_d2, uint32_t* d_rounds) {
  static const char* const who = "sc_settle_poses_frame_device";
  if (!c) return SC_EINVAL;
  if (!sp || !d_pose || !d_pol || !d_label) return refuse(c, who, "a NULL argument");
  SC_TRY(stl_frame_check(c, sp, pose_stride, n_poses, d_sel, who));
  ENSURE(c, c->ppose_tmp, (size_t)n_poses * polish_poses_scratch_bytes(c->pass.n));
  return stl_frame_enqueue(c, sp, d_pose, pose_stride, n_poses, d_sel, d_pol, d_label, d_d2, d_rounds);  // (no wait: the outputs are complete in stream order)
}

int sc_settle_poses_frame(sc_ctx* c, const sc_settle_params* sp, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                          const uint8_t* sel, sc_polish_batch_result* pol, int32_t* label, float* d2, uint32_t* rounds) {
  static const char* const who = "sc_settle_poses_frame";
  if (!c) return SC_EINVAL;
  if (!sp || !pose || !pol || !label) return refuse(c, who, "a NULL argument");
  SC_TRY(stl_frame_check(c, sp, pose_stride, n_poses, sel, who));
  const size_t n = (size_t)c->pass.n;
  const bool masked = sp->sel_mode == SC_ASSIGN_SEL_MASK;
  HostArrays h(c);
  h.in(c->stl_pose, pose, (size_t)settle_pose_bytes(n_poses, pose_stride, sp, false));
  if (masked) h.in(c->stl_sel, sel, n);
  h.out(c->stl_out, pol, (size_t)n_poses * sizeof(sc_polish_batch_result));
  h.out(c->stl_label, label, n * 4);
  if (d2) h.out(c->stl_d2, d2, n * 4);
  if (rounds) h.out(c->stl_rounds, rounds, 8);
  SC_TRY(h.room());
  ENSURE(c, c->ppose_tmp, (size_t)n_poses * polish_poses_scratch_bytes(c->pass.n));
  SC_TRY(h.send());
  SC_TRY(stl_frame_enqueue(c, sp, c->stl_pose.p, pose_stride, n_poses, masked ? c->stl_sel.as<uint8_t>() : nullptr,
                           c->stl_out.as<sc_polish_batch_result>(), c->stl_label.as<int32_t>(), d2 ? c->stl_d2.as<float>() : nullptr,
                           rounds ? c->stl_rounds.as<uint32_t>() : nullptr));
  SC_TRY(h.fetch());
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

int sc_settle_poses_batch_device(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                                 const sc_params* p, const sc_settle_params* sp, const void* d_pose, uint32_t pose_stride,
                                 uint32_t n_poses, sc_polish_batch_result* d_pol, int32_t* d_label, uint32_t* d_rounds) {
  static const char* const who = "sc_settle_poses_batch_device";
  if (!c) return SC_EINVAL;
  if (!d_src || !d_tgt || !offset || !p || !sp || !d_pose || !d_pol || !d_label) return refuse(c, who, "a NULL argument");
  SC_TRY(stl_batch_check(c, offset, n_problems, p, sp, pose_stride, n_poses, who));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  return stl_batch_enqueue(c, d_src, d_tgt, offset, n_problems, p, sp, d_pose, pose_stride, n_poses, d_pol, d_label, d_rounds);
}

int sc_settle_poses_batch(sc_ctx* c, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                          const sc_settle_params* sp, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                          sc_polish_batch_result* pol, int32_t* label, uint32_t* rounds) {
  static const char* const who = "sc_settle_poses_batch";
  if (!c) return SC_EINVAL;
  if (!src || !tgt || !offset || !p || !sp || !pose || !pol || !label) return refuse(c, who, "a NULL argument");
  SC_TRY(stl_batch_check(c, offset, n_problems, p, sp, pose_stride, n_poses, who));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  const size_t total = offset[n_problems], pts = total * 12, records = (size_t)n_poses * n_problems;
  HostArrays h(c);
  h.in(c->stl_src, src, pts);
  h.in(c->stl_tgt, tgt, pts);
  h.in(c->stl_pose, pose, (size_t)settle_pose_bytes(records, pose_stride, sp, true));
  h.out(c->stl_out, pol, records * sizeof(sc_polish_batch_result));
  h.out(c->stl_label, label, total * 4);
  if (rounds) h.out(c->stl_rounds, rounds, (size_t)n_problems * 8);
  SC_TRY(h.room());
  SC_TRY(h.send());
  SC_TRY(stl_batch_enqueue(c, c->stl_src.as<float>(), c->stl_tgt.as<float>(), offset, n_problems, p, sp, c->stl_pose.p, pose_stride, n_poses,
                           c->stl_out.as<sc_polish_batch_result>(), c->stl_label.as<int32_t>(), rounds ? c->stl_rounds.as<uint32_t>() : nullptr));
  return h.fetch();
}

}  // extern "C"
