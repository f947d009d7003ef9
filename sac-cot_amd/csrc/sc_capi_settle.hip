// sc_capi_settle.hip — the C ABI's relabel-and-refit loop (include/saccot.h, sc_settle_poses): sc_settle_default_params,
// sc_settle_poses_frame_device, sc_settle_poses_frame, sc_settle_poses_batch_device and sc_settle_poses_batch.  Host-only, on the
// context and the helpers of sc_ctx.hpp; the kernels are sc_settle_frame.hip's and sc_settle_batch.hip's, the rules of the
// parameters sc_settle_check.hpp's.
//
// The frame form: ONE launch of one workgroup — one stream operation whatever n, n_poses and max_iter are — and no wait in the
// device form: the stop is decided on the device and is a word of the output.  The round's member bits and chunk sums live in
// ppose_tmp, the scratch of sc_polish_poses (one layout: sc_chunks.hpp; stream-ordered use).  The batch form: offsets -> pinned staging (the
// area and event every batch entry shares) -> device copy (enqueued) -> ONE launch, a workgroup per problem.  Nothing is read back
// by either.  Everything that can refuse a call is decided on the host before anything is enqueued.
#include "sc_capi_pose.hpp"
#include "sc_settle_check.hpp"

using namespace sc;

static_assert(sizeof(sc_settle_params) == 32, "sc_settle_params is 32 bytes");

namespace {

// ---- the frame form (its scratch: ppose_tmp)
// the scratch has its room (the caller's last ENSURE): the launch
int stl_frame_enqueue(sc_ctx* c, const sc_settle_params* sp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                      const uint8_t* d_sel, sc_polish_batch_result* d_pol, int32_t* d_label, float* d_d2, uint32_t* d_rounds) {
  SettleFrameJob job{};
  pose_frame_head(c, &job, d_pose, pose_stride, n_poses, settle_reads_status(sp, false));
  job.max_iter = sp->max_iter;
  job.sel = sp->sel_mode == SC_ASSIGN_SEL_MASK ? d_sel : nullptr;
  job.scratch = c->ppose_tmp.as<double>();
  job.out = reinterpret_cast<PolishBatchRecord*>(d_pol);
  job.label = d_label; job.d2 = d_d2; job.rounds = d_rounds;
  launch_settle_frame(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// ---- the batch form
int stl_batch_enqueue(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                      const sc_settle_params* sp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                      sc_polish_batch_result* d_pol, int32_t* d_label, uint32_t* d_rounds) {
  SettleBatchJob job{};
  SC_TRY(pose_batch_head(c, &job, c->stl_off, d_src, d_tgt, offset, n_problems, p, d_pose, pose_stride, n_poses));
  job.max_iter = sp->max_iter;
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
  SC_TRY(pose_frame_check(c, who, settle_params_error(sp, pose_stride, n_poses, false, d_sel != nullptr)));
  ENSURE(c, c->ppose_tmp, pose_frame_scratch_bytes(c, n_poses));
  return stl_frame_enqueue(c, sp, d_pose, pose_stride, n_poses, d_sel, d_pol, d_label, d_d2, d_rounds);  // (no wait: the outputs are complete in stream order)
}

int sc_settle_poses_frame(sc_ctx* c, const sc_settle_params* sp, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                          const uint8_t* sel, sc_polish_batch_result* pol, int32_t* label, float* d2, uint32_t* rounds) {
  static const char* const who = "sc_settle_poses_frame";
  if (!c) return SC_EINVAL;
  if (!sp || !pose || !pol || !label) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_frame_check(c, who, settle_params_error(sp, pose_stride, n_poses, false, sel != nullptr)));
  const size_t n = (size_t)c->pass.n;
  const bool masked = sp->sel_mode == SC_ASSIGN_SEL_MASK;
  HostArrays h(c);  // the family's list: src, tgt, pose, sel, pol, label, d2, rounds
  h.absent(2);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(n_poses, pose_stride, settle_reads_status(sp, false)));
  const int a_sel = h.in(masked ? sel : nullptr, n);
  const int a_pol = h.out(pol, (size_t)n_poses * sizeof(sc_polish_batch_result));
  const int a_label = h.out(label, n * 4), a_d2 = h.out(d2, n * 4), a_rounds = h.out(rounds, 8);
  h.also(c->ppose_tmp, pose_frame_scratch_bytes(c, n_poses));
  return h.run([&] {
    return stl_frame_enqueue(c, sp, h.at<void>(a_pose), pose_stride, n_poses, h.at<uint8_t>(a_sel), h.at<sc_polish_batch_result>(a_pol),
                             h.at<int32_t>(a_label), h.at<float>(a_d2), h.at<uint32_t>(a_rounds));
  });
}

int sc_settle_poses_batch_device(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                                 const sc_params* p, const sc_settle_params* sp, const void* d_pose, uint32_t pose_stride,
                                 uint32_t n_poses, sc_polish_batch_result* d_pol, int32_t* d_label, uint32_t* d_rounds) {
  static const char* const who = "sc_settle_poses_batch_device";
  if (!c) return SC_EINVAL;
  if (!d_src || !d_tgt || !offset || !p || !sp || !d_pose || !d_pol || !d_label) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_batch_check(c, who, p, settle_params_error(sp, pose_stride, n_poses, true, false), offset, n_problems));
  return stl_batch_enqueue(c, d_src, d_tgt, offset, n_problems, p, sp, d_pose, pose_stride, n_poses, d_pol, d_label, d_rounds);
}

int sc_settle_poses_batch(sc_ctx* c, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                          const sc_settle_params* sp, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                          sc_polish_batch_result* pol, int32_t* label, uint32_t* rounds) {
  static const char* const who = "sc_settle_poses_batch";
  if (!c) return SC_EINVAL;
  if (!src || !tgt || !offset || !p || !sp || !pose || !pol || !label) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_batch_check(c, who, p, settle_params_error(sp, pose_stride, n_poses, true, false), offset, n_problems));
  const size_t total = offset[n_problems], pts = total * 12, records = (size_t)n_poses * n_problems;
  HostArrays h(c);  // the family's list: src, tgt, pose, sel, pol, label, d2, rounds
  const int a_src = h.in(src, pts), a_tgt = h.in(tgt, pts);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(records, pose_stride, true));
  h.absent();
  const int a_pol = h.out(pol, records * sizeof(sc_polish_batch_result));
  const int a_label = h.out(label, total * 4);
  h.absent();
  const int a_rounds = h.out(rounds, (size_t)n_problems * 8);
  h.also(c->stl_off, batch_offsets_bytes(n_problems));
  return h.run([&] {
    return stl_batch_enqueue(c, h.at<float>(a_src), h.at<float>(a_tgt), offset, n_problems, p, sp, h.at<void>(a_pose), pose_stride, n_poses,
                             h.at<sc_polish_batch_result>(a_pol), h.at<int32_t>(a_label), h.at<uint32_t>(a_rounds));
  });
}

}  // extern "C"
