// sc_capi_merge.hip — the C ABI's folding of duplicate poses (include/saccot.h, sc_merge_poses): sc_merge_default_params,
// sc_merge_poses_frame_device, sc_merge_poses_frame, sc_merge_poses_batch_device and sc_merge_poses_batch.  Host-only, on the
// context and the helpers of sc_ctx.hpp and sc_capi_pose.hpp; the kernels are sc_merge_frame.hip's and sc_merge_batch.hip's, the
// rules of the parameters sc_merge_check.hpp's.
//
// The frame form: a memset of the tally words, then THREE launches — support, overlap, decide — four stream operations whatever n
// and n_poses are, and no wait in the device form: the fold is decided on the device.  The bit rows and the tally words live in
// mrg_rows, the overlap table in the caller's array or in mrg_table.  The batch form: offsets -> pinned staging (the area and event
// every batch entry shares) -> device copy (enqueued) -> ONE launch, a workgroup per problem.  Nothing is read back by either.
// Everything that can refuse a call is decided on the host before anything is enqueued.
#include "sc_capi_pose.hpp"
#include "sc_merge_check.hpp"

using namespace sc;

static_assert(sizeof(sc_merge_params) == 32 && sizeof(sc_merge_pose) == 64, "sc_merge_params is 32 bytes, sc_merge_pose 64");

namespace {

MergeRule rule_of(const sc_merge_params* mp) {
  return MergeRule{mp->measure, mp->num, mp->den, mp->min_count, (mp->flags & SC_MERGE_COMPACT) != 0};
}

// ---- the frame form (its scratch: mrg_rows, and mrg_table where the caller passes no table)
int mrg_frame_room(sc_ctx* c, uint32_t n_poses, bool own_table) {
  ENSURE(c, c->mrg_rows, (size_t)merge_scratch_bytes((uint64_t)c->pass.n, n_poses));
  if (own_table) ENSURE(c, c->mrg_table, (size_t)merge_table_bytes(n_poses));
  return SC_OK;
}
// the scratch has its room: the memset and the three launches
int mrg_frame_enqueue(sc_ctx* c, const sc_merge_params* mp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                      const uint8_t* d_sel, sc_merge_pose* d_out, int32_t* d_parent, uint32_t* d_overlap, uint32_t* d_count) {
  MergeFrameJob job{};
  pose_frame_head(c, &job, d_pose, pose_stride, n_poses, merge_reads_status(mp, false));
  job.sel = mp->sel_mode == SC_ASSIGN_SEL_MASK ? d_sel : nullptr;
  job.rule = rule_of(mp);
  job.rows = c->mrg_rows.as<uint64_t>();
  job.tally = reinterpret_cast<uint32_t*>(static_cast<char*>(c->mrg_rows.p) + merge_rows_bytes((uint64_t)c->pass.n, n_poses));
  job.overlap = d_overlap ? d_overlap : c->mrg_table.as<uint32_t>();
  job.out = reinterpret_cast<MergeRecord*>(d_out);
  job.parent = d_parent; job.count = d_count;
  HIPCHK(c, hipMemsetAsync(job.tally, 0, (size_t)n_poses * 8, c->stream));  // the workgroups add their tallies into it
  launch_merge_frame(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// ---- the batch form
int mrg_batch_enqueue(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                      const sc_merge_params* mp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses, sc_merge_pose* d_out,
                      int32_t* d_parent, uint32_t* d_count) {
  MergeBatchJob job{};
  SC_TRY(pose_batch_head(c, &job, c->mrg_off, d_src, d_tgt, offset, n_problems, p, d_pose, pose_stride, n_poses));
  job.rule = rule_of(mp);
  job.out = reinterpret_cast<MergeRecord*>(d_out);
  job.parent = d_parent; job.count = d_count;
  launch_merge_batch(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_merge_default_params(sc_merge_params* mp) {
  if (!mp) return SC_EINVAL;
  memset(mp, 0, sizeof(*mp));
  mp->size = sizeof(sc_merge_params);
  mp->measure = SC_MERGE_OVER_MIN;
  mp->num = 1; mp->den = 2;
  return SC_OK;
}

int sc_merge_poses_frame_device(sc_ctx* c, const sc_merge_params* mp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                                const uint8_t* d_sel, sc_merge_pose* d_out, int32_t* d_parent, uint32_t* d_overlap, uint32_t* d_count) {
  static const char* const who = "sc_merge_poses_frame_device";
  if (!c) return SC_EINVAL;
  if (!mp || !d_pose || !d_out || !d_parent) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_frame_check(c, who, merge_params_error(mp, pose_stride, n_poses, false, d_sel != nullptr)));
  SC_TRY(mrg_frame_room(c, n_poses, d_overlap == nullptr));
  return mrg_frame_enqueue(c, mp, d_pose, pose_stride, n_poses, d_sel, d_out, d_parent, d_overlap, d_count);  // (no wait: the outputs are complete in stream order)
}

int sc_merge_poses_frame(sc_ctx* c, const sc_merge_params* mp, const void* pose, uint32_t pose_stride, uint32_t n_poses,
                         const uint8_t* sel, sc_merge_pose* out, int32_t* parent, uint32_t* overlap, uint32_t* count) {
  static const char* const who = "sc_merge_poses_frame";
  if (!c) return SC_EINVAL;
  if (!mp || !pose || !out || !parent) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_frame_check(c, who, merge_params_error(mp, pose_stride, n_poses, false, sel != nullptr)));
  const size_t n = (size_t)c->pass.n;
  const bool masked = mp->sel_mode == SC_ASSIGN_SEL_MASK;
  HostArrays h(c);  // the family's list: src, tgt, pose, sel, out, parent, overlap, count
  h.absent(2);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(n_poses, pose_stride, merge_reads_status(mp, false)));
  const int a_sel = h.in(masked ? sel : nullptr, n);
  const int a_out = h.out(out, (size_t)n_poses * sizeof(sc_merge_pose)), a_parent = h.out(parent, (size_t)n_poses * 4);
  const int a_overlap = h.out(overlap, (size_t)merge_table_bytes(n_poses)), a_count = h.out(count, 8);
  h.also(c->mrg_rows, (size_t)merge_scratch_bytes(n, n_poses));
  if (!overlap) h.also(c->mrg_table, (size_t)merge_table_bytes(n_poses));
  return h.run([&] {
    return mrg_frame_enqueue(c, mp, h.at<void>(a_pose), pose_stride, n_poses, h.at<uint8_t>(a_sel), h.at<sc_merge_pose>(a_out),
                             h.at<int32_t>(a_parent), h.at<uint32_t>(a_overlap), h.at<uint32_t>(a_count));
  });
}

int sc_merge_poses_batch_device(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                                const sc_params* p, const sc_merge_params* mp, const void* d_pose, uint32_t pose_stride, uint32_t n_poses,
                                sc_merge_pose* d_out, int32_t* d_parent, uint32_t* d_count) {
  static const char* const who = "sc_merge_poses_batch_device";
  if (!c) return SC_EINVAL;
  if (!d_src || !d_tgt || !offset || !p || !mp || !d_pose || !d_out || !d_parent) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_batch_check(c, who, p, merge_params_error(mp, pose_stride, n_poses, true, false), offset, n_problems));
  return mrg_batch_enqueue(c, d_src, d_tgt, offset, n_problems, p, mp, d_pose, pose_stride, n_poses, d_out, d_parent, d_count);
}

int sc_merge_poses_batch(sc_ctx* c, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                         const sc_merge_params* mp, const void* pose, uint32_t pose_stride, uint32_t n_poses, sc_merge_pose* out,
                         int32_t* parent, uint32_t* count) {
  static const char* const who = "sc_merge_poses_batch";
  if (!c) return SC_EINVAL;
  if (!src || !tgt || !offset || !p || !mp || !pose || !out || !parent) return refuse(c, who, "a NULL argument");
  SC_TRY(pose_batch_check(c, who, p, merge_params_error(mp, pose_stride, n_poses, true, false), offset, n_problems));
  const size_t total = offset[n_problems], pts = total * 12, records = (size_t)n_poses * n_problems;
  HostArrays h(c);  // the family's list: src, tgt, pose, sel, out, parent, overlap, count
  const int a_src = h.in(src, pts), a_tgt = h.in(tgt, pts);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(records, pose_stride, true));
  h.absent();
  const int a_out = h.out(out, records * sizeof(sc_merge_pose)), a_parent = h.out(parent, records * 4);
  h.absent();
  const int a_count = h.out(count, (size_t)n_problems * 8);
  h.also(c->mrg_off, batch_offsets_bytes(n_problems));
  return h.run([&] {
    return mrg_batch_enqueue(c, h.at<float>(a_src), h.at<float>(a_tgt), offset, n_problems, p, mp, h.at<void>(a_pose), pose_stride, n_poses,
                             h.at<sc_merge_pose>(a_out), h.at<int32_t>(a_parent), h.at<uint32_t>(a_count));
  });
}

}  // extern "C"
