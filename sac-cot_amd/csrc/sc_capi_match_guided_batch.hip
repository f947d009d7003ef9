// sc_capi_match_guided_batch.hip — the C ABI's pose-gated matching for batches and pairs (include/saccot.h, sc_match_guided_batch):
// sc_match_guided_batch_device, sc_match_guided_batch, sc_register_guided_batch_features_device and the pairs forms
// sc_match_guided_pairs_device, sc_match_guided_pairs, sc_register_guided_pairs_features_device.  Host-only, on the context and the
// helpers of sc_ctx.hpp; the kernels are the guided instantiations of sc_match_batch.hip, and sc_batch.hip's kernel on the slots.
//
// The sequence is the unguided forms' (sc_capi_match_batch.hip, sc_capi_pairs.hip): mbatch_check / pairs_check, mbatch_room,
// mbatch_enqueue — the staging copy, the memset, the two launches —, mbatch_register.  What these entries add is decided on the host
// before anything is enqueued (the guide block, the pose stride: sc_match_guided_batch_check.hpp) and travels in the job's
// MatchBatchGuide: the points, the pose records, gate2, the optional g2.  The pose records are read by the two match launches only,
// so a features entry's d_pose may be the d_res that its registration launch, enqueued behind them, overwrites.
#include "sc_ctx.hpp"
#include "sc_match_guided_batch_check.hpp"
#include "sc_pairs_check.hpp"

using namespace sc;

namespace {

using Sizes = MatchBatchSizes;

// the rules of the guide block and of the pose stride -> the guide but for its pointers
int guide_check(sc_ctx* c, const char* who, const sc_guide_params* gp, uint32_t pose_stride, MatchBatchGuide* gd) {
  if (const char* why = guide_batch_params_error(gp)) return refuse(c, who, why);
  if (const char* why = guide_pose_stride_error(gp->flags, pose_stride)) return refuse(c, who, why);
  gd->gate2 = guide_gate2(gp->gate);
  gd->pose_stride = pose_stride;
  gd->use_status = (gp->flags & SC_GUIDE_POSE_STATUS) ? 1u : 0u;
  return SC_OK;
}
// the points of both sides in the guide's layout (src_rows / tgt_rows of them), the pose records and g2
void guide_inputs(MatchBatchGuide* gd, const float* src, size_t src_rows, const float* tgt, size_t tgt_rows, uint32_t layout, const void* d_pose,
                  float* d_g2) {
  guide_points(gd, src, src_rows, tgt, tgt_rows, layout);
  gd->pose = d_pose; gd->g2 = d_g2;
}

// the guided match on packed problems (mbatch_room has been called; gd is complete).  p: a features entry's sc_params, for the
// gather into mbatch_gsrc / _gtgt (nullptr: the match alone)
int packed_match(sc_ctx* c, const MatchJob& mj, const Sizes& sz, const MatchBatchGuide& gd, const float* d_fsrc, const float* d_ftgt,
                 const uint32_t* src_off, const uint32_t* tgt_off, int32_t* d_corr, float* d_d2, uint32_t* d_count, const sc_params* p = nullptr) {
  const uint32_t* meta = c->mbatch_meta.as<uint32_t>();
  MatchGuidedBatchJob job{};
  job.fsrc = d_fsrc; job.ftgt = d_ftgt;
  job.src_off = meta; job.tgt_off = meta + (size_t)sz.n_problems + 1; job.slot = meta + sz.meta.slot_at;
  job.gd = gd;
  const MatchGather g = p ? gather_of(gd.src, (uint32_t)sz.total_s, gd.tgt, (uint32_t)sz.total_t, p->layout, c->mbatch_gsrc.as<float>(),
                                      c->mbatch_gtgt.as<float>())
                          : MatchGather{};
  return mbatch_enqueue(
      c, mj, sz, job, [&](uint32_t* h) { match_batch_meta_fill(src_off, tgt_off, sz.n_problems, mj.knn, MATCH_BATCH_ROWS, sz.meta, h); },
      d_corr, d_d2, d_count, g);
}

// the same on listed pairs of the table (`total` rows: gd.src == gd.tgt are its points)
int pairs_match(sc_ctx* c, const MatchJob& mj, const Sizes& sz, const MatchBatchGuide& gd, const float* d_feat, const uint32_t* set_off,
                const uint32_t* pairs, uint32_t total, int32_t* d_corr, float* d_d2, uint32_t* d_count, const sc_params* p = nullptr) {
  MatchGuidedPairsJob job{};
  job.feat = d_feat;
  job.rec = c->mbatch_meta.as<uint32_t>();
  job.gd = gd;
  const MatchGather g = p ? gather_of(gd.src, total, gd.tgt, total, p->layout, c->mbatch_gsrc.as<float>(), c->mbatch_gtgt.as<float>()) : MatchGather{};
  return mbatch_enqueue(
      c, mj, sz, job, [&](uint32_t* h) { pairs_meta_fill(set_off, pairs, sz.n_problems, mj.knn, MATCH_BATCH_ROWS, sz.meta, h); },
      d_corr, d_d2, d_count, g);
}

}  // namespace

extern "C" {

int sc_match_guided_batch_device(sc_ctx* c, const float* d_src_pts, const float* d_fsrc, const uint32_t* src_off, const float* d_tgt_pts,
                                 const float* d_ftgt, const uint32_t* tgt_off, uint32_t n_problems, const sc_match_params* mp,
                                 const sc_guide_params* gp, const void* d_pose, uint32_t pose_stride, int32_t* d_corr, float* d_d2,
                                 float* d_g2, uint32_t* d_count) {
  static const char* const who = "sc_match_guided_batch_device";
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, d_src_pts); SC_NOT_NULL(c, who, d_fsrc); SC_NOT_NULL(c, who, src_off); SC_NOT_NULL(c, who, d_tgt_pts);
  SC_NOT_NULL(c, who, d_ftgt); SC_NOT_NULL(c, who, tgt_off); SC_NOT_NULL(c, who, mp); SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, d_pose);
  SC_NOT_NULL(c, who, d_corr); SC_NOT_NULL(c, who, d_d2); SC_NOT_NULL(c, who, d_count);
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(mbatch_check(c, src_off, tgt_off, n_problems, mp, nullptr, nullptr, &mj, &sz));
  MatchBatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, pose_stride, &gd));
  HIPCHK(c, hipSetDevice(c->device));
  SC_TRY(mbatch_room(c, mj, sz, false));
  guide_inputs(&gd, d_src_pts, sz.total_s, d_tgt_pts, sz.total_t, gp->layout, d_pose, d_g2);
  return packed_match(c, mj, sz, gd, d_fsrc, d_ftgt, src_off, tgt_off, d_corr, d_d2, d_count);
}

int sc_match_guided_batch(sc_ctx* c, const float* src_pts, const float* fsrc, const uint32_t* src_off, const float* tgt_pts,
                          const float* ftgt, const uint32_t* tgt_off, uint32_t n_problems, const sc_match_params* mp,
                          const sc_guide_params* gp, const void* pose, uint32_t pose_stride, int32_t* corr, float* d2, float* g2,
                          uint32_t* count) {
  static const char* const who = "sc_match_guided_batch";
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, src_pts); SC_NOT_NULL(c, who, fsrc); SC_NOT_NULL(c, who, src_off); SC_NOT_NULL(c, who, tgt_pts);
  SC_NOT_NULL(c, who, ftgt); SC_NOT_NULL(c, who, tgt_off); SC_NOT_NULL(c, who, mp); SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, pose);
  SC_NOT_NULL(c, who, corr); SC_NOT_NULL(c, who, d2); SC_NOT_NULL(c, who, count);
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(mbatch_check(c, src_off, tgt_off, n_problems, mp, nullptr, nullptr, &mj, &sz));
  MatchBatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, pose_stride, &gd));
  HIPCHK(c, hipSetDevice(c->device));
  SC_TRY(mbatch_room(c, mj, sz, false));
  HostArrays h(c);
  const MatchBatchArrays a = mbatch_arrays(h, sz, mj.dim, fsrc, sz.total_s, ftgt, sz.total_t, src_pts, tgt_pts, corr, d2, count);
  const int a_pose = h.in(pose, (size_t)n_problems * pose_stride);  // the records as given
  const int a_g2 = h.out(g2, sz.slots * 4);                         // fetched only when asked for
  return h.run([&] {
    guide_inputs(&gd, h.at<float>(a.psrc), sz.total_s, h.at<float>(a.ptgt), sz.total_t, gp->layout, h.at<void>(a_pose), h.at<float>(a_g2));
    return packed_match(c, mj, sz, gd, h.at<float>(a.fsrc), h.at<float>(a.ftgt), src_off, tgt_off, h.at<int32_t>(a.corr), h.at<float>(a.d2),
                        h.at<uint32_t>(a.count));
  });
}

int sc_register_guided_batch_features_device(sc_ctx* c, const float* d_src_pts, const float* d_fsrc, const uint32_t* src_off,
                                             const float* d_tgt_pts, const float* d_ftgt, const uint32_t* tgt_off, uint32_t n_problems,
                                             const sc_match_params* mp, const sc_guide_params* gp, const void* d_pose,
                                             uint32_t pose_stride, const sc_params* p, sc_batch_result* d_res, int32_t* d_corr,
                                             float* d_d2, float* d_g2, uint32_t* d_count, uint8_t* d_mask) {
  static const char* const who = "sc_register_guided_batch_features_device";
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, d_src_pts); SC_NOT_NULL(c, who, d_fsrc); SC_NOT_NULL(c, who, src_off); SC_NOT_NULL(c, who, d_tgt_pts);
  SC_NOT_NULL(c, who, d_ftgt); SC_NOT_NULL(c, who, tgt_off); SC_NOT_NULL(c, who, mp); SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, d_pose);
  SC_NOT_NULL(c, who, p); SC_NOT_NULL(c, who, d_res); SC_NOT_NULL(c, who, d_corr); SC_NOT_NULL(c, who, d_d2); SC_NOT_NULL(c, who, d_count);
  SC_NOT_NULL(c, who, d_mask);
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(mbatch_check(c, src_off, tgt_off, n_problems, mp, p, "sc_register_guided_batch_features", &mj, &sz));
  MatchBatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, pose_stride, &gd));
  SC_TRY(layouts_agree(c, who, gp, p));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  SC_TRY(mbatch_room(c, mj, sz, true));
  guide_inputs(&gd, d_src_pts, sz.total_s, d_tgt_pts, sz.total_t, gp->layout, d_pose, d_g2);
  SC_TRY(packed_match(c, mj, sz, gd, d_fsrc, d_ftgt, src_off, tgt_off, d_corr, d_d2, d_count, p));
  return mbatch_register(c, sz, p, d_count, d_res, d_mask);
}

int sc_match_guided_pairs_device(sc_ctx* c, const float* d_pts, const float* d_feat, const uint32_t* set_off, uint32_t n_sets,
                                 const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp, const sc_guide_params* gp,
                                 const void* d_pose, uint32_t pose_stride, int32_t* d_corr, float* d_d2, float* d_g2, uint32_t* d_count) {
  static const char* const who = "sc_match_guided_pairs_device";
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, d_pts); SC_NOT_NULL(c, who, d_feat); SC_NOT_NULL(c, who, set_off); SC_NOT_NULL(c, who, pairs); SC_NOT_NULL(c, who, mp);
  SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, d_pose); SC_NOT_NULL(c, who, d_corr); SC_NOT_NULL(c, who, d_d2); SC_NOT_NULL(c, who, d_count);
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(pairs_check(c, set_off, n_sets, pairs, n_pairs, mp, nullptr, nullptr, &mj, &sz));
  MatchBatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, pose_stride, &gd));
  HIPCHK(c, hipSetDevice(c->device));
  SC_TRY(mbatch_room(c, mj, sz, false));
  const uint32_t total = set_off[n_sets];
  guide_inputs(&gd, d_pts, total, d_pts, total, gp->layout, d_pose, d_g2);  // both sides of a pair are rows of the one table
  return pairs_match(c, mj, sz, gd, d_feat, set_off, pairs, total, d_corr, d_d2, d_count);
}

int sc_match_guided_pairs(sc_ctx* c, const float* pts, const float* feat, const uint32_t* set_off, uint32_t n_sets, const uint32_t* pairs,
                          uint32_t n_pairs, const sc_match_params* mp, const sc_guide_params* gp, const void* pose, uint32_t pose_stride,
                          int32_t* corr, float* d2, float* g2, uint32_t* count) {
  static const char* const who = "sc_match_guided_pairs";
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, pts); SC_NOT_NULL(c, who, feat); SC_NOT_NULL(c, who, set_off); SC_NOT_NULL(c, who, pairs); SC_NOT_NULL(c, who, mp);
  SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, pose); SC_NOT_NULL(c, who, corr); SC_NOT_NULL(c, who, d2); SC_NOT_NULL(c, who, count);
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(pairs_check(c, set_off, n_sets, pairs, n_pairs, mp, nullptr, nullptr, &mj, &sz));
  MatchBatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, pose_stride, &gd));
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t total = set_off[n_sets];
  SC_TRY(mbatch_room(c, mj, sz, false));
  HostArrays h(c);
  // the table, descriptors and points: one copy of each serves both sides
  const MatchBatchArrays a = mbatch_arrays(h, sz, mj.dim, feat, total, nullptr, 0, pts, nullptr, corr, d2, count);
  const int a_pose = h.in(pose, (size_t)n_pairs * pose_stride);  // the records as given
  const int a_g2 = h.out(g2, sz.slots * 4);                      // fetched only when asked for
  return h.run([&] {
    guide_inputs(&gd, h.at<float>(a.psrc), total, h.at<float>(a.psrc), total, gp->layout, h.at<void>(a_pose), h.at<float>(a_g2));
    return pairs_match(c, mj, sz, gd, h.at<float>(a.fsrc), set_off, pairs, total, h.at<int32_t>(a.corr), h.at<float>(a.d2), h.at<uint32_t>(a.count));
  });
}

int sc_register_guided_pairs_features_device(sc_ctx* c, const float* d_pts, const float* d_feat, const uint32_t* set_off, uint32_t n_sets,
                                             const uint32_t* pairs, uint32_t n_pairs, const sc_match_params* mp, const sc_guide_params* gp,
                                             const void* d_pose, uint32_t pose_stride, const sc_params* p, sc_batch_result* d_res,
                                             int32_t* d_corr, float* d_d2, float* d_g2, uint32_t* d_count, uint8_t* d_mask) {
  static const char* const who = "sc_register_guided_pairs_features_device";
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, d_pts); SC_NOT_NULL(c, who, d_feat); SC_NOT_NULL(c, who, set_off); SC_NOT_NULL(c, who, pairs); SC_NOT_NULL(c, who, mp);
  SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, d_pose); SC_NOT_NULL(c, who, p); SC_NOT_NULL(c, who, d_res); SC_NOT_NULL(c, who, d_corr);
  SC_NOT_NULL(c, who, d_d2); SC_NOT_NULL(c, who, d_count); SC_NOT_NULL(c, who, d_mask);
  MatchJob mj{};
  Sizes sz{};
  SC_TRY(pairs_check(c, set_off, n_sets, pairs, n_pairs, mp, p, "sc_register_guided_pairs_features", &mj, &sz));
  MatchBatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, pose_stride, &gd));
  SC_TRY(layouts_agree(c, who, gp, p));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  SC_TRY(mbatch_room(c, mj, sz, true));
  const uint32_t total = set_off[n_sets];
  guide_inputs(&gd, d_pts, total, d_pts, total, gp->layout, d_pose, d_g2);
  SC_TRY(pairs_match(c, mj, sz, gd, d_feat, set_off, pairs, total, d_corr, d_d2, d_count, p));
  return mbatch_register(c, sz, p, d_count, d_res, d_mask);
}

}  // extern "C"
