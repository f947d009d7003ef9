// sc_capi_match_guided_poses.hip — the C ABI's descriptor matching gated by several poses (include/saccot.h, sc_match_guided_poses):
// sc_match_guided_poses_device, sc_match_guided_poses and sc_register_guided_poses_features.  Host-only, on the context and on the
// steps of sc_capi_match.hip (sc_ctx.hpp: match_check, match_enqueue, match_host, match_register_gathered); the kernels are
// sc_match.hip's, with the gate of several poses.
//
// The sequence is sc_match_guided's — memset -> distance + select -> finish, no host wait; the host entries poll ONE word.  What
// these entries add is decided on the host before anything is enqueued (the guide block with SC_GUIDE_POSE_STATUS, the stride, the
// number of records: sc_match_guided_poses_check.hpp) and travels in the MatchGuide: the records' place in HBM, their stride, how
// many there are and whether they carry a status.  The host entries copy the records as given, in front of the memset.
#include "sc_ctx.hpp"
#include "sc_match_guided_poses_check.hpp"

using namespace sc;

namespace {

// the rules of the guide block, the stride and the number of records -> the guide but for its pointers
int poses_check(sc_ctx* c, const char* who, const sc_guide_params* gp, uint32_t pose_stride, uint32_t n_poses, MatchGuide* gd) {
  if (const char* why = guide_poses_error(gp, pose_stride, n_poses)) return refuse(c, who, why);
  gd->gate2 = guide_gate2(gp->gate);
  gd->pose_stride = pose_stride;
  gd->n_poses = n_poses;
  gd->use_status = (gp->flags & SC_GUIDE_POSE_STATUS) ? 1u : 0u;
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_match_guided_poses_device(sc_ctx* c, const float* d_src_pts, const float* d_fsrc, int64_t ns, const float* d_tgt_pts,
                                 const float* d_ftgt, int64_t nt, const sc_match_params* mp, const sc_guide_params* gp, const void* d_pose,
                                 uint32_t pose_stride, uint32_t n_poses, int32_t* d_corr, float* d_d2, float* d_g2, int32_t* d_label,
                                 uint32_t* d_count) {
  static const char* const who = "sc_match_guided_poses_device";
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, d_src_pts); SC_NOT_NULL(c, who, d_fsrc); SC_NOT_NULL(c, who, d_tgt_pts); SC_NOT_NULL(c, who, d_ftgt);
  SC_NOT_NULL(c, who, mp); SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, d_pose); SC_NOT_NULL(c, who, d_corr);
  SC_NOT_NULL(c, who, d_d2); SC_NOT_NULL(c, who, d_count);
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{d_fsrc, d_ftgt};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(poses_check(c, who, gp, pose_stride, n_poses, &gd));
  guide_points(&gd, d_src_pts, job.ns, d_tgt_pts, job.nt, gp->layout);
  gd.pose = d_pose;
  HIPCHK(c, hipSetDevice(c->device));
  MatchOut o{};
  o.corr = d_corr; o.d2 = d_d2; o.count = d_count; o.gd = &gd; o.g2 = d_g2; o.label = d_label;
  return match_enqueue(c, job, o);
}

int sc_match_guided_poses(sc_ctx* c, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts, const float* ftgt,
                          int64_t nt, const sc_match_params* mp, const sc_guide_params* gp, const void* pose, uint32_t pose_stride,
                          uint32_t n_poses, int32_t* corr, float* d2, float* g2, int32_t* label, uint32_t* n) {
  static const char* const who = "sc_match_guided_poses";
  if (n) *n = 0;
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, src_pts); SC_NOT_NULL(c, who, fsrc); SC_NOT_NULL(c, who, tgt_pts); SC_NOT_NULL(c, who, ftgt);
  SC_NOT_NULL(c, who, mp); SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, pose); SC_NOT_NULL(c, who, corr);
  SC_NOT_NULL(c, who, d2); SC_NOT_NULL(c, who, n);
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(poses_check(c, who, gp, pose_stride, n_poses, &gd));
  HIPCHK(c, hipSetDevice(c->device));
  MatchHost h{};
  h.fsrc = fsrc; h.ftgt = ftgt; h.src_pts = src_pts; h.tgt_pts = tgt_pts; h.gd = &gd; h.layout = gp->layout; h.pose = pose;
  h.corr = corr; h.d2 = d2; h.g2 = g2; h.label = label;
  uint32_t found = 0;
  SC_TRY(match_host(c, job, h, &found));
  *n = found;
  return SC_OK;
}

int sc_register_guided_poses_features(sc_ctx* c, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts,
                                      const float* ftgt, int64_t nt, const sc_match_params* mp, const sc_guide_params* gp, const void* pose,
                                      uint32_t pose_stride, uint32_t n_poses, const sc_params* p, float R[9], float t[3], int32_t* corr,
                                      float* d2, float* g2, int32_t* label, uint32_t* n, uint8_t* mask, sc_stats* stats) {
  static const char* const who = "sc_register_guided_poses_features";
  if (n) *n = 0;
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, src_pts); SC_NOT_NULL(c, who, fsrc); SC_NOT_NULL(c, who, tgt_pts); SC_NOT_NULL(c, who, ftgt);
  SC_NOT_NULL(c, who, mp); SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, pose); SC_NOT_NULL(c, who, p);
  SC_NOT_NULL(c, who, R); SC_NOT_NULL(c, who, t); SC_NOT_NULL(c, who, corr); SC_NOT_NULL(c, who, d2);
  SC_NOT_NULL(c, who, n); SC_NOT_NULL(c, who, mask);
  SC_TRY(entry_checks(c, p, ENDS_FRAME | NOT_BUSY | PARAMS | ONE_RANK));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(poses_check(c, who, gp, pose_stride, n_poses, &gd));
  SC_TRY(layouts_agree(c, who, gp, p));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  MatchHost h{};
  h.fsrc = fsrc; h.ftgt = ftgt; h.src_pts = src_pts; h.tgt_pts = tgt_pts; h.gd = &gd; h.layout = gp->layout; h.pose = pose; h.p = p;
  h.corr = corr; h.d2 = d2; h.g2 = g2; h.label = label;
  uint32_t found = 0;
  SC_TRY(match_host(c, job, h, &found));  // the one host wait between matching and registration
  *n = found;
  return match_register_gathered(c, p, found, R, t, mask, stats);
}

}  // extern "C"
