// sc_capi_match_guided_poses.hip — the C ABI's descriptor matching gated by several poses (include/saccot.h, sc_match_guided_poses):
// sc_match_guided_poses_device, sc_match_guided_poses and sc_register_guided_poses_features.  Host-only, on the context and on the
// steps of sc_capi_match.hip (sc_ctx.hpp: match_check, match_stage_host, guided_stage_points, match_enqueue, match_results_to_host);
// the kernels are sc_match.hip's, with the gate of several poses.
//
// The sequence is sc_match_guided's — memset -> distance + select -> finish, no host wait; the host entries poll ONE word.  What
// these entries add is decided on the host before anything is enqueued (the guide block with SC_GUIDE_POSE_STATUS, the stride, the
// number of records: sc_match_guided_poses_check.hpp) and travels in the MatchGuide: the records' place in HBM, their stride, how
// many there are and whether they carry a status.  The host entries copy the records as given, in front of the memset.
#include "sc_ctx.hpp"
#include "sc_match_guided_poses_check.hpp"

using namespace sc;

namespace {

// a refused NULL argument, named (the context is there: sc_last_error can say which)
#define GP_NOT_NULL(c, who, arg) do { if (!(arg)) return refuse((c), (who), #arg " is NULL"); } while (0)

// the rules of the guide block, the stride and the number of records -> the guide but for its pointers
int poses_check(sc_ctx* c, const char* who, const sc_guide_params* gp, uint32_t pose_stride, uint32_t n_poses, MatchGuide* gd) {
  if (const char* why = guide_poses_error(gp, pose_stride, n_poses)) return refuse(c, who, why);
  gd->gate2 = guide_gate2(gp->gate);
  gd->pose_stride = pose_stride;
  gd->n_poses = n_poses;
  gd->use_status = (gp->flags & SC_GUIDE_POSE_STATUS) ? 1u : 0u;
  return SC_OK;
}

// the host entries' pose records -> their device copy (enqueued), and room for the labels
int poses_stage_host(sc_ctx* c, const MatchJob& job, const void* pose, MatchGuide* gd) {
  const size_t bytes = (size_t)gd->n_poses * gd->pose_stride;
  ENSURE(c, c->match_pose, bytes);
  ENSURE(c, c->match_label, (size_t)job.ns * job.knn * 4);
  HIPCHK(c, hipMemcpyAsync(c->match_pose.p, pose, bytes, hipMemcpyHostToDevice, c->stream));
  gd->pose = c->match_pose.p;
  return SC_OK;
}

// behind the one wait: the optional arrays of `found` entries -> the caller's (enqueued: the caller synchronises)
int poses_results_to_host(sc_ctx* c, uint32_t found, float* g2, int32_t* label) {
  if (found && g2) HIPCHK(c, hipMemcpyAsync(g2, c->match_g2.p, (size_t)found * 4, hipMemcpyDeviceToHost, c->stream));
  if (found && label) HIPCHK(c, hipMemcpyAsync(label, c->match_label.p, (size_t)found * 4, hipMemcpyDeviceToHost, c->stream));
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
  GP_NOT_NULL(c, who, d_src_pts); GP_NOT_NULL(c, who, d_fsrc); GP_NOT_NULL(c, who, d_tgt_pts); GP_NOT_NULL(c, who, d_ftgt);
  GP_NOT_NULL(c, who, mp); GP_NOT_NULL(c, who, gp); GP_NOT_NULL(c, who, d_pose); GP_NOT_NULL(c, who, d_corr);
  GP_NOT_NULL(c, who, d_d2); GP_NOT_NULL(c, who, d_count);
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{d_fsrc, d_ftgt};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(poses_check(c, who, gp, pose_stride, n_poses, &gd));
  guide_points(&gd, d_src_pts, job.ns, d_tgt_pts, job.nt, gp->layout);
  gd.pose = d_pose;
  HIPCHK(c, hipSetDevice(c->device));
  return match_enqueue(c, job, d_corr, d_d2, d_count, MatchGather{}, false, &gd, nullptr, d_g2, d_label);
}

int sc_match_guided_poses(sc_ctx* c, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts, const float* ftgt,
                          int64_t nt, const sc_match_params* mp, const sc_guide_params* gp, const void* pose, uint32_t pose_stride,
                          uint32_t n_poses, int32_t* corr, float* d2, float* g2, int32_t* label, uint32_t* n) {
  static const char* const who = "sc_match_guided_poses";
  if (n) *n = 0;
  if (!c) return SC_EINVAL;
  GP_NOT_NULL(c, who, src_pts); GP_NOT_NULL(c, who, fsrc); GP_NOT_NULL(c, who, tgt_pts); GP_NOT_NULL(c, who, ftgt);
  GP_NOT_NULL(c, who, mp); GP_NOT_NULL(c, who, gp); GP_NOT_NULL(c, who, pose); GP_NOT_NULL(c, who, corr);
  GP_NOT_NULL(c, who, d2); GP_NOT_NULL(c, who, n);
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(poses_check(c, who, gp, pose_stride, n_poses, &gd));
  HIPCHK(c, hipSetDevice(c->device));
  SC_TRY(guided_stage_points(c, job, src_pts, tgt_pts));
  SC_TRY(match_stage_host(c, &job, fsrc, ftgt));
  SC_TRY(poses_stage_host(c, job, pose, &gd));
  guide_points(&gd, c->match_psrc.as<float>(), job.ns, c->match_ptgt.as<float>(), job.nt, gp->layout);
  SC_TRY(match_enqueue(c, job, c->match_corr.as<int32_t>(), c->match_d2.as<float>(), nullptr, MatchGather{}, true, &gd, nullptr,
                       c->match_g2.as<float>(), c->match_label.as<int32_t>()));
  uint32_t found = 0;
  SC_TRY(match_results_to_host(c, corr, d2, &found, MATCH_GUIDED_FLAGGED));
  SC_TRY(poses_results_to_host(c, found, g2, label));
  HIPCHK(c, hipStreamSynchronize(c->stream));
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
  GP_NOT_NULL(c, who, src_pts); GP_NOT_NULL(c, who, fsrc); GP_NOT_NULL(c, who, tgt_pts); GP_NOT_NULL(c, who, ftgt);
  GP_NOT_NULL(c, who, mp); GP_NOT_NULL(c, who, gp); GP_NOT_NULL(c, who, pose); GP_NOT_NULL(c, who, p);
  GP_NOT_NULL(c, who, R); GP_NOT_NULL(c, who, t); GP_NOT_NULL(c, who, corr); GP_NOT_NULL(c, who, d2);
  GP_NOT_NULL(c, who, n); GP_NOT_NULL(c, who, mask);
  SC_TRY(entry_checks(c, p, ENDS_FRAME | NOT_BUSY | PARAMS | ONE_RANK));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(poses_check(c, who, gp, pose_stride, n_poses, &gd));
  if ((int32_t)gp->layout != p->layout) return refuse(c, who, "guide->layout must be params->layout: the keypoints are one pair of arrays");
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  hipStream_t st = c->stream;
  const size_t cap = (size_t)job.ns * job.knn;
  ENSURE(c, c->match_gsrc, cap * 12);
  ENSURE(c, c->match_gtgt, cap * 12);
  SC_TRY(guided_stage_points(c, job, src_pts, tgt_pts));
  SC_TRY(match_stage_host(c, &job, fsrc, ftgt));
  SC_TRY(poses_stage_host(c, job, pose, &gd));
  guide_points(&gd, c->match_psrc.as<float>(), job.ns, c->match_ptgt.as<float>(), job.nt, gp->layout);
  const MatchGather g = gather_of(c->match_psrc.as<float>(), job.ns, c->match_ptgt.as<float>(), job.nt, p->layout, c->match_gsrc.as<float>(),
                                  c->match_gtgt.as<float>());
  SC_TRY(match_enqueue(c, job, c->match_corr.as<int32_t>(), c->match_d2.as<float>(), nullptr, g, true, &gd, nullptr, c->match_g2.as<float>(),
                       c->match_label.as<int32_t>()));
  uint32_t found = 0;
  SC_TRY(match_results_to_host(c, corr, d2, &found, MATCH_GUIDED_FLAGGED));  // the one host wait between matching and registration
  SC_TRY(poses_results_to_host(c, found, g2, label));
  *n = found;
  if (found < 3) {
    HIPCHK(c, hipStreamSynchronize(st));
    const float ident[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    memcpy(R, ident, 36);
    memset(t, 0, 12);
    return SC_ENOHYP;
  }
  sc_params pg = *p;
  pg.layout = SC_AOS;  // (the gathered correspondences are n x 3 whatever the caller's layout)
  ENSURE(c, c->rt12, 64);
  ENSURE(c, c->mask, (size_t)found);
  const int rc = sc_register_device(c, c->match_gsrc.as<float>(), c->match_gtgt.as<float>(), found, &pg, c->rt12.as<float>(),
                                    c->mask.as<uint8_t>(), stats);
  if (rc != SC_OK && rc != SC_ENOHYP) { (void)hipStreamSynchronize(st); return rc; }
  SC_TRY(outputs_to_host(c, (size_t)found, R, t, mask));
  return rc;
}

}  // extern "C"
