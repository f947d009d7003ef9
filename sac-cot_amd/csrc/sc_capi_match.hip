// sc_capi_match.hip — the C ABI's descriptor matching (include/saccot.h, sc_match): sc_match_default_params, sc_match_device,
// sc_match and sc_register_features, and the same under a pose prior (sc_match_guided): sc_guide_default_params,
// sc_match_guided_device, sc_match_guided and sc_register_guided_features.  Host-only, on the context and the helpers of sc_ctx.hpp;
// the kernels are sc_match.hip's.  The host forms' sequence (match_host) and the features forms' tail (match_register_gathered) are
// said once here, for these entries and for sc_capi_match_guided_poses.hip's.
//
// memset (the "clean" word and, for SC_MATCH_MUTUAL, the column minima: all ones) -> distance + select -> finish: three stream
// operations, no host wait — with or without a guide.  The host entries then poll ONE word (count | non-finite flag << 32).
#include "sc_ctx.hpp"
#include "sc_match_guided_check.hpp"

using namespace sc;

namespace sc {

int match_check(sc_ctx* c, const sc_match_params* mp, int64_t ns, int64_t nt, MatchJob* job) {
  if (!mp || mp->size != sizeof(sc_match_params)) { c->last_error = "sc_match: bad sc_match_params.size"; return SC_EINVAL; }
  if (mp->dim < 1 || mp->dim > 1024 || mp->knn < 1 || mp->knn > 4 || (mp->flags & ~SC_MATCH_MUTUAL) != 0 || mp->reserved[0] != 0 ||
      mp->reserved[1] != 0 || mp->reserved[2] != 0 || ns < 1 || nt < 1 || ns > (1 << 24) || nt > (1 << 24)) {
    c->last_error = "sc_match: dim 1 .. 1024, knn 1 .. 4, known flags, reserved words 0, 1 <= ns, nt <= 2^24";
    return SC_EINVAL;
  }
  if (!(mp->ratio >= 0.f && mp->ratio < 1.f)) { c->last_error = "sc_match: ratio must be 0 (off) or in (0, 1)"; return SC_EINVAL; }
  if (mp->knn != 1 && ((mp->flags & SC_MATCH_MUTUAL) || mp->ratio > 0.f)) {
    c->last_error = "sc_match: SC_MATCH_MUTUAL and the ratio test need knn == 1";
    return SC_EINVAL;
  }
  job->ns = (uint32_t)ns; job->nt = (uint32_t)nt; job->dim = mp->dim; job->knn = mp->knn;
  job->mutual = (mp->flags & SC_MATCH_MUTUAL) ? 1u : 0u;
  job->r2 = mp->ratio > 0.f ? (float)((double)mp->ratio * (double)mp->ratio) : 0.f;
  return SC_OK;
}

// ---- the sequence's steps, shared with sc_capi_match_guided_poses.hip (declared in sc_ctx.hpp)
// match_words: [0] clean, [2], [3] the host entries' count pair, [4 .. 15] the guided host entries' copy of the pose; the column minima from byte 64
constexpr size_t MATCH_WORDS_HEAD = 64, MATCH_WORDS_POSE = 16;

int match_enqueue(sc_ctx* c, const MatchJob& job, MatchOut o) {
  hipStream_t st = c->stream;
  const MatchPlan plan = match_plan(job.ns, job.nt, job.knn, job.r2);
  ENSURE(c, c->match_part, plan.part_bytes);
  const size_t words_bytes = MATCH_WORDS_HEAD + (job.mutual ? (size_t)job.nt * 8 : 0);
  ENSURE(c, c->match_words, words_bytes);
  HIPCHK(c, hipMemsetAsync(c->match_words.p, 0xFF, words_bytes, st));
  LbArgs lb;
  SC_TRY(lb_next(c, (size_t)match_finish_tiles(job.ns) * 8, 3, 0, &lb));
  uint32_t* clean = c->match_words.as<uint32_t>();
  uint64_t* colmin = job.mutual ? reinterpret_cast<uint64_t*>(static_cast<char*>(c->match_words.p) + MATCH_WORDS_HEAD) : nullptr;
  MatchGuide guide{};
  if (o.gd) {
    guide = *o.gd;
    if (o.h_Rt) {
      float* d_pose = reinterpret_cast<float*>(static_cast<char*>(c->match_words.p) + MATCH_WORDS_POSE);
      HIPCHK(c, hipMemcpyAsync(d_pose, o.h_Rt, 48, hipMemcpyHostToDevice, st));
      guide.Rt = d_pose;
    }
    o.gd = &guide;
  }
  if (o.to_host) {  // a host form: it polls ONE word
    arm_word(c, HW_MATCH);
    o.count = clean + 2;
    o.host_word = &c->pinned[HW_MATCH];
  }
  launch_match_dist(job, plan, c->match_part.as<uint64_t>(), colmin, clean, o.gd, st);
  launch_match_finish(job, plan, c->match_part.as<uint64_t>(), colmin, clean, lb, o, st);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

int match_host(sc_ctx* c, MatchJob job, const MatchHost& h, uint32_t* found) {
  hipStream_t st = c->stream;
  const size_t cap = (size_t)job.ns * job.knn, sb = (size_t)job.ns * job.dim * 4, tb = (size_t)job.nt * job.dim * 4;
  const size_t sp = (size_t)job.ns * 12, tp = (size_t)job.nt * 12, pose_bytes = h.pose ? (size_t)h.gd->n_poses * h.gd->pose_stride : 0;
  *found = 0;
  // room for the device copies and for what a match can write
  ENSURE(c, c->match_fsrc, sb);
  ENSURE(c, c->match_ftgt, tb);
  ENSURE(c, c->match_corr, cap * 8);
  ENSURE(c, c->match_d2, cap * 4);
  if (h.src_pts) { ENSURE(c, c->match_psrc, sp); ENSURE(c, c->match_ptgt, tp); }
  if (h.p) { ENSURE(c, c->match_gsrc, cap * 12); ENSURE(c, c->match_gtgt, cap * 12); }
  if (h.gd) ENSURE(c, c->match_g2, cap * 4);
  if (h.pose) { ENSURE(c, c->match_pose, pose_bytes); ENSURE(c, c->match_label, cap * 4); }
  // the copies in (enqueued).  A guided form's keypoints go in front of its descriptors, sc_register_features' behind them: the
  // order either always had.
  const auto points_in = [&]() -> int {
    HIPCHK(c, hipMemcpyAsync(c->match_psrc.p, h.src_pts, sp, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->match_ptgt.p, h.tgt_pts, tp, hipMemcpyHostToDevice, st));
    return SC_OK;
  };
  if (h.gd) SC_TRY(points_in());
  HIPCHK(c, hipMemcpyAsync(c->match_fsrc.p, h.fsrc, sb, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->match_ftgt.p, h.ftgt, tb, hipMemcpyHostToDevice, st));
  if (!h.gd && h.src_pts) SC_TRY(points_in());
  if (h.pose) HIPCHK(c, hipMemcpyAsync(c->match_pose.p, h.pose, pose_bytes, hipMemcpyHostToDevice, st));  // the records as given
  // the match on the copies
  job.fsrc = c->match_fsrc.as<float>(); job.ftgt = c->match_ftgt.as<float>();
  MatchOut o{};
  o.corr = c->match_corr.as<int32_t>(); o.d2 = c->match_d2.as<float>(); o.to_host = true;
  // (the gathered correspondences are written n x 3 whatever the caller's layout: n is not known while they are written)
  if (h.p) o.g = gather_of(c->match_psrc.as<float>(), job.ns, c->match_ptgt.as<float>(), job.nt, h.p->layout, c->match_gsrc.as<float>(),
                           c->match_gtgt.as<float>());
  if (h.gd) {
    guide_points(h.gd, c->match_psrc.as<float>(), job.ns, c->match_ptgt.as<float>(), job.nt, h.layout);
    o.gd = h.gd; o.h_Rt = h.Rt; o.g2 = c->match_g2.as<float>();
    if (h.pose) { h.gd->pose = c->match_pose.p; o.label = c->match_label.as<int32_t>(); }
  }
  SC_TRY(match_enqueue(c, job, o));
  // the one wait — the count, or SC_EINVAL for something not finite — and the read-back of that many entries (enqueued)
  SC_TRY(wait_word(c, HW_MATCH));
  const uint64_t w = c->pinned[HW_MATCH];
  if (w >> 32) { c->last_error = h.gd ? "non-finite descriptor, point or pose" : "non-finite descriptor"; return SC_EINVAL; }
  const size_t n = *found = (uint32_t)w;
  if (n) {
    HIPCHK(c, hipMemcpyAsync(h.corr, c->match_corr.p, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h.d2, c->match_d2.p, n * 4, hipMemcpyDeviceToHost, st));
    if (h.g2) HIPCHK(c, hipMemcpyAsync(h.g2, c->match_g2.p, n * 4, hipMemcpyDeviceToHost, st));
    if (h.label) HIPCHK(c, hipMemcpyAsync(h.label, c->match_label.p, n * 4, hipMemcpyDeviceToHost, st));
  }
  if (!h.p) HIPCHK(c, hipStreamSynchronize(st));  // (a features form goes on: match_register_gathered)
  return SC_OK;
}

int match_register_gathered(sc_ctx* c, const sc_params* p, uint32_t found, float R[9], float t[3], uint8_t* mask, sc_stats* stats) {
  hipStream_t st = c->stream;
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

}  // namespace sc

namespace {

// the rules of sc_guide_params (sc_match_guided_check.hpp) -> the guide but for its pointers
int guide_check(sc_ctx* c, const char* who, const sc_guide_params* gp, MatchGuide* gd) {
  if (const char* why = guide_params_error(gp)) return refuse(c, who, why);
  gd->gate2 = guide_gate2(gp->gate);
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_match_default_params(sc_match_params* mp) {
  if (!mp) return SC_EINVAL;
  memset(mp, 0, sizeof *mp);
  mp->size = sizeof(sc_match_params);
  mp->knn = 1;
  return SC_OK;
}

int sc_match_device(sc_ctx* c, const float* d_fsrc, int64_t ns, const float* d_ftgt, int64_t nt, const sc_match_params* mp,
                    int32_t* d_corr, float* d_d2, uint32_t* d_count) {
  if (!c || !d_fsrc || !d_ftgt || !d_corr || !d_d2 || !d_count) return SC_EINVAL;
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{d_fsrc, d_ftgt};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  HIPCHK(c, hipSetDevice(c->device));
  MatchOut o{};
  o.corr = d_corr; o.d2 = d_d2; o.count = d_count;
  return match_enqueue(c, job, o);
}

int sc_match(sc_ctx* c, const float* fsrc, int64_t ns, const float* ftgt, int64_t nt, const sc_match_params* mp, int32_t* corr,
             float* d2, uint32_t* n) {
  if (!c || !fsrc || !ftgt || !corr || !d2 || !n) return SC_EINVAL;
  *n = 0;
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  HIPCHK(c, hipSetDevice(c->device));
  MatchHost h{};
  h.fsrc = fsrc; h.ftgt = ftgt; h.corr = corr; h.d2 = d2;
  uint32_t found = 0;
  SC_TRY(match_host(c, job, h, &found));
  *n = found;
  return SC_OK;
}

int sc_register_features(sc_ctx* c, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts, const float* ftgt,
                         int64_t nt, const sc_match_params* mp, const sc_params* p, float R[9], float t[3], int32_t* corr, float* d2,
                         uint32_t* n, uint8_t* mask, sc_stats* stats) {
  if (!c || !src_pts || !fsrc || !tgt_pts || !ftgt || !R || !t || !corr || !d2 || !n || !mask) return SC_EINVAL;
  *n = 0;
  SC_TRY(entry_checks(c, p, ENDS_FRAME | NOT_BUSY | PARAMS | ONE_RANK));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  MatchHost h{};
  h.fsrc = fsrc; h.ftgt = ftgt; h.src_pts = src_pts; h.tgt_pts = tgt_pts; h.p = p; h.corr = corr; h.d2 = d2;
  uint32_t found = 0;
  SC_TRY(match_host(c, job, h, &found));  // the one host wait between matching and registration
  *n = found;
  return match_register_gathered(c, p, found, R, t, mask, stats);
}

int sc_guide_default_params(sc_guide_params* gp) {
  if (!gp) return SC_EINVAL;
  memset(gp, 0, sizeof *gp);
  gp->size = sizeof(sc_guide_params);
  gp->layout = SC_AOS;
  return SC_OK;
}

int sc_match_guided_device(sc_ctx* c, const float* d_src_pts, const float* d_fsrc, int64_t ns, const float* d_tgt_pts, const float* d_ftgt,
                           int64_t nt, const sc_match_params* mp, const sc_guide_params* gp, const float* d_Rt, int32_t* d_corr,
                           float* d_d2, float* d_g2, uint32_t* d_count) {
  static const char* const who = "sc_match_guided_device";
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, d_src_pts); SC_NOT_NULL(c, who, d_fsrc); SC_NOT_NULL(c, who, d_tgt_pts); SC_NOT_NULL(c, who, d_ftgt);
  SC_NOT_NULL(c, who, mp); SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, d_Rt); SC_NOT_NULL(c, who, d_corr);
  SC_NOT_NULL(c, who, d_d2); SC_NOT_NULL(c, who, d_count);
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{d_fsrc, d_ftgt};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, &gd));
  guide_points(&gd, d_src_pts, job.ns, d_tgt_pts, job.nt, gp->layout);
  gd.Rt = d_Rt;
  HIPCHK(c, hipSetDevice(c->device));
  MatchOut o{};
  o.corr = d_corr; o.d2 = d_d2; o.count = d_count; o.gd = &gd; o.g2 = d_g2;
  return match_enqueue(c, job, o);
}

int sc_match_guided(sc_ctx* c, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts, const float* ftgt, int64_t nt,
                    const sc_match_params* mp, const sc_guide_params* gp, const float Rt[12], int32_t* corr, float* d2, float* g2,
                    uint32_t* n) {
  static const char* const who = "sc_match_guided";
  if (n) *n = 0;
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, src_pts); SC_NOT_NULL(c, who, fsrc); SC_NOT_NULL(c, who, tgt_pts); SC_NOT_NULL(c, who, ftgt);
  SC_NOT_NULL(c, who, mp); SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, Rt); SC_NOT_NULL(c, who, corr);
  SC_NOT_NULL(c, who, d2); SC_NOT_NULL(c, who, n);
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, &gd));
  HIPCHK(c, hipSetDevice(c->device));
  MatchHost h{};
  h.fsrc = fsrc; h.ftgt = ftgt; h.src_pts = src_pts; h.tgt_pts = tgt_pts; h.gd = &gd; h.layout = gp->layout; h.Rt = Rt;
  h.corr = corr; h.d2 = d2; h.g2 = g2;
  uint32_t found = 0;
  SC_TRY(match_host(c, job, h, &found));
  *n = found;
  return SC_OK;
}

int sc_register_guided_features(sc_ctx* c, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts, const float* ftgt,
                                int64_t nt, const sc_match_params* mp, const sc_guide_params* gp, const float Rt_prior[12],
                                const sc_params* p, float R[9], float t[3], int32_t* corr, float* d2, float* g2, uint32_t* n,
                                uint8_t* mask, sc_stats* stats) {
  static const char* const who = "sc_register_guided_features";
  if (n) *n = 0;
  if (!c) return SC_EINVAL;
  SC_NOT_NULL(c, who, src_pts); SC_NOT_NULL(c, who, fsrc); SC_NOT_NULL(c, who, tgt_pts); SC_NOT_NULL(c, who, ftgt);
  SC_NOT_NULL(c, who, mp); SC_NOT_NULL(c, who, gp); SC_NOT_NULL(c, who, Rt_prior); SC_NOT_NULL(c, who, p);
  SC_NOT_NULL(c, who, R); SC_NOT_NULL(c, who, t); SC_NOT_NULL(c, who, corr); SC_NOT_NULL(c, who, d2);
  SC_NOT_NULL(c, who, n); SC_NOT_NULL(c, who, mask);
  SC_TRY(entry_checks(c, p, ENDS_FRAME | NOT_BUSY | PARAMS | ONE_RANK));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, &gd));
  SC_TRY(layouts_agree(c, who, gp, p));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  MatchHost h{};
  h.fsrc = fsrc; h.ftgt = ftgt; h.src_pts = src_pts; h.tgt_pts = tgt_pts; h.gd = &gd; h.layout = gp->layout; h.Rt = Rt_prior; h.p = p;
  h.corr = corr; h.d2 = d2; h.g2 = g2;
  uint32_t found = 0;
  SC_TRY(match_host(c, job, h, &found));  // the one host wait between matching and registration
  *n = found;
  return match_register_gathered(c, p, found, R, t, mask, stats);
}

}  // extern "C"
