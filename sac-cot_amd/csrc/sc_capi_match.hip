// sc_capi_match.hip — the C ABI's descriptor matching (include/saccot.h, sc_match): sc_match_default_params, sc_match_device,
// sc_match and sc_register_features, and the same under a pose prior (sc_match_guided): sc_guide_default_params,
// sc_match_guided_device, sc_match_guided and sc_register_guided_features.  Host-only, on the context and the helpers of sc_ctx.hpp;
// the kernels are sc_match.hip's.
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

// gd (sc_match_guided; nullptr: none): the points, the strides and gate2; its pose is gd->Rt in HBM, or — h_Rt, the host entries —
// 12 host floats that are copied into the head of match_words behind the memset.  d_g2: optional with a guide.  With pose records
// (gd->n_poses > 0: sc_match_guided_poses) gd->pose is their place in HBM, and d_label optional.
int match_enqueue(sc_ctx* c, const MatchJob& job, int32_t* d_corr, float* d_d2, uint32_t* d_count, const MatchGather& g, bool to_host,
                  const MatchGuide* gd, const float* h_Rt, float* d_g2, int32_t* d_label) {
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
  if (gd) {
    guide = *gd;
    if (h_Rt) {
      float* d_pose = reinterpret_cast<float*>(static_cast<char*>(c->match_words.p) + MATCH_WORDS_POSE);
      HIPCHK(c, hipMemcpyAsync(d_pose, h_Rt, 48, hipMemcpyHostToDevice, st));
      guide.Rt = d_pose;
    }
  }
  if (to_host) arm_word(c, HW_MATCH);
  launch_match_dist(job, plan, c->match_part.as<uint64_t>(), colmin, clean, gd ? &guide : nullptr, st);
  launch_match_finish(job, plan, c->match_part.as<uint64_t>(), colmin, clean, d_corr, d_d2, d_count ? d_count : clean + 2, g, lb,
                      to_host ? &c->pinned[HW_MATCH] : nullptr, gd ? &guide : nullptr, d_g2, st, d_label);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// the host entries' descriptors -> their device copies (enqueued), and room for what a match can write; the job then reads the copies
int match_stage_host(sc_ctx* c, MatchJob* job, const float* fsrc, const float* ftgt) {
  const size_t sb = (size_t)job->ns * job->dim * 4, tb = (size_t)job->nt * job->dim * 4, cap = (size_t)job->ns * job->knn;
  ENSURE(c, c->match_fsrc, sb);
  ENSURE(c, c->match_ftgt, tb);
  ENSURE(c, c->match_corr, cap * 8);
  ENSURE(c, c->match_d2, cap * 4);
  HIPCHK(c, hipMemcpyAsync(c->match_fsrc.p, fsrc, sb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->match_ftgt.p, ftgt, tb, hipMemcpyHostToDevice, c->stream));
  job->fsrc = c->match_fsrc.as<float>(); job->ftgt = c->match_ftgt.as<float>();
  return SC_OK;
}

// the host entries' one wait — the count, or SC_EINVAL for a non-finite descriptor — and the read-back of that many matches
// (enqueued: the caller synchronises)
int match_results_to_host(sc_ctx* c, int32_t* corr, float* d2, uint32_t* found, const char* flagged) {
  *found = 0;
  SC_TRY(wait_word(c, HW_MATCH));
  const uint64_t w = c->pinned[HW_MATCH];
  if (w >> 32) { c->last_error = flagged; return SC_EINVAL; }
  *found = (uint32_t)w;
  if (*found) {
    HIPCHK(c, hipMemcpyAsync(corr, c->match_corr.p, (size_t)*found * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(d2, c->match_d2.p, (size_t)*found * 4, hipMemcpyDeviceToHost, c->stream));
  }
  return SC_OK;
}

// ---- sc_match_guided --------------------------------------------------------------------------------------------------------------
// the points of both sets in the guide's layout, as the kernels are told (MatchGather's strides)
void guide_points(MatchGuide* gd, const float* src, uint32_t ns, const float* tgt, uint32_t nt, uint32_t layout) {
  const MatchGather g = gather_of(src, ns, tgt, nt, (int)layout, nullptr, nullptr);
  gd->src = g.src; gd->tgt = g.tgt;
  gd->s_elem = g.s_elem; gd->s_comp = g.s_comp; gd->t_elem = g.t_elem; gd->t_comp = g.t_comp;
}

// the guided host entries' keypoints -> their device copies (enqueued), and room for g2
int guided_stage_points(sc_ctx* c, const MatchJob& job, const float* src_pts, const float* tgt_pts) {
  ENSURE(c, c->match_psrc, (size_t)job.ns * 12);
  ENSURE(c, c->match_ptgt, (size_t)job.nt * 12);
  ENSURE(c, c->match_g2, (size_t)job.ns * job.knn * 4);
  HIPCHK(c, hipMemcpyAsync(c->match_psrc.p, src_pts, (size_t)job.ns * 12, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->match_ptgt.p, tgt_pts, (size_t)job.nt * 12, hipMemcpyHostToDevice, c->stream));
  return SC_OK;
}

}  // namespace sc

namespace {

constexpr const char* GUIDED_FLAGGED = MATCH_GUIDED_FLAGGED;

// the rules of sc_guide_params (sc_match_guided_check.hpp) -> the guide but for its pointers
int guide_check(sc_ctx* c, const char* who, const sc_guide_params* gp, MatchGuide* gd) {
  if (const char* why = guide_params_error(gp)) return refuse(c, who, why);
  gd->gate2 = guide_gate2(gp->gate);
  return SC_OK;
}

// a refused NULL argument, named (the context is there: sc_last_error can say which)
#define GUIDED_NOT_NULL(c, who, arg) do { if (!(arg)) return refuse((c), (who), #arg " is NULL"); } while (0)

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
  return match_enqueue(c, job, d_corr, d_d2, d_count, MatchGather{}, false);
}

int sc_match(sc_ctx* c, const float* fsrc, int64_t ns, const float* ftgt, int64_t nt, const sc_match_params* mp, int32_t* corr,
             float* d2, uint32_t* n) {
  if (!c || !fsrc || !ftgt || !corr || !d2 || !n) return SC_EINVAL;
  *n = 0;
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  HIPCHK(c, hipSetDevice(c->device));
  SC_TRY(match_stage_host(c, &job, fsrc, ftgt));
  SC_TRY(match_enqueue(c, job, c->match_corr.as<int32_t>(), c->match_d2.as<float>(), nullptr, MatchGather{}, true));
  uint32_t found = 0;
  SC_TRY(match_results_to_host(c, corr, d2, &found));
  HIPCHK(c, hipStreamSynchronize(c->stream));
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
  hipStream_t st = c->stream;
  const size_t cap = (size_t)job.ns * job.knn;
  ENSURE(c, c->match_psrc, (size_t)job.ns * 12);
  ENSURE(c, c->match_ptgt, (size_t)job.nt * 12);
  ENSURE(c, c->match_gsrc, cap * 12);
  ENSURE(c, c->match_gtgt, cap * 12);
  SC_TRY(match_stage_host(c, &job, fsrc, ftgt));
  HIPCHK(c, hipMemcpyAsync(c->match_psrc.p, src_pts, (size_t)job.ns * 12, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(c->match_ptgt.p, tgt_pts, (size_t)job.nt * 12, hipMemcpyHostToDevice, st));
  // the gathered correspondences are written n x 3 whatever the caller's layout: n is not known while they are written
  const MatchGather g = gather_of(c->match_psrc.as<float>(), job.ns, c->match_ptgt.as<float>(), job.nt, p->layout, c->match_gsrc.as<float>(),
                                  c->match_gtgt.as<float>());
  SC_TRY(match_enqueue(c, job, c->match_corr.as<int32_t>(), c->match_d2.as<float>(), nullptr, g, true));
  uint32_t found = 0;
  SC_TRY(match_results_to_host(c, corr, d2, &found));  // the one host wait between matching and registration
  *n = found;
  if (found < 3) {
    HIPCHK(c, hipStreamSynchronize(st));
    const float ident[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    memcpy(R, ident, 36);
    memset(t, 0, 12);
    return SC_ENOHYP;
  }
  sc_params pg = *p;
  pg.layout = SC_AOS;
  ENSURE(c, c->rt12, 64);
  ENSURE(c, c->mask, (size_t)found);
  const int rc = sc_register_device(c, c->match_gsrc.as<float>(), c->match_gtgt.as<float>(), found, &pg, c->rt12.as<float>(),
                          c->mask.as<uint8_t>(), stats);
  if (rc != SC_OK && rc != SC_ENOHYP) { (void)hipStreamSynchronize(st); return rc; }
  SC_TRY(outputs_to_host(c, (size_t)found, R, t, mask));
  return rc;
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
  GUIDED_NOT_NULL(c, who, d_src_pts); GUIDED_NOT_NULL(c, who, d_fsrc); GUIDED_NOT_NULL(c, who, d_tgt_pts); GUIDED_NOT_NULL(c, who, d_ftgt);
  GUIDED_NOT_NULL(c, who, mp); GUIDED_NOT_NULL(c, who, gp); GUIDED_NOT_NULL(c, who, d_Rt); GUIDED_NOT_NULL(c, who, d_corr);
  GUIDED_NOT_NULL(c, who, d_d2); GUIDED_NOT_NULL(c, who, d_count);
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{d_fsrc, d_ftgt};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, &gd));
  guide_points(&gd, d_src_pts, job.ns, d_tgt_pts, job.nt, gp->layout);
  gd.Rt = d_Rt;
  HIPCHK(c, hipSetDevice(c->device));
  return match_enqueue(c, job, d_corr, d_d2, d_count, MatchGather{}, false, &gd, nullptr, d_g2);
}

int sc_match_guided(sc_ctx* c, const float* src_pts, const float* fsrc, int64_t ns, const float* tgt_pts, const float* ftgt, int64_t nt,
                    const sc_match_params* mp, const sc_guide_params* gp, const float Rt[12], int32_t* corr, float* d2, float* g2,
                    uint32_t* n) {
  static const char* const who = "sc_match_guided";
  if (n) *n = 0;
  if (!c) return SC_EINVAL;
  GUIDED_NOT_NULL(c, who, src_pts); GUIDED_NOT_NULL(c, who, fsrc); GUIDED_NOT_NULL(c, who, tgt_pts); GUIDED_NOT_NULL(c, who, ftgt);
  GUIDED_NOT_NULL(c, who, mp); GUIDED_NOT_NULL(c, who, gp); GUIDED_NOT_NULL(c, who, Rt); GUIDED_NOT_NULL(c, who, corr);
  GUIDED_NOT_NULL(c, who, d2); GUIDED_NOT_NULL(c, who, n);
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, &gd));
  HIPCHK(c, hipSetDevice(c->device));
  SC_TRY(guided_stage_points(c, job, src_pts, tgt_pts));
  SC_TRY(match_stage_host(c, &job, fsrc, ftgt));
  guide_points(&gd, c->match_psrc.as<float>(), job.ns, c->match_ptgt.as<float>(), job.nt, gp->layout);
  SC_TRY(match_enqueue(c, job, c->match_corr.as<int32_t>(), c->match_d2.as<float>(), nullptr, MatchGather{}, true, &gd, Rt,
                       c->match_g2.as<float>()));
  uint32_t found = 0;
  SC_TRY(match_results_to_host(c, corr, d2, &found, GUIDED_FLAGGED));
  if (found && g2) HIPCHK(c, hipMemcpyAsync(g2, c->match_g2.p, (size_t)found * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
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
  GUIDED_NOT_NULL(c, who, src_pts); GUIDED_NOT_NULL(c, who, fsrc); GUIDED_NOT_NULL(c, who, tgt_pts); GUIDED_NOT_NULL(c, who, ftgt);
  GUIDED_NOT_NULL(c, who, mp); GUIDED_NOT_NULL(c, who, gp); GUIDED_NOT_NULL(c, who, Rt_prior); GUIDED_NOT_NULL(c, who, p);
  GUIDED_NOT_NULL(c, who, R); GUIDED_NOT_NULL(c, who, t); GUIDED_NOT_NULL(c, who, corr); GUIDED_NOT_NULL(c, who, d2);
  GUIDED_NOT_NULL(c, who, n); GUIDED_NOT_NULL(c, who, mask);
  SC_TRY(entry_checks(c, p, ENDS_FRAME | NOT_BUSY | PARAMS | ONE_RANK));
  MatchJob job{};
  SC_TRY(match_check(c, mp, ns, nt, &job));
  MatchGuide gd{};
  SC_TRY(guide_check(c, who, gp, &gd));
  if ((int32_t)gp->layout != p->layout) return refuse(c, who, "guide->layout must be params->layout: the keypoints are one pair of arrays");
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  hipStream_t st = c->stream;
  const size_t cap = (size_t)job.ns * job.knn;
  ENSURE(c, c->match_gsrc, cap * 12);
  ENSURE(c, c->match_gtgt, cap * 12);
  SC_TRY(guided_stage_points(c, job, src_pts, tgt_pts));
  SC_TRY(match_stage_host(c, &job, fsrc, ftgt));
  guide_points(&gd, c->match_psrc.as<float>(), job.ns, c->match_ptgt.as<float>(), job.nt, gp->layout);
  const MatchGather g = gather_of(c->match_psrc.as<float>(), job.ns, c->match_ptgt.as<float>(), job.nt, p->layout, c->match_gsrc.as<float>(),
                                  c->match_gtgt.as<float>());
  SC_TRY(match_enqueue(c, job, c->match_corr.as<int32_t>(), c->match_d2.as<float>(), nullptr, g, true, &gd, Rt_prior, c->match_g2.as<float>()));
  uint32_t found = 0;
  SC_TRY(match_results_to_host(c, corr, d2, &found, GUIDED_FLAGGED));  // the one host wait between matching and registration
  if (found && g2) HIPCHK(c, hipMemcpyAsync(g2, c->match_g2.p, (size_t)found * 4, hipMemcpyDeviceToHost, st));
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
