// sc_capi_peel.hip — the C ABI's rounds on a scored frame (include/saccot.h, sc_peel): sc_peel_device, sc_peel and
// sc_register_instances.  Host-only, on the context and the helpers of sc_ctx.hpp; the kernels are sc_peel.hip's.
//
// claim + compact -> score -> arg-max -> winner / mask (+ refit): four launches of a dependent chain (five with SC_FLAG_REFINE), then
// the wait for the winner.  Stage C2 of a round is the PLAIN fp32 kernel (launch_score) on the compacted planes, in every score
// mode: exact by construction.  The frame's filter path is not reused: its tile, its coefficient permutation and its reference
// frame are built inside the frame's Kabsch launch for the frame's n correspondences (FilterPlan is planned by n, the Gram cut's
// reference was elected for the frame's winner, whose correspondences are the first to go) — a round would have to rebuild all
// three for n_alive points, which costs more launches than the filter saves at a round's size.
#include "sc_ctx.hpp"

using namespace sc;

extern "C" {

static int peel_round(sc_ctx* c, float* d_Rt, uint8_t* d_mask, sc_stats* stats) {
  SC_TRY(scored_frame_begin(c, "sc_peel"));
  Pass& ps = c->pass;
  const sc_params* p = &ps.params;
  const Shard& sh = ps.sh;  // one rank: n_local == T_eff, a position in the selection IS the index into c->rt
  hipStream_t st = c->stream;
  const size_t n = (size_t)ps.n, ld = (size_t)ps.ld;
  ENSURE(c, c->peel_planes, 6 * ld * sizeof(float));
  ENSURE(c, c->peel_claimed, n);
  if (!c->peel_words.p) {
    ENSURE(c, c->peel_words, sizeof(PeelWords));
    HIPCHK(c, hipMemsetAsync(c->peel_words.p, 0, c->peel_words.cap, st));
  }
  PeelWords* words = c->peel_words.as<PeelWords>();
  const Hyps h{sh, c->rt.as<float>(), nullptr, nullptr};  // (the scored frame's: no call of a round grows c->rt)
  SC_TRY(rec(c, 0));
  LbArgs lb;
  SC_TRY(lb_next(c, (size_t)peel_compact_tiles(ps.n) * 8, 2, 0, &lb));
  // the host sizes the scoring launch by n_alive: in inlier-count mode it knows it (n minus the best_counts so far: best_count ==
  // popcount(mask) there); in the truncated modes the compaction hands it over (one word, polled)
  const bool read_alive = p->score_mode != SC_SCORE_COUNT;
  if (read_alive) arm_word(c, HW_PEEL_ALIVE);
  launch_peel_compact(points_of(c), h, PeelSets{c->peel_claimed.as<uint8_t>(), c->peel_planes.as<float>(), read_alive ? &c->pinned[HW_PEEL_ALIVE] : nullptr},
                      ps.peel_prev, ps.dv.tau2, ps.peel_round == 0, words, lb, st);
  ps.peel_prev = 0xFFFFFFFFu;  // folded in
  SC_TRY(rec(c, 1));
  uint64_t n_alive = n - ps.peel_claimed;
  if (read_alive) {
    SC_TRY(wait_word(c, HW_PEEL_ALIVE));
    n_alive = c->pinned[HW_PEEL_ALIVE];
    if (n_alive > n) { c->last_error = "internal: the compaction kept more correspondences than the frame has"; return SC_EHIP; }
  }
  int npairs = 0;
  if (n_alive != 0) {  // (nothing alive: every score is 0 — the winner kernel reports "no hypothesis" from zero pairs)
    const Points alive{c->peel_planes.as<float>(), (int)n_alive, ps.ld};  // (the six planes only: the plain kernel reads nothing else)
    const uint32_t rows = score_chunks((int)n_alive, sh.ld_local);
    ENSURE(c, c->partial, (size_t)rows * sh.ld_local * 4);
    const Partial partial{c->partial.as<uint32_t>(), rows};
    launch_score(alive, h, partial, Stamps{}, ps.dv, p->score_mode, c->tn, st);
    SC_TRY(rec(c, 2));
    ENSURE(c, c->peel_cnt, (size_t)sh.ld_local * 4);  // (not c->cnt: the frame's scores stay for sc_polish)
    ENSURE(c, c->amx_pairs, argmax_scratch_bytes(sh.ld_local));
    launch_argmax(sh, partial, ArgmaxOut{c->sel_key.as<uint32_t>(), c->peel_cnt.as<uint32_t>(), c->amx_pairs.as<uint64_t>(),
                                         &c->ctl.as<ControlBlock>()->amx_ticket, nullptr}, st);  // (one pair per workgroup: the winner kernel reduces them)
    npairs = (int)argmax_blocks(sh.ld_local);
  } else SC_TRY(rec(c, 2));
  SC_TRY(rec(c, 3));
  arm_word(c, HW_WINNER);
  launch_peel_winner(points_of(c), h, WinnerIn{c->sel_key.as<uint32_t>(), ps.T_eff, c->amx_pairs.as<uint64_t>(), npairs},
                     WinnerOut{d_Rt, d_mask, &c->pinned[HW_WINNER]}, c->peel_claimed.as<uint8_t>(), ps.dv.tau2, words, st);
  if (ps.refine) {  // fp64 refit over mask_r, in refine_kernel's canonical order over the ORIGINAL indices (the mask stays the fp32 winner's)
    ENSURE(c, c->refine_tmp, refine_scratch_bytes(ps.n));
    launch_refine(points_of(c), d_mask, reinterpret_cast<const uint64_t*>(words->key2), c->refine_tmp.as<double>(), d_Rt, st);
  }
  SC_TRY(rec(c, 4));
  SC_TRY(scored_frame_wait(c));
  const uint64_t key = c->pinned[HW_WINNER];
  ps.peel_round++;
  if (key) {
    ps.peel_prev = (uint32_t)c->pinned[HW_WINNER_POS];
    if (!read_alive) ps.peel_claimed += (uint32_t)(key >> 32);
  }
  scored_frame_stats(c, stats, (uint32_t)(key >> 32), key ? (uint32_t)(c->pinned[HW_WINNER_POS] >> 32) : 0u, 4);  // (us_stage: claim + compact)
  return key ? SC_OK : SC_ENOHYP;
}

int sc_peel_device(sc_ctx* c, float* d_Rt, uint8_t* d_mask, sc_stats* stats) {
  if (!c || !d_Rt || !d_mask) return SC_EINVAL;
  return peel_round(c, d_Rt, d_mask, stats);
}

int sc_peel(sc_ctx* c, float R[9], float t[3], uint8_t* mask, sc_stats* stats) {
  if (!c || !R || !t || !mask) return SC_EINVAL;
  SC_TRY(busy(c));
  if (!c->pass.peelable) return peel_round(c, nullptr, nullptr, stats);  // (refused there, with the text)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->pass.n;
  ENSURE(c, c->rt12, 64);
  ENSURE(c, c->mask, n);
  const int rc = peel_round(c, c->rt12.as<float>(), c->mask.as<uint8_t>(), stats);
  if (rc != SC_OK && rc != SC_ENOHYP) return rc;
  SC_TRY(outputs_to_host(c, n, R, t, mask));
  return rc;
}

int sc_register_instances(sc_ctx* c, const float* src, const float* tgt, int64_t n, const sc_params* p, uint32_t max_instances,
                          uint32_t min_score, float* Rt, uint32_t* score, int32_t* label, uint32_t* n_found, sc_stats* stats) {
  if (c) peel_end(c);
  if (!c || !src || !tgt || !Rt || !score || !label || !n_found || max_instances == 0 || max_instances > 65536 || n < 3 || n > (1 << 24))
    return SC_EINVAL;
  *n_found = 0;
  SC_TRY(entry_checks(c, p, PARAMS | ONE_RANK));  // (the frame ended above, before the arguments were looked at;
  SC_TRY(busy(c));                                 //  and this entry asks "busy" AFTER the parameters)
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  ENSURE(c, c->rt12, (size_t)max_instances * 48 + 16);
  ENSURE(c, c->mask, (size_t)n);
  ENSURE(c, c->peel_label, (size_t)n * 4);
  hipStream_t st = c->stream;
  SC_TRY(points_to_device(c, src, tgt, n));
  HIPCHK(c, hipMemsetAsync(c->peel_label.p, 0xFF, (size_t)n * 4, st));  // -1: claimed by no motion
  sc_stats fs{}; fs.size = sizeof(sc_stats);
  const int rc = sc_register_device(c, c->in_src.as<float>(), c->in_tgt.as<float>(), n, p, c->rt12.as<float>(), c->mask.as<uint8_t>(), &fs);
  copy_stats(stats, fs);
  if (rc != SC_OK && rc != SC_ENOHYP) return rc;
  uint32_t k = 0;
  // motion 0 is the frame's winner; motion k the winner of round k.  The label is built on the device, one launch per accepted
  // motion, and copied out once; a round's n mask bytes never travel
  if (rc == SC_OK && fs.best_count >= min_score) {
    launch_peel_label(c->mask.as<uint8_t>(), (int)n, 0, c->peel_label.as<int32_t>(), st);
    score[0] = fs.best_count;
    for (k = 1; k < max_instances; k++) {
      sc_stats rs{}; rs.size = sizeof(sc_stats);
      const int prc = peel_round(c, c->rt12.as<float>() + 12 * (size_t)k, c->mask.as<uint8_t>(), &rs);
      if (prc == SC_ENOHYP) break;
      if (prc != SC_OK) return prc;
      if (rs.best_count < min_score) break;
      launch_peel_label(c->mask.as<uint8_t>(), (int)n, (int32_t)k, c->peel_label.as<int32_t>(), st);
      score[k] = rs.best_count;
    }
  }
  if (k) HIPCHK(c, hipMemcpyAsync(Rt, c->rt12.p, (size_t)k * 48, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(label, c->peel_label.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  *n_found = k;
  return rc;
}

}  // extern "C"
