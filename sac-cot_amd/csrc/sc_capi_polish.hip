// sc_capi_polish.hip — the C ABI's local optimisation on a scored frame (include/saccot.h, sc_polish): sc_polish_default_params,
// sc_polish_device and sc_polish.  Host-only, on the context and the helpers of sc_ctx.hpp; the kernels are sc_polish.hip's.
//
// select -> polish -> winner / mask: three launches of a dependent chain, then the wait for the winner.  The refits themselves —
// up to candidates x max_iter of them — all run inside the second launch.  The winner and its mask are a launch of their own, not
// the tail of the polish launch: the mask wants ceil(n / 256) workgroups and the polish launch has one per candidate, so the tail
// would be one workgroup walking all n behind a "last one out" ticket; a further dependent launch costs 3.0 - 3.5 us
// (profiles/r04b_ubench_dispatch_rate.txt), which at C2 is what that walk would cost, without the ticket.
// Everything is read from what the frame left — c->rt, c->sel_key, c->cnt, the staged planes — and nothing of it is written: the
// rounds of sc_peel keep their scores in a buffer of their own (peel_cnt), so the frame's stay in c->cnt.
#include "sc_ctx.hpp"

using namespace sc;

static_assert(sizeof(sc_polish_cand) == sizeof(PolishCand) && sizeof(sc_polish_cand) == 64 && sizeof(sc_polish_params) == 32,
              "sc_polish_cand is PolishCand, 64 bytes; sc_polish_params is 32");

extern "C" {

int sc_polish_default_params(sc_polish_params* pp) {
  if (!pp) return SC_EINVAL;
  memset(pp, 0, sizeof(*pp));
  pp->size = sizeof(sc_polish_params);
  pp->candidates = 8;
  pp->max_iter = 16;
  return SC_OK;
}

static int polish_check(sc_ctx* c, const sc_polish_params* pp) {
  const char* what = nullptr;
  if (!pp) what = "sc_polish: params is NULL";
  else if (pp->size != sizeof(sc_polish_params)) what = "sc_polish: params->size is not sizeof(sc_polish_params)";
  else if (pp->candidates < 1 || pp->candidates > POLISH_MAX_CAND) what = "sc_polish: candidates must be 1 .. 64";
  else if (pp->max_iter < 1 || pp->max_iter > 64) what = "sc_polish: max_iter must be 1 .. 64";
  else if (pp->flags || pp->reserved[0] || pp->reserved[1] || pp->reserved[2] || pp->reserved[3]) what = "sc_polish: flags and reserved fields must be 0";
  if (!what) return SC_OK;
  c->last_error = what;
  return SC_EINVAL;
}

static int polish_run(sc_ctx* c, const sc_polish_params* pp, float* d_Rt, uint8_t* d_mask, sc_polish_cand* d_cand, uint32_t* d_ncand,
                      sc_stats* stats) {
  SC_TRY(busy(c));
  SC_TRY(polish_check(c, pp));
  SC_TRY(scored_frame_begin(c, "sc_polish"));
  const Pass& ps = c->pass;
  const sc_params* p = &ps.params;
  const Shard& sh = ps.sh;  // one rank: a position in the selection IS the index into c->rt and c->cnt
  hipStream_t st = c->stream;
  const uint32_t want = pp->candidates;
  ENSURE(c, c->polish_cand, (size_t)POLISH_MAX_CAND * sizeof(PolishCand) + 64);
  ENSURE(c, c->polish_tmp, (size_t)want * chunk_scratch_bytes(ps.n));
  PolishCand* cand = c->polish_cand.as<PolishCand>();
  uint32_t* n_cand = reinterpret_cast<uint32_t*>(cand + POLISH_MAX_CAND);
  SC_TRY(rec(c, 0));
  const PolishSet set{cand, n_cand, want};
  launch_polish_select(set, c->cnt.as<uint32_t>(), c->sel_key.as<uint32_t>(), ps.T_eff, c->rt.as<float>(), sh.ld_local, st);
  SC_TRY(rec(c, 1));
  launch_polish(points_of(c), set, pp->max_iter, ps.dv.tau2, score_thr(ps.dv, p->score_mode), p->score_mode, c->polish_tmp.as<double>(), st);
  SC_TRY(rec(c, 2));
  arm_word(c, HW_WINNER);
  launch_polish_winner(points_of(c), set, WinnerOut{d_Rt, d_mask, &c->pinned[HW_WINNER]}, reinterpret_cast<PolishCand*>(d_cand), d_ncand,
                       ps.dv.tau2, st);
  SC_TRY(rec(c, 3));
  SC_TRY(scored_frame_wait(c));
  const uint32_t K = (uint32_t)c->pinned[HW_WINNER];
  scored_frame_stats(c, stats, K ? (uint32_t)c->pinned[HW_WINNER_POS] : 0u, K ? (uint32_t)(c->pinned[HW_WINNER_POS] >> 32) : 0u, 3);
  return K ? SC_OK : SC_ENOHYP;
}

int sc_polish_device(sc_ctx* c, const sc_polish_params* pp, float* d_Rt, uint8_t* d_mask, sc_polish_cand* d_cand, uint32_t* d_ncand,
                     sc_stats* stats) {
  if (!c || !pp || !d_Rt || !d_mask) return SC_EINVAL;
  return polish_run(c, pp, d_Rt, d_mask, d_cand, d_ncand, stats);
}

int sc_polish(sc_ctx* c, const sc_polish_params* pp, float R[9], float t[3], uint8_t* mask, sc_polish_cand* cand, uint32_t* n_cand,
              sc_stats* stats) {
  if (!c || !pp || !R || !t || !mask) return SC_EINVAL;
  SC_TRY(busy(c));
  SC_TRY(polish_check(c, pp));
  if (!c->pass.peelable) return polish_run(c, pp, nullptr, nullptr, nullptr, nullptr, stats);  // (refused there, with the text)
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)c->pass.n;
  ENSURE(c, c->rt12, 64);
  ENSURE(c, c->mask, n);
  const int rc = polish_run(c, pp, c->rt12.as<float>(), c->mask.as<uint8_t>(), nullptr, nullptr, stats);
  if (rc != SC_OK && rc != SC_ENOHYP) return rc;
  // the records come from the context's own list (the launch that made them is behind us on the stream)
  if (cand) HIPCHK(c, hipMemcpyAsync(cand, c->polish_cand.p, (size_t)pp->candidates * sizeof(sc_polish_cand), hipMemcpyDeviceToHost, c->stream));
  SC_TRY(outputs_to_host(c, n, R, t, mask));
  if (n_cand) *n_cand = (uint32_t)c->pinned[HW_WINNER];
  return rc;
}

}  // extern "C"
