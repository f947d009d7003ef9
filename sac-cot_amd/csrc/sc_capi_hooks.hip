// sc_capi_hooks.hip — the C ABI's stage hooks (include/saccot.h, sc_*_host): one stage at a time on host arrays, for the tests that
// compare a stage with the CPU restatement.  Host-only, on the context and the stage sequencers of sc_capi.hip, sc_capi_compat.hip and sc_capi_tri.hip (sc_ctx.hpp).
#include "sc_ctx.hpp"

using namespace sc;

namespace {

// The stage hooks start no pass: they run on whatever the last one left, and clear what would change their kernels
int host_to_planes(sc_ctx* c, const float* src, const float* tgt, int64_t n, const sc_params* p) {
  SC_TRY(busy(c));
  c->pass.mode.host_free = false;  // (a host-free call that was never finalized must not leave its covers to a stage hook)
  c->pass.mode.may_estimate = false;  // (a hook cannot repeat itself: certified bounds only)
  c->pass.form.build = false;  // (stage hooks: the separate kernels)
  c->pass.timing = c->pass.timing_hot = false; c->pass.timing_one = -1;  // (... and no event brackets)
  c->cap_bytes = workspace_cap(p);
  c->pass.dv = derive(p);
  if (!src || !tgt || n < 3 || n > (1 << 24)) return SC_EINVAL;
  SC_TRY(points_to_device(c, src, tgt, n));
  return stage_inputs(c, c->in_src.as<float>(), c->in_tgt.as<float>(), n, p);
}

// what every hook does first (sc_compat_host spells it out: it has a refusal of its own between the last two steps): the parameters,
// the device, no hypothesize half or frame left behind, the correspondences staged
int hook_begin(sc_ctx* c, const float* src, const float* tgt, int64_t n, const sc_params* p) {
  SC_TRY(check_params(p));
  HIPCHK(c, hipSetDevice(c->device));
  c->pass.have_hyp = false; peel_end(c);
  return host_to_planes(c, src, tgt, n, p);
}

int check_flag(sc_ctx* c) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((uint32_t)c->pinned[HW_BAD_INPUT] != 0) { c->last_error = "non-finite input coordinate"; return SC_EINVAL; }
  return SC_OK;
}

// ... and last: the copies out have arrived, and nothing went wrong on the way
int hook_end(sc_ctx* c) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

extern "C" {

int sc_compat_host(sc_ctx* c, const float* src, const float* tgt, int64_t n, const sc_params* p, float* S,
                   uint64_t* bits, uint32_t* deg) {
  if (!c) return SC_EINVAL;
  SC_TRY(check_params(p));
  HIPCHK(c, hipSetDevice(c->device));
  c->pass.have_hyp = false; peel_end(c);
  const bool dense = S != nullptr && !(p->flags & SC_FLAG_NO_DENSE_S);
  if (S && !dense) { c->last_error = "sc_compat_host: S requested together with SC_FLAG_NO_DENSE_S"; return SC_EINVAL; }
  SC_TRY(host_to_planes(c, src, tgt, n, p));
  SC_TRY(run_compat(c, dense));
  SC_TRY(run_row_stats(c, false));
  SC_TRY(check_flag(c));
  const size_t W = (size_t)c->pass.ld >> 6;
  if (S)
    HIPCHK(c, hipMemcpy2DAsync(S, (size_t)n * 4, c->S.p, (size_t)c->pass.ld * 4, (size_t)n * 4, (size_t)n,
                               hipMemcpyDeviceToHost, c->stream));
  if (bits) HIPCHK(c, hipMemcpyAsync(bits, c->bits.p, (size_t)n * W * 8, hipMemcpyDeviceToHost, c->stream));
  if (deg) HIPCHK(c, hipMemcpyAsync(deg, c->deg.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  return hook_end(c);
}

int sc_triangles_host(sc_ctx* c, const float* src, const float* tgt, int64_t n, const sc_params* p, uint32_t* tri,
                      uint32_t* key, uint32_t* t_eff, uint64_t* tri_total, uint64_t* edges) {
  if (!c || !tri || !t_eff) return SC_EINVAL;
  SC_TRY(hook_begin(c, src, tgt, n, p));
  SC_TRY(run_compat(c, false));  // the ranked list needs the bit rows only
  SC_TRY(run_row_stats(c, may_prune(p)));
  sc_params pe = *p;
  pe.flags |= SC_FLAG_EXACT_TOTAL;  // the hook reports the 3-clique count of the whole graph
  SC_TRY(run_triangles(c, &pe, true));
  *t_eff = c->pass.T_eff;
  if (tri_total) *tri_total = c->pass.M_total;
  if (edges) *edges = c->pass.E;
  if (c->pass.T_eff) {
    // the hook returns the RANKED list; the hot path itself never sorts
    const size_t T = c->pass.T_eff, sort_bytes = sort_temp_bytes(T);
    ENSURE(c, c->sortkey, T * 8);
    ENSURE(c, c->sorted, T * 8);
    ENSURE(c, c->sort_tmp, sort_bytes + 16);
    ENSURE(c, c->tri_rk, T * 12);
    ENSURE(c, c->key_rk, T * 4);
    launch_rank_order(c->tri.as<uint32_t>(), selection_of(c), c->pass.T_eff, c->sortkey.as<uint64_t>(),
                      c->sorted.as<uint64_t>(), c->sort_tmp.p, sort_bytes, c->tri_rk.as<uint32_t>(),
                      c->key_rk.as<uint32_t>(), c->stream);
    HIPCHK(c, hipMemcpyAsync(tri, c->tri_rk.p, T * 12, hipMemcpyDeviceToHost, c->stream));
    if (key) HIPCHK(c, hipMemcpyAsync(key, c->key_rk.p, T * 4, hipMemcpyDeviceToHost, c->stream));
  }
  return hook_end(c);
}

int sc_kabsch_host(sc_ctx* c, const float* src, const float* tgt, int64_t n, const sc_params* p,
                   const uint32_t* tri, uint32_t n_tri, float* Rt) {
  if (!c || !tri || !Rt) return SC_EINVAL;
  // (ahead of the parameter check it used to follow: both refuse with SC_EINVAL, neither leaves a text or touches the context)
  for (size_t k = 0; k < (size_t)n_tri * 3; k++) if ((int64_t)tri[k] >= n) return SC_EINVAL;
  SC_TRY(hook_begin(c, src, tgt, n, p));
  if (n_tri == 0) return check_flag(c);
  ENSURE(c, c->tri, (size_t)n_tri * 12);
  ENSURE(c, c->rt_aos, (size_t)n_tri * 48);
  HIPCHK(c, hipMemcpyAsync(c->tri.p, tri, (size_t)n_tri * 12, hipMemcpyHostToDevice, c->stream));
  launch_kabsch_aos(points_of(c), c->tri.as<uint32_t>(), n_tri, c->rt_aos.as<float>(), c->stream);
  SC_TRY(check_flag(c));
  HIPCHK(c, hipMemcpyAsync(Rt, c->rt_aos.p, (size_t)n_tri * 48, hipMemcpyDeviceToHost, c->stream));
  return hook_end(c);
}

int sc_score_host(sc_ctx* c, const float* src, const float* tgt, int64_t n, const sc_params* p, const float* Rt,
                  uint32_t n_hyp, uint32_t* cnt, uint64_t* key) {
  if (!c || !Rt || !key) return SC_EINVAL;
  SC_TRY(hook_begin(c, src, tgt, n, p));
  Shard sh;
  sh.T_eff = n_hyp; sh.block = 0x40000000u; sh.rank = 0; sh.world = 1; sh.n_local = n_hyp;
  sh.ld_local = (uint32_t)(((uint64_t)n_hyp + 255u) / 256u * 256u);
  ENSURE(c, c->key, 64);
  if (n_hyp) {
    ENSURE(c, c->rt_aos, (size_t)sh.ld_local * 48);  // (the scoring kernel may read whole 256-hypothesis groups)
    ENSURE(c, c->rt, (size_t)12 * sh.ld_local * 4);
    HIPCHK(c, hipMemcpyAsync(c->rt_aos.p, Rt, (size_t)n_hyp * 48, hipMemcpyHostToDevice, c->stream));
    if (sh.ld_local > n_hyp)  // the padding hypotheses read as zeros in both layouts
      HIPCHK(c, hipMemsetAsync(c->rt_aos.as<char>() + (size_t)n_hyp * 48, 0, (size_t)(sh.ld_local - n_hyp) * 48, c->stream));
    launch_rt_to_soa(c->rt_aos.as<float>(), n_hyp, sh.ld_local, c->rt.as<float>(), c->stream);
  }
  // the choice of the C2 kernel looks at the coordinate maxima the staging kernel publishes: wait for them (the path
  // proper never has to — it has polled later results of the same stream by the time it gets here)
  if (!c->tn.filter_blind) SC_TRY(wait_word(c, HW_COORD_MAX));
  c->pass.sh = sh;
  SC_TRY(decide_filter(c, p, sh));
  const Hyps h{sh, c->rt.as<float>(), c->rt_aos.as<float>(), nullptr};  // (behind the ENSUREs above; decide_filter touches neither array)
  Partial partial{};
  SC_TRY(run_score(c, p, h, &partial, false, Stamps{}));
  ENSURE(c, c->cnt, (size_t)(sh.ld_local ? sh.ld_local : 256) * 4);
  ENSURE(c, c->amx_pairs, argmax_scratch_bytes(sh.ld_local));
  launch_argmax(sh, partial, ArgmaxOut{nullptr, c->cnt.as<uint32_t>(), c->amx_pairs.as<uint64_t>(), &c->ctl.as<ControlBlock>()->amx_ticket,
                                       c->key.as<uint64_t>()}, c->stream);  // positions in Rt ARE the rank indices here: single-stage key
  SC_TRY(check_flag(c));
  if (cnt && n_hyp) HIPCHK(c, hipMemcpyAsync(cnt, c->cnt.p, (size_t)n_hyp * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(key, c->key.p, 8, hipMemcpyDeviceToHost, c->stream));
  return hook_end(c);
}

int sc_mask_host(sc_ctx* c, const float* src, const float* tgt, int64_t n, const sc_params* p, const float Rt[12],
                 uint8_t* mask) {
  if (!c || !Rt || !mask) return SC_EINVAL;
  SC_TRY(hook_begin(c, src, tgt, n, p));
  ENSURE(c, c->rt12, 64);
  ENSURE(c, c->mask, (size_t)n);
  HIPCHK(c, hipMemcpyAsync(c->rt12.p, Rt, 48, hipMemcpyHostToDevice, c->stream));
  launch_mask(points_of(c), c->rt12.as<float>(), c->pass.dv.tau2, c->mask.as<uint8_t>(), c->stream);
  SC_TRY(check_flag(c));
  HIPCHK(c, hipMemcpyAsync(mask, c->mask.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  return hook_end(c);
}

}  // extern "C"
