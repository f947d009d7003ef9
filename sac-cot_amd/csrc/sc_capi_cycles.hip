// sc_capi_cycles.hip — the C ABI's loop-consistency check of a pair list (include/saccot.h, sc_pairs_cycles): sc_cycles_default_params,
// sc_cycles_thresholds, sc_pairs_cycles_device and sc_pairs_cycles.  Host-only, on the context and the helpers of sc_ctx.hpp; the
// kernels are sc_cycles.hip's, the rules of the parameters and of the list, the adjacency build and the staged image
// sc_cycles_check.hpp's.
//
// The host steps are every pair-list entry's (sc_capi_graph.hpp): the check, then the image of the list staged once per call — the
// pairs' records and the sorted neighbour entries, without the list starts — -> a memset of the round words -> prepare, max_rounds
// round launches, finish: max_rounds + 4 stream operations whatever the list, and no wait in the device form — the stop is decided
// on the device (sc_cycles.hip).  Everything that can refuse a call is decided on the host before anything is enqueued.
#include "sc_capi_graph.hpp"

using namespace sc;

static_assert(sizeof(sc_cycle_params) == 32 && sizeof(sc_cycle_result) == 48 && sizeof(sc_cycle_summary) == 32,
              "sc_cycle_params is 32 bytes, sc_cycle_result 48, sc_cycle_summary 32");

namespace {

// the workspace of the device form
int cyc_room(sc_ctx* c, const PairGraph& g) {
  ENSURE(c, c->cyc_meta, pair_graph_meta_bytes(g, false));
  ENSURE(c, c->cyc_wide, (size_t)cycles_pose_bytes(g.n_pairs));
  ENSURE(c, c->cyc_state, (size_t)cycles_state_bytes(g.n_pairs));
  return SC_OK;
}

struct CycArrays {
  const void* pose; const uint8_t* keep;
  sc_cycle_result* res; sc_cycle_summary* sum;
};

// the workspace has its room: the image staged, the memset and the launches
int cyc_enqueue(sc_ctx* c, PairGraph& g, const sc_cycle_params* cp, uint32_t pose_stride, const CycArrays& d) {
  PairGraphStaged m;
  SC_TRY(pair_graph_stage(c, g, c->cyc_meta, false, &m));
  double thr[2];
  cycles_thresholds(cp, thr);
  CyclesJob job{};
  job.rec = m.rec; job.entries = m.entries;
  job.pose = d.pose; job.pose_stride = pose_stride; job.status = cycles_reads_status(cp);
  job.keep = d.keep;
  job.wide = c->cyc_wide.as<double>();
  job.ctl = c->cyc_state.as<CyclesCtl>();
  job.alive = c->cyc_state.as<uint8_t>() + CYCLES_CTL_BYTES;
  job.res = reinterpret_cast<CycleRecord*>(d.res); job.sum = reinterpret_cast<CycleSummary*>(d.sum);
  job.tr_min = thr[0]; job.e2_max = thr[1];
  job.n_pairs = g.n_pairs; job.min_ok = cp->min_ok; job.max_rounds = cp->max_rounds;
  HIPCHK(c, hipMemsetAsync(job.ctl, 0, CYCLES_CTL_BYTES, c->stream));  // the rounds add into the words
  launch_pairs_cycles(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// Both forms.  host: the arrays are the caller's, staged around the enqueue (HostArrays); else the device's, and there is no wait.
int cyc_call(sc_ctx* c, const char* who, bool host, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_cycle_params* cp,
             uint32_t pose_stride, const CycArrays& a) {
  if (!c) return SC_EINVAL;
  if (!pairs || !cp || !a.pose || !a.res || !a.sum) return refuse(c, who, "a NULL argument");
  const char* broken = cycles_params_error(cp);
  if (!broken) broken = cycles_stride_error(cp, pose_stride);
  PairGraph g;
  SC_TRY(pair_graph_check(c, who, broken, n_sets, pairs, n_pairs, nullptr, &g));
  SC_TRY(cyc_room(c, g));
  if (!host) return cyc_enqueue(c, g, cp, pose_stride, a);
  HostArrays h(c);
  const int a_pose = h.in(a.pose, (size_t)pose_bytes_read(n_pairs, pose_stride, cycles_reads_status(cp)));
  const int a_keep = h.in(a.keep, n_pairs);
  const int a_res = h.out(a.res, (size_t)n_pairs * sizeof(sc_cycle_result)), a_sum = h.out(a.sum, sizeof(sc_cycle_summary));
  return h.run([&] {
    return cyc_enqueue(c, g, cp, pose_stride, CycArrays{h.at<void>(a_pose), h.at<uint8_t>(a_keep), h.at<sc_cycle_result>(a_res), h.at<sc_cycle_summary>(a_sum)});
  });
}

}  // namespace

extern "C" {

int sc_cycles_default_params(sc_cycle_params* cp) {
  if (!cp) return SC_EINVAL;
  memset(cp, 0, sizeof(*cp));
  cp->size = sizeof(sc_cycle_params);
  cp->min_ok = 1;
  cp->max_rounds = 16;
  return SC_OK;
}

int sc_cycles_thresholds(const sc_cycle_params* cp, double out[2]) {
  if (!cp || !out) return SC_EINVAL;
  if (cycles_params_error(cp)) return SC_EINVAL;
  cycles_thresholds(cp, out);
  return SC_OK;
}

int sc_pairs_cycles_device(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_cycle_params* cp,
                           const void* d_pose, uint32_t pose_stride, const uint8_t* d_keep, sc_cycle_result* d_res, sc_cycle_summary* d_sum) {
  return cyc_call(c, "sc_pairs_cycles_device", false, n_sets, pairs, n_pairs, cp, pose_stride, CycArrays{d_pose, d_keep, d_res, d_sum});
}

int sc_pairs_cycles(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_cycle_params* cp, const void* pose,
                    uint32_t pose_stride, const uint8_t* keep, sc_cycle_result* res, sc_cycle_summary* sum) {
  return cyc_call(c, "sc_pairs_cycles", true, n_sets, pairs, n_pairs, cp, pose_stride, CycArrays{pose, keep, res, sum});
}

}  // extern "C"
