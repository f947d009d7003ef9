// sc_capi_solve.hip — the C ABI's Gauss-Newton pose-graph solve of a pair list's sets (include/saccot.h, sc_pairs_solve):
// sc_solve_default_params, sc_solve_thresholds, sc_pairs_solve_device and sc_pairs_solve.  Host-only, on the context and the helpers
// of sc_ctx.hpp; the kernels are sc_solve.hip's, the rules of the list, the adjacency build and the staged image
// sc_cycles_check.hpp's, the rules of the parameters and the strides and the layout of the workspace sc_solve_check.hpp's.
//
// The host steps are every pair-list entry's (sc_capi_graph.hpp): the check, then the image of the list staged once per call, with
// the list starts -> a memset of the control words and the sets' tallies -> the launches:
// 2 + 5 + max_outer * (4 + 2 * max_inner) stream operations whatever the list, and no wait in the device form.  Everything that can
// refuse a call is decided on the host before anything is enqueued.
#include "sc_capi_graph.hpp"
#include "sc_solve_check.hpp"

using namespace sc;

static_assert(sizeof(sc_solve_params) == 32 && sizeof(sc_solve_set) == 160 && sizeof(sc_solve_pair) == 48 && sizeof(sc_solve_summary) == 64,
              "sc_solve_params is 32 bytes, sc_solve_set 160, sc_solve_pair 48, sc_solve_summary 64");

namespace {

// the workspace of the device form
int solve_room(sc_ctx* c, const PairGraph& g) {
  const SolveLayout l = solve_layout(g.n_sets, g.n_pairs);
  ENSURE(c, c->solve_meta, pair_graph_meta_bytes(g, true));
  ENSURE(c, c->solve_pair, (size_t)l.pair_bytes);
  ENSURE(c, c->solve_set, (size_t)l.set_bytes);
  ENSURE(c, c->solve_ctl, (size_t)l.ctl_bytes);
  return SC_OK;
}

struct SolveStrides { uint32_t pose, use, info, init; };
struct SolveArrays {
  const void* pose; const void* use; const void* info; const void* init;
  sc_solve_set* set; sc_solve_pair* pair; sc_solve_summary* sum;
};

// the workspace has its room: the image staged, the memset and the launches
int solve_enqueue(sc_ctx* c, PairGraph& g, const sc_solve_params* sp, const SolveStrides& st, const SolveArrays& d) {
  PairGraphStaged m;
  SC_TRY(pair_graph_stage(c, g, c->solve_meta, true, &m));
  double thr[3];
  solve_thresholds(sp, thr);
  const SolveLayout l = solve_layout(g.n_sets, g.n_pairs);
  char* const pa = static_cast<char*>(c->solve_pair.p);
  char* const sa = static_cast<char*>(c->solve_set.p);
  char* const ca = static_cast<char*>(c->solve_ctl.p);
  SolveJob job{};
  job.rec = m.rec; job.entries = m.entries; job.off = m.starts;
  job.pose = d.pose; job.pose_stride = st.pose; job.status = solve_reads_status(sp);
  job.use = d.use; job.use_stride = st.use;
  job.info = d.info; job.info_stride = st.info; job.info_status = solve_reads_info_status(sp);
  job.init = d.init; job.init_stride = st.init;
  job.wide = reinterpret_cast<double*>(pa + l.wide); job.W = reinterpret_cast<double*>(pa + l.W); job.g = reinterpret_cast<double*>(pa + l.g);
  job.err = reinterpret_cast<double*>(pa + l.err); job.usable = reinterpret_cast<uint32_t*>(pa + l.usable);
  job.X = reinterpret_cast<double*>(sa + l.X); job.x = reinterpret_cast<double*>(sa + l.x); job.r = reinterpret_cast<double*>(sa + l.r);
  job.z = reinterpret_cast<double*>(sa + l.z); job.q = reinterpret_cast<double*>(sa + l.q); job.p = reinterpret_cast<double*>(sa + l.p);
  job.fac = reinterpret_cast<double*>(sa + l.fac); job.sinfo = reinterpret_cast<SolveInfo*>(sa + l.sinfo);
  job.ctl = reinterpret_cast<SolveCtl*>(ca); job.deg = reinterpret_cast<uint32_t*>(ca + l.deg);
  job.rzc = reinterpret_cast<double*>(ca + l.rzc); job.pqc = reinterpret_cast<double*>(ca + l.pqc); job.costc = reinterpret_cast<double*>(ca + l.costc);
  job.set = reinterpret_cast<SolveSetRecord*>(d.set); job.pair = reinterpret_cast<SolvePairRecord*>(d.pair);
  job.sum = reinterpret_cast<SolveSummary*>(d.sum);
  job.r2_max = thr[0]; job.e2_max = thr[1]; job.cg2 = thr[2];
  job.n_sets = g.n_sets; job.n_pairs = g.n_pairs; job.anchor = sp->anchor; job.max_outer = sp->max_outer; job.max_inner = sp->max_inner;
  HIPCHK(c, hipMemsetAsync(ca, 0, (size_t)l.zero_bytes, c->stream));  // the control words and the sets' tallies of usable pairs
  launch_pairs_solve(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// Both forms.  host: the arrays are the caller's, staged around the enqueue (HostArrays); else the device's, and there is no wait.
int solve_call(sc_ctx* c, const char* who, bool host, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_solve_params* sp,
               const SolveStrides& st, const SolveArrays& a) {
  if (!c) return SC_EINVAL;
  if (!pairs || !sp || !a.pose || !a.init || !a.set || !a.pair || !a.sum) return refuse(c, who, "a NULL argument");
  const char* broken = solve_params_error(sp);
  if (!broken) broken = solve_stride_error(sp, st.pose, a.use != nullptr, st.use, a.info != nullptr, st.info, st.init);
  PairGraph g;
  SC_TRY(pair_graph_check(c, who, broken, n_sets, pairs, n_pairs, &sp->anchor, &g));
  SC_TRY(solve_room(c, g));
  if (!host) return solve_enqueue(c, g, sp, st, a);
  HostArrays h(c);
  const int a_pose = h.in(a.pose, (size_t)pose_bytes_read(n_pairs, st.pose, solve_reads_status(sp)));
  const int a_use = h.in(a.use, a.use ? (size_t)sync_use_bytes_read(n_pairs, st.use) : 0);
  const int a_info = h.in(a.info, a.info ? (size_t)solve_info_bytes_read(n_pairs, st.info, solve_reads_info_status(sp)) : 0);
  const int a_init = h.in(a.init, (size_t)solve_init_bytes_read(n_sets, st.init));
  const int a_set = h.out(a.set, (size_t)n_sets * sizeof(sc_solve_set)), a_pair = h.out(a.pair, (size_t)n_pairs * sizeof(sc_solve_pair)),
            a_sum = h.out(a.sum, sizeof(sc_solve_summary));
  return h.run([&] {
    return solve_enqueue(c, g, sp, st,
                         SolveArrays{h.at<void>(a_pose), h.at<void>(a_use), h.at<void>(a_info), h.at<void>(a_init), h.at<sc_solve_set>(a_set),
                                     h.at<sc_solve_pair>(a_pair), h.at<sc_solve_summary>(a_sum)});
  });
}

}  // namespace

extern "C" {

int sc_solve_default_params(sc_solve_params* sp) {
  if (!sp) return SC_EINVAL;
  memset(sp, 0, sizeof(*sp));
  sp->size = sizeof(sc_solve_params);
  sp->max_outer = 8;
  sp->max_inner = 64;
  return SC_OK;
}

int sc_solve_thresholds(const sc_solve_params* sp, double out[3]) {
  if (!sp || !out) return SC_EINVAL;
  if (solve_params_error(sp)) return SC_EINVAL;
  solve_thresholds(sp, out);
  return SC_OK;
}

int sc_pairs_solve_device(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_solve_params* sp, const void* d_pose,
                          uint32_t pose_stride, const void* d_use, uint32_t use_stride, const void* d_info, uint32_t info_stride,
                          const void* d_init, uint32_t init_stride, sc_solve_set* d_set, sc_solve_pair* d_pair, sc_solve_summary* d_sum) {
  return solve_call(c, "sc_pairs_solve_device", false, n_sets, pairs, n_pairs, sp, SolveStrides{pose_stride, use_stride, info_stride, init_stride},
                    SolveArrays{d_pose, d_use, d_info, d_init, d_set, d_pair, d_sum});
}

int sc_pairs_solve(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_solve_params* sp, const void* pose,
                   uint32_t pose_stride, const void* use, uint32_t use_stride, const void* info, uint32_t info_stride, const void* init,
                   uint32_t init_stride, sc_solve_set* set, sc_solve_pair* pair, sc_solve_summary* sum) {
  return solve_call(c, "sc_pairs_solve", true, n_sets, pairs, n_pairs, sp, SolveStrides{pose_stride, use_stride, info_stride, init_stride},
                    SolveArrays{pose, use, info, init, set, pair, sum});
}

}  // extern "C"
