// sc_capi_sync.hip — the C ABI's absolute poses of a pair list's sets (include/saccot.h, sc_pairs_sync): sc_sync_default_params,
// sc_sync_thresholds, sc_pairs_sync_device and sc_pairs_sync.  Host-only, on the context and the helpers of sc_ctx.hpp; the kernels
// are sc_sync.hip's, the rules of the list, the adjacency build and the staged image sc_cycles_check.hpp's, the rules of the
// parameters and the strides and the layout of the workspace sc_sync_check.hpp's.
//
// The host steps are every pair-list entry's (sc_capi_graph.hpp): the check, then the image of the list staged once per call — with
// the n_sets + 1 list starts: a round's wave owns a set, not a pair — -> a memset of the round words -> prepare, max_rounds round
// launches, finish: max_rounds + 4 stream operations whatever the list, and no wait in the device form.  Everything that can refuse
// a call is decided on the host before anything is enqueued.
#include "sc_capi_graph.hpp"
#include "sc_sync_check.hpp"

using namespace sc;

static_assert(sizeof(sc_sync_params) == 32 && sizeof(sc_sync_set) == 160 && sizeof(sc_sync_pair) == 32 && sizeof(sc_sync_summary) == 32,
              "sc_sync_params is 32 bytes, sc_sync_set 160, sc_sync_pair 32, sc_sync_summary 32");

namespace {

// the workspace of the device form
int sync_room(sc_ctx* c, const PairGraph& g) {
  ENSURE(c, c->sync_meta, pair_graph_meta_bytes(g, true));
  ENSURE(c, c->sync_wide, (size_t)sync_wide_bytes(g.n_pairs));
  ENSURE(c, c->sync_state, (size_t)sync_state_bytes(g.n_sets));
  return SC_OK;
}

struct SyncArrays {
  const void* pose; const void* use; const float* weight;
  sc_sync_set* set; sc_sync_pair* pair; sc_sync_summary* sum;
};

// the workspace has its room: the image staged, the memset and the launches
int sync_enqueue(sc_ctx* c, PairGraph& g, const sc_sync_params* sp, uint32_t pose_stride, uint32_t use_stride, const SyncArrays& d) {
  PairGraphStaged m;
  SC_TRY(pair_graph_stage(c, g, c->sync_meta, true, &m));
  double thr[2];
  sync_thresholds(sp, thr);
  char* const state = static_cast<char*>(c->sync_state.p);
  SyncJob job{};
  job.rec = m.rec; job.entries = m.entries; job.off = m.starts;
  job.pose = d.pose; job.pose_stride = pose_stride; job.status = sync_reads_status(sp);
  job.use = d.use; job.use_stride = use_stride; job.weight = d.weight;
  job.wide = c->sync_wide.as<double>();
  job.wt = reinterpret_cast<double*>(static_cast<char*>(c->sync_wide.p) + sync_weight_at(g.n_pairs));
  job.ctl = reinterpret_cast<SyncCtl*>(state);
  job.state = reinterpret_cast<SyncState*>(state + SYNC_CTL_BYTES);
  job.info = reinterpret_cast<SyncInfo*>(state + sync_info_at(g.n_sets));
  job.set = reinterpret_cast<SyncSetRecord*>(d.set); job.pair = reinterpret_cast<SyncPairRecord*>(d.pair);
  job.sum = reinterpret_cast<SyncSummary*>(d.sum);
  job.r2_max = thr[0]; job.e2_max = thr[1];
  job.n_sets = g.n_sets; job.n_pairs = g.n_pairs; job.anchor = sp->anchor; job.max_rounds = sp->max_rounds;
  HIPCHK(c, hipMemsetAsync(job.ctl, 0, SYNC_CTL_BYTES, c->stream));  // the rounds add into the words, finish into its tallies
  launch_pairs_sync(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

// Both forms.  host: the arrays are the caller's, staged around the enqueue (HostArrays); else the device's, and there is no wait.
int sync_call(sc_ctx* c, const char* who, bool host, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_sync_params* sp,
              uint32_t pose_stride, uint32_t use_stride, const SyncArrays& a) {
  if (!c) return SC_EINVAL;
  if (!pairs || !sp || !a.pose || !a.set || !a.pair || !a.sum) return refuse(c, who, "a NULL argument");
  const char* broken = sync_params_error(sp);
  if (!broken) broken = sync_stride_error(sp, pose_stride, a.use != nullptr, use_stride);
  PairGraph g;
  SC_TRY(pair_graph_check(c, who, broken, n_sets, pairs, n_pairs, &sp->anchor, &g));
  SC_TRY(sync_room(c, g));
  if (!host) return sync_enqueue(c, g, sp, pose_stride, use_stride, a);
  HostArrays h(c);
  const int a_pose = h.in(a.pose, (size_t)pose_bytes_read(n_pairs, pose_stride, sync_reads_status(sp)));
  const int a_use = h.in(a.use, a.use ? (size_t)sync_use_bytes_read(n_pairs, use_stride) : 0);
  const int a_weight = h.in(a.weight, (size_t)n_pairs * 4);
  const int a_set = h.out(a.set, (size_t)n_sets * sizeof(sc_sync_set)), a_pair = h.out(a.pair, (size_t)n_pairs * sizeof(sc_sync_pair)),
            a_sum = h.out(a.sum, sizeof(sc_sync_summary));
  return h.run([&] {
    return sync_enqueue(c, g, sp, pose_stride, use_stride,
                        SyncArrays{h.at<void>(a_pose), h.at<void>(a_use), h.at<float>(a_weight), h.at<sc_sync_set>(a_set), h.at<sc_sync_pair>(a_pair),
                                   h.at<sc_sync_summary>(a_sum)});
  });
}

}  // namespace

extern "C" {

int sc_sync_default_params(sc_sync_params* sp) {
  if (!sp) return SC_EINVAL;
  memset(sp, 0, sizeof(*sp));
  sp->size = sizeof(sc_sync_params);
  sp->max_rounds = 32;
  return SC_OK;
}

int sc_sync_thresholds(const sc_sync_params* sp, double out[2]) {
  if (!sp || !out) return SC_EINVAL;
  if (sync_params_error(sp)) return SC_EINVAL;
  sync_thresholds(sp, out);
  return SC_OK;
}

int sc_pairs_sync_device(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_sync_params* sp, const void* d_pose,
                         uint32_t pose_stride, const void* d_use, uint32_t use_stride, const float* d_weight, sc_sync_set* d_set,
                         sc_sync_pair* d_pair, sc_sync_summary* d_sum) {
  return sync_call(c, "sc_pairs_sync_device", false, n_sets, pairs, n_pairs, sp, pose_stride, use_stride,
                   SyncArrays{d_pose, d_use, d_weight, d_set, d_pair, d_sum});
}

int sc_pairs_sync(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_sync_params* sp, const void* pose,
                  uint32_t pose_stride, const void* use, uint32_t use_stride, const float* weight, sc_sync_set* set, sc_sync_pair* pair,
                  sc_sync_summary* sum) {
  return sync_call(c, "sc_pairs_sync", true, n_sets, pairs, n_pairs, sp, pose_stride, use_stride, SyncArrays{pose, use, weight, set, pair, sum});
}

}  // extern "C"
