// sc_capi_solve.hip — the C ABI's Gauss-Newton pose-graph solve of a pair list's sets (include/saccot.h, sc_pairs_solve):
// sc_solve_default_params, sc_solve_thresholds, sc_pairs_solve_device and sc_pairs_solve.  Host-only, on the context and the helpers
// of sc_ctx.hpp; the kernels are sc_solve.hip's, the rules of the list and the adjacency build sc_cycles_check.hpp's, the staged
// words sc_sync_check.hpp's, the rules of the parameters, the strides and the anchor and the layout of the workspace
// sc_solve_check.hpp's.
//
// The sequence is sc_pairs_sync's (sc_capi_sync.hip): the adjacency built once per call from the list alone -> pinned staging -> ONE
// device copy (enqueued) -> a memset of the control words and the sets' tallies -> the launches:
// 2 + 5 + max_outer * (4 + 2 * max_inner) stream operations whatever the list, and no wait in the device form.  Everything that can
// refuse a call is decided on the host before anything is enqueued.
#include <new>
#include <vector>

#include "sc_ctx.hpp"
#include "sc_solve_check.hpp"

using namespace sc;

static_assert(sizeof(sc_solve_params) == 32 && sizeof(sc_solve_set) == 160 && sizeof(sc_solve_pair) == 48 && sizeof(sc_solve_summary) == 64,
              "sc_solve_params is 32 bytes, sc_solve_set 160, sc_solve_pair 48, sc_solve_summary 64");

namespace {

// every refusal of the two entries, in this order: the frame ends, a call outstanding, the parameter block, the strides, the list,
// the anchor.  off: n_sets + 1 words on return — scratch of the list check, and then the adjacency's offsets.
int solve_check(sc_ctx* c, const char* who, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_solve_params* sp,
                uint32_t pose_stride, bool has_use, uint32_t use_stride, bool has_info, uint32_t info_stride, uint32_t init_stride,
                std::vector<uint32_t>* off) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  if (const char* what = solve_params_error(sp)) return refuse(c, who, what);
  if (const char* what = solve_stride_error(sp, pose_stride, has_use, use_stride, has_info, info_stride, init_stride)) return refuse(c, who, what);
  if (const char* what = cycles_counts_error(n_sets, n_pairs)) return refuse(c, who, what);
  try {
    off->assign((size_t)n_sets + 1, 0u);
  } catch (const std::bad_alloc&) {
    c->last_error = std::string(who) + ": no host memory for n_sets + 1 words";
    return SC_ENOMEM;
  }
  if (const char* what = cycles_list_error(n_sets, pairs, n_pairs, off->data())) return refuse(c, who, what);
  if (const char* what = solve_anchor_error(sp, n_sets)) return refuse(c, who, what);
  HIPCHK(c, hipSetDevice(c->device));
  return SC_OK;
}

// the workspace of the device form
int solve_room(sc_ctx* c, uint32_t n_sets, uint32_t n_pairs, uint64_t n_entries) {
  const SolveLayout l = solve_layout(n_sets, n_pairs);
  ENSURE(c, c->solve_meta, (size_t)sync_meta_bytes(n_sets, n_pairs, n_entries));
  ENSURE(c, c->solve_pair, (size_t)l.pair_bytes);
  ENSURE(c, c->solve_set, (size_t)l.set_bytes);
  ENSURE(c, c->solve_ctl, (size_t)l.ctl_bytes);
  return SC_OK;
}

struct SolveArrays {
  const void* pose; const void* use; const void* info; const void* init;
  sc_solve_set* set; sc_solve_pair* pair; sc_solve_summary* sum;
};

// the workspace has its room: the adjacency and the list starts into the staging area, its copy, the memset and the launches
int solve_enqueue(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, uint64_t n_entries, const sc_solve_params* sp,
                  uint32_t* off, uint32_t pose_stride, uint32_t use_stride, uint32_t info_stride, uint32_t init_stride, const SolveArrays& d) {
  const size_t rec_bytes = (size_t)CYCLES_REC_WORDS * 4 * n_pairs, off_at = (size_t)sync_off_at(n_pairs, n_entries),
               meta_bytes = (size_t)sync_meta_bytes(n_sets, n_pairs, n_entries);
  SC_TRY(batch_staging_begin(c, meta_bytes));
  char* const h = static_cast<char*>(c->h_batch_off);
  cycles_adjacency(n_sets, pairs, n_pairs, off, reinterpret_cast<uint64_t*>(h + rec_bytes), reinterpret_cast<uint32_t*>(h));
  memcpy(h + off_at, off, ((size_t)n_sets + 1) * 4);
  SC_TRY(batch_staging_send(c, c->solve_meta, meta_bytes));
  double thr[3];
  solve_thresholds(sp, thr);
  const SolveLayout l = solve_layout(n_sets, n_pairs);
  const char* const meta = static_cast<const char*>(c->solve_meta.p);
  char* const pa = static_cast<char*>(c->solve_pair.p);
  char* const sa = static_cast<char*>(c->solve_set.p);
  char* const ca = static_cast<char*>(c->solve_ctl.p);
  SolveJob job{};
  job.rec = reinterpret_cast<const uint32_t*>(meta);
  job.entries = reinterpret_cast<const uint64_t*>(meta + rec_bytes);
  job.off = reinterpret_cast<const uint32_t*>(meta + off_at);
  job.pose = d.pose; job.pose_stride = pose_stride; job.status = solve_reads_status(sp);
  job.use = d.use; job.use_stride = use_stride;
  job.info = d.info; job.info_stride = info_stride; job.info_status = solve_reads_info_status(sp);
  job.init = d.init; job.init_stride = init_stride;
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
  job.n_sets = n_sets; job.n_pairs = n_pairs; job.anchor = sp->anchor; job.max_outer = sp->max_outer; job.max_inner = sp->max_inner;
  HIPCHK(c, hipMemsetAsync(ca, 0, (size_t)l.zero_bytes, c->stream));  // the control words and the sets' tallies of usable pairs
  launch_pairs_solve(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
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
  static const char* const who = "sc_pairs_solve_device";
  if (!c) return SC_EINVAL;
  if (!pairs || !sp || !d_pose || !d_init || !d_set || !d_pair || !d_sum) return refuse(c, who, "a NULL argument");
  std::vector<uint32_t> off;
  SC_TRY(solve_check(c, who, n_sets, pairs, n_pairs, sp, pose_stride, d_use != nullptr, use_stride, d_info != nullptr, info_stride, init_stride, &off));
  const uint64_t n_entries = cycles_entry_count(pairs, n_pairs);
  SC_TRY(solve_room(c, n_sets, n_pairs, n_entries));
  return solve_enqueue(c, n_sets, pairs, n_pairs, n_entries, sp, off.data(), pose_stride, use_stride, info_stride, init_stride,
                       SolveArrays{d_pose, d_use, d_info, d_init, d_set, d_pair, d_sum});  // (no wait: the outputs are complete in stream order)
}

int sc_pairs_solve(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_solve_params* sp, const void* pose,
                   uint32_t pose_stride, const void* use, uint32_t use_stride, const void* info, uint32_t info_stride, const void* init,
                   uint32_t init_stride, sc_solve_set* set, sc_solve_pair* pair, sc_solve_summary* sum) {
  static const char* const who = "sc_pairs_solve";
  if (!c) return SC_EINVAL;
  if (!pairs || !sp || !pose || !init || !set || !pair || !sum) return refuse(c, who, "a NULL argument");
  std::vector<uint32_t> off;
  SC_TRY(solve_check(c, who, n_sets, pairs, n_pairs, sp, pose_stride, use != nullptr, use_stride, info != nullptr, info_stride, init_stride, &off));
  const uint64_t n_entries = cycles_entry_count(pairs, n_pairs);
  SC_TRY(solve_room(c, n_sets, n_pairs, n_entries));
  HostArrays h(c);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(n_pairs, pose_stride, solve_reads_status(sp)));
  const int a_use = h.in(use, use ? (size_t)sync_use_bytes_read(n_pairs, use_stride) : 0);
  const int a_info = h.in(info, info ? (size_t)solve_info_bytes_read(n_pairs, info_stride, solve_reads_info_status(sp)) : 0);
  const int a_init = h.in(init, (size_t)solve_init_bytes_read(n_sets, init_stride));
  const int a_set = h.out(set, (size_t)n_sets * sizeof(sc_solve_set)), a_pair = h.out(pair, (size_t)n_pairs * sizeof(sc_solve_pair)),
            a_sum = h.out(sum, sizeof(sc_solve_summary));
  return h.run([&] {
    return solve_enqueue(c, n_sets, pairs, n_pairs, n_entries, sp, off.data(), pose_stride, use_stride, info_stride, init_stride,
                         SolveArrays{h.at<void>(a_pose), h.at<void>(a_use), h.at<void>(a_info), h.at<void>(a_init), h.at<sc_solve_set>(a_set),
                                     h.at<sc_solve_pair>(a_pair), h.at<sc_solve_summary>(a_sum)});
  });
}

}  // extern "C"
