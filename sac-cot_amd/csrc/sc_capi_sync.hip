// sc_capi_sync.hip — the C ABI's absolute poses of a pair list's sets (include/saccot.h, sc_pairs_sync): sc_sync_default_params,
// sc_sync_thresholds, sc_pairs_sync_device and sc_pairs_sync.  Host-only, on the context and the helpers of sc_ctx.hpp; the kernels
// are sc_sync.hip's, the rules of the list and the adjacency build sc_cycles_check.hpp's, the rules of the parameters, the strides
// and the anchor and the layout of the staged words sc_sync_check.hpp's.
//
// The sequence is sc_pairs_cycles's (sc_capi_cycles.hip): the adjacency built once per call from the list alone -> pinned staging
// -> ONE device copy (enqueued) -> a memset of the round words -> prepare, max_rounds round launches, finish: max_rounds + 4 stream
// operations whatever the list, and no wait in the device form.  The staged words gain the n_sets + 1 list starts: a round's wave
// owns a set, not a pair.  Everything that can refuse a call is decided on the host before anything is enqueued.
#include <new>
#include <vector>

#include "sc_ctx.hpp"
#include "sc_sync_check.hpp"

using namespace sc;

static_assert(sizeof(sc_sync_params) == 32 && sizeof(sc_sync_set) == 160 && sizeof(sc_sync_pair) == 32 && sizeof(sc_sync_summary) == 32,
              "sc_sync_params is 32 bytes, sc_sync_set 160, sc_sync_pair 32, sc_sync_summary 32");

namespace {

// every refusal of the two entries, in this order: the frame ends, a call outstanding, the parameter block, the strides, the list,
// the anchor.  off: n_sets + 1 words on return — scratch of the list check, and then the adjacency's offsets.
int sync_check(sc_ctx* c, const char* who, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_sync_params* sp,
               uint32_t pose_stride, bool has_use, uint32_t use_stride, std::vector<uint32_t>* off) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  if (const char* what = sync_params_error(sp)) return refuse(c, who, what);
  if (const char* what = sync_stride_error(sp, pose_stride, has_use, use_stride)) return refuse(c, who, what);
  if (const char* what = cycles_counts_error(n_sets, n_pairs)) return refuse(c, who, what);
  try {
    off->assign((size_t)n_sets + 1, 0u);
  } catch (const std::bad_alloc&) {
    c->last_error = std::string(who) + ": no host memory for n_sets + 1 words";
    return SC_ENOMEM;
  }
  if (const char* what = cycles_list_error(n_sets, pairs, n_pairs, off->data())) return refuse(c, who, what);
  if (const char* what = sync_anchor_error(sp, n_sets)) return refuse(c, who, what);
  HIPCHK(c, hipSetDevice(c->device));
  return SC_OK;
}

// the workspace of the device form
int sync_room(sc_ctx* c, uint32_t n_sets, uint32_t n_pairs, uint64_t n_entries) {
  ENSURE(c, c->sync_meta, (size_t)sync_meta_bytes(n_sets, n_pairs, n_entries));
  ENSURE(c, c->sync_wide, (size_t)sync_wide_bytes(n_pairs));
  ENSURE(c, c->sync_state, (size_t)sync_state_bytes(n_sets));
  return SC_OK;
}

struct SyncArrays {
  const void* pose; const void* use; const float* weight;
  sc_sync_set* set; sc_sync_pair* pair; sc_sync_summary* sum;
};

// the workspace has its room: the adjacency and the list starts into the staging area, its copy, the memset and the launches
int sync_enqueue(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, uint64_t n_entries, const sc_sync_params* sp,
                 uint32_t* off, uint32_t pose_stride, uint32_t use_stride, const SyncArrays& d) {
  const size_t rec_bytes = (size_t)CYCLES_REC_WORDS * 4 * n_pairs, off_at = (size_t)sync_off_at(n_pairs, n_entries),
               meta_bytes = (size_t)sync_meta_bytes(n_sets, n_pairs, n_entries);
  SC_TRY(batch_staging_begin(c, meta_bytes));
  char* const h = static_cast<char*>(c->h_batch_off);
  cycles_adjacency(n_sets, pairs, n_pairs, off, reinterpret_cast<uint64_t*>(h + rec_bytes), reinterpret_cast<uint32_t*>(h));
  memcpy(h + off_at, off, ((size_t)n_sets + 1) * 4);
  SC_TRY(batch_staging_send(c, c->sync_meta, meta_bytes));
  double thr[2];
  sync_thresholds(sp, thr);
  const char* const meta = static_cast<const char*>(c->sync_meta.p);
  char* const state = static_cast<char*>(c->sync_state.p);
  SyncJob job{};
  job.rec = reinterpret_cast<const uint32_t*>(meta);
  job.entries = reinterpret_cast<const uint64_t*>(meta + rec_bytes);
  job.off = reinterpret_cast<const uint32_t*>(meta + off_at);
  job.pose = d.pose; job.pose_stride = pose_stride; job.status = sync_reads_status(sp);
  job.use = d.use; job.use_stride = use_stride; job.weight = d.weight;
  job.wide = c->sync_wide.as<double>();
  job.wt = reinterpret_cast<double*>(static_cast<char*>(c->sync_wide.p) + sync_weight_at(n_pairs));
  job.ctl = reinterpret_cast<SyncCtl*>(state);
  job.state = reinterpret_cast<SyncState*>(state + SYNC_CTL_BYTES);
  job.info = reinterpret_cast<SyncInfo*>(state + sync_info_at(n_sets));
  job.set = reinterpret_cast<SyncSetRecord*>(d.set); job.pair = reinterpret_cast<SyncPairRecord*>(d.pair);
  job.sum = reinterpret_cast<SyncSummary*>(d.sum);
  job.r2_max = thr[0]; job.e2_max = thr[1];
  job.n_sets = n_sets; job.n_pairs = n_pairs; job.anchor = sp->anchor; job.max_rounds = sp->max_rounds;
  HIPCHK(c, hipMemsetAsync(job.ctl, 0, SYNC_CTL_BYTES, c->stream));  // the rounds add into the words, finish into its tallies
  launch_pairs_sync(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
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
  static const char* const who = "sc_pairs_sync_device";
  if (!c) return SC_EINVAL;
  if (!pairs || !sp || !d_pose || !d_set || !d_pair || !d_sum) return refuse(c, who, "a NULL argument");
  std::vector<uint32_t> off;
  SC_TRY(sync_check(c, who, n_sets, pairs, n_pairs, sp, pose_stride, d_use != nullptr, use_stride, &off));
  const uint64_t n_entries = cycles_entry_count(pairs, n_pairs);
  SC_TRY(sync_room(c, n_sets, n_pairs, n_entries));
  return sync_enqueue(c, n_sets, pairs, n_pairs, n_entries, sp, off.data(), pose_stride, use_stride,
                      SyncArrays{d_pose, d_use, d_weight, d_set, d_pair, d_sum});  // (no wait: the outputs are complete in stream order)
}

int sc_pairs_sync(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_sync_params* sp, const void* pose,
                  uint32_t pose_stride, const void* use, uint32_t use_stride, const float* weight, sc_sync_set* set, sc_sync_pair* pair,
                  sc_sync_summary* sum) {
  static const char* const who = "sc_pairs_sync";
  if (!c) return SC_EINVAL;
  if (!pairs || !sp || !pose || !set || !pair || !sum) return refuse(c, who, "a NULL argument");
  std::vector<uint32_t> off;
  SC_TRY(sync_check(c, who, n_sets, pairs, n_pairs, sp, pose_stride, use != nullptr, use_stride, &off));
  const uint64_t n_entries = cycles_entry_count(pairs, n_pairs);
  SC_TRY(sync_room(c, n_sets, n_pairs, n_entries));
  HostArrays h(c);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(n_pairs, pose_stride, sync_reads_status(sp)));
  const int a_use = h.in(use, use ? (size_t)sync_use_bytes_read(n_pairs, use_stride) : 0);
  const int a_weight = h.in(weight, (size_t)n_pairs * 4);
  const int a_set = h.out(set, (size_t)n_sets * sizeof(sc_sync_set)), a_pair = h.out(pair, (size_t)n_pairs * sizeof(sc_sync_pair)),
            a_sum = h.out(sum, sizeof(sc_sync_summary));
  return h.run([&] {
    return sync_enqueue(c, n_sets, pairs, n_pairs, n_entries, sp, off.data(), pose_stride, use_stride,
                        SyncArrays{h.at<void>(a_pose), h.at<void>(a_use), h.at<float>(a_weight), h.at<sc_sync_set>(a_set), h.at<sc_sync_pair>(a_pair),
                                   h.at<sc_sync_summary>(a_sum)});
  });
}

}  // extern "C"
