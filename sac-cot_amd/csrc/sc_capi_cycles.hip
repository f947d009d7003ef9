// sc_capi_cycles.hip — the C ABI's loop-consistency check of a pair list (include/saccot.h, sc_pairs_cycles): sc_cycles_default_params,
// sc_cycles_thresholds, sc_pairs_cycles_device and sc_pairs_cycles.  Host-only, on the context and the helpers of sc_ctx.hpp; the
// kernels are sc_cycles.hip's, the rules of the parameters and of the list and the adjacency build sc_cycles_check.hpp's.
//
// The host knows the graph: it builds the adjacency once per call from the list alone and reads nothing from the device.  The pairs'
// records and the sorted neighbour entries -> pinned staging (the area and event every batch entry shares) -> ONE device copy
// (enqueued) -> a memset of the round words -> prepare, max_rounds round launches, finish: max_rounds + 4 stream operations whatever
// the list, and no wait in the device form — the stop is decided on the device (sc_cycles.hip).  Everything that can refuse a call
// is decided on the host before anything is enqueued.
#include <new>
#include <vector>

#include "sc_ctx.hpp"
#include "sc_cycles_check.hpp"

using namespace sc;

static_assert(sizeof(sc_cycle_params) == 32 && sizeof(sc_cycle_result) == 48 && sizeof(sc_cycle_summary) == 32,
              "sc_cycle_params is 32 bytes, sc_cycle_result 48, sc_cycle_summary 32");

namespace {

// every refusal of the two entries, in this order: the frame ends, a call outstanding, the parameter block, the stride, the list.
// off: n_sets + 1 words on return — scratch of the list check, and then the adjacency's offsets.
int cyc_check(sc_ctx* c, const char* who, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_cycle_params* cp,
              uint32_t pose_stride, std::vector<uint32_t>* off) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  if (const char* what = cycles_params_error(cp)) return refuse(c, who, what);
  if (const char* what = cycles_stride_error(cp, pose_stride)) return refuse(c, who, what);
  if (const char* what = cycles_counts_error(n_sets, n_pairs)) return refuse(c, who, what);
  try {
    off->assign((size_t)n_sets + 1, 0u);
  } catch (const std::bad_alloc&) {
    c->last_error = std::string(who) + ": no host memory for n_sets + 1 words";
    return SC_ENOMEM;
  }
  if (const char* what = cycles_list_error(n_sets, pairs, n_pairs, off->data())) return refuse(c, who, what);
  HIPCHK(c, hipSetDevice(c->device));
  return SC_OK;
}

// the workspace of the device form
int cyc_room(sc_ctx* c, uint32_t n_pairs, uint64_t n_entries) {
  ENSURE(c, c->cyc_meta, (size_t)cycles_meta_bytes(n_pairs, n_entries));
  ENSURE(c, c->cyc_wide, (size_t)cycles_pose_bytes(n_pairs));
  ENSURE(c, c->cyc_state, (size_t)cycles_state_bytes(n_pairs));
  return SC_OK;
}

// the workspace has its room: the adjacency into the staging area, its copy, the memset and the launches
int cyc_enqueue(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, uint64_t n_entries, const sc_cycle_params* cp,
                uint32_t* off, const void* d_pose, uint32_t pose_stride, const uint8_t* d_keep, sc_cycle_result* d_res, sc_cycle_summary* d_sum) {
  const size_t rec_bytes = (size_t)CYCLES_REC_WORDS * 4 * n_pairs, meta_bytes = (size_t)cycles_meta_bytes(n_pairs, n_entries);
  SC_TRY(batch_staging_begin(c, meta_bytes));
  char* const h = static_cast<char*>(c->h_batch_off);
  cycles_adjacency(n_sets, pairs, n_pairs, off, reinterpret_cast<uint64_t*>(h + rec_bytes), reinterpret_cast<uint32_t*>(h));
  SC_TRY(batch_staging_send(c, c->cyc_meta, meta_bytes));
  double thr[2];
  cycles_thresholds(cp, thr);
  CyclesJob job{};
  job.rec = c->cyc_meta.as<uint32_t>();
  job.entries = reinterpret_cast<const uint64_t*>(static_cast<const char*>(c->cyc_meta.p) + rec_bytes);
  job.pose = d_pose; job.pose_stride = pose_stride; job.status = cycles_reads_status(cp);
  job.keep = d_keep;
  job.wide = c->cyc_wide.as<double>();
  job.ctl = c->cyc_state.as<CyclesCtl>();
  job.alive = c->cyc_state.as<uint8_t>() + CYCLES_CTL_BYTES;
  job.res = reinterpret_cast<CycleRecord*>(d_res); job.sum = reinterpret_cast<CycleSummary*>(d_sum);
  job.tr_min = thr[0]; job.e2_max = thr[1];
  job.n_pairs = n_pairs; job.min_ok = cp->min_ok; job.max_rounds = cp->max_rounds;
  HIPCHK(c, hipMemsetAsync(job.ctl, 0, CYCLES_CTL_BYTES, c->stream));  // the rounds add into the words
  launch_pairs_cycles(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
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
  static const char* const who = "sc_pairs_cycles_device";
  if (!c) return SC_EINVAL;
  if (!pairs || !cp || !d_pose || !d_res || !d_sum) return refuse(c, who, "a NULL argument");
  std::vector<uint32_t> off;
  SC_TRY(cyc_check(c, who, n_sets, pairs, n_pairs, cp, pose_stride, &off));
  const uint64_t n_entries = cycles_entry_count(pairs, n_pairs);
  SC_TRY(cyc_room(c, n_pairs, n_entries));
  return cyc_enqueue(c, n_sets, pairs, n_pairs, n_entries, cp, off.data(), d_pose, pose_stride, d_keep, d_res, d_sum);  // (no wait: the outputs are complete in stream order)
}

int sc_pairs_cycles(sc_ctx* c, uint32_t n_sets, const uint32_t* pairs, uint32_t n_pairs, const sc_cycle_params* cp, const void* pose,
                    uint32_t pose_stride, const uint8_t* keep, sc_cycle_result* res, sc_cycle_summary* sum) {
  static const char* const who = "sc_pairs_cycles";
  if (!c) return SC_EINVAL;
  if (!pairs || !cp || !pose || !res || !sum) return refuse(c, who, "a NULL argument");
  std::vector<uint32_t> off;
  SC_TRY(cyc_check(c, who, n_sets, pairs, n_pairs, cp, pose_stride, &off));
  const uint64_t n_entries = cycles_entry_count(pairs, n_pairs);
  SC_TRY(cyc_room(c, n_pairs, n_entries));
  HostArrays h(c);
  const int a_pose = h.in(pose, (size_t)pose_bytes_read(n_pairs, pose_stride, cycles_reads_status(cp)));
  const int a_keep = h.in(keep, n_pairs);
  const int a_res = h.out(res, (size_t)n_pairs * sizeof(sc_cycle_result)), a_sum = h.out(sum, sizeof(sc_cycle_summary));
  return h.run([&] {
    return cyc_enqueue(c, n_sets, pairs, n_pairs, n_entries, cp, off.data(), h.at<void>(a_pose), pose_stride, h.at<uint8_t>(a_keep),
                       h.at<sc_cycle_result>(a_res), h.at<sc_cycle_summary>(a_sum));
  });
}

}  // extern "C"
