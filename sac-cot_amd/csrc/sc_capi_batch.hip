// sc_capi_batch.hip — the C ABI's batched registration (include/saccot.h, sc_register_batch): sc_register_batch_device and
// sc_register_batch.  Host-only, on the context and the helpers of sc_ctx.hpp; the kernel is sc_batch.hip's.  What every batch
// entry shares on the host is defined here as well: batch_params_check, batch_offsets_error, the pinned staging area
// (batch_staging_begin / _send), batch_offsets_to_device, and HostArrays, the one statement of a host-array entry.
//
// offsets -> pinned staging -> device copy (enqueued) -> ONE launch, a workgroup per problem.  Nothing is read back: a problem's
// status is a field of its record.  Everything that can refuse the call is decided on the host before anything is enqueued.
#include "sc_ctx.hpp"

using namespace sc;

namespace {

constexpr uint32_t BATCH_FLAGS_IGNORED = SC_FLAG_NO_DENSE_S | SC_FLAG_NO_PRUNE | SC_FLAG_EXACT_TOTAL;  // result-neutral

int batch_check(sc_ctx* c, const uint32_t* offset, uint32_t n_problems, const sc_params* p) {
  SC_TRY(entry_checks(c, nullptr, ENDS_FRAME | NOT_BUSY));
  SC_TRY(batch_params_check(c, p, "sc_register_batch"));
  if (const char* what = batch_offsets_error(offset, n_problems)) return refuse(c, "sc_register_batch", what);
  return SC_OK;
}

int batch_enqueue(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                  sc_batch_result* d_res, uint8_t* d_mask) {
  SC_TRY(batch_offsets_to_device(c, offset, n_problems, c->batch_off));
  BatchJob job = batch_job_of(p);
  job.src = d_src; job.tgt = d_tgt; job.offset = c->batch_off.as<uint32_t>();
  job.n_problems = n_problems; job.total = offset[n_problems];
  job.res = reinterpret_cast<BatchRecord*>(d_res); job.mask = d_mask;
  launch_batch_register(job, c->stream);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace

namespace sc {

int batch_params_check(sc_ctx* c, const sc_params* p, const char* who) {
  if (check_params(p) != SC_OK) return refuse(c, who, "bad sc_params (size, a range, or a mode)");
  if (p->shard_world != 1) return refuse(c, who, "shard_world must be 1");
  if (p->flags & ~BATCH_FLAGS_IGNORED)
    return refuse(c, who, "only SC_FLAG_NO_DENSE_S, SC_FLAG_NO_PRUNE and SC_FLAG_EXACT_TOTAL are accepted (no refit, no timing, no estimated bound in a batch)");
  return SC_OK;
}

const char* batch_offsets_error(const uint32_t* offset, uint32_t n_problems) {
  if (n_problems == 0) return "n_problems == 0";
  for (uint32_t b = 0; b < n_problems; b++) {
    if (offset[b + 1] < offset[b]) return "offsets decrease";
    const uint32_t nb = offset[b + 1] - offset[b];
    if (nb < 3 || nb > SC_BATCH_MAX_N) return "a problem has fewer than 3 or more than SC_BATCH_MAX_N correspondences";
  }
  if (offset[n_problems] > (1u << 31)) return "more than 2^31 correspondences in all";
  return nullptr;
}

int batch_staging_begin(sc_ctx* c, size_t bytes) {
  if (!c->batch_off_ev) HIPCHK(c, hipEventCreateWithFlags(&c->batch_off_ev, hipEventDisableTiming));
  else HIPCHK(c, hipEventSynchronize(c->batch_off_ev));
  if (c->h_batch_off_cap < bytes) {
    if (c->h_batch_off) { (void)hipHostFree(c->h_batch_off); c->h_batch_off = nullptr; c->h_batch_off_cap = 0; }
    const size_t sz = bytes + bytes / 4 + 4096;
    if (hipHostMalloc(&c->h_batch_off, sz, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError(); c->h_batch_off = nullptr; c->last_error = "hipHostMalloc failed"; return SC_ENOMEM;
    }
    c->h_batch_off_cap = sz;
  }
  return SC_OK;
}

int batch_staging_send(sc_ctx* c, Buf& dst, size_t bytes) {
  HIPCHK(c, hipMemcpyAsync(dst.p, c->h_batch_off, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->batch_off_ev, c->stream));
  return SC_OK;
}

int batch_offsets_to_device(sc_ctx* c, const uint32_t* offset, uint32_t n_problems, Buf& dst) {
  const size_t bytes = batch_offsets_bytes(n_problems);
  ENSURE(c, dst, bytes);
  SC_TRY(batch_staging_begin(c, bytes));
  memcpy(c->h_batch_off, offset, bytes);
  return batch_staging_send(c, dst, bytes);
}

int HostArrays::room() {
  if (n > MAX || n_also > MAX_ALSO) return refuse(c, "HostArrays", "more arrays than it holds");
  if (c->host_arr_live) return refuse(c, "HostArrays", "a second one on this context");
  for (int i = 0; i < n; i++)
    if (arr[i].from || arr[i].to) ENSURE(c, c->host_arr[i], arr[i].bytes);
  for (int i = 0; i < n_also; i++) ENSURE(c, *more[i], more_bytes[i]);
  c->host_arr_live = true;  // until finish
  return SC_OK;
}

int HostArrays::send() {
  for (int i = 0; i < n; i++)
    if (arr[i].from) HIPCHK(c, hipMemcpyAsync(c->host_arr[i].p, arr[i].from, arr[i].bytes, hipMemcpyHostToDevice, c->stream));
  return SC_OK;
}

int HostArrays::fetch() {
  for (int pass = 0; pass < 2; pass++)  // those declared `first`, then the others
    for (int i = 0; i < n; i++)
      if (arr[i].to && arr[i].first == (pass == 0))
        HIPCHK(c, hipMemcpyAsync(arr[i].to, c->host_arr[i].p, arr[i].bytes, hipMemcpyDeviceToHost, c->stream));
  return SC_OK;
}

// rc: what the copies in and the enqueue came to.  The wait comes whatever rc is, and a failed step's status before the wait's own.
int HostArrays::finish(int rc) {
  if (rc == SC_OK) rc = fetch();
  const hipError_t waited = hipStreamSynchronize(c->stream);
  c->host_arr_live = false;
  SC_TRY(rc);
  HIPCHK(c, waited);
  HIPCHK(c, hipGetLastError());
  return SC_OK;
}

}  // namespace sc

extern "C" {

int sc_register_batch_device(sc_ctx* c, const float* d_src, const float* d_tgt, const uint32_t* offset, uint32_t n_problems,
                             const sc_params* p, sc_batch_result* d_res, uint8_t* d_mask) {
  if (!c) return SC_EINVAL;
  if (!d_src || !d_tgt || !offset || !p || !d_res || !d_mask) return refuse(c, "sc_register_batch_device", "a NULL argument");
  SC_TRY(batch_check(c, offset, n_problems, p));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  return batch_enqueue(c, d_src, d_tgt, offset, n_problems, p, d_res, d_mask);
}

int sc_register_batch(sc_ctx* c, const float* src, const float* tgt, const uint32_t* offset, uint32_t n_problems, const sc_params* p,
                      sc_batch_result* res, uint8_t* mask) {
  if (!c) return SC_EINVAL;
  if (!src || !tgt || !offset || !p || !res || !mask) return refuse(c, "sc_register_batch", "a NULL argument");
  SC_TRY(batch_check(c, offset, n_problems, p));
  HIPCHK(c, hipSetDevice(c->device));
  c->cap_bytes = workspace_cap(p);
  const size_t total = offset[n_problems], pts = total * 12;
  HostArrays h(c);
  const int a_src = h.in(src, pts), a_tgt = h.in(tgt, pts);
  const int a_res = h.out(res, (size_t)n_problems * sizeof(sc_batch_result)), a_mask = h.out(mask, total);
  h.also(c->batch_off, batch_offsets_bytes(n_problems));
  return h.run([&] {
    return batch_enqueue(c, h.at<float>(a_src), h.at<float>(a_tgt), offset, n_problems, p, h.at<sc_batch_result>(a_res), h.at<uint8_t>(a_mask));
  });
}

}  // extern "C"
