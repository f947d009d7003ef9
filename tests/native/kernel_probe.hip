// kernel_probe.hip — test access to the integer primitives under stage A's tail and stage B: extern "C" wrappers around launchers
// of sac-cot_amd/csrc/sc_kernels.hpp, linked against libsaccot.so (which exports them).  HOST CODE ONLY: no kernel lives here.
// A wrapper takes device pointers and a stream, builds the views and the Tuning from scalars, enqueues, and returns
// hipGetLastError().  Scratch is the caller's (tests put a sentinel behind it): kp_*_bytes says how much a wrapper carves, by the
// library's own helpers (scan_temp_bytes, sort_temp_bytes, row_stats_scan_state_bytes, compact_blocks); too little is KP_ESCRATCH
// before anything is launched.  tests/kernel_probe.py builds and loads this file.
//
// What each wrapper restates:
//   kp_scan, kp_scan_pair     the call sites of launch_scan_u32 / launch_scan_u32_pair; their ticket / err / desc / epoch arguments
//                             are an LbArgs as lb_next (sc_capi.hip) hands it out: ticket and err outside the descriptor area, the
//                             ticket zero at launch, the area zeroed when new and after epoch 4095, one epoch in 1 .. 4095 per launch
//   kp_sort                   launch_rank_order's call of launch_sort_u64 (sc_tri.hip)
//   kp_row_stats*, kp_shard_split   run_row_stats (sc_capi_compat.hip) and the split of run_edges (sc_capi_tri.hip)
//   kp_select_init            what key_range_kernel (preset == 0) or the key kernel's preset (preset == 1; sc_tri.hip) leave in a
//                             SelectState that the staging kernel had zeroed: kmin, kmax, st[0], want_req
//   kp_select_run             select_and_compact -> run_compaction (sc_capi_tri.hip): launch_select_rounds, launch_compact_count,
//                             launch_scan_u32_pair unless the write kernel sums the tile counts itself (the rule of run_compaction:
//                             tiles <= compact_self_max and M < 2^32), launch_compact_write
//   kp_select_read            the result words and the three histograms, copied out (the layout of SelectState stays in this file)
#include <cstring>

#include "../../sac-cot_amd/csrc/sc_kernels.hpp"

namespace {

constexpr int KP_ESCRATCH = -1001;

size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

sc::Tuning tuning(long long scan_self_max, long long compact_self_max, unsigned sel_blocks) {
  sc::Tuning tn;
  if (scan_self_max >= 0) tn.scan_self_max = (size_t)scan_self_max;
  if (compact_self_max >= 0) tn.compact_self_max = (size_t)compact_self_max;
  tn.sel_blocks = sel_blocks;
  return tn;
}

sc::Points rows_only(int n, int ld) { return sc::Points{nullptr, n, ld}; }  // (the row launches read n and ld alone)

// the compaction's scratch: tile counts, their prefixes, the scan's own
struct CompactScratch { uint32_t* blk_gt; uint32_t* blk_eq; uint64_t* off_gt; uint64_t* off_eq; void* scan_tmp; size_t bytes; };
CompactScratch carve(void* scratch, uint64_t M) {
  const size_t nb = sc::compact_blocks(M);
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(scratch);
  uintptr_t p = p0;
  CompactScratch s;
  s.blk_gt = reinterpret_cast<uint32_t*>(p); p += al256(nb * 4);
  s.blk_eq = reinterpret_cast<uint32_t*>(p); p += al256(nb * 4);
  s.off_gt = reinterpret_cast<uint64_t*>(p); p += al256((nb + 1) * 8);
  s.off_eq = reinterpret_cast<uint64_t*>(p); p += al256((nb + 1) * 8);
  s.scan_tmp = reinterpret_cast<void*>(p); p += al256(sc::scan_temp_bytes(nb));
  s.bytes = (size_t)(p - p0);
  return s;
}

}  // namespace

extern "C" {

// ---- scans ----------------------------------------------------------------------------------------------------------------
size_t kp_scan_temp_bytes(size_t n) { return sc::scan_temp_bytes(n); }

// scan_self_max < 0: the library's default.  epoch == 0: no LbArgs.  range, deg / degp / ebase, host_total: optional (null).
int kp_scan(const uint32_t* in, size_t n, uint64_t* out, void* temp, size_t temp_bytes, long long scan_self_max, uint32_t* ticket,
            uint32_t* err, uint64_t* desc, uint32_t epoch, const uint64_t* range, const uint32_t* deg, const uint32_t* degp,
            uint32_t* ebase, uint64_t* host_total, void* stream) {
  if (temp_bytes < sc::scan_temp_bytes(n)) return KP_ESCRATCH;
  const sc::Tuning tn = tuning(scan_self_max, -1, 0);
  sc::ScanExtra x;
  if (epoch) x.lb = sc::LbArgs{ticket, err, desc, epoch};
  x.range = range; x.deg = deg; x.degp = degp; x.ebase = ebase; x.host_total = host_total;
  sc::launch_scan_u32(sc::ScanWork{temp, tn}, in, n, out, x, (hipStream_t)stream);
  return (int)hipGetLastError();
}

// two arrays of one length (in_b null: one); host_total is array a's
int kp_scan_pair(const uint32_t* in_a, uint64_t* out_a, const uint32_t* in_b, uint64_t* out_b, size_t n, void* temp, size_t temp_bytes,
                 long long scan_self_max, uint64_t* host_total, void* stream) {
  if (temp_bytes < sc::scan_temp_bytes(n)) return KP_ESCRATCH;
  const sc::Tuning tn = tuning(scan_self_max, -1, 0);
  sc::ScanJob a{in_a, out_a, sc::ScanExtra{}}, b{in_b, out_b, sc::ScanExtra{}};
  a.x.host_total = host_total;
  sc::launch_scan_u32_pair(sc::ScanWork{temp, tn}, a, b, n, (hipStream_t)stream);
  return (int)hipGetLastError();
}

// ---- sort -----------------------------------------------------------------------------------------------------------------
size_t kp_sort_temp_bytes(size_t n) { return sc::sort_temp_bytes(n); }

int kp_sort(const uint64_t* in, uint64_t* out, size_t n, void* temp, size_t temp_bytes, void* stream) {
  if (temp_bytes < sc::sort_temp_bytes(n)) return KP_ESCRATCH;
  sc::launch_sort_u64(in, out, n, temp, sc::sort_temp_bytes(n), (hipStream_t)stream);
  return (int)hipGetLastError();
}

// ---- row statistics and the shard split ------------------------------------------------------------------------------------
int kp_row_stats(const uint64_t* bits, int n, int ld, uint32_t* deg, uint32_t* degp, uint32_t* wpre, uint64_t* zero_rows, uint32_t* rowcost,
                 void* stream) {
  sc::launch_row_stats(rows_only(n, ld), bits, sc::RowStats{deg, degp, wpre, zero_rows, rowcost}, (hipStream_t)stream);
  return (int)hipGetLastError();
}

size_t kp_row_stats_scan_state_bytes(int n) { return sc::row_stats_scan_state_bytes(n); }

int kp_row_stats_scan(const uint64_t* bits, int n, int ld, uint32_t* deg, uint32_t* degp, uint32_t* wpre, uint64_t* zero_rows,
                      uint64_t* edge_off, uint32_t* ebase, uint64_t* cost_pre, uint32_t* ticket, uint32_t* err, uint64_t* desc,
                      size_t desc_bytes, uint32_t epoch, uint64_t* host_total, void* stream) {
  if (desc_bytes < sc::row_stats_scan_state_bytes(n) || epoch == 0 || epoch > 4095) return KP_ESCRATCH;
  sc::launch_row_stats_scan(rows_only(n, ld), bits, sc::RowStats{deg, degp, wpre, zero_rows, nullptr}, sc::RowOffsets{edge_off, ebase, cost_pre},
                            sc::LbArgs{ticket, err, desc, epoch}, host_total, (hipStream_t)stream);
  return (int)hipGetLastError();
}

int kp_shard_split(const uint64_t* cost_pre, const uint64_t* edge_off, int n, uint32_t rank, uint32_t world, uint32_t* own_row,
                   uint64_t* own_edge, void* stream) {
  sc::launch_shard_split(sc::RowOffsets{const_cast<uint64_t*>(edge_off), nullptr, const_cast<uint64_t*>(cost_pre)},
                         sc::ShardCut{rank, world, own_row, own_edge}, n, (hipStream_t)stream);
  return (int)hipGetLastError();
}

// ---- select and compaction -------------------------------------------------------------------------------------------------
size_t kp_select_state_bytes(void) { return sizeof(sc::SelectState); }
size_t kp_compact_blocks(uint64_t M) { return sc::compact_blocks(M); }
size_t kp_select_scratch_bytes(uint64_t M) { return carve(nullptr, M).bytes; }

// fresh != 0: the whole state zeroed first (a new call's control block); 0: the histograms stay as the select before left them.
// preset == 0: the measured key range [kmin, kmax] (key_range_kernel); 1: the window [kmin, kmax] preset (the key kernel).
int kp_select_init(void* state, int fresh, int preset, uint32_t kmin, uint32_t kmax, uint64_t want, uint64_t want_req, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  sc::SelectState* d = static_cast<sc::SelectState*>(state);
  if (fresh) { if (hipMemsetAsync(d, 0, sizeof(sc::SelectState), st) != hipSuccess) return (int)hipGetLastError(); }
  static_assert(offsetof(sc::SelectState, hist) < 4096, "the words in front of the histograms");
  unsigned char head[offsetof(sc::SelectState, hist)];
  std::memset(head, 0, sizeof head);
  sc::SelectState* h = reinterpret_cast<sc::SelectState*>(head);  // (only the words in front of hist are touched)
  h->kmin = kmin; h->kmax = kmax; h->want_req = want_req;
  if (preset) {
    const uint32_t range_m1 = kmax - kmin;
    h->st[0] = sc::SelSnap{kmin, range_m1 == 0 ? 0u : (uint32_t)(32 - __builtin_clz(range_m1)), 1u, 0u, want, 0ull, 0ull, 0ull};
  } else {
    h->st[0] = sc::SelSnap{0u, 0u, 0u, 0u, want, 0ull, 0ull, 0ull};
  }
  if (hipStreamSynchronize(st) != hipSuccess) return (int)hipGetLastError();
  if (hipMemcpy(d, head, sizeof head, hipMemcpyHostToDevice) != hipSuccess) return (int)hipGetLastError();
  return (int)hipGetLastError();
}

// The view: seg_len == 0 plain (M keys at base), else M = segments x seg_len with valid / strides as KeyView has them.
// compact_self_max < 0: the library's default.  self_summed (optional, host): 1 when the write kernel summed the tile counts itself.
int kp_select_run(const uint32_t* base, uint64_t M, uint64_t seg_len, uint64_t seg_stride, const uint64_t* valid, uint64_t valid_stride,
                  void* state, int rounds, uint32_t sel_blocks, long long compact_self_max, void* scratch, size_t scratch_bytes,
                  uint64_t* sel_ord, uint32_t* sel_key, uint64_t n_sel, uint64_t* host_short, int* self_summed, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const CompactScratch cs = carve(scratch, M);
  if (scratch_bytes < cs.bytes) return KP_ESCRATCH;
  const sc::Tuning tn = tuning(-1, compact_self_max, sel_blocks);
  sc::SelectState* sel = static_cast<sc::SelectState*>(state);
  sc::KeyView view = sc::plain_view(base, M);
  if (seg_len) { view.seg_len = seg_len; view.seg_stride = seg_stride; view.valid = valid; view.valid_stride = valid_stride; }
  const size_t nb = sc::compact_blocks(M);
  sc::launch_select_rounds(view, sel, rounds, host_short, tn, st);
  sc::launch_compact_count(view, sel, rounds, cs.blk_gt, cs.blk_eq, host_short, st);
  const bool self_off = nb <= tn.compact_self_max && view.M < (1ull << 32);
  if (!self_off)
    sc::launch_scan_u32_pair(sc::ScanWork{cs.scan_tmp, tn}, sc::ScanJob{cs.blk_gt, cs.off_gt}, sc::ScanJob{cs.blk_eq, cs.off_eq}, nb, st);
  sc::launch_compact_write(view, sel, cs.blk_gt, cs.blk_eq, self_off ? nullptr : cs.off_gt, self_off ? nullptr : cs.off_eq,
                           sc::Selection{sel_ord, sel_key, n_sel}, st);
  if (self_summed) *self_summed = self_off ? 1 : 0;
  return (int)hipGetLastError();
}

// res[0..3] = kstar, done, want, need_eq; hist: 3 x 4096 words (waits for the stream)
int kp_select_read(const void* state, uint64_t* res, uint32_t* hist, void* stream) {
  static sc::SelectState h;  // (49 KiB: not on the stack)
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return (int)hipGetLastError();
  if (hipMemcpy(&h, state, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return (int)hipGetLastError();
  res[0] = h.kstar; res[1] = h.done; res[2] = h.want; res[3] = h.need_eq;
  std::memcpy(hist, h.hist, sizeof h.hist);
  return (int)hipGetLastError();
}

}  // extern "C"
