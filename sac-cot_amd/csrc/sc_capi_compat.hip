// sc_capi_compat.hip — stage A's host side: input staging (stage_inputs), the tile launch with its cache of XCD-aware block orders
// (run_compat) and the row statistics (run_row_stats), with the views of the row arrays (rows_of, offsets_of).  Host-only, on the
// context (sc_ctx.hpp); the kernels are sc_stage.hip's, sc_compat.hip's and sc_rows.hip's.  sc_capi.hip's hyp_begin and the stage hooks
// call the three; stage B's sequencer, which starts at the scan of the degrees, is sc_capi_tri.hip.
#include <vector>

#include "sc_ctx.hpp"

namespace sc {

// The views of the row arrays (sc_kernels.hpp), as they stand NOW: taken again behind whatever grows an array.
// deg / degp / wpre (run_compat ENSUREs them); whoever wants zero_rows or rowcost written sets them
RowStats rows_of(const sc_ctx* c) {
  return RowStats{c->deg.as<uint32_t>(), c->degp.as<uint32_t>(), c->wpre.as<uint32_t>(), nullptr, nullptr};
}
// the CSR row offsets and bases; sharded stage B: also the prefix of the row costs
RowOffsets offsets_of(const sc_ctx* c) {
  return RowOffsets{c->edge_off.as<uint64_t>(), c->ebase.as<uint32_t>(), c->pass.sharded_ab ? c->cost_pre.as<uint64_t>() : nullptr};
}

// user points (device) -> padded planes; zero the "non-finite" flag first
int stage_inputs(sc_ctx* c, const float* d_src, const float* d_tgt, int64_t n, const sc_params* p) {
  if (n < 3 || n > (1 << 24)) return SC_EINVAL;
  if (p->score_mode != SC_SCORE_COUNT && n > (1 << 21)) {  // 1024 n must stay below 2^31 (the score rides a u32)
    c->last_error = "score_mode MSE / MAE needs n <= 2^21";
    return SC_EINVAL;
  }
  c->pass.n = (int)n;
  c->pass.ld = round_up((int)n, 64);
  ENSURE(c, c->planes, (size_t)(6 + 8) * c->pass.ld * sizeof(float));  // 6 SoA planes + the AoS copy (8 floats each)
  // per-call control block (flags, histograms, counters, select state): cleared by the staging kernel itself
  ENSURE(c, c->ctl, sizeof(ControlBlock));
  static_assert(sizeof(ControlBlock) % 4 == 0, "cleared word-wise");
  c->pinned[HW_BAD_INPUT] = 0;  // "non-finite input" flag lives in host-pinned memory: the kernel only touches it on bad data
  if (!c->fx_mx.p) {  // coordinate statistics for C2's filters (written whole by every call's staging kernel) + its ticket
    ENSURE(c, c->fx_mx, (FX_MX_WORDS + 1) * 4);
    HIPCHK(c, hipMemsetAsync(c->fx_mx.p, 0, (FX_MX_WORDS + 1) * 4, c->stream));
  }
  ENSURE(c, c->fx_part, stage_part_words(c->pass.ld) * 4);
  c->pinned[HW_COORD_MAX] = ~0ull;  // "maxima not known yet"
  if (c->pass.form.build) ENSURE(c, c->degp, (size_t)c->pass.ld * sizeof(uint32_t));  // stage A accumulates deg+ there: cleared on the way
  const bool hf = c->pass.mode.host_free;  // (host-free: no ticket — stage A's launch reduces the rows, run_compat; finalize hands the words over, DeferredPub)
  const CoordStatsOut cs{c->fx_mx.as<uint32_t>(), c->fx_part.as<uint32_t>(), hf ? nullptr : c->fx_mx.as<uint32_t>() + FX_MX_WORDS,
                         hf ? nullptr : &c->pinned[HW_COORD_MAX], hf ? nullptr : &c->pinned[HW_BOX]};
  const ZeroSpan zero[2] = {{c->ctl.as<uint32_t>(), (uint32_t)(sizeof(ControlBlock) / 4)}, {c->pass.form.build ? c->degp.as<uint32_t>() : nullptr, c->pass.form.build ? (uint32_t)c->pass.ld : 0u}};
  launch_stage_points(cs, zero, d_src, d_tgt, c->pass.n, c->pass.ld, p->layout, c->planes.as<float>(),
                      reinterpret_cast<uint32_t*>(&c->pinned[HW_BAD_INPUT]), c->stream);
  return SC_OK;
}

// dense: also write the n x n weight matrix S (SC_FLAG_NO_DENSE_S clears it: nothing after stage A reads S)
// (r02 / r03 experiment, removed in r04: S from a second, low-priority stream while stage B runs — slower on every config,
// DESIGN.md §5 "measured and dropped")
int run_compat(sc_ctx* c, bool dense) {
  const size_t n = c->pass.n, ld = c->pass.ld, W = ld >> 6;
  if (dense) ENSURE(c, c->S, n * ld * sizeof(float));
  ENSURE(c, c->bits, n * W * sizeof(uint64_t));
  ENSURE(c, c->deg, n * sizeof(uint32_t));
  ENSURE(c, c->degp, ld * sizeof(uint32_t));
  ENSURE(c, c->wpre, n * W * sizeof(uint32_t));
  c->pass.bits_cur = c->bits.as<uint64_t>();
  c->pass.sharded_ab = false; c->pass.shard_phase = 0; c->pass.cand_all = nullptr;
  const uint32_t* map = nullptr;
  uint32_t map_len = 0;
  // The XCD-aware block order (sc_compat.hip compat_wg_map; made once per row width).  Measured r04 (profiles/r04_pmc_compat_xcd_order.txt):
  // HBM write bytes C2 115.8 -> 106.9 MB (algorithmic 103.2: 1.035 x), bits only 13.0 -> 5.1 MB; C3 1820 -> 1683 MB (1.02 x).  Time:
  // C2 25.0 -> 23.7 us, but at C3 the index order is FASTER (352 vs 369 - 389 us, alternating three times in one process) although it
  // writes more: each XCD then streams its S rows into one 512 x 512 corner of the matrix at a time.  So: by size, like the tile height.
  if (!c->tn.compat_linear_order && c->tn.compat_rows != 64 && (c->pass.n < 10000 || c->tn.compat_rows == 16)) {
    sc_ctx::WgMap* slot = nullptr;
    for (sc_ctx::WgMap& m : c->wg_maps) if (m.W == (int)W) slot = &m;
    if (!slot) {  // a width not met before (or evicted): the least recently used slot
      slot = &c->wg_maps[0];
      for (sc_ctx::WgMap& m : c->wg_maps) if (m.used < slot->used) slot = &m;
      const std::vector<uint32_t> m = compat_wg_map((int)W);
      ENSURE(c, slot->buf, m.size() * 4);
      HIPCHK(c, hipMemcpyAsync(slot->buf.p, m.data(), m.size() * 4, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));  // (m is a local: the copy must have left it; once per size)
      slot->W = (int)W; slot->len = (uint32_t)m.size();
    }
    slot->used = ++c->wg_map_clock;
    map = slot->buf.as<uint32_t>(); map_len = slot->len;
  }
  const CompatOpts opts{c->pass.form.build ? c->degp.as<uint32_t>() : nullptr, map, map_len,
                        c->pass.mode.host_free ? c->fx_part.as<uint32_t>() : nullptr, c->fx_mx.as<uint32_t>()};
  launch_compat(points_of(c), opts, c->pass.dv, dense ? c->S.as<float>() : nullptr, c->pass.bits_cur, 0, c->pass.n, c->tn, c->stream);
  return SC_OK;
}

// deg / deg+ / word-prefix popcounts from the bit rows (first kernel of stage B's timing bracket)
// hot: the fused form (row statistics + CSR offsets + edge count in one launch; run_edges then launches no scan)
int run_row_stats(sc_ctx* c, bool will_prune, bool hot) {
  c->pass.rows_fused = false;
  if (hot && c->pass.form.build) {  // launch_edge_build (run_edges) does all of it
    ENSURE(c, c->bits2, (size_t)c->pass.n * (c->pass.ld >> 6) * sizeof(uint64_t));
    return SC_OK;
  }
  if (will_prune)  // the pruned bit matrix is cleared on the way (no separate memset)
    ENSURE(c, c->bits2, (size_t)c->pass.n * (c->pass.ld >> 6) * sizeof(uint64_t));
  if (c->pass.sharded_ab)  // per-row work estimate: its prefix splits the rows between the ranks
    ENSURE(c, c->rowcost, ((size_t)c->pass.n + 4 + 1024) * 4);  // (cost_split_kernel reads whole 16-byte pieces)
  RowStats rs = rows_of(c);  // (deg, degp, wpre: run_compat's; the ENSUREs below are of the offsets)
  if (will_prune) rs.zero_rows = c->bits2.as<uint64_t>();
  if (c->pass.sharded_ab) rs.rowcost = c->rowcost.as<uint32_t>();
  // The fused form pays while the look-back stays shallow: 157 tiles at N = 5000 (12.7 us against 5.5 + 7.5 and a launch
  // gap, and edge_fill gets the precomputed bases: 15.8 -> 14.6); at N = 20 000 its 625 tiles cost 61 us against ~40.
  if (hot && !c->tn.rows_unfused && c->pass.n <= 8192) {
    const size_t n = c->pass.n;
    ENSURE(c, c->edge_off, (n + 1) * sizeof(uint64_t));
    ENSURE(c, c->ebase, n * 4);
    if (c->pass.sharded_ab) ENSURE(c, c->cost_pre, (n + 1) * sizeof(uint64_t));
    LbArgs lb;
    SC_TRY(lb_next(c, row_stats_scan_state_bytes(c->pass.n), 0, 0, &lb));
    arm_word(c, HW_EDGES);  // read-back #1 (the edge count) is published by this kernel
    launch_row_stats_scan(points_of(c), c->pass.bits_cur, rs, offsets_of(c), lb, &c->pinned[HW_EDGES], c->stream);
    c->pass.rows_fused = true;
    return SC_OK;
  }
  launch_row_stats(points_of(c), c->pass.bits_cur, rs, c->stream);
  return SC_OK;
}

}  // namespace sc
