// Stand-alone program for the host-only rules of sc_pairs_solve (sac-cot_amd/csrc/sc_solve_check.hpp): every refusal of the
// parameter block, of the four strides and of the anchor with its text, the three thresholds, the bytes of the strided info and init
// arrays that a call reads, and where the workspace areas lie — on exactly sized heap copies, so that a read past one ends the run
// when this is built with -fsanitize=address,undefined (tests/test_solve_abi.py builds and runs it that way; no GPU, no Python in the
// process).  The list's rules, the adjacency and the staged words are sc_cycles_check.hpp's and sc_sync_check.hpp's and have programs
// of their own (cycles_check_main.cpp, sync_check_main.cpp).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../sac-cot_amd/csrc/sc_solve_check.hpp"

static int failures = 0;

static void check(const char* what, bool ok) {
  if (!ok) { printf("FAIL %s\n", what); failures++; }
}

static sc_solve_params params(uint32_t max_outer = 8, uint32_t max_inner = 64, uint32_t flags = 0, float rot_tol = 1e-6f, float trans_tol = 1e-6f,
                              float cg_tol = 1e-3f, uint32_t anchor = 0) {
  sc_solve_params sp;
  memset(&sp, 0, sizeof(sp));
  sp.size = sizeof(sp); sp.anchor = anchor; sp.max_outer = max_outer; sp.max_inner = max_inner; sp.flags = flags;
  sp.rot_tol = rot_tol; sp.trans_tol = trans_tol; sp.cg_tol = cg_tol;
  return sp;
}

struct Strides { uint32_t pose = 48; bool has_use = false; uint32_t use = 0; bool has_info = false; uint32_t info = 0; uint32_t init = 160; };

// the first rule that refuses (params, then the strides, then the anchor), as sc_capi_solve.hip asks them
static void expect(const char* what, const sc_solve_params& sp, const Strides& st, uint32_t n_sets, const char* want) {
  sc_solve_params* p = new sc_solve_params(sp);  // a heap copy of the exact size
  const char* got = sc::solve_params_error(p);
  if (!got) got = sc::solve_stride_error(p, st.pose, st.has_use, st.use, st.has_info, st.info, st.init);
  if (!got) got = sc::solve_anchor_error(p, n_sets);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  if (!ok) { printf("FAIL %s: got %s\n", what, got ? got : "(accepted)"); failures++; }
  delete p;
}

static Strides with(uint32_t pose, bool has_use, uint32_t use, bool has_info, uint32_t info, uint32_t init) {
  Strides s; s.pose = pose; s.has_use = has_use; s.use = use; s.has_info = has_info; s.info = info; s.init = init;
  return s;
}

int main() {
  const Strides plain;
  // ---- the parameter block
  expect("defaults", params(), plain, 3, nullptr);
  { sc_solve_params sp = params(); sp.size = 28; expect("size", sp, plain, 3, "params->size is not sizeof(sc_solve_params)"); }
  expect("max_outer 0", params(0), plain, 3, "max_outer must be 1 .. 32");
  expect("max_outer 33", params(33), plain, 3, "max_outer must be 1 .. 32");
  expect("max_outer 32", params(32), plain, 3, nullptr);
  expect("max_inner 0", params(8, 0), plain, 3, "max_inner must be 1 .. 256");
  expect("max_inner 257", params(8, 257), plain, 3, "max_inner must be 1 .. 256");
  expect("8 x 256", params(8, 256), plain, 3, nullptr);
  expect("9 x 256", params(9, 256), plain, 3, "max_outer * max_inner must not exceed 2048");
  expect("32 x 64", params(32, 64), plain, 3, nullptr);
  expect("32 x 65", params(32, 65), plain, 3, "max_outer * max_inner");
  expect("1 x 1", params(1, 1), plain, 3, nullptr);
  expect("rot_tol negative", params(8, 64, 0, -1e-9f), plain, 3, "rot_tol must be finite and in [0, pi]");
  expect("rot_tol NaN", params(8, 64, 0, NAN), plain, 3, "rot_tol");
  expect("rot_tol past pi", params(8, 64, 0, 3.1415930f), plain, 3, "rot_tol");
  expect("rot_tol pi", params(8, 64, 0, sc::CYCLES_ROT_TOL_MAX), plain, 3, nullptr);
  expect("trans_tol negative", params(8, 64, 0, 0.f, -1e-9f), plain, 3, "trans_tol must be finite and >= 0");
  expect("trans_tol inf", params(8, 64, 0, 0.f, INFINITY), plain, 3, "trans_tol");
  expect("cg_tol 1", params(8, 64, 0, 0.f, 0.f, 1.f), plain, 3, "cg_tol must be finite and in [0, 1)");
  expect("cg_tol negative", params(8, 64, 0, 0.f, 0.f, -1e-9f), plain, 3, "cg_tol");
  expect("cg_tol NaN", params(8, 64, 0, 0.f, 0.f, NAN), plain, 3, "cg_tol");
  expect("cg_tol inf", params(8, 64, 0, 0.f, 0.f, INFINITY), plain, 3, "cg_tol");
  expect("cg_tol just below 1", params(8, 64, 0, 0.f, 0.f, 0.99999994f), plain, 3, nullptr);
  expect("every tolerance 0", params(8, 64, 0, 0.f, 0.f, 0.f), plain, 3, nullptr);
  expect("unknown flag", params(8, 64, 4), with(52, false, 0, false, 0, 160), 3, "an unknown flag");
  // ---- the strides
  expect("pose_stride 44", params(), with(44, false, 0, false, 0, 160), 3, "pose_stride must be a multiple of 4 and at least 48 (52 with SC_SOLVE_STATUS)");
  expect("pose_stride 50", params(), with(50, false, 0, false, 0, 160), 3, "pose_stride");
  expect("pose_stride 48 with the status", params(8, 64, SC_SOLVE_STATUS), with(48, false, 0, false, 0, 160), 3, "pose_stride");
  expect("pose_stride 52 with the status", params(8, 64, SC_SOLVE_STATUS), with(52, false, 0, false, 0, 160), 3, nullptr);
  expect("use_stride 0", params(), with(48, true, 0, false, 0, 160), 3, "use_stride must be a multiple of 4 and at least 4");
  expect("use_stride 6", params(), with(48, true, 6, false, 0, 160), 3, "use_stride");
  expect("use_stride 48", params(), with(48, true, 48, false, 0, 160), 3, nullptr);
  expect("use_stride 6 without use", params(), with(48, false, 6, false, 0, 160), 3, nullptr);  // ignored with NULL
  expect("info_stride 280", params(), with(48, false, 0, true, 280, 160), 3, "info_stride must be a multiple of 8 and at least 288 (300 with SC_SOLVE_INFO_STATUS)");
  expect("info_stride 292", params(), with(48, false, 0, true, 292, 160), 3, "info_stride");
  expect("info_stride 288", params(), with(48, false, 0, true, 288, 160), 3, nullptr);
  expect("info_stride 296 with the status", params(8, 64, SC_SOLVE_INFO_STATUS), with(48, false, 0, true, 296, 160), 3, "info_stride");
  expect("info_stride 304 with the status", params(8, 64, SC_SOLVE_INFO_STATUS), with(48, false, 0, true, 304, 160), 3, nullptr);
  expect("info_stride 320 with the status", params(8, 64, SC_SOLVE_INFO_STATUS), with(48, false, 0, true, 320, 160), 3, nullptr);
  expect("info_stride 7 without info", params(8, 64, SC_SOLVE_INFO_STATUS), with(48, false, 0, false, 7, 160), 3, nullptr);  // ignored with NULL
  expect("init_stride 152", params(), with(48, false, 0, false, 0, 152), 3, "init_stride must be a multiple of 8 and at least 160");
  expect("init_stride 164", params(), with(48, false, 0, false, 0, 164), 3, "init_stride");
  expect("init_stride 168", params(), with(48, false, 0, false, 0, 168), 3, nullptr);
  // ---- the anchor
  expect("anchor == n_sets", params(8, 64, 0, 0.f, 0.f, 0.f, 3), plain, 3, "anchor must be less than n_sets");
  expect("anchor all ones", params(8, 64, 0, 0.f, 0.f, 0.f, 0xFFFFFFFFu), plain, 3, "anchor");
  expect("anchor n_sets - 1", params(8, 64, 0, 0.f, 0.f, 0.f, 2), plain, 3, nullptr);

  // ---- the thresholds: sync's two, and cg2
  {
    double out[3], two[2];
    const sc_solve_params sp = params(8, 64, 0, 0.25f, 0.5f, 0.125f);
    sc::solve_thresholds(&sp, out);
    check("thresholds", out[0] == 0.125 && out[1] == 0.25 && out[2] == 0.015625);
    sc_sync_params yp;
    memset(&yp, 0, sizeof(yp));
    yp.size = sizeof(yp); yp.max_rounds = 32; yp.rot_tol = 1e-6f; yp.trans_tol = 3e-5f;
    const sc_solve_params like = params(8, 64, 0, 1e-6f, 3e-5f, 1e-3f);
    sc::solve_thresholds(&like, out);
    sc::sync_thresholds(&yp, two);
    check("the first two are sync's", out[0] == two[0] && out[1] == two[1] && out[2] == (double)1e-3f * (double)1e-3f);
    const sc_solve_params zero = params(8, 64, 0, 0.f, 0.f, 0.f);
    sc::solve_thresholds(&zero, out);
    check("thresholds at 0", out[0] == 0.0 && out[1] == 0.0 && out[2] == 0.0);
  }

  // ---- the bytes read and the workspace
  check("info bytes", sc::solve_info_bytes_read(0, 320, true) == 0 && sc::solve_info_bytes_read(1, 320, true) == 300 && sc::solve_info_bytes_read(1, 288, false) == 288 &&
                          sc::solve_info_bytes_read(276, 320, true) == 275 * 320 + 300 && sc::solve_info_bytes_read(276, 288, false) == 276 * 288 &&
                          sc::solve_info_bytes_read(1u << 22, 0xFFFFFFF8u, false) == ((1ull << 22) - 1) * 0xFFFFFFF8ull + 288);
  check("init bytes", sc::solve_init_bytes_read(0, 160) == 0 && sc::solve_init_bytes_read(24, 160) == 24 * 160 && sc::solve_init_bytes_read(24, 176) == 23 * 176 + 160);
  {
    const sc::SolveLayout l = sc::solve_layout(65, 130);
    check("pair area", l.wide == 0 && l.W == 192 * 130 && l.g == l.W + 288 * 130 && l.err == l.g + 48 * 130 && l.usable == l.err + 48 * 130 && l.pair_bytes == 584 * 130);
    check("set area", l.X == 0 && l.x == 192 * 65 && l.p == l.x + 4 * 48 * 65 && l.fac == l.p + 96 * 65 && l.sinfo == l.fac + 168 * 65 && l.set_bytes == 664 * 65);
    check("ctl area", l.deg == sc::SOLVE_CTL_BYTES && l.zero_bytes == (sc::SOLVE_CTL_BYTES + 4 * 65 + 15) / 16 * 16 && l.zero_bytes % 16 == 0 && l.rzc == l.zero_bytes &&
                          l.pqc == l.rzc + 16 * 2 && l.costc == l.pqc + 8 * 2 && l.ctl_bytes == l.costc + 8 * 3 && l.rzc % 8 == 0);
    check("chunks", sc::solve_chunks(0) == 0 && sc::solve_chunks(1) == 1 && sc::solve_chunks(64) == 1 && sc::solve_chunks(65) == 2 && sc::solve_chunks(4097) == 65);
    const sc::SolveLayout big = sc::solve_layout(0xFFFFFFFFu, 1u << 22);
    check("no overflow", big.set_bytes == 664ull * 0xFFFFFFFFull && big.pair_bytes == 584ull << 22);
  }

  if (failures) { printf("%d failed\n", failures); return 1; }
  printf("all passed\n");
  return 0;
}
