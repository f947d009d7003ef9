// The yardstick of tools/pairs_cycles_bench.py: round 1 of sc_pairs_cycles — every pair's cycles and ok — by ONE host thread over the
// same adjacency (sac-cot_amd/csrc/sc_cycles_check.hpp), the same fp64 chains in the same order.  Reads a file the tool wrote:
//   u32 n_sets, u32 n_pairs, f64 tr_min, f64 e2_max, then 2 x n_pairs u32 of pairs, then 12 x n_pairs f32 of poses (all finite).
// Prints one line: build_ms (the adjacency), loop_ms (widening and the counting pass), triangles, consistent, and a checksum of the
// per-pair counts (the sum of cycles * 3 + ok over the pairs) that the tool holds against the GPU's records.
//   g++ -O2 -std=c++17 -ffp-contract=off tools/pairs_cycles_host.cpp -o tools/pairs_cycles_host
#include <chrono>
#include <cstdio>
#include <vector>

#include "../sac-cot_amd/csrc/sc_cycles_check.hpp"

struct T64 { double R[9], t[3]; };

static T64 inverse(const T64& A) {
  T64 I;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) I.R[3 * i + j] = A.R[3 * j + i];
  for (int c = 0; c < 3; c++) I.t[c] = -((A.R[c] * A.t[0] + A.R[3 + c] * A.t[1]) + A.R[6 + c] * A.t[2]);
  return I;
}
static T64 compose(const T64& B, const T64& A) {
  T64 M;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) M.R[3 * i + j] = ((B.R[3 * i] * A.R[j] + B.R[3 * i + 1] * A.R[3 + j]) + B.R[3 * i + 2] * A.R[6 + j]);
    M.t[i] = ((B.R[3 * i] * A.t[0] + B.R[3 * i + 1] * A.t[1]) + B.R[3 * i + 2] * A.t[2]) + B.t[i];
  }
  return M;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[2];
  double thr[2];
  if (fread(head, 4, 2, f) != 2 || fread(thr, 8, 2, f) != 2) return 2;
  const uint32_t n_sets = head[0], n_pairs = head[1];
  std::vector<uint32_t> pairs(2 * (size_t)n_pairs);
  std::vector<float> rt(12 * (size_t)n_pairs);
  if (fread(pairs.data(), 4, pairs.size(), f) != pairs.size() || fread(rt.data(), 4, rt.size(), f) != rt.size()) return 2;
  fclose(f);
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  std::vector<uint32_t> off((size_t)n_sets + 1), rec((size_t)sc::CYCLES_REC_WORDS * n_pairs);
  if (sc::cycles_list_error(n_sets, pairs.data(), n_pairs, off.data())) return 3;
  std::vector<uint64_t> ent(sc::cycles_entry_count(pairs.data(), n_pairs));
  sc::cycles_adjacency(n_sets, pairs.data(), n_pairs, off.data(), ent.data(), rec.data());
  const auto t1 = clk::now();
  std::vector<T64> up(n_pairs), down(n_pairs);  // lower -> higher set, higher -> lower
  for (uint32_t p = 0; p < n_pairs; p++) {
    T64 A;
    for (int c = 0; c < 9; c++) A.R[c] = rt[12 * (size_t)p + c];
    for (int c = 0; c < 3; c++) A.t[c] = rt[12 * (size_t)p + 9 + c];
    const bool fwd = rec[(size_t)sc::CYCLES_REC_WORDS * p + sc::CW_FWD] != 0;
    up[p] = fwd ? A : inverse(A);
    down[p] = fwd ? inverse(A) : A;
  }
  uint64_t triangles = 0, consistent = 0, checksum = 0;
  for (uint32_t p = 0; p < n_pairs; p++) {
    const uint32_t* r = &rec[(size_t)sc::CYCLES_REC_WORDS * p];
    const uint32_t lo = r[sc::CW_LO], hi = r[sc::CW_HI];
    uint32_t i = r[sc::CW_LO_BEGIN], j = r[sc::CW_HI_BEGIN], cnt = 0, ok = 0;
    const uint32_t ie = r[sc::CW_LO_END], je = r[sc::CW_HI_END];
    while (i < ie && j < je) {  // the two sorted lists merged; a run against a run is every combination
      const uint32_t zi = sc::cycles_entry_set(ent[i]), zj = sc::cycles_entry_set(ent[j]);
      if (zi < zj) { i++; continue; }
      if (zj < zi) { j++; continue; }
      uint32_t i1 = i, j1 = j;
      while (i1 < ie && sc::cycles_entry_set(ent[i1]) == zi) i1++;
      while (j1 < je && sc::cycles_entry_set(ent[j1]) == zi) j1++;
      for (uint32_t x = i; x < i1; x++)
        for (uint32_t y = j; y < j1; y++) {
          const uint32_t e1 = sc::cycles_entry_pair(ent[x]), e2 = sc::cycles_entry_pair(ent[y]);
          const T64 *P, *Q, *C;
          if (zi < lo)      { P = &up[e1]; Q = &up[p];  C = &down[e2]; }
          else if (zi < hi) { P = &up[e1]; Q = &up[e2]; C = &down[p]; }
          else              { P = &up[p];  Q = &up[e2]; C = &down[e1]; }
          const T64 E = compose(*C, compose(*Q, *P));
          const double tr = (E.R[0] + E.R[4]) + E.R[8], e2v = (E.t[0] * E.t[0] + E.t[1] * E.t[1]) + E.t[2] * E.t[2];
          const bool good = tr >= thr[0] && e2v <= thr[1];
          cnt++; ok += good;
          if (zi > hi) { triangles++; consistent += good; }
        }
      i = i1; j = j1;
    }
    checksum += (uint64_t)cnt * 3 + ok;
  }
  const auto t2 = clk::now();
  printf("{\"build_ms\": %.3f, \"loop_ms\": %.3f, \"triangles\": %llu, \"consistent\": %llu, \"checksum\": %llu}\n",
         std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count(),
         (unsigned long long)triangles, (unsigned long long)consistent, (unsigned long long)checksum);
  return 0;
}
