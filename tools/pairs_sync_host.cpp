// The yardstick of tools/pairs_sync_bench.py: the rounds of sc_pairs_sync (include/saccot.h) by ONE host thread over the same
// adjacency (sac-cot_amd/csrc/sc_cycles_check.hpp), the same fp64 chains in the same order — the 64 slots, the fold, rot(M) —, every
// pair usable with weight 1.0, anchor 0.  Reads a file the tool wrote:
//   u32 n_sets, u32 n_pairs, u32 max_rounds, u32 0, f64 r2_max, f64 e2_max, then 2 x n_pairs u32 of pairs, then 12 x n_pairs f32 of
//   poses (all finite).
// Prints one line: build_ms (the adjacency), solve_ms (widening and the rounds), rounds, converged, known, and a checksum — the XOR
// of the bit patterns of every known set's twelve doubles — that the tool holds against the GPU's records.
//   g++ -O2 -std=c++17 -ffp-contract=off tools/pairs_sync_host.cpp -o tools/pairs_sync_host
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
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
static double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
// the header's rot(M)
static void rot(const double* M, double* R) {
  double B[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) B[c][r] = M[3 * c + r];
  for (int sweep = 0; sweep < 10; sweep++)
    for (int pr = 0; pr < 3; pr++) {
      const int ip = (pr == 2) ? 1 : 0, iq = (pr == 0) ? 1 : 2;
      const double alpha = dot3(B[ip], B[ip]), beta = dot3(B[iq], B[iq]), gamma = dot3(B[ip], B[iq]);
      if (gamma != 0.0) {
        const double zeta = (beta - alpha) / (gamma + gamma);
        double tt = 1.0 / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
        if (zeta < 0.0) tt = -tt;
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = cs * tt;
        for (int r = 0; r < 3; r++) {
          double x = B[ip][r], y = B[iq][r];
          B[ip][r] = cs * x - sn * y; B[iq][r] = sn * x + cs * y;
          x = V[ip][r]; y = V[iq][r];
          V[ip][r] = cs * x - sn * y; V[iq][r] = sn * x + cs * y;
        }
      }
    }
  const double n[3] = {dot3(B[0], B[0]), dot3(B[1], B[1]), dot3(B[2], B[2])};
  int i1 = 0; double m1 = n[0];
  if (n[1] > m1) { i1 = 1; m1 = n[1]; }
  if (n[2] > m1) { i1 = 2; m1 = n[2]; }
  int i2 = (i1 == 0) ? 1 : 0;
  const int c = 3 - i1 - i2;
  if (n[c] > n[i2]) i2 = c;
  const double s1 = sqrt(dot3(B[i1], B[i1])), s2 = sqrt(dot3(B[i2], B[i2]));
  double u1[3], u2[3], u3[3], v3[3];
  for (int r = 0; r < 3; r++) { u1[r] = B[i1][r] / s1; u2[r] = B[i2][r] / s2; }
  cross3(u1, u2, u3);
  cross3(V[i1], V[i2], v3);
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) R[3 * r + k] = (V[i1][r] * u1[k] + V[i2][r] * u2[k]) + v3[r] * u3[k];
}

struct State { double X[12]; bool known; };

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[4];
  double thr[2];
  if (fread(head, 4, 4, f) != 4 || fread(thr, 8, 2, f) != 2) return 2;
  const uint32_t n_sets = head[0], n_pairs = head[1], max_rounds = head[2];
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
  std::vector<T64> wide(2 * (size_t)n_pairs);  // lower -> higher set, higher -> lower
  for (uint32_t p = 0; p < n_pairs; p++) {
    T64 A;
    for (int c = 0; c < 9; c++) A.R[c] = rt[12 * (size_t)p + c];
    for (int c = 0; c < 3; c++) A.t[c] = rt[12 * (size_t)p + 9 + c];
    const bool fwd = rec[(size_t)sc::CYCLES_REC_WORDS * p + sc::CW_FWD] != 0;
    wide[2 * (size_t)p] = fwd ? A : inverse(A);
    wide[2 * (size_t)p + 1] = fwd ? inverse(A) : A;
  }
  std::vector<State> buf[2];
  buf[0].assign(n_sets, State{});
  buf[1].assign(n_sets, State{});
  buf[0][0].X[0] = buf[0][0].X[4] = buf[0][0].X[8] = 1.0; buf[0][0].known = true;
  uint32_t K = max_rounds, converged = 0;
  for (uint32_t k = 1; k <= max_rounds; k++) {
    const std::vector<State>& prev = buf[(k - 1) & 1];
    std::vector<State>& cur = buf[k & 1];
    uint32_t changed = 0;
    for (uint32_t s = 0; s < n_sets; s++) {
      cur[s] = prev[s];
      if (s == 0) continue;
      double slot[64][13];
      memset(slot, 0, sizeof(slot));
      uint32_t live = 0;
      for (uint32_t i = off[s]; i < off[s + 1]; i++) {
        const uint32_t nb = sc::cycles_entry_set(ent[i]), p = sc::cycles_entry_pair(ent[i]);
        if (!prev[nb].known) continue;
        T64 Xn;
        memcpy(Xn.R, prev[nb].X, 72); memcpy(Xn.t, prev[nb].X + 9, 24);
        const T64 P = compose(Xn, wide[2 * (size_t)p + (s < nb ? 0 : 1)]);
        double* a = slot[(i - off[s]) & 63];
        for (int c = 0; c < 9; c++) a[c] = a[c] + 1.0 * P.R[c];
        for (int c = 0; c < 3; c++) a[9 + c] = a[9 + c] + 1.0 * P.t[c];
        a[12] = a[12] + 1.0;
        live++;
      }
      if (!live) continue;
      for (int h = 32; h > 0; h >>= 1)
        for (int j = 0; j < h; j++)
          for (int c = 0; c < 13; c++) slot[j][c] = slot[j][c] + slot[j + h][c];
      double X[12];
      rot(slot[0], X);
      bool fin = true;
      for (int c = 0; c < 3; c++) X[9 + c] = slot[0][9 + c] / slot[0][12];
      for (int c = 0; c < 12; c++) fin = fin && std::isfinite(X[c]);
      if (!fin) continue;
      double dR2 = 0, dt2 = 0;
      for (int c = 0; c < 9; c++) { const double d = X[c] - prev[s].X[c]; dR2 = c ? dR2 + d * d : d * d; }
      for (int c = 0; c < 3; c++) { const double d = X[9 + c] - prev[s].X[9 + c]; dt2 = c ? dt2 + d * d : d * d; }
      if (!prev[s].known || dR2 > thr[0] || dt2 > thr[1]) changed++;
      memcpy(cur[s].X, X, sizeof(X));
      cur[s].known = true;
    }
    if (!changed) { K = k; converged = 1; break; }
  }
  const auto t2 = clk::now();
  uint64_t checksum = 0; uint32_t known = 0;
  for (const State& s : buf[K & 1])
    if (s.known) {
      known++;
      for (int c = 0; c < 12; c++) { uint64_t b; memcpy(&b, &s.X[c], 8); checksum ^= b; }
    }
  printf("{\"build_ms\": %.3f, \"solve_ms\": %.3f, \"rounds\": %u, \"converged\": %u, \"known\": %u, \"checksum\": %llu}\n",
         std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count(), K, converged, known,
         (unsigned long long)checksum);
  return 0;
}
