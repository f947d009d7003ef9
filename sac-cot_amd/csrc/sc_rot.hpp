// sc_rot.hpp — rot(M) of include/saccot.h (sc_pairs_sync's Definitions): the rotation nearest a 3 x 3 matrix, with the two small
// vector operations it is written in.  Every operation is a plain rounded product, sum, quotient or square root in the order
// written: the files that include this say `#pragma clang fp contract(off)` themselves, and the library is built with
// -ffp-contract=off.  Device code only; two users, which must agree bit for bit: sc_sync.hip (a round's update) and sc_solve.hip (a
// Gauss-Newton step).
#pragma once
#include <hip/hip_runtime.h>

namespace sc {

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// The header's rot(M): refine_solve's construction (sc_refine.hpp) on H = M^T with every fma taken apart.  R may come out not
// finite (a sum of rank below two): the caller looks.
__device__ __forceinline__ void rot_plain(const double (&M)[9], double (&R)[9]) {
  double B[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int r = 0; r < 3; r++) B[c][r] = M[3 * c + r];
#pragma unroll 1
  for (int sweep = 0; sweep < 10; sweep++) {
#pragma unroll
    for (int pr = 0; pr < 3; pr++) {
      const int ip = (pr == 2) ? 1 : 0, iq = (pr == 0) ? 1 : 2;
      const double alpha = dot3(B[ip], B[ip]), beta = dot3(B[iq], B[iq]), gamma = dot3(B[ip], B[iq]);
      if (gamma != 0.0) {
        const double zeta = (beta - alpha) / (gamma + gamma);
        double tt = 1.0 / (__builtin_fabs(zeta) + __builtin_sqrt(zeta * zeta + 1.0));
        if (zeta < 0.0) tt = -tt;
        const double cs = 1.0 / __builtin_sqrt(tt * tt + 1.0);
        const double sn = cs * tt;
#pragma unroll
        for (int r = 0; r < 3; r++) {
          double x = B[ip][r], y = B[iq][r];
          B[ip][r] = cs * x - sn * y;
          B[iq][r] = sn * x + cs * y;
          x = V[ip][r]; y = V[iq][r];
          V[ip][r] = cs * x - sn * y;
          V[iq][r] = sn * x + cs * y;
        }
      }
    }
  }
  const double n0 = dot3(B[0], B[0]), n1 = dot3(B[1], B[1]), n2 = dot3(B[2], B[2]);
  int i1 = 0; double m1 = n0;
  if (n1 > m1) { i1 = 1; m1 = n1; }
  if (n2 > m1) { i1 = 2; m1 = n2; }
  int i2 = (i1 == 0) ? 1 : 0;
  {
    const int c = 3 - i1 - i2;
    const double nc = (c == 0) ? n0 : (c == 1 ? n1 : n2), ni2 = (i2 == 0) ? n0 : (i2 == 1 ? n1 : n2);
    if (nc > ni2) i2 = c;
  }
  double b1[3], b2[3], v1[3], v2[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    b1[r] = (i1 == 0) ? B[0][r] : (i1 == 1 ? B[1][r] : B[2][r]);
    b2[r] = (i2 == 0) ? B[0][r] : (i2 == 1 ? B[1][r] : B[2][r]);
    v1[r] = (i1 == 0) ? V[0][r] : (i1 == 1 ? V[1][r] : V[2][r]);
    v2[r] = (i2 == 0) ? V[0][r] : (i2 == 1 ? V[1][r] : V[2][r]);
  }
  const double s1 = __builtin_sqrt(dot3(b1, b1)), s2 = __builtin_sqrt(dot3(b2, b2));
  double u1[3], u2[3], u3[3], v3[3];
#pragma unroll
  for (int r = 0; r < 3; r++) { u1[r] = b1[r] / s1; u2[r] = b2[r] / s2; }
  cross3(u1, u2, u3);
  cross3(v1, v2, v3);
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) R[3 * r + c] = (v1[r] * u1[c] + v2[r] * u2[c]) + v3[r] * u3[c];
}

}  // namespace sc
