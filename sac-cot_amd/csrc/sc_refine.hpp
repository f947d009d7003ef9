// sc_refine.hpp — the fp64 solve of the least-squares rigid refit: refine_solve, run by one thread behind the sums
// of the centroids and H in the canonical order of oracle/saccot_oracle.c::so_refine.  Two callers: refine_kernel (sc_final.hip: one
// refit over a given n-sized mask, a thread per chunk — its own lane deal) and refit_iterate (sc_refit.hpp: refits iterated to a
// fixed point, a lane per (chunk, component)), which polish_kernel (sc_polish.hip) and polish_batch_kernel (sc_polish_batch.hip)
// both instantiate.  Only the solve is shared between the two callers; the iteration around it is shared between the two kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace sc {

__device__ __forceinline__ double ddot3(const double* a, const double* b) {
  return __builtin_fma(a[2], b[2], __builtin_fma(a[1], b[1], a[0] * b[0]));
}
__device__ __forceinline__ void dcross3(const double* a, const double* b, double* c) {
  c[0] = __builtin_fma(a[1], b[2], -(a[2] * b[1]));
  c[1] = __builtin_fma(a[2], b[0], -(a[0] * b[2]));
  c[2] = __builtin_fma(a[0], b[1], -(a[1] * b[0]));
}

// H (row-major, sum (p - pc)(q - qc)^T), the centroids -> (R, t) rounded to fp32 in out[12]: the two-dominant-pairs + cross-product
// construction of kabsch3 in double with 10 Jacobi sweeps.  false (out untouched): the result is not finite.
__device__ __forceinline__ bool refine_solve(const double (&H)[9], const double (&pc)[3], const double (&qc)[3], float* out) {
  double B[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) B[c][r] = H[3 * r + c];
#pragma unroll 1
  for (int sweep = 0; sweep < 10; sweep++) {
#pragma unroll
    for (int pr = 0; pr < 3; pr++) {
      const int ip = (pr == 2) ? 1 : 0, iq = (pr == 0) ? 1 : 2;
      const double alpha = ddot3(B[ip], B[ip]), beta = ddot3(B[iq], B[iq]), gamma = ddot3(B[ip], B[iq]);
      if (gamma != 0.0) {
        const double zeta = (beta - alpha) / (gamma + gamma);
        double tt = 1.0 / (__builtin_fabs(zeta) + __builtin_sqrt(__builtin_fma(zeta, zeta, 1.0)));
        if (zeta < 0.0) tt = -tt;
        const double cs = 1.0 / __builtin_sqrt(__builtin_fma(tt, tt, 1.0));
        const double sn = cs * tt;
#pragma unroll
        for (int r = 0; r < 3; r++) {
          double x = B[ip][r], y = B[iq][r];
          B[ip][r] = __builtin_fma(-sn, y, cs * x);
          B[iq][r] = __builtin_fma(sn, x, cs * y);
          x = V[ip][r]; y = V[iq][r];
          V[ip][r] = __builtin_fma(-sn, y, cs * x);
          V[iq][r] = __builtin_fma(sn, x, cs * y);
        }
      }
    }
  }
  const double n0 = ddot3(B[0], B[0]), n1 = ddot3(B[1], B[1]), n2 = ddot3(B[2], B[2]);
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
  const double s1 = __builtin_sqrt(ddot3(b1, b1)), s2 = __builtin_sqrt(ddot3(b2, b2));
  double u1[3], u2[3], u3[3], v3[3];
#pragma unroll
  for (int r = 0; r < 3; r++) { u1[r] = b1[r] / s1; u2[r] = b2[r] / s2; }
  dcross3(u1, u2, u3);
  dcross3(v1, v2, v3);
  double R[9], t[3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) R[3 * r + c] = __builtin_fma(v3[r], u3[c], __builtin_fma(v2[r], u2[c], v1[r] * u1[c]));
#pragma unroll
  for (int r = 0; r < 3; r++)
    t[r] = qc[r] - __builtin_fma(R[3 * r + 2], pc[2], __builtin_fma(R[3 * r + 1], pc[1], R[3 * r] * pc[0]));
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; k++) ok = ok && (__builtin_fabs(R[k]) < __builtin_inf());
#pragma unroll
  for (int k = 0; k < 3; k++) ok = ok && (__builtin_fabs(t[k]) < __builtin_inf());
  if (!ok) return false;
#pragma unroll
  for (int k = 0; k < 9; k++) out[k] = (float)R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) out[9 + k] = (float)t[k];
  return true;
}

}  // namespace sc
