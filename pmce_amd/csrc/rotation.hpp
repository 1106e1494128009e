// Device primitives on 3 x 3 matrices that more than one unit needs, each written once: the fp64 SVD by one-sided Jacobi with its small
// vector helpers (metrics.hip: the Procrustes alignment of PA-MPJPE; smpl_fit.hip: the per-joint orthogonal Procrustes step) and the
// rotation matrix -> axis-angle rule of the reference's geometry.py (hmr_head.hip: theta; smpl_fit.hip: the fitted pose).
#pragma once
#include "common.hpp"

// SVD of a 3x3 matrix by one-sided (Hestenes) Jacobi in fp64: the columns of A = H*V are rotated in pairs until they are mutually
// orthogonal; their norms are then the singular values and V holds the right singular vectors.  H itself is worked on, never H^T H:
// squaring H squares its condition number and leaves a small singular value known only to sqrt(eps) of the largest, which is what a
// thin, planar or collinear joint set (in a plane that is not axis-aligned) needs to be resolved.  On return A[:,c] = H V[:,c].
static __device__ void jacobi_svd3(double A[3][3], double V[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int k = 0; k < 3; ++k) {
          al += A[k][p] * A[k][p];
          be += A[k][q] * A[k][q];
          ga += A[k][p] * A[k][q];
        }
        if (!(ga * ga > 1e-30 * al * be)) continue;  // columns orthogonal to 1e-15 (or one of them zero, or NaN): nothing to do
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {  // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {  // V <- V J
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
    if (!rotated) break;
  }
}

// a <- a / |a|; false (a untouched) when |a|^2 is not above floor2, i.e. a is zero, rounding noise or NaN
static __device__ bool normalise3(double a[3], double floor2) {
  const double n2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
  if (!(n2 > floor2)) return false;
  const double inv = 1.0 / sqrt(n2);
  for (int k = 0; k < 3; ++k) a[k] *= inv;
  return true;
}

// r <- the coordinate axis that is furthest from the unit vector u, made orthogonal to u and normalised
static __device__ void any_orthogonal3(const double u[3], double r[3]) {
  const int k = (fabs(u[0]) <= fabs(u[1]) && fabs(u[0]) <= fabs(u[2])) ? 0 : (fabs(u[1]) <= fabs(u[2]) ? 1 : 2);
  for (int i = 0; i < 3; ++i) r[i] = (i == k ? 1.0 : 0.0) - u[k] * u[i];
  normalise3(r, 0.0);
}

static __device__ void cross3(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// rotation_matrix_to_angle_axis (reference lib/geometry.py:84-249) for one row-major matrix R[9], operation by operation as torch's fp32
// runs it (contraction off: torch fuses nothing): the four-case quaternion of :169-249 on the transpose the reference takes
// (rmat_t[i][j] = R[j][i]), then quaternion_to_angle_axis (:146-166), then aa[isnan(aa)] = 0 (:112).
__device__ __forceinline__ void rotmat_to_angle_axis(const float* R, float* aa) {
#pragma clang fp contract(off)
  const float R00 = R[0], R01 = R[1], R02 = R[2], R10 = R[3], R11 = R[4], R12 = R[5], R20 = R[6], R21 = R[7], R22 = R[8];
  const bool d2 = R22 < 1e-6f, d0_d1 = R00 > R11, d0_nd1 = R00 < -R11;
  float q0, q1, q2, q3, t;
  if (d2 && d0_d1) {
    t = 1.0f + R00 - R11 - R22;
    q0 = R21 - R12, q1 = t, q2 = R10 + R01, q3 = R02 + R20;
  } else if (d2) {
    t = 1.0f - R00 + R11 - R22;
    q0 = R02 - R20, q1 = R10 + R01, q2 = t, q3 = R21 + R12;
  } else if (d0_nd1) {
    t = 1.0f - R00 - R11 + R22;
    q0 = R10 - R01, q1 = R02 + R20, q2 = R21 + R12, q3 = t;
  } else {
    t = 1.0f + R00 + R11 + R22;
    q0 = t, q1 = R21 - R12, q2 = R02 - R20, q3 = R10 - R01;
  }
  const float rt = sqrtf(t);  // (t < 0: NaN, t = 0: a division by zero - both as in the reference, and NaN becomes 0 below)
  q0 = q0 / rt * 0.5f, q1 = q1 / rt * 0.5f, q2 = q2 / rt * 0.5f, q3 = q3 / rt * 0.5f;
  // geometry.py:146-166
  const float s2 = q1 * q1 + q2 * q2 + q3 * q3;
  const float sn = sqrtf(s2);
  const float two_theta = 2.0f * (q0 < 0.0f ? atan2f(-sn, -q0) : atan2f(sn, q0));
  const float k = s2 > 0.0f ? two_theta / sn : 2.0f;
  const float ax = q1 * k, ay = q2 * k, az = q3 * k;
  aa[0] = ax != ax ? 0.0f : ax;  // :112, aa[isnan(aa)] = 0
  aa[1] = ay != ay ? 0.0f : ay;
  aa[2] = az != az ? 0.0f : az;
}
