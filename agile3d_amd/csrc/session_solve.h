// The plane through a set of points from its integer sums -- stage B of a3d_estimate_normals -- one definition for every file
// that fits one: k_normals_solve (session_normals.hip), a3d_normals_solve on the host, and the rounds of a3d_find_planes
// (session_planes.hip).  The rule is stated in include/agile3d_hip.h at a3d_estimate_normals; a file includes this header, it
// does not copy from it.
#pragma once
#include "session_device.h"

namespace a3d {

constexpr int kNrmSweeps = 6;

// ---- stage B: one sequential double-precision computation per voxel ---------------------------------------------------------
// One Jacobi rotation of the pair (p, q), r the third index: the header's lines, one rounding each.
#define A3D_NRM_ROTATE(p, q, r)                                                          \
  do {                                                                                   \
    const double apq = C[p][q];                                                          \
    if (apq != 0.0) {                                                                    \
      const double app = C[p][p], aqq = C[q][q];                                         \
      const double theta = (aqq - app) / (2.0 * apq);                                    \
      double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));                        \
      if (theta < 0.0) t = -t;                                                           \
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, h = t * apq;                  \
      C[p][p] = app - h, C[q][q] = aqq + h, C[p][q] = 0.0;                               \
      const double arp = C[r][p], arq = C[r][q];                                         \
      C[r][p] = c * arp - s * arq, C[r][q] = s * arp + c * arq;                          \
      C[p][r] = C[r][p], C[q][r] = C[r][q], C[q][p] = 0.0;                               \
      _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                    \
        const double vkp = V[k][p], vkq = V[k][q];                                       \
        V[k][p] = c * vkp - s * vkq, V[k][q] = s * vkp + c * vkq;                        \
      }                                                                                  \
    }                                                                                    \
  } while (0)

// normal[3], variation of one neighbourhood from its integer sums; false: no valid normal (zeros)
__host__ __device__ inline bool nrm_solve(const long long N, const u64* S, const u64* M, const a3d_estimate_normals_args& a,
                                          float* normal, float& variation) {
#pragma clang fp contract(off)
  normal[0] = normal[1] = normal[2] = 0.f, variation = 0.f;
  if (N < 3) return false;
  // recentring about R = floor(S / N), in WRAPPING 64-bit arithmetic: the true s and m fit (header), so they come out exact
  long long R[3];
  u64 s[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long Sk = (long long)S[k];
    long long q = Sk / N;
    if (Sk % N < 0) --q;                       // floor
    R[k] = q;
    s[k] = S[k] - (u64)N * (u64)q;
  }
  double sd[3], C[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
  for (int k = 0; k < 3; ++k) sd[k] = (double)(long long)s[k];
  const double nd = (double)N;
  {
    constexpr int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int x = A[k], y = B[k];
      const u64 m = M[k] - (u64)R[x] * S[y] - (u64)R[y] * S[x] + (u64)N * (u64)R[x] * (u64)R[y];
      const double c = (double)(long long)m - (sd[x] * sd[y]) / nd;
      C[x][y] = c, C[y][x] = c;
    }
  }
  for (int sweep = 0; sweep < kNrmSweeps; ++sweep) {
    A3D_NRM_ROTATE(0, 1, 2);
    A3D_NRM_ROTATE(0, 2, 1);
    A3D_NRM_ROTATE(1, 2, 0);
  }
  const double d0 = C[0][0], d1 = C[1][1], d2 = C[2][2];
  int imin = 0, imax = 0;
  double dmin = d0, dmax = d0;
  if (d1 < dmin) imin = 1, dmin = d1;
  if (d2 < dmin) imin = 2, dmin = d2;
  if (d1 > dmax) imax = 1, dmax = d1;
  if (d2 > dmax) imax = 2, dmax = d2;
  const int imid = imin != imax ? 3 - imin - imax : imin;
  const double dmid = imid == 0 ? d0 : imid == 1 ? d1 : d2;
  if (!(dmid * 1048576.0 > dmax && dmax < __builtin_inf())) return false;
  double v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = imin == 0 ? V[k][0] : imin == 1 ? V[k][1] : V[k][2];
  bool flip;
  if (a.has_viewpoint) {
    double w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double mean = a.origin[k] + a.quantum * ((double)R[k] + sd[k] / nd);
      w[k] = a.viewpoint[k] - mean;
    }
    const double g = (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2];
    flip = g < 0.0;
  } else {
    double big = v[0];
    if (fabs(v[1]) > fabs(big)) big = v[1];
    if (fabs(v[2]) > fabs(big)) big = v[2];
    flip = big < 0.0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) normal[k] = (float)(flip ? -v[k] : v[k]);
  const double total = (d0 + d1) + d2;
  variation = total > 0.0 ? (float)((dmin > 0.0 ? dmin : 0.0) / total) : 0.f;
  return true;
}

}  // namespace a3d
