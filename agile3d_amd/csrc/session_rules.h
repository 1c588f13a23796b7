// The two rules of the session's view that more than one translation unit evaluates (session.hip, session_region.hip):
// the ray of a pixel and the side of a section's planes a vertex lies on.  Stated in include/agile3d_hip.h at a3d_camera
// and a3d_section; every operation rounded on its own, in the order written.
#pragma once
#include "common.h"

#include <cmath>

namespace a3d {

// The ray of pixel (u, v): the header's formula, one rounding per operation.
__host__ __device__ inline void ses_pixel_ray(const a3d_camera& c, int u, int v, float* d) {
#pragma clang fp contract(off)
  const float fu = (float)u, fv = (float)v;
  const float x = (c.d00[0] + fu * c.du[0]) + fv * c.dv[0];
  const float y = (c.d00[1] + fu * c.du[1]) + fv * c.dv[1];
  const float z = (c.d00[2] + fu * c.du[2]) + fv * c.dv[2];
  const float len = sqrtf((x * x + y * y) + z * z);
  d[0] = x / len, d[1] = y / len, d[2] = z / len;
}

// Whether a cloud's vertex shows: on the kept side of every plane (a NaN fails).
__device__ __forceinline__ bool ses_keeps(const a3d_section& s, float x, float y, float z) {
#pragma clang fp contract(off)
  bool keep = true;
  for (int k = 0; k < s.n_planes; ++k) {
    const float side = (s.planes[k][0] * x + s.planes[k][1] * y) + s.planes[k][2] * z;
    keep = keep && side >= s.planes[k][3];
  }
  return keep;
}

}  // namespace a3d
