// libagile3d_hip -- dropout of the training decoder outside the flash kernels: the keep mask for tests,
// the materialised attention path's probabilities (a3d_attn_dropout), and the row-wise sites -- the out_proj / linear2
// outputs before their residual add and the FFN's hidden activations (a3d_dropout_rows_forward / _backward).  Every
// kernel decides four consecutive columns of one logical row per Philox call (common.h: drop_keep4), exactly like the
// flash kernels of attn_flash.hip do, so all paths draw the same masks.
#include "common.h"

namespace a3d {

int drop_params(const a3d_dropout& d, const char* what, DropParams* out) {
  if (!(d.p >= 0.f && d.p < 1.f) || d.sample < 0 || d.site_code < 0) {
    set_error("%s: dropout p = %g must lie in [0, 1), sample %d and site %d must not be negative", what, (double)d.p,
              d.sample, d.site_code);
    return A3D_ERR_INVALID;
  }
  const double t = floor((double)d.p * 4294967296.0);
  out->k0 = (uint32_t)d.seed;
  out->k1 = (uint32_t)(d.seed >> 32);
  out->thr = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
  out->sample = (uint32_t)d.sample;
  out->site = (uint32_t)d.site_code;
  out->scale = 1.f / (1.f - d.p);
  return A3D_OK;
}

namespace {
// one thread per four columns of one logical row of [H][rows][cols]: mask[(h rows + i) cols + j] = keep
__global__ void k_drop_mask(DropParams dp, int64_t nrows, int cols, unsigned char* __restrict__ out) {
  const int c4 = (cols + 3) / 4;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nrows * c4) return;
  const int64_t r = e / c4;
  const int j0 = (int)(e % c4) * 4;
  const unsigned km = drop_keep4(dp, (uint32_t)r, (uint32_t)j0);
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (j0 + t < cols) out[r * cols + j0 + t] = (unsigned char)((km >> t) & 1u);
}

// out = Z o P over [H][Lq][Lk], stored as is (tr = 0) or as [H][Lk][Lq] (tr = 1); out may be P
__global__ void k_attn_drop(const float* P, int Lq, int Lk, int tr, float* out, int64_t nrows,
                            DropParams dp) {
  const int c4 = (Lk + 3) / 4;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nrows * c4) return;
  const int64_t r = e / c4;                    // h * Lq + i
  const int j0 = (int)(e % c4) * 4;
  const unsigned km = drop_keep4(dp, (uint32_t)r, (uint32_t)j0);
  const int64_t h = r / Lq, i = r % Lq;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = j0 + t;
    if (j < Lk) {
      const int64_t at = tr ? (h * Lk + j) * Lq + i : r * Lk + j;
      out[at] = (km >> t) & 1u ? P[at] * dp.scale : 0.f;
    }
  }
}

// y = res + Z o f(x) (fwd) / dx = Z o dy o [x_pre > 0] (bwd) over [rows][cols], cols % 4 == 0: one float4 per thread
template <bool BWD>
__global__ void k_rows_drop(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, int64_t rows,
                            int cols, int relu, DropParams dp) {
  const int c4 = cols / 4;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * c4) return;
  const int64_t r = e / c4;
  const int j0 = (int)(e % c4) * 4;
  const unsigned km = drop_keep4(dp, (uint32_t)r, (uint32_t)j0);
  const float4 x = *(const float4*)(a + r * cols + j0);
  float v[4] = {x.x, x.y, x.z, x.w};
  float o[4] = {0.f, 0.f, 0.f, 0.f};
  if (BWD) {
    if (b) {
      const float4 xp = *(const float4*)(b + r * cols + j0);
      const float p[4] = {xp.x, xp.y, xp.z, xp.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = p[t] > 0.f ? v[t] : 0.f;
    }
  } else {
    if (b) {
      const float4 rr = *(const float4*)(b + r * cols + j0);
      o[0] = rr.x, o[1] = rr.y, o[2] = rr.z, o[3] = rr.w;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = relu ? fmaxf(v[t], 0.f) : v[t];
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) o[t] += (km >> t) & 1u ? v[t] * dp.scale : 0.f;
  *(float4*)(y + r * cols + j0) = make_float4(o[0], o[1], o[2], o[3]);
}

unsigned nblocks(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }
}  // namespace
}  // namespace a3d

using namespace a3d;

extern "C" int a3d_dropout_mask(uint64_t seed, int sample, int site_code, float p, int heads, int64_t rows, int64_t cols,
                                unsigned char* out_dev, void* stream) {
  a3d_dropout d = {seed, p, sample, site_code, 0};
  DropParams dp;
  if (int rc = drop_params(d, "a3d_dropout_mask", &dp)) return rc;
  if (!out_dev || heads <= 0 || rows <= 0 || cols <= 0 || (int64_t)heads * rows >= (int64_t(1) << 32) || cols > (1 << 30)) {
    set_error("a3d_dropout_mask: bad arguments");
    return A3D_ERR_INVALID;
  }
  const int64_t nrows = (int64_t)heads * rows;
  k_drop_mask<<<nblocks(nrows * ((cols + 3) / 4), 256), 256, 0, (hipStream_t)stream>>>(dp, nrows, (int)cols, out_dev);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_attn_dropout(const float* P_dev, int H, int64_t Lq, int64_t Lk, int transposed, float* out_dev,
                                a3d_dropout drop, void* stream) {
  DropParams dp;
  if (int rc = drop_params(drop, "a3d_attn_dropout", &dp)) return rc;
  if (!P_dev || !out_dev || H <= 0 || Lq <= 0 || Lk <= 0 || (int64_t)H * Lq >= (int64_t(1) << 31) || Lk > (1 << 30)) {
    set_error("a3d_attn_dropout: bad arguments");
    return A3D_ERR_INVALID;
  }
  const int64_t nrows = (int64_t)H * Lq;
  k_attn_drop<<<nblocks(nrows * ((Lk + 3) / 4), 256), 256, 0, (hipStream_t)stream>>>(P_dev, (int)Lq, (int)Lk, transposed ? 1 : 0,
                                                                                     out_dev, nrows, dp);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

static int rows_check(const char* what, const void* a, const void* y, int64_t rows, int cols) {
  if (!a || !y || rows <= 0 || rows >= (int64_t(1) << 31) || cols <= 0 || cols % 4 || ((uintptr_t)a & 15) || ((uintptr_t)y & 15)) {
    set_error("%s: bad arguments (cols a multiple of 4, 16-byte aligned rows)", what);
    return A3D_ERR_INVALID;
  }
  return A3D_OK;
}

extern "C" int a3d_dropout_rows_forward(const float* x_dev, const float* res_dev, float* y_dev, int64_t rows, int cols, int relu,
                                        a3d_dropout drop, void* stream) {
  DropParams dp;
  if (int rc = drop_params(drop, "a3d_dropout_rows_forward", &dp)) return rc;
  if (int rc = rows_check("a3d_dropout_rows_forward", x_dev, y_dev, rows, cols)) return rc;
  if ((uintptr_t)res_dev & 15) {
    set_error("a3d_dropout_rows_forward: misaligned residual");
    return A3D_ERR_INVALID;
  }
  k_rows_drop<false><<<nblocks(rows * (cols / 4), 256), 256, 0, (hipStream_t)stream>>>(x_dev, res_dev, y_dev, rows, cols,
                                                                                        relu ? 1 : 0, dp);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_dropout_rows_backward(const float* dy_dev, const float* x_pre_dev, float* dx_dev, int64_t rows, int cols,
                                         a3d_dropout drop, void* stream) {
  DropParams dp;
  if (int rc = drop_params(drop, "a3d_dropout_rows_backward", &dp)) return rc;
  if (int rc = rows_check("a3d_dropout_rows_backward", dy_dev, dx_dev, rows, cols)) return rc;
  if ((uintptr_t)x_pre_dev & 15) {
    set_error("a3d_dropout_rows_backward: misaligned pre-activation");
    return A3D_ERR_INVALID;
  }
  k_rows_drop<true><<<nblocks(rows * (cols / 4), 256), 256, 0, (hipStream_t)stream>>>(dy_dev, x_pre_dev, dx_dev, rows, cols, 0,
                                                                                       dp);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
