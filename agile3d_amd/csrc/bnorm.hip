// libagile3d_hip -- BatchNorm in TRAINING mode over the [N, C] rows of a sparse tensor (ME.MinkowskiBatchNorm =
// nn.BatchNorm1d over the concatenated rows of the batch, models/modules/common.py:22), forward and backward, with the
// residual add and the ReLU of BasicBlock.forward (resnet_block.py:48-64) fused in; the same in pieces for statistics
// that span the data-parallel ranks (SyncBN); the column sums of a matrix; LayerNorm over the channels of a row.  Second
// kernel family of the training path.  All of it is HBM-bound statistics + element-wise work:
//   forward : mean_c, var_c (the variance is taken around a mean, never as E[x^2] - E[x]^2: one sweep that gives every
//             row block its own mean and M2, merged in fp64), y = (x-mean) rstd g + b (+ res) (ReLU); running statistics
//             updated with the unbiased variance
//   backward: g = dy (y > 0);  dbeta = sum g, dgamma = sum g xhat;  dx = gamma rstd (g - dbeta/N - xhat dgamma/N);
//             the residual branch receives g
// Column reductions are two-stage and deterministic: row blocks -> partial[block][columns] (fp32) -> col_reduce: a
// workgroup per 16 columns, its lanes take the blocks in strides and are folded in ascending order, all in fp64.
// Order of the file: kernels, host helpers, entry points.
#include "common.h"

namespace a3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBnThreads = 192;     // divisible by C/4 for every channel count of the net (8..96 float4 columns)
constexpr int kBnMaxBlocks = 1024;

// the ReLU of the forward seen from the backward: the gradient passes where the OUTPUT y was positive
__device__ __forceinline__ f32x4 relu_gate(f32x4 g, const f32x4 y) {
#pragma unroll
  for (int t = 0; t < 4; ++t) g[t] = y[t] > 0.f ? g[t] : 0.f;
  return g;
}

// ---- first level: sums over the rows of a row block --------------------------------------------------------------
// mode 0: sum x            mode 1: sum (x - m)^2
// mode 2: two sums for the backward: g = dy * (y > 0 or 1), sum g and sum g * (x - m) * rstd   (out: [2][C])
struct ColArgs {
  const float *x, *y, *dy, *mean, *rstd;
  int ldx, ldy, lddy, n, C, relu, mode, rows_per_block;
  float* partial;   // [blocks][nsum][C]
};

__global__ void __launch_bounds__(kBnThreads) k_col_partial(const ColArgs a) {
  __shared__ f32x4 red[2][kBnThreads];
  const int c4n = a.C >> 2;
  const int col = threadIdx.x % c4n, rsub = threadIdx.x / c4n, rstep = kBnThreads / c4n;
  const int r0 = blockIdx.x * a.rows_per_block, r1 = min(a.n, r0 + a.rows_per_block);
  f32x4 s0 = (f32x4){0.f, 0.f, 0.f, 0.f}, s1 = s0;
  f32x4 m = s0, rs = s0;
  if (a.mode != 0) m = *(const f32x4*)(a.mean + 4 * col);
  if (a.mode == 2) rs = *(const f32x4*)(a.rstd + 4 * col);
  // four rows per round: their loads are independent and issued together (one row per round left a wave with a single 1 KB
  // access in flight -- 12 KB per CU, a fifth of what the HBM pipe needs); the sums are still added row by row, in order
  constexpr int U = 4;
  for (int rb = r0 + rsub; rb < r1; rb += U * rstep) {
    f32x4 xv[U], gv[U], yv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = rb + u * rstep;
      const bool ok = r < r1;
      const size_t rr = ok ? (size_t)r : (size_t)r0;
      xv[u] = *(const f32x4*)(a.x + rr * a.ldx + 4 * col);
      if (a.mode == 2) {
        gv[u] = *(const f32x4*)(a.dy + rr * a.lddy + 4 * col);
        if (a.relu) yv[u] = *(const f32x4*)(a.y + rr * a.ldy + 4 * col);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (rb + u * rstep >= r1) break;
      if (a.mode == 0) {
        s0 += xv[u];
      } else if (a.mode == 1) {
        const f32x4 d = xv[u] - m;
        s0 += d * d;
      } else {
        const f32x4 g = a.relu ? relu_gate(gv[u], yv[u]) : gv[u];
        s0 += g;
        s1 += g * ((xv[u] - m) * rs);
      }
    }
  }
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  __syncthreads();
  if (rsub == 0) {   // fold the row sub-lanes of this column in a fixed order
    for (int k = 1; k < rstep; ++k) {
      s0 += red[0][k * c4n + col];
      s1 += red[1][k * c4n + col];
    }
    const int nsum = a.mode == 2 ? 2 : 1;
    float* p = a.partial + (size_t)blockIdx.x * nsum * a.C + 4 * col;
    *(f32x4*)p = s0;
    if (nsum == 2) *(f32x4*)(p + a.C) = s1;
  }
}

// Forward statistics in ONE sweep kernel + one combine kernel (3 launches per BatchNorm layer with the apply pass;
// the first version took 7): every row block sums its rows, takes ITS mean, and sums the squared deviations from it in a
// second loop over the same rows (L2-resident by then); k_bn_combine merges the blocks' (count, mean, M2) in block order
// with Chan's update in fp64 -- the variance is still taken around a mean, never as E[x^2] - E[x]^2.
// The merge is first-order sensitive to an error of a block's sum (2 (m_b - mean) err in the variance), and an fp32 sum of
// 512 values near 100 is off by 1e-2: on x = 100 + 0.05 randn that cost save_rstd 4e-6 to 1.3e-5 relative, where torch's
// fp32 two-pass variance loses 3e-7.  So every row is taken relative to ROW 0 of its column (an exact subtraction wherever
// the mean is large against the spread, one more fp32 rounding elsewhere): the sums are sums of small numbers, and
// k_bn_combine adds row 0 back to the merged mean.
__global__ void __launch_bounds__(kBnThreads) k_bn_block_stats(const ColArgs a) {
  __shared__ f32x4 red[kBnThreads];
  __shared__ f32x4 bmean[kBnThreads];
  const int c4n = a.C >> 2;
  const int col = threadIdx.x % c4n, rsub = threadIdx.x / c4n, rstep = kBnThreads / c4n;
  const int r0 = blockIdx.x * a.rows_per_block, r1 = min(a.n, r0 + a.rows_per_block);
  const f32x4 pv = *(const f32x4*)(a.x + 4 * col);
  f32x4 s0 = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int r = r0 + rsub; r < r1; r += rstep) s0 += *(const f32x4*)(a.x + (size_t)r * a.ldx + 4 * col) - pv;
  red[threadIdx.x] = s0;
  __syncthreads();
  if (rsub == 0) {
    for (int k = 1; k < rstep; ++k) s0 += red[k * c4n + col];
    bmean[col] = s0 * (1.f / (float)(r1 - r0));
    *(f32x4*)(a.partial + (size_t)blockIdx.x * 2 * a.C + 4 * col) = s0;
  }
  __syncthreads();
  const f32x4 m = bmean[col];
  f32x4 s1 = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int r = r0 + rsub; r < r1; r += rstep) {
    const f32x4 d = (*(const f32x4*)(a.x + (size_t)r * a.ldx + 4 * col) - pv) - m;
    s1 += d * d;
  }
  red[threadIdx.x] = s1;
  __syncthreads();
  if (rsub == 0) {
    for (int k = 1; k < rstep; ++k) s1 += red[k * c4n + col];
    *(f32x4*)(a.partial + (size_t)blockIdx.x * 2 * a.C + a.C + 4 * col) = s1;
  }
}

// ---- second level: the block partials of a column, summed in fp64 ------------------------------------------------
// One thread per column walking up to 1024 block partials is a chain of a thousand dependent L2 loads (38 us for a few KB
// of arithmetic; 130 of these launches per training iteration).  So a workgroup takes kFinCols = 16 consecutive columns
// with LANES block lanes each: lane bl sums the blocks bl, bl + LANES, ..., then thread c < 16 folds the LANES results of
// its column in ascending lane order (col_fold) -- fixed orders.  Two geometries run:
//   LANES = 16,  VEC = 1: 256 threads, thread (bl, cc) loads one float per block (64-byte row segments per load): the at
//                         most 1024 row blocks of bn_blocks
//   LANES = 256, VEC = 4: 1024 threads, thread (bl, q) loads the 16 bytes of column quad q per block: the MANY small
//                         blocks of the conv epilogues (one per 64-row tile or 16-row group: 5 000 - 20 000 at 320 k
//                         rows, 20 rounds per lane; 16 lanes per column walked 300+ blocks each)
constexpr int kFinCols = 16, kFinLanes = 16, kFinTileLanes = 256;
template <int LANES, int VEC>
using FinShared = double[LANES][kFinCols + VEC / 4];      // (the 16-byte geometry pads its rows by one double)

// -> in thread c < kFinCols the sum over the lanes, in lane order, of the s[] that belongs to column blockIdx.x * kFinCols + c
template <int LANES, int VEC>
__device__ __forceinline__ double col_fold(const double (&s)[VEC], FinShared<LANES, VEC>& sh) {
  const int q = threadIdx.x % (kFinCols / VEC), bl = threadIdx.x / (kFinCols / VEC);
#pragma unroll
  for (int t = 0; t < VEC; ++t) sh[bl][VEC * q + t] = s[t];
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x < kFinCols)
    for (int k = 0; k < LANES; ++k) t += sh[k][threadIdx.x];
  return t;
}
// -> in thread c < kFinCols the sum over the blocks of column blockIdx.x * kFinCols + c of partial [nblocks][stride]; columns
// from ncol on are not read
template <int LANES, int VEC>
__device__ __forceinline__ double col_reduce(const float* __restrict__ partial, int nblocks, int stride, int ncol,
                                             FinShared<LANES, VEC>& sh) {
  const int q = threadIdx.x % (kFinCols / VEC), bl = threadIdx.x / (kFinCols / VEC);
  const int c0 = blockIdx.x * kFinCols + VEC * q;
  double s[VEC] = {};
  if (c0 < ncol)
    for (int b = bl; b < nblocks; b += LANES) {
      if constexpr (VEC == 4) {
        const f32x4 v = *(const f32x4*)(partial + (size_t)b * stride + c0);
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] += (double)v[t];
      } else {
        s[0] += (double)partial[(size_t)b * stride + c0];
      }
    }
  return col_fold<LANES, VEC>(s, sh);
}

// out[c] = the column sums of partial [nblocks][ncol], as fp64 or rounded to fp32 (launch: ceil(ncol / 16) workgroups of
// 16 * LANES / VEC threads).  Three builds run: <16, 1, double>, <16, 1, float> (a3d_column_sums: one launch instead of
// a sum + a conversion kernel) and <256, 4, double> (bn_sums_from_partials from 64 blocks on).
template <int LANES, int VEC, typename OUT>
__global__ void __launch_bounds__(kFinCols* LANES / VEC) k_col_final(const float* __restrict__ partial, int nblocks, int ncol, OUT* out) {
  __shared__ FinShared<LANES, VEC> sh;
  const double t = col_reduce<LANES, VEC>(partial, nblocks, ncol, ncol, sh);
  const int c = blockIdx.x * kFinCols + threadIdx.x;
  if (threadIdx.x < kFinCols && c < ncol) out[c] = (OUT)t;
}

// The end of the forward statistics of column c, from the merged (mean, M2 = sum of squared deviations, row count):
// save_mean, save_rstd, and the running statistics moved towards the batch's with the UNBIASED variance, as torch does
// (one row has none: the biased value, 0, takes its place).
__device__ __forceinline__ void bn_write_stats(int c, double mean, double m2, double cnt, float eps, float momentum, float* mean_out,
                                               float* rstd_out, float* running_mean, float* running_var) {
  const float var = (float)(m2 / cnt);
  mean_out[c] = (float)mean;
  rstd_out[c] = 1.0f / sqrtf(var + eps);
  if (running_mean) {
    const float unbiased = cnt > 1.0 ? (float)(m2 / (cnt - 1.0)) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
}

// The merge of k_bn_block_stats' partials in the 16-lane geometry above: thread (bl, cc) merges the blocks bl, bl + 16, ...
// of column cc, then one thread per column merges the 16 triples in bl order -- fp64.
// The partials are those of x - pivot (k_bn_block_stats: pivot = row 0 of x); the mean gets the pivot back.
__global__ void __launch_bounds__(256) k_bn_combine(const float* __restrict__ partial, const float* __restrict__ pivot,
                                                    int nblocks, int rows_per_block, int n, int C, float eps, float* mean_out, float* rstd_out, float* running_mean,
                                                    float* running_var, float momentum) {
  __shared__ double s_cnt[kFinLanes][kFinCols], s_mean[kFinLanes][kFinCols], s_m2[kFinLanes][kFinCols];
  const int cc = threadIdx.x % kFinCols, bl = threadIdx.x / kFinCols;
  const int c = blockIdx.x * kFinCols + cc;
  double cnt = 0.0, mean = 0.0, m2 = 0.0;
  if (c < C) {
    for (int b = bl; b < nblocks; b += kFinLanes) {
      const double nb = (double)(min(n, (b + 1) * rows_per_block) - b * rows_per_block);
      const double bs = (double)partial[(size_t)b * 2 * C + c], bm2 = (double)partial[(size_t)b * 2 * C + C + c];
      // the block's M2 was taken around the fp32 block mean the kernel used, not around bs / nb: shift it (exact identity)
      const double bm_used = (double)((float)bs * (1.f / (float)nb)), bm = bs / nb;
      const double bm2c = bm2 - nb * (bm - bm_used) * (bm - bm_used);
      const double delta = bm - mean, tot = cnt + nb;
      mean += delta * nb / tot;
      m2 += bm2c + delta * delta * cnt * nb / tot;
      cnt = tot;
    }
  }
  s_cnt[bl][cc] = cnt, s_mean[bl][cc] = mean, s_m2[bl][cc] = m2;
  __syncthreads();
  if (bl != 0 || c >= C) return;
  for (int k = 1; k < kFinLanes; ++k) {          // Chan's merge of two partial (count, mean, M2) triples, in bl order
    const double nb = s_cnt[k][cc];
    if (nb == 0.0) continue;
    const double delta = s_mean[k][cc] - mean, tot = cnt + nb;
    mean += delta * nb / tot;
    m2 += s_m2[k][cc] + delta * delta * cnt * nb / tot;
    cnt = tot;
  }
  bn_write_stats(c, mean + (double)pivot[c], m2, cnt, eps, momentum, mean_out, rstd_out, running_mean, running_var);
}

// The same merge for the MANY small blocks of the conv kernels' epilogues (one (sum, M2 around the block mean) pair per
// 64-row tile or 16-row group), in the 256-lane geometry and without a dependent chain of divisions: pass 1 sums the block
// sums (col_reduce) -> the batch mean; pass 2 shifts every block's M2 to that mean with the exact identity
//   sum (v - mean)^2 = M2_b + 2 (m_b - mean) (S_b - n_b m_b) + n_b (m_b - mean)^2        (m_b = the fp32 mean the block used)
// and folds the lanes like pass 1.
__global__ void __launch_bounds__(1024) k_bn_combine_tiles(const float* __restrict__ partial, int nblocks, int rows_per_block, int n,
                                                           int C, float eps, float* mean_out, float* rstd_out, float* running_mean,
                                                           float* running_var, float momentum) {
  __shared__ FinShared<kFinTileLanes, 4> sh;
  __shared__ double s_mean[kFinCols];
  const int q = threadIdx.x & 3, bl = threadIdx.x >> 2;
  const int c0 = blockIdx.x * kFinCols + 4 * q;      // C is a multiple of 4 (of 32): a column quad is live or not as a whole
  const double sum = col_reduce<kFinTileLanes, 4>(partial, nblocks, 2 * C, C, sh);
  if (threadIdx.x < kFinCols) s_mean[threadIdx.x] = sum / (double)n;
  __syncthreads();
  double m2s[4] = {0.0, 0.0, 0.0, 0.0};
  if (c0 < C)
    for (int b = bl; b < nblocks; b += kFinTileLanes) {
      const int nbi = min(n, (b + 1) * rows_per_block) - b * rows_per_block;
      const f32x4 bsf = *(const f32x4*)(partial + (size_t)b * 2 * C + c0);
      const f32x4 bq = *(const f32x4*)(partial + (size_t)b * 2 * C + C + c0);
      const double nb = (double)nbi;
      const float invf = 1.f / (float)nbi;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double m_used = (double)(bsf[t] * invf);
        const double dm = m_used - s_mean[4 * q + t];
        m2s[t] += (double)bq[t] + 2.0 * dm * ((double)bsf[t] - nb * m_used) + nb * dm * dm;
      }
    }
  __syncthreads();
  double m2 = col_fold<kFinTileLanes, 4>(m2s, sh);
  const int c = blockIdx.x * kFinCols + threadIdx.x;
  if (threadIdx.x >= kFinCols || c >= C) return;
  if (m2 < 0.0) m2 = 0.0;
  bn_write_stats(c, s_mean[threadIdx.x], m2, (double)n, eps, momentum, mean_out, rstd_out, running_mean, running_var);
}

// a3d_bn_local_stats hands its mean to the second sweep in fp32 and to the caller in fp64
__global__ void k_scale_f64(const double* in, int C, double f, double* out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) out[c] = in[c] * f;
}
__global__ void k_bn_mean(const double* sums, int C, double n, float* mean) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) mean[c] = (float)(sums[c] / n);
}

// ---- element-wise passes -------------------------------------------------------------------------------------------
struct ApplyArgs {
  const float *x, *mean, *rstd, *gamma, *beta, *res;
  int ldx, ldr, ldy, n, C, relu;
  int zero_row;   // != 0: row n of y is written as zeros (the row a missing neighbour gathers in the next conv)
  float* y;
};
__global__ void k_bn_apply(const ApplyArgs a) {
  const int c4n = a.C >> 2;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a.zero_row && e < (size_t)c4n) *(f32x4*)(a.y + (size_t)a.n * a.ldy + 4 * e) = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (e >= (size_t)a.n * c4n) return;
  const int r = (int)(e / c4n), col = (int)(e % c4n);
  const f32x4 xv = *(const f32x4*)(a.x + (size_t)r * a.ldx + 4 * col);
  const f32x4 m = *(const f32x4*)(a.mean + 4 * col), rs = *(const f32x4*)(a.rstd + 4 * col);
  const f32x4 ga = *(const f32x4*)(a.gamma + 4 * col), be = *(const f32x4*)(a.beta + 4 * col);
  f32x4 y = (xv - m) * rs * ga + be;
  if (a.res) y += *(const f32x4*)(a.res + (size_t)r * a.ldr + 4 * col);
  if (a.relu) {
#pragma unroll
    for (int t = 0; t < 4; ++t) y[t] = fmaxf(y[t], 0.f);
  }
  *(f32x4*)(a.y + (size_t)r * a.ldy + 4 * col) = y;
}

struct BwdArgs {
  const float *x, *y, *dy, *mean, *rstd, *gamma;
  const double* sums;         // [2][C]: sum g, sum g xhat over the rows the statistics were taken over
  const double* param_sums;   // [2][C]: the same over THIS call's rows (dgamma / dbeta)
  double n_stat;              // number of rows the statistics were taken over
  int zero_row;               // != 0: dx (and dres) have n + 1 rows, row n is written as zeros
  int ldx, ldy, lddy, lddx, lddres, n, C, relu;
  float *dx, *dres, *dgamma, *dbeta;
};
__global__ void k_bn_bwd_apply(const BwdArgs a) {
  const int c4n = a.C >> 2;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a.zero_row && e < (size_t)c4n) {
    *(f32x4*)(a.dx + (size_t)a.n * a.lddx + 4 * e) = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (a.dres) *(f32x4*)(a.dres + (size_t)a.n * a.lddres + 4 * e) = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  if (e >= (size_t)a.n * c4n) return;
  const int r = (int)(e / c4n), col = (int)(e % c4n);
  const f32x4 xv = *(const f32x4*)(a.x + (size_t)r * a.ldx + 4 * col);
  f32x4 g = *(const f32x4*)(a.dy + (size_t)r * a.lddy + 4 * col);
  if (a.relu) g = relu_gate(g, *(const f32x4*)(a.y + (size_t)r * a.ldy + 4 * col));
  if (a.dres) *(f32x4*)(a.dres + (size_t)r * a.lddres + 4 * col) = g;
  const f32x4 m = *(const f32x4*)(a.mean + 4 * col), rs = *(const f32x4*)(a.rstd + 4 * col);
  const f32x4 ga = *(const f32x4*)(a.gamma + 4 * col);
  const float inv_n = (float)(1.0 / a.n_stat);
  f32x4 dx;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float xh = (xv[t] - m[t]) * rs[t];
    const float db = (float)a.sums[4 * col + t], dg = (float)a.sums[a.C + 4 * col + t];
    dx[t] = ga[t] * rs[t] * (g[t] - db * inv_n - xh * dg * inv_n);
  }
  *(f32x4*)(a.dx + (size_t)r * a.lddx + 4 * col) = dx;
  if (r == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a.dbeta[4 * col + t] = (float)a.param_sums[4 * col + t];
      a.dgamma[4 * col + t] = (float)a.param_sums[a.C + 4 * col + t];
    }
  }
}

// ---- LayerNorm over the channels of every row (nn.LayerNorm(128) of the decoder: attention_block.py:38,98,155,
// agile3d.py:137), forward and backward: one wave per row, lane = C / 64 channels (C <= 512).
//   backward: gh = dy * gamma;  dx = rstd * (gh - mean(gh) - xhat * mean(gh * xhat));  dgamma = sum_rows dy * xhat,
//             dbeta = sum_rows dy  (row-block partials -> k_col_final, deterministic)
constexpr int kLnMaxPerLane = 8;
struct LnArgs {
  const float *x, *dy, *gamma, *beta;
  float *y, *dx, *partial;   // partial [blocks][2][C]
  int ldx, ldy, n, C, rows_per_block;
  float eps;
};
__device__ __forceinline__ float ln64_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the wave loads row xrow (lane: channels lane, lane + 64, ...) into v -> the row's mean and rstd, two-pass
__device__ __forceinline__ void ln_row_stats(const float* xrow, int lane, int per, int C, float eps, float (&v)[kLnMaxPerLane],
                                             float& mean, float& rstd) {
  float s = 0.f;
  for (int i = 0; i < per; ++i) {
    v[i] = xrow[lane + 64 * i];
    s += v[i];
  }
  mean = ln64_sum(s) / (float)C;
  float q = 0.f;
  for (int i = 0; i < per; ++i) q += (v[i] - mean) * (v[i] - mean);
  rstd = 1.0f / sqrtf(ln64_sum(q) / (float)C + eps);
}
__global__ void __launch_bounds__(256) k_ln_forward(const LnArgs a) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.n) return;
  const int per = a.C >> 6;
  float v[kLnMaxPerLane], mean, rstd;
  ln_row_stats(a.x + (size_t)row * a.ldx, lane, per, a.C, a.eps, v, mean, rstd);
  for (int i = 0; i < per; ++i) {
    const int c = lane + 64 * i;
    a.y[(size_t)row * a.ldy + c] = (v[i] - mean) * rstd * a.gamma[c] + a.beta[c];
  }
}
__global__ void __launch_bounds__(256) k_ln_backward(const LnArgs a) {
  __shared__ float red[2][4][64 * kLnMaxPerLane];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = a.C >> 6;
  const int r0 = blockIdx.x * a.rows_per_block, r1 = min(a.n, r0 + a.rows_per_block);
  float dg[kLnMaxPerLane], db[kLnMaxPerLane], ga[kLnMaxPerLane];
  for (int i = 0; i < per; ++i) dg[i] = db[i] = 0.f, ga[i] = a.gamma[lane + 64 * i];
  for (int row = r0 + wave; row < r1; row += 4) {
    float v[kLnMaxPerLane], g[kLnMaxPerLane], mean, rstd;
    for (int i = 0; i < per; ++i) g[i] = a.dy[(size_t)row * a.ldy + lane + 64 * i];
    ln_row_stats(a.x + (size_t)row * a.ldx, lane, per, a.C, a.eps, v, mean, rstd);
    float m1 = 0.f, m2 = 0.f;
    for (int i = 0; i < per; ++i) {
      v[i] = (v[i] - mean) * rstd;                  // xhat
      dg[i] += g[i] * v[i];
      db[i] += g[i];
      g[i] *= ga[i];                                // gh
      m1 += g[i];
      m2 += g[i] * v[i];
    }
    m1 = ln64_sum(m1) / (float)a.C, m2 = ln64_sum(m2) / (float)a.C;
    for (int i = 0; i < per; ++i) a.dx[(size_t)row * a.ldx + lane + 64 * i] = rstd * (g[i] - m1 - v[i] * m2);
  }
  for (int i = 0; i < per; ++i) {
    red[0][wave][lane + 64 * i] = dg[i];
    red[1][wave][lane + 64 * i] = db[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < a.C; c += 256) {
    // [2][C]: dbeta sums first, dgamma second (k_col_final sums column-wise over the blocks)
    a.partial[(size_t)blockIdx.x * 2 * a.C + c] = red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c];
    a.partial[(size_t)blockIdx.x * 2 * a.C + a.C + c] = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c];
  }
}
// C = 128 (every LayerNorm of the decoder): FOUR rows per wave -- 16 lanes per row, 8 channels (two 16-byte accesses) per
// lane, the row reductions over 16 lanes --, the next four rows' loads in flight behind the current ones' arithmetic.  The
// one-row-per-wave kernels above issue 4-byte accesses and four dependent shuffle trees per row: 950 us for the backward
// over 320 k rows (0.5 GB: 100 us at the HBM rate).
__device__ __forceinline__ float ln16_sum(float v) {
  v += __shfl_xor(v, 1, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 8, 16);
  return v;
}
// a lane's eight channels, summed / multiplied and summed as a fixed tree (the tests pin values that depend on it)
__device__ __forceinline__ float sum8(const f32x4 a, const f32x4 b) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((b[0] + b[1]) + (b[2] + b[3])); }
__device__ __forceinline__ float dot8(const f32x4 a0, const f32x4 a1, const f32x4 b0, const f32x4 b1) {
  return ((a0[0] * b0[0] + a0[1] * b0[1]) + (a0[2] * b0[2] + a0[3] * b0[3])) + ((a1[0] * b1[0] + a1[1] * b1[1]) + (a1[2] * b1[2] + a1[3] * b1[3]));
}
// the row whose 16 lanes hold (v0, v1) -> d = v - mean(row) and the row's rstd
__device__ __forceinline__ float ln128_row_stats(const f32x4 v0, const f32x4 v1, float eps, f32x4& d0, f32x4& d1) {
  const float mean = ln16_sum(sum8(v0, v1)) * (1.f / 128.f);
  d0 = v0 - mean, d1 = v1 - mean;
  return 1.0f / sqrtf(ln16_sum(dot8(d0, d1, d0, d1)) * (1.f / 128.f) + eps);
}
__global__ void __launch_bounds__(256) k_ln_forward128(const LnArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane >> 4, j = lane & 15;
  const int row = blockIdx.x * 16 + wave * 4 + r;
  if (row >= a.n) return;
  const float* xp = a.x + (size_t)row * a.ldx + 8 * j;
  f32x4 d0, d1;
  const float rstd = ln128_row_stats(*(const f32x4*)xp, *(const f32x4*)(xp + 4), a.eps, d0, d1);
  const f32x4 g0 = *(const f32x4*)(a.gamma + 8 * j), g1 = *(const f32x4*)(a.gamma + 8 * j + 4);
  const f32x4 b0 = *(const f32x4*)(a.beta + 8 * j), b1 = *(const f32x4*)(a.beta + 8 * j + 4);
  float* yp = a.y + (size_t)row * a.ldy + 8 * j;
  *(f32x4*)yp = d0 * rstd * g0 + b0;
  *(f32x4*)(yp + 4) = d1 * rstd * g1 + b1;
}
__global__ void __launch_bounds__(256) k_ln_backward128(const LnArgs a) {
  __shared__ __attribute__((aligned(16))) float red[2][4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane >> 4, j = lane & 15;
  const int r0 = blockIdx.x * a.rows_per_block, r1 = min(a.n, r0 + a.rows_per_block);
  const f32x4 ga0 = *(const f32x4*)(a.gamma + 8 * j), ga1 = *(const f32x4*)(a.gamma + 8 * j + 4);
  f32x4 dg0 = (f32x4){0.f, 0.f, 0.f, 0.f}, dg1 = dg0, db0 = dg0, db1 = dg0;
  int row = r0 + wave * 4 + r;
  f32x4 nv0 = dg0, nv1 = dg0, ng0 = dg0, ng1 = dg0;
  auto fetch = [&](int rw) {
    if (rw < r1) {
      const float* xp = a.x + (size_t)rw * a.ldx + 8 * j;
      const float* gp = a.dy + (size_t)rw * a.ldy + 8 * j;
      nv0 = *(const f32x4*)xp, nv1 = *(const f32x4*)(xp + 4);
      ng0 = *(const f32x4*)gp, ng1 = *(const f32x4*)(gp + 4);
    }
  };
  fetch(row);
  // (a wave's four row slots run in lock step: the loop bound is the slot-0 row, slots past the end are masked)
  for (int base = r0 + wave * 4; base < r1; base += 16) {
    const bool ok = row < r1;
    f32x4 v0 = nv0, v1 = nv1, g0 = ng0, g1 = ng1;
    if (!ok) v0 = v1 = g0 = g1 = (f32x4){0.f, 0.f, 0.f, 0.f};
    fetch(row + 16);
    f32x4 x0, x1;
    const float rstd = ln128_row_stats(v0, v1, a.eps, x0, x1);
    x0 = x0 * rstd, x1 = x1 * rstd;            // xhat
    dg0 += g0 * x0, dg1 += g1 * x1;
    db0 += g0, db1 += g1;
    g0 = g0 * ga0, g1 = g1 * ga1;              // gh
    const float m1 = ln16_sum(sum8(g0, g1)) * (1.f / 128.f);
    const float m2 = ln16_sum(dot8(g0, g1, x0, x1)) * (1.f / 128.f);
    if (ok) {
      float* dp = a.dx + (size_t)row * a.ldx + 8 * j;
      *(f32x4*)dp = rstd * (g0 - m1 - x0 * m2);
      *(f32x4*)(dp + 4) = rstd * (g1 - m1 - x1 * m2);
    }
    row += 16;
  }
  // fold the four row slots of the wave (lanes j, j + 16, j + 32, j + 48), then the four waves through LDS: fixed orders
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    dg0[t] += __shfl_xor(dg0[t], 16, 64), dg0[t] += __shfl_xor(dg0[t], 32, 64);
    dg1[t] += __shfl_xor(dg1[t], 16, 64), dg1[t] += __shfl_xor(dg1[t], 32, 64);
    db0[t] += __shfl_xor(db0[t], 16, 64), db0[t] += __shfl_xor(db0[t], 32, 64);
    db1[t] += __shfl_xor(db1[t], 16, 64), db1[t] += __shfl_xor(db1[t], 32, 64);
  }
  if (r == 0) {
    *(f32x4*)&red[0][wave][8 * j] = dg0, *(f32x4*)&red[0][wave][8 * j + 4] = dg1;
    *(f32x4*)&red[1][wave][8 * j] = db0, *(f32x4*)&red[1][wave][8 * j + 4] = db1;
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int c = threadIdx.x;
    // [2][C]: dbeta sums first, dgamma second (k_col_final sums column-wise over the blocks)
    a.partial[(size_t)blockIdx.x * 256 + c] = red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c];
    a.partial[(size_t)blockIdx.x * 256 + 128 + c] = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c];
  }
}
__global__ void k_ln_params(const double* sums, int C, float* dgamma, float* dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) dbeta[c] = (float)sums[c], dgamma[c] = (float)sums[C + c];
}

// ---- host helpers --------------------------------------------------------------------------------------------------
static bool bn_shape_ok(int64_t n, int C, int ld0, int ld1, int ld2) {
  return n > 0 && n <= (int64_t)1 << 30 && C >= 32 && C % 32 == 0 && kBnThreads % (C / 4) == 0 && ld0 % 4 == 0 &&
         ld1 % 4 == 0 && ld2 % 4 == 0;
}
// the row blocks of the first-level kernels: 512 rows each, at most kBnMaxBlocks of them
static int bn_blocks(int64_t n, int& rows_per_block) {
  int blocks = (int)((n + 511) / 512);
  if (blocks > kBnMaxBlocks) blocks = kBnMaxBlocks;
  rows_per_block = (int)((n + blocks - 1) / blocks);
  return (int)((n + rows_per_block - 1) / rows_per_block);
}
static unsigned fin_grid(int ncol) { return (unsigned)((ncol + kFinCols - 1) / kFinCols); }
static unsigned elem_grid(int64_t n, int C) { return (unsigned)(((size_t)n * (C / 4) + 255) / 256); }

// The workspace of a3d_bn_workspace_bytes: the first level's partials, then [2][C] fp64 sums, then [C] floats.
struct BnWs { float* partial; double* sums; float* meanf; };
static size_t bn_partial_bytes(int C) { return align256((size_t)kBnMaxBlocks * 2 * C * sizeof(float)); }
static size_t bn_sums_bytes(int C) { return align256((size_t)2 * C * sizeof(double)); }
// -> A3D_OK and the carve, or the workspace error of entry point `who`
static int bn_carve(const char* who, void* workspace, size_t bytes, int64_t n, int C, BnWs& w, const char* hint = "") {
  if (bytes < a3d_bn_workspace_bytes(n, C) || ((uintptr_t)workspace & 15)) {
    set_error("%s: workspace too small or misaligned%s", who, hint);
    return A3D_ERR_WORKSPACE;
  }
  w.partial = (float*)workspace;
  w.sums = (double*)((char*)workspace + bn_partial_bytes(C));
  w.meanf = (float*)((char*)w.sums + bn_sums_bytes(C));
  return A3D_OK;
}

// One launcher per kernel family; none of them checks its arguments (the entry points do) or the launch (the entry points
// end with A3D_LAUNCH_CHECK).
// k_col_partial in `mode` (kColBlockStats: k_bn_block_stats) over x [n][C] -> the number of row blocks written to `partial`,
// of *rows_per_block rows; `bw`: the operands of mode 2
constexpr int kColBlockStats = -1;
struct ColBwd {
  const float *y, *dy, *rstd;
  int ldy, lddy, relu;
};
static int col_partial(int mode, const float* x, int ldx, int64_t n, int C, const float* mean, const ColBwd* bw, float* partial,
                       hipStream_t st, int* rows_per_block = nullptr) {
  ColArgs c = {};
  c.x = x, c.ldx = ldx, c.n = (int)n, c.C = C, c.mean = mean, c.mode = mode, c.partial = partial;
  if (bw) c.y = bw->y, c.dy = bw->dy, c.rstd = bw->rstd, c.ldy = bw->ldy, c.lddy = bw->lddy, c.relu = bw->relu;
  const int blocks = bn_blocks(n, c.rows_per_block);
  if (rows_per_block) *rows_per_block = c.rows_per_block;
  if (mode == kColBlockStats) k_bn_block_stats<<<blocks, kBnThreads, 0, st>>>(c);
  else k_col_partial<<<blocks, kBnThreads, 0, st>>>(c);
  return blocks;
}
// the first half of the backward: sums [2][C] (fp64) = sum g, sum g xhat over the n rows
static void bn_backward_sums(const float* x, int ldx, const float* y, int ldy, const float* dy, int lddy, int64_t n, int C,
                             const float* mean, const float* rstd, int relu, float* partial, double* sums, hipStream_t st) {
  const ColBwd bw = {y, dy, rstd, ldy, lddy, relu};
  const int blocks = col_partial(2, x, ldx, n, C, mean, &bw, partial, st);
  k_col_final<kFinLanes, 1, double><<<fin_grid(2 * C), 256, 0, st>>>(partial, blocks, 2 * C, sums);
}
static void bn_apply(const float* x, int ldx, int64_t n, int C, const float* gamma, const float* beta, const float* mean,
                     const float* rstd, const float* res, int ldr, int relu, float* y, int ldy, int zero_row, hipStream_t st) {
  ApplyArgs a;
  a.x = x, a.mean = mean, a.rstd = rstd, a.gamma = gamma, a.beta = beta, a.res = res;
  a.ldx = ldx, a.ldr = ldr, a.ldy = ldy, a.n = (int)n, a.C = C, a.relu = relu, a.y = y, a.zero_row = zero_row;
  k_bn_apply<<<elem_grid(n, C), 256, 0, st>>>(a);
}
// the second half of the backward: dx (and dres) from `sums` over n_stat rows, dgamma / dbeta = param_sums
static void bn_bwd_apply(const float* x, int ldx, const float* y, int ldy, const float* dy, int lddy, int64_t n, int C,
                         const float* gamma, const float* mean, const float* rstd, int relu, const double* sums, int64_t n_stat,
                         const double* param_sums, float* dx, int lddx, float* dres, int lddres, float* dgamma, float* dbeta,
                         int zero_row, hipStream_t st) {
  BwdArgs b;
  b.x = x, b.y = y, b.dy = dy, b.mean = mean, b.rstd = rstd, b.gamma = gamma;
  b.sums = sums, b.param_sums = param_sums, b.n_stat = (double)n_stat, b.zero_row = zero_row;
  b.ldx = ldx, b.ldy = ldy, b.lddy = lddy, b.lddx = lddx, b.lddres = lddres, b.n = (int)n, b.C = C;
  b.relu = relu, b.dx = dx, b.dres = dres, b.dgamma = dgamma, b.dbeta = dbeta;
  k_bn_bwd_apply<<<elem_grid(n, C), 256, 0, st>>>(b);
}
// dx and the row-block partials of dgamma / dbeta -> their column sums -> dgamma, dbeta
static void ln_backward(const float* x, int ldx, const float* dy, int lddy, int64_t n, int C, const float* gamma, float eps,
                        float* dx, float* dgamma, float* dbeta, const BnWs& w, hipStream_t st) {
  LnArgs a = {};
  a.x = x, a.dy = dy, a.gamma = gamma, a.dx = dx, a.partial = w.partial;
  a.ldx = ldx, a.ldy = lddy, a.n = (int)n, a.C = C, a.eps = eps;
  const int blocks = bn_blocks(n, a.rows_per_block);
  if (C == 128 && !(ldx & 3) && !(lddy & 3)) k_ln_backward128<<<blocks, 256, 0, st>>>(a);
  else k_ln_backward<<<blocks, 256, 0, st>>>(a);
  k_col_final<kFinLanes, 1, double><<<fin_grid(2 * C), 256, 0, st>>>(w.partial, blocks, 2 * C, w.sums);
  k_ln_params<<<(unsigned)((C + 255) / 256), 256, 0, st>>>(w.sums, C, dgamma, dbeta);
}

// ---- for the conv kernels' epilogues (spconv.hip) ------------------------------------------------------------------
// BatchNorm(train) from the block partials of a3d_conv_bn_train_forward's epilogue: merge + apply
int bn_finish_from_partials(const float* partial, int nblocks, int rows_per_block, const float* x, int ldx, int64_t n, int C,
                            const float* gamma, const float* beta, float eps, const float* res, int ldr, int relu, float* y,
                            int ldy, int y_zero_row, float* save_mean, float* save_rstd, float* running_mean,
                            float* running_var, float momentum, hipStream_t st) {
  if (!partial || !x || !gamma || !beta || !y || !save_mean || !save_rstd || n <= 0 || n > (int64_t)1 << 30 || C < 32 || C % 32 ||
      (ldx & 3) || (ldy & 3) || (res && (ldr & 3)) || (running_mean == nullptr) != (running_var == nullptr) || nblocks < 1 ||
      (int64_t)(nblocks - 1) * rows_per_block >= n) {
    set_error("bn_finish_from_partials: bad arguments");
    return A3D_ERR_INVALID;
  }
  k_bn_combine_tiles<<<fin_grid(C), 1024, 0, st>>>(partial, nblocks, rows_per_block, (int)n, C, eps, save_mean, save_rstd,
                                                    running_mean, running_var, momentum);
  bn_apply(x, ldx, n, C, gamma, beta, save_mean, save_rstd, res, ldr, relu, y, ldy, y_zero_row, st);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
// [blocks][2][C] fp32 partials (the epilogue of a3d_conv_dgrad_bn) -> sums [2][C] fp64, blocks added in a fixed order
int bn_sums_from_partials(const float* partial, int nblocks, int C, double* sums, hipStream_t st) {
  if (nblocks >= 64) k_col_final<kFinTileLanes, 4, double><<<fin_grid(2 * C), 1024, 0, st>>>(partial, nblocks, 2 * C, sums);
  else k_col_final<kFinLanes, 1, double><<<fin_grid(2 * C), 256, 0, st>>>(partial, nblocks, 2 * C, sums);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

}  // namespace a3d

using namespace a3d;

// ---- entry points ------------------------------------------------------------------------------------------------------
extern "C" size_t a3d_bn_workspace_bytes(int64_t n, int C) {
  if (n <= 0 || C <= 0) return 0;
  return bn_partial_bytes(C) + bn_sums_bytes(C) + align256((size_t)C * sizeof(float)) + 256;
}

extern "C" int a3d_bn_train_forward(const float* x_dev, int ldx, int64_t n, int C, const float* gamma_dev,
                                    const float* beta_dev, float eps, const float* res_dev, int ldr, int relu,
                                    float* y_dev, int ldy, float* save_mean_dev, float* save_rstd_dev,
                                    float* running_mean_dev, float* running_var_dev, float momentum, int y_zero_row,
                                    void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!x_dev || !gamma_dev || !beta_dev || !y_dev || !save_mean_dev || !save_rstd_dev || !workspace_dev ||
      !bn_shape_ok(n, C, ldx, ldy, res_dev ? ldr : 4) || (running_mean_dev == nullptr) != (running_var_dev == nullptr)) {
    set_error("a3d_bn_train_forward: bad arguments (C a multiple of 32 dividing 768, leading dimensions multiples of 4)");
    return A3D_ERR_INVALID;
  }
  BnWs w;
  if (int rc = bn_carve("a3d_bn_train_forward", workspace_dev, workspace_bytes, n, C, w)) return rc;
  hipStream_t st = (hipStream_t)stream;
  int rows_per_block;
  const int blocks = col_partial(kColBlockStats, x_dev, ldx, n, C, nullptr, nullptr, w.partial, st, &rows_per_block);
  k_bn_combine<<<fin_grid(C), 256, 0, st>>>(w.partial, x_dev, blocks, rows_per_block, (int)n, C, eps, save_mean_dev, save_rstd_dev,
                                            running_mean_dev, running_var_dev, momentum);
  bn_apply(x_dev, ldx, n, C, gamma_dev, beta_dev, save_mean_dev, save_rstd_dev, res_dev, ldr, relu, y_dev, ldy, y_zero_row, st);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_bn_train_backward(const float* x_dev, int ldx, const float* y_dev, int ldy, const float* dy_dev,
                                     int lddy, int64_t n, int C, const float* gamma_dev, const float* save_mean_dev,
                                     const float* save_rstd_dev, int relu, float* dx_dev, int lddx, float* dres_dev,
                                     int lddres, float* dgamma_dev, float* dbeta_dev, int zero_row, void* workspace_dev,
                                     size_t workspace_bytes, void* stream) {
  if (!x_dev || !dy_dev || !gamma_dev || !save_mean_dev || !save_rstd_dev || !dx_dev || !dgamma_dev || !dbeta_dev ||
      !workspace_dev || (relu && !y_dev) || !bn_shape_ok(n, C, ldx, lddy, lddx) || (relu && ldy % 4) ||
      (dres_dev && lddres % 4)) {
    set_error("a3d_bn_train_backward: bad arguments");
    return A3D_ERR_INVALID;
  }
  BnWs w;
  if (int rc = bn_carve("a3d_bn_train_backward", workspace_dev, workspace_bytes, n, C, w)) return rc;
  hipStream_t st = (hipStream_t)stream;
  // a3d_bn_backward_sums, then a3d_bn_backward_apply with the statistics' rows = this call's rows
  bn_backward_sums(x_dev, ldx, y_dev, ldy, dy_dev, lddy, n, C, save_mean_dev, save_rstd_dev, relu, w.partial, w.sums, st);
  bn_bwd_apply(x_dev, ldx, y_dev, ldy, dy_dev, lddy, n, C, gamma_dev, save_mean_dev, save_rstd_dev, relu, w.sums, n, w.sums, dx_dev,
               lddx, dres_dev, lddres, dgamma_dev, dbeta_dev, zero_row, st);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

// ---- the same BatchNorm in pieces, for statistics that span the data-parallel ranks (SyncBN): the caller exchanges
// the per-rank numbers (torch.distributed) between the calls.  Reference semantics: ME.MinkowskiBatchNorm normalises
// over ALL rows of the batch on one device (models/modules/common.py:20-22); with one scene per rank the strict
// equivalent needs [2C+1] numbers per layer across the ranks.
//   a3d_bn_local_stats     : stats[0..C) = mean of this rank's rows, stats[C..2C) = sum (x - that mean)^2   (fp64)
//   a3d_bn_apply           : y = relu?((x - mean) rstd gamma + beta (+ res)) with the GIVEN mean / rstd
//   a3d_bn_backward_sums   : sums[0..C) = sum g, sums[C..2C) = sum g xhat over this rank's rows (fp64), g = dy (y > 0)
//   a3d_bn_backward_apply  : dx from the GLOBAL sums and row count; dgamma / dbeta = the LOCAL sums (averaged over the
//                            ranks with every other parameter gradient afterwards, as DDP + SyncBatchNorm do)
extern "C" int a3d_bn_local_stats(const float* x_dev, int ldx, int64_t n, int C, double* stats_dev, void* workspace_dev,
                                  size_t workspace_bytes, void* stream) {
  if (!x_dev || !stats_dev || !workspace_dev || !bn_shape_ok(n, C, ldx, 4, 4)) {
    set_error("a3d_bn_local_stats: bad arguments");
    return A3D_ERR_INVALID;
  }
  BnWs w;
  if (int rc = bn_carve("a3d_bn_local_stats", workspace_dev, workspace_bytes, n, C, w)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const unsigned cb = (unsigned)((2 * C + 255) / 256);
  int blocks = col_partial(0, x_dev, ldx, n, C, nullptr, nullptr, w.partial, st);
  k_col_final<kFinLanes, 1, double><<<fin_grid(C), 256, 0, st>>>(w.partial, blocks, C, w.sums);
  k_bn_mean<<<cb, 256, 0, st>>>(w.sums, C, (double)n, w.meanf);
  k_scale_f64<<<cb, 256, 0, st>>>(w.sums, C, 1.0 / (double)n, stats_dev);              // the mean in fp64
  blocks = col_partial(1, x_dev, ldx, n, C, w.meanf, nullptr, w.partial, st);
  k_col_final<kFinLanes, 1, double><<<fin_grid(C), 256, 0, st>>>(w.partial, blocks, C, stats_dev + C);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_bn_apply(const float* x_dev, int ldx, int64_t n, int C, const float* gamma_dev, const float* beta_dev,
                            const float* mean_dev, const float* rstd_dev, const float* res_dev, int ldr, int relu,
                            float* y_dev, int ldy, int y_zero_row, void* stream) {
  if (!x_dev || !gamma_dev || !beta_dev || !mean_dev || !rstd_dev || !y_dev || !bn_shape_ok(n, C, ldx, ldy, res_dev ? ldr : 4)) {
    set_error("a3d_bn_apply: bad arguments");
    return A3D_ERR_INVALID;
  }
  bn_apply(x_dev, ldx, n, C, gamma_dev, beta_dev, mean_dev, rstd_dev, res_dev, ldr, relu, y_dev, ldy, y_zero_row, (hipStream_t)stream);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_bn_backward_sums(const float* x_dev, int ldx, const float* y_dev, int ldy, const float* dy_dev, int lddy,
                                    int64_t n, int C, const float* mean_dev, const float* rstd_dev, int relu,
                                    double* sums_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!x_dev || !dy_dev || !mean_dev || !rstd_dev || !sums_dev || !workspace_dev || (relu && !y_dev) ||
      !bn_shape_ok(n, C, ldx, lddy, 4) || (relu && ldy % 4)) {
    set_error("a3d_bn_backward_sums: bad arguments");
    return A3D_ERR_INVALID;
  }
  BnWs w;
  if (int rc = bn_carve("a3d_bn_backward_sums", workspace_dev, workspace_bytes, n, C, w)) return rc;
  bn_backward_sums(x_dev, ldx, y_dev, ldy, dy_dev, lddy, n, C, mean_dev, rstd_dev, relu, w.partial, sums_dev, (hipStream_t)stream);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_bn_backward_apply(const float* x_dev, int ldx, const float* y_dev, int ldy, const float* dy_dev, int lddy,
                                     int64_t n, int C, const float* gamma_dev, const float* mean_dev, const float* rstd_dev,
                                     int relu, const double* global_sums_dev, int64_t n_global, const double* local_sums_dev,
                                     float* dx_dev, int lddx, float* dres_dev, int lddres, float* dgamma_dev,
                                     float* dbeta_dev, int zero_row, void* stream) {
  if (!x_dev || !dy_dev || !gamma_dev || !mean_dev || !rstd_dev || !global_sums_dev || !local_sums_dev || !dx_dev ||
      !dgamma_dev || !dbeta_dev || n_global < n || (relu && !y_dev) || !bn_shape_ok(n, C, ldx, lddy, lddx) ||
      (relu && ldy % 4) || (dres_dev && lddres % 4)) {
    set_error("a3d_bn_backward_apply: bad arguments");
    return A3D_ERR_INVALID;
  }
  bn_bwd_apply(x_dev, ldx, y_dev, ldy, dy_dev, lddy, n, C, gamma_dev, mean_dev, rstd_dev, relu, global_sums_dev, n_global,
               local_sums_dev, dx_dev, lddx, dres_dev, lddres, dgamma_dev, dbeta_dev, zero_row, (hipStream_t)stream);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

// column sums of a [n][C] matrix (bias gradient of lin_squeeze_head: sum over rows of dy)
extern "C" int a3d_column_sums(const float* x_dev, int ldx, int64_t n, int C, float* out_dev, void* workspace_dev,
                               size_t workspace_bytes, void* stream) {
  if (!x_dev || !out_dev || !workspace_dev || !bn_shape_ok(n, C, ldx, 4, 4)) {
    set_error("a3d_column_sums: bad arguments");
    return A3D_ERR_INVALID;
  }
  BnWs w;
  if (int rc = bn_carve("a3d_column_sums", workspace_dev, workspace_bytes, n, C, w)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = col_partial(0, x_dev, ldx, n, C, nullptr, nullptr, w.partial, st);
  k_col_final<kFinLanes, 1, float><<<fin_grid(C), 256, 0, st>>>(w.partial, blocks, C, out_dev);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_layernorm_forward(const float* x_dev, int ldx, int64_t n, int C, const float* gamma_dev,
                                     const float* beta_dev, float eps, float* y_dev, int ldy, void* stream) {
  if (!x_dev || !gamma_dev || !beta_dev || !y_dev || n <= 0 || n > (int64_t)1 << 30 || C < 64 || C % 64 ||
      C > 64 * kLnMaxPerLane || ldx < C || ldy < C) {
    set_error("a3d_layernorm_forward: bad arguments (C a multiple of 64, <= 512)");
    return A3D_ERR_INVALID;
  }
  LnArgs a = {};
  a.x = x_dev, a.gamma = gamma_dev, a.beta = beta_dev, a.y = y_dev, a.ldx = ldx, a.ldy = ldy, a.n = (int)n, a.C = C, a.eps = eps;
  if (C == 128 && !(ldx & 3) && !(ldy & 3)) k_ln_forward128<<<(unsigned)((n + 15) / 16), 256, 0, (hipStream_t)stream>>>(a);
  else k_ln_forward<<<(unsigned)((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(a);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_layernorm_backward(const float* x_dev, int ldx, const float* dy_dev, int lddy, int64_t n, int C,
                                      const float* gamma_dev, float eps, float* dx_dev, float* dgamma_dev,
                                      float* dbeta_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  if (!x_dev || !dy_dev || !gamma_dev || !dx_dev || !dgamma_dev || !dbeta_dev || !workspace_dev || n <= 0 ||
      n > (int64_t)1 << 30 || C < 64 || C % 64 || C > 64 * kLnMaxPerLane || ldx < C || lddy < C) {
    set_error("a3d_layernorm_backward: bad arguments (C a multiple of 64, <= 512; dx has the layout of x)");
    return A3D_ERR_INVALID;
  }
  BnWs w;
  if (int rc = bn_carve("a3d_layernorm_backward", workspace_dev, workspace_bytes, n, C, w, " (a3d_bn_workspace_bytes)")) return rc;
  ln_backward(x_dev, ldx, dy_dev, lddy, n, C, gamma_dev, eps, dx_dev, dgamma_dev, dbeta_dev, w, (hipStream_t)stream);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
