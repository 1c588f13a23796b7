// session_guide.hip -- how sure the last inference is, voxel by voxel and vertex by vertex, and which rows a next click
// should look at (gfx950).  One entry point, a3d_session_guide, two launches: the voxel pass and the full-resolution pass.
//
// The reference has no counterpart: its tool keeps the arg-max of forward_mask's logits and drops the logits
// (interactive_segmentation_user.py:78-81).  THE RULE (ours, stated in include/agile3d_hip.h at a3d_session_guide):
//   voxel     label = first maximum of the row, runner = first maximum of the OTHER columns, margin = logit[label] -
//             logit[runner] (one fp32 subtraction); clicked rows: label = runner = the click's object, margin = +inf;
//             want = runner where margin < threshold ("contested"), else label
//   summary   rows and contested rows per label, the finite margin that is smallest (ties: the lowest row), an error word
//   vertex    margin_full = margin[inverse_map]; colour = base * s + doubt * (1 - s), s = min(margin / full_margin, 1),
//             base = the palette entry of the label (a3d_session_paint's), the vertex's own colour for label 0
//
// THE VOXEL PASS reads the logits the way they lie in memory.  k_argmax_labels (clicks.hip) gives every lane a row, so the
// lanes of a wave read 4 C bytes apart: at C = 21 a wave's load instruction touches 64 different 84-byte stretches.  Here a
// workgroup takes a TILE of consecutive rows -- one per thread, fewer when a row is long: rows x (C | 1) <= kGuideTile floats
// -- and copies its rows x C floats into LDS by their flat index: lane l of a load reads the dword behind lane l - 1's, 256
// contiguous bytes per wave instruction whatever C is.  In LDS a row starts (C | 1) floats behind the one before: the
// stride is odd, so the 32 lanes that one ds_read_b32 cycle serves (column c of 32 consecutive rows) fall on 32 different
// banks; the staging stores are consecutive dwords but for one skipped word per row end.  Each thread then scans its row
// twice from LDS (the label, then the runner among the others) -- the rule word for word, NaNs included.
// The clicks (<= 256, by value in the arguments) are staged once per workgroup; a thread walks them from the back and
// leaves at the first match -- the LAST entry of a row wins -- every lane reading the same LDS address, a broadcast, as
// the cube walk of k_session_paint does.
// THE SUMMARY is integer only: per-label counts go through an LDS histogram (one LDS atomic per row, two for a contested
// one), flushed with one global atomicAdd per non-empty bin and workgroup; the least confident row is a minimum over packed
// (margin bits, row) keys -- registers, wave shuffles, LDS, one 64-bit atomic per workgroup: an atomicMax of the key's
// COMPLEMENT, so that the record's one clear to zero also means "no row yet" (a second clear, to all ones, is a second
// operation on the stream, and at a scene's size the call is a handful of those).  Sums of integers and a maximum do not
// depend on the order of arrival: the record is the same from run to run.
#include "common.h"

#include <cmath>

namespace a3d {

constexpr int kGuideBlock = 256;
constexpr int kGuideTile = 8448;               // floats of LDS per tile: 256 rows up to C = 32, 32 rows at C = 256 (stride 257)
constexpr int kGuideMaxBlocks = 1024;          // 4 workgroups per CU; longer inputs take further passes of the grid
constexpr unsigned long long kGuideNoKey = ~0ull;
static_assert(kGuideBlock == A3D_MAX_CLICKS && kGuideBlock == 256, "one click and one histogram bin per thread");

__global__ __launch_bounds__(kGuideBlock) void k_guide_voxels(const a3d_session_guide_args a, const int tile_rows,
                                                              const long long n_tiles) {
  __shared__ float tile[kGuideTile];
  __shared__ int32_t crow[A3D_MAX_CLICKS];
  __shared__ int32_t cobj[A3D_MAX_CLICKS];
  __shared__ int hist[2 * 256];                 // rows per label, contested rows per label
  __shared__ unsigned long long wave_key[kGuideBlock / 64];
  const int t = threadIdx.x;
  const int C = a.n_classes, Cp = C | 1;
  if (t < a.n_clicks) crow[t] = a.click_row[t], cobj[t] = a.click_obj[t];
  hist[t] = 0, hist[256 + t] = 0;
  const int step_row = kGuideBlock / C, step_col = kGuideBlock % C;     // where flat index f + 256 lies, seen from f
  const int row_t = t / C, col_t = t - row_t * C;
  unsigned long long least = kGuideNoKey;
  for (long long tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const long long row0 = tl * tile_rows;
    const int rows = (int)(a.n_qv - row0 < tile_rows ? a.n_qv - row0 : tile_rows);
    const int n_flat = rows * C;
    const float* __restrict__ src = a.logits_dev + row0 * C;
    __syncthreads();                             // the scan of the tile before (and, the first time, the staging above) is over
    int row = row_t, col = col_t;
#pragma unroll 4
    for (int f = t; f < n_flat; f += kGuideBlock) {
      tile[row * Cp + col] = src[f];
      row += step_row, col += step_col;
      if (col >= C) col -= C, ++row;
    }
    __syncthreads();
    if (t < rows) {
      const float* r = tile + t * Cp;
      float best = r[0];
      int lab = 0;
      for (int c = 1; c < C; ++c) {              // the first maximum, exactly as k_argmax_labels scans
        const float v = r[c];
        if (v > best) best = v, lab = c;
      }
      int run = lab == 0 ? 1 : 0;                // the same scan over the other columns
      float second = r[run];
#pragma unroll 4
      for (int c = run + 1; c < C; ++c) {
        const float v = r[c];
        if (c != lab && v > second) second = v, run = c;
      }
      float margin = best - second;
      if (margin != margin) atomicOr(&a.summary_dev->err, 1);
      const long long i = row0 + t;
      for (int k = a.n_clicks - 1; k >= 0; --k)  // the last click on a row wins: the first hit from the back
        if (crow[k] == i) {
          lab = run = cobj[k];
          margin = __builtin_inff();
          break;
        }
      const bool contested = margin < a.threshold;
      a.labels_qv_dev[i] = lab;
      a.runner_qv_dev[i] = run;
      a.margin_qv_dev[i] = margin;
      a.want_qv_dev[i] = contested ? run : lab;
      atomicAdd(&hist[lab], 1);
      if (contested) atomicAdd(&hist[256 + lab], 1);
      const unsigned bits = __float_as_uint(margin);       // finite margins are >= 0: their bits order like they do
      if ((bits & 0x7f800000u) != 0x7f800000u) {
        const unsigned long long key = ((unsigned long long)bits << 32) | (unsigned)i;
        least = key < least ? key : least;
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(least, o);
    least = other < least ? other : least;
  }
  if ((t & 63) == 0) wave_key[t >> 6] = least;
  __syncthreads();                               // the keys of the waves, and every LDS atomic on the histogram
  if (t == 0) {
    for (int w = 1; w < kGuideBlock / 64; ++w) least = wave_key[w] < least ? wave_key[w] : least;
    if (least != kGuideNoKey) atomicMax((unsigned long long*)&a.summary_dev->least_key, ~least);
  }
  if (hist[t]) atomicAdd(&a.summary_dev->voxels[t], hist[t]);
  if (hist[256 + t]) atomicAdd(&a.summary_dev->contested[t], hist[256 + t]);
}

// One thread per vertex, grid-stride, the palette staged in LDS as k_session_paint stages it.  The blend is written one
// operation at a time with contraction off: both products, the difference and the sum round once each.
__global__ __launch_bounds__(kGuideBlock) void k_guide_full(const a3d_session_guide_args a, const float inv_full_margin) {
#pragma clang fp contract(off)
  __shared__ float pal[256 * 3];
  for (int i = threadIdx.x; i < a.n_palette * 3; i += kGuideBlock) pal[i] = a.palette_dev[i];
  __syncthreads();
  const float dr = a.doubt[0], dg = a.doubt[1], db = a.doubt[2];
  const long long stride = (long long)gridDim.x * kGuideBlock;
  for (long long i = (long long)blockIdx.x * kGuideBlock + threadIdx.x; i < a.n_full; i += stride) {
    const long long src = a.inverse_map_dev ? a.inverse_map_dev[i] : i;
    if (src < 0 || src >= a.n_qv) {
      atomicOr(&a.summary_dev->err, 2);         // reported through the error word; the vertex is left unwritten, as paint leaves it
      continue;
    }
    const int lab = a.labels_qv_dev[src];
    const float m = a.margin_qv_dev[src];
    float r = a.colors_full_dev[3 * i], g = a.colors_full_dev[3 * i + 1], b = a.colors_full_dev[3 * i + 2];
    if (lab > 0) {
      const int e = lab < a.n_palette ? lab : 1 + (lab - 1) % (a.n_palette - 1);   // a3d_session_paint's wrap
      r = pal[3 * e], g = pal[3 * e + 1], b = pal[3 * e + 2];
    }
    const float x = m * inv_full_margin;
    const float s = x < 1.f ? x : 1.f;          // (a comparison, not fminf: a NaN margin counts as sure)
    const float w = 1.f - s;
    const float r0 = r * s, r1 = dr * w, g0 = g * s, g1 = dg * w, b0 = b * s, b1 = db * w;
    a.margin_full_dev[i] = m;
    a.colors_out_dev[3 * i] = r0 + r1, a.colors_out_dev[3 * i + 1] = g0 + g1, a.colors_out_dev[3 * i + 2] = b0 + b1;
  }
}

}  // namespace a3d

using namespace a3d;

extern "C" int a3d_session_guide(const a3d_session_guide_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_session_guide: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_session_guide_args& a = *args;
  const bool bad_sizes = a.n_classes < 2 || a.n_classes > 256 || a.n_qv < 0 || a.n_qv > 0x7fffffffll || a.n_full < 0 ||
                         a.n_clicks < 0 || a.n_clicks > A3D_MAX_CLICKS;
  const bool bad_numbers = !std::isfinite(a.threshold) || !(a.threshold > 0.f) || !std::isfinite(a.full_margin) ||
                           !(a.full_margin > 0.f);
  const bool bad_voxels = a.n_qv > 0 && (!a.logits_dev || !a.labels_qv_dev || !a.runner_qv_dev || !a.margin_qv_dev || !a.want_qv_dev);
  const bool bad_full = a.n_full > 0 && (!a.colors_full_dev || !a.palette_dev || !a.margin_full_dev || !a.colors_out_dev ||
                                         a.n_palette < 2 || a.n_palette > 256 ||
                                         (a.n_qv > 0 && (!a.labels_qv_dev || !a.margin_qv_dev)));
  if (bad_sizes || bad_numbers || bad_voxels || bad_full || !a.summary_dev) {
    set_error("a3d_session_guide: bad arguments (n_qv=%lld classes=%d clicks=%d n_full=%lld palette=%d threshold=%g "
              "full_margin=%g)", (long long)a.n_qv, a.n_classes, a.n_clicks, (long long)a.n_full, a.n_palette,
              (double)a.threshold, (double)a.full_margin);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.summary_dev, 0, sizeof(a3d_session_guide_summary), st));   // (least_key 0: no row yet)
  if (a.n_qv > 0) {
    const int fit = kGuideTile / (a.n_classes | 1);
    const int tile_rows = fit < kGuideBlock ? fit : kGuideBlock;
    const long long n_tiles = (a.n_qv + tile_rows - 1) / tile_rows;
    k_guide_voxels<<<(unsigned)(n_tiles < kGuideMaxBlocks ? n_tiles : kGuideMaxBlocks), kGuideBlock, 0, st>>>(a, tile_rows, n_tiles);
    A3D_LAUNCH_CHECK();
  }
  if (a.n_full > 0) {
    const long long want = (a.n_full + kGuideBlock - 1) / kGuideBlock;
    k_guide_full<<<(unsigned)(want < 2048 ? want : 2048), kGuideBlock, 0, st>>>(a, 1.f / a.full_margin);
    A3D_LAUNCH_CHECK();
  }
  return A3D_OK;
}
