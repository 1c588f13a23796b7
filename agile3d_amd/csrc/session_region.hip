// session_region.hip -- correcting a labelling by hand (gfx950): a region of the screen as a mask image, the vertices a
// camera sees inside it, and a manual label layer laid over the model's labels.  Three entry points, one launch each.
//
// The reference has no counterpart: Open3D gives its tool no lasso, so a labelling that is nearly right can only be changed
// by another click, which runs the model again and may move other borders.  THE RULES (ours, stated in full in
// include/agile3d_hip.h at a3d_region_mask, a3d_select_vertices and a3d_session_overlay):
//   mask      per pixel: even-odd parity of a polygon's edges, or the distance to a stroke's segments against its radius;
//             REPLACE / ADD / SUBTRACT into a uint8 image
//   select    per vertex: project with the rows of [du dv d00]^-1, round to a pixel, the section's vertex rule, the mask, and
//             -- in the visible mode -- the depth test tt - t[pixel] <= slack with tt = k_pick_ray's t for the pixel's ray
//   overlay   per vertex: paint / erase the manual layer where selected, label = on ? manual : model, colour by
//             a3d_session_paint's palette rule
// All fp32 arithmetic is written one operation at a time with contraction off: a numpy float32 restatement gives the same
// bits (tests/region_rule.py).
//
// THE MASK is bound by its edge walk, not by memory: a pixel tests up to 256 edges.  The points travel by value in the kernel
// arguments (2 KB, like the click tables of session_guide.hip) and are staged in LDS once per workgroup; every lane of a
// wave then reads the same LDS address, a broadcast.  A workgroup is a 64 x 4 strip of pixels: a wave's stores are 64
// consecutive bytes of one image row.
// SELECT AND OVERLAY are streaming grid-stride passes over the vertices, memory bound, no MFMA: 12 bytes read and 1 written
// per vertex in select plus, for a vertex in view, one byte of the mask and four of the t image wherever it projects to
// (neighbouring vertices of a scan project to neighbouring pixels; both images of a 1024 x 768 view together are 3.75 MB and
// stay in L2); 22 bytes read and 16 written per vertex in an overlay with outputs.  Their summaries are integer sums:
// registers, wave shuffles, LDS, then ONE 64-bit atomic per workgroup and counter (none for a zero) -- sums of integers do not
// depend on the order of arrival, the record is the same from run to run.  Those atomics all land on the same two or three
// addresses and are served one after the other, about 15 ns each: at 1 M vertices a grid of 2048 workgroups of 256 spent
// 70 us in select, 45 of them in that queue.  Hence workgroups of 1024 threads and at most one per CU (256): 256 - 768
// atomics a call, 27 us (profiles/region_timing.txt); 16 waves per CU still hide the latency of the loads.
#include "session_device.h"
#include "session_rules.h"

namespace a3d {

constexpr int kMaskBlock = 256;
constexpr int kRegStripW = 64, kRegStripH = kMaskBlock / kRegStripW;  // the mask's workgroup: 64 x 4 pixels
constexpr int kRegBlock = 1024;               // select and overlay: FEW, FAT workgroups (see above) ...
constexpr int kRegMaxBlocks = 256;            // ... one per CU; longer inputs take further passes of the grid
static_assert(kMaskBlock >= A3D_REGION_MAX_POINTS, "k_region_mask stages one point per thread");
static_assert(sizeof(a3d_select_args) == 152 && sizeof(a3d_select_summary) == 24, "lib.py: SelectArgs, SelectSummary");
static_assert(sizeof(a3d_session_overlay_args) == 96 && sizeof(a3d_overlay_summary) == 32, "lib.py: SessionOverlayArgs, OverlaySummary");

struct MaskTab {
  float pt[A3D_REGION_MAX_POINTS][2];
  uint8_t* mask;
  int k, shape, mode;
  int width, height;
  float r2;                                   // radius * radius, one fp32 product
};

__global__ __launch_bounds__(kMaskBlock) void k_region_mask(const MaskTab t) {
#pragma clang fp contract(off)
  __shared__ float sx[A3D_REGION_MAX_POINTS], sy[A3D_REGION_MAX_POINTS];
  if ((int)threadIdx.x < t.k) sx[threadIdx.x] = t.pt[threadIdx.x][0], sy[threadIdx.x] = t.pt[threadIdx.x][1];
  __syncthreads();
  const int u = blockIdx.x * kRegStripW + (threadIdx.x & (kRegStripW - 1));
  const int v = blockIdx.y * kRegStripH + (threadIdx.x / kRegStripW);
  if (u >= t.width || v >= t.height) return;
  const float fx = (float)u, fy = (float)v;
  bool covered = false;
  if (t.shape == A3D_REGION_POLYGON) {
    for (int j = 0; j < t.k; ++j) {
      const int jn = j + 1 == t.k ? 0 : j + 1;
      const float ax = sx[j], ay = sy[j], bx = sx[jn], by = sy[jn];
      if ((ay > fy) != (by > fy)) {
        const float num = (bx - ax) * (fy - ay);
        const float xi = num / (by - ay) + ax;
        if (fx < xi) covered = !covered;
      }
    }
  } else {
    const int segments = t.k > 1 ? t.k - 1 : 1;
    for (int j = 0; j < segments && !covered; ++j) {
      const int jn = t.k > 1 ? j + 1 : j;
      const float ax = sx[j], ay = sy[j];
      const float ex = sx[jn] - ax, ey = sy[jn] - ay;
      const float wx = fx - ax, wy = fy - ay;
      const float L = ex * ex + ey * ey;
      float h = 0.f;
      if (L > 0.f) {
        const float q = (wx * ex + wy * ey) / L;
        h = q < 0.f ? 0.f : (q > 1.f ? 1.f : q);
      }
      const float dx = wx - h * ex, dy = wy - h * ey;
      covered = dx * dx + dy * dy <= t.r2;
    }
  }
  uint8_t* m = t.mask + (size_t)v * t.width + u;
  bool out = covered;
  if (t.mode == A3D_REGION_ADD)
    out = *m != 0 || covered;
  else if (t.mode == A3D_REGION_SUBTRACT)
    out = *m != 0 && !covered;
  *m = out ? 1 : 0;
}

struct SelectTab {
  const float* xyz;
  long long n;
  a3d_camera cam;
  float R[9];
  float slack;
  const uint8_t* mask;
  const float* t;
  uint8_t* selected;
  a3d_select_summary* summary;
};

__global__ __launch_bounds__(kRegBlock) void k_select_vertices(const SelectTab t, const a3d_section sec) {
#pragma clang fp contract(off)
  __shared__ int wave_sum[kRegBlock / 64];
  const float* __restrict__ xyz = t.xyz;
  const float fw = (float)t.cam.width, fh = (float)t.cam.height;
  int n_selected = 0, n_view = 0, odd = 0;     // (n < 2^31: a thread's share fits an int)
  const long long stride = (long long)gridDim.x * kRegBlock;
  for (long long i = (long long)blockIdx.x * kRegBlock + threadIdx.x; i < t.n; i += stride) {
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    if (not_finite(px) || not_finite(py) || not_finite(pz)) odd = 1;
    const float wx = px - t.cam.o[0], wy = py - t.cam.o[1], wz = pz - t.cam.o[2];
    const float a = (t.R[0] * wx + t.R[1] * wy) + t.R[2] * wz;
    const float b = (t.R[3] * wx + t.R[4] * wy) + t.R[5] * wz;
    const float c = (t.R[6] * wx + t.R[7] * wy) + t.R[8] * wz;
    const float x = a / c, y = b / c;
    const float xr = floorf(x + 0.5f), yr = floorf(y + 0.5f);
    const bool in_image = xr >= 0.f && xr < fw && yr >= 0.f && yr < fh;      // (a NaN fails)
    const bool in_view = c > 0.f && in_image && ses_keeps(sec, px, py, pz);
    bool sel = false;
    if (in_view) {                             // (in_image: the conversions below stay inside the image)
      const int u = (int)xr, v = (int)yr;
      const size_t pixel = (size_t)v * t.cam.width + u;
      sel = t.mask[pixel] != 0;
      if (sel && t.t) {
        float d[3];
        ses_pixel_ray(t.cam, u, v, d);
        const float tt = (wx * d[0] + wy * d[1]) + wz * d[2];               // k_pick_ray's t for this pixel's ray
        sel = tt - t.t[pixel] <= t.slack;
      }
    }
    t.selected[i] = sel ? 1 : 0;
    n_view += in_view, n_selected += sel;
  }
  const long long s_sel = block_sum<kRegBlock>(n_selected, wave_sum), s_view = block_sum<kRegBlock>(n_view, wave_sum);
  const long long s_odd = block_sum<kRegBlock>(odd, wave_sum);
  if (threadIdx.x == 0) {
    add_i64(&t.summary->selected, s_sel);
    add_i64(&t.summary->in_view, s_view);
    if (s_odd) atomicOr(&t.summary->flags, A3D_SELECT_NOT_FINITE);
  }
}

// One thread per vertex, grid-stride, the palette staged in LDS as k_session_paint stages it.
__global__ __launch_bounds__(kRegBlock) void k_session_overlay(const a3d_session_overlay_args a) {
  __shared__ float pal[256 * 3];
  __shared__ int wave_sum[kRegBlock / 64];
  const bool outputs = a.labels_out_dev != nullptr;
  if (outputs)
    for (int i = threadIdx.x; i < a.n_palette * 3; i += kRegBlock) pal[i] = a.palette_dev[i];
  __syncthreads();
  const bool edit = a.op != A3D_OVERLAY_NONE && a.selected_dev != nullptr;
  int n_changed = 0, n_on = 0, n_differ = 0, bad = 0;
  const long long stride = (long long)gridDim.x * kRegBlock;
  for (long long i = (long long)blockIdx.x * kRegBlock + threadIdx.x; i < a.n; i += stride) {
    bool on = a.manual_on_dev[i] != 0;
    int32_t obj = a.manual_obj_dev[i];
    const int32_t model = a.labels_in_dev[i];
    if (edit && a.selected_dev[i] != 0) {
      if (a.op == A3D_OVERLAY_PAINT) {
        if (!on || obj != a.obj) {
          ++n_changed;
          if (!on) a.manual_on_dev[i] = 1;
          if (obj != a.obj) a.manual_obj_dev[i] = a.obj;
          on = true, obj = a.obj;
        }
      } else if (on) {                         // A3D_OVERLAY_ERASE
        ++n_changed;
        a.manual_on_dev[i] = 0;
        on = false;
      }
    }
    n_on += on, n_differ += on && obj != model;
    const int32_t lab = on ? obj : model;
    if (lab < 0 || lab > 255) {
      bad = 1;                                 // reported through the error word; the vertex is left unwritten, as paint leaves it
      continue;
    }
    if (!outputs) continue;
    a.labels_out_dev[i] = lab;
    float r = a.colors_full_dev[3 * i], g = a.colors_full_dev[3 * i + 1], b = a.colors_full_dev[3 * i + 2];
    if (lab > 0) {
      const int e = lab < a.n_palette ? lab : 1 + (lab - 1) % (a.n_palette - 1);   // a3d_session_paint's wrap
      r = pal[3 * e], g = pal[3 * e + 1], b = pal[3 * e + 2];
    }
    a.colors_out_dev[3 * i] = r, a.colors_out_dev[3 * i + 1] = g, a.colors_out_dev[3 * i + 2] = b;
  }
  const long long s_changed = block_sum<kRegBlock>(n_changed, wave_sum), s_on = block_sum<kRegBlock>(n_on, wave_sum);
  const long long s_differ = block_sum<kRegBlock>(n_differ, wave_sum), s_bad = block_sum<kRegBlock>(bad, wave_sum);
  if (threadIdx.x == 0) {
    add_i64(&a.summary_dev->changed, s_changed);
    add_i64(&a.summary_dev->overridden, s_on);
    add_i64(&a.summary_dev->differing, s_differ);
    if (s_bad) atomicOr(&a.summary_dev->err, 1);
  }
}

}  // namespace a3d

using namespace a3d;

extern "C" int a3d_region_mask(int width, int height, int shape, const float* points, int n_points, float radius, int mode,
                               uint8_t* mask_dev, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool polygon = shape == A3D_REGION_POLYGON, stroke = shape == A3D_REGION_STROKE;
  const bool bad_sizes = width < 1 || height < 1 || width > A3D_RENDER_MAX_SIZE || height > A3D_RENDER_MAX_SIZE ||
                         n_points > A3D_REGION_MAX_POINTS || n_points < (polygon ? 3 : 1);
  const bool bad_radius = stroke && (!std::isfinite(radius) || !(radius > 0.f));
  if ((!polygon && !stroke) || mode < A3D_REGION_REPLACE || mode > A3D_REGION_SUBTRACT || bad_sizes || bad_radius || !points ||
      !mask_dev) {
    set_error("a3d_region_mask: bad arguments (%d x %d, shape=%d, points=%d%s, radius=%g, mode=%d%s)", width, height, shape,
              n_points, points ? "" : " (NULL)", (double)radius, mode, mask_dev ? "" : ", no mask");
    return A3D_ERR_INVALID;
  }
  MaskTab t;
  for (int j = 0; j < n_points; ++j) {
    if (!std::isfinite(points[2 * j]) || !std::isfinite(points[2 * j + 1])) {
      set_error("a3d_region_mask: point %d is not finite", j);
      return A3D_ERR_INVALID;
    }
    t.pt[j][0] = points[2 * j], t.pt[j][1] = points[2 * j + 1];
  }
  for (int j = n_points; j < A3D_REGION_MAX_POINTS; ++j) t.pt[j][0] = t.pt[j][1] = 0.f;
  t.mask = mask_dev, t.k = n_points, t.shape = shape, t.mode = mode, t.width = width, t.height = height;
  t.r2 = stroke ? radius * radius : 0.f;
  const dim3 grid((width + kRegStripW - 1) / kRegStripW, (height + kRegStripH - 1) / kRegStripH);
  k_region_mask<<<grid, kMaskBlock, 0, st>>>(t);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_select_vertices(const a3d_select_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_select_vertices: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_select_args& a = *args;
  double bounds[13];
  if (a3d_render_camera_bounds(&a.camera, bounds) != A3D_OK) {
    set_error("a3d_select_vertices: a camera the renders refuse");
    return A3D_ERR_INVALID;
  }
  const float zero[3] = {0.f, 0.f, 0.f};
  float cut[3];
  if (a3d_section_ray(a.section, zero, zero, cut) != A3D_OK) {       // (the section calls' own check; its text names the plane)
    char why[256];
    snprintf(why, sizeof why, "%s", get_error());
    set_error("a3d_select_vertices: %s", why);
    return A3D_ERR_INVALID;
  }
  bool rows_ok = true;
  for (int k = 0; k < 9; ++k) rows_ok = rows_ok && std::isfinite(a.rows[k]);
  if (!rows_ok || !std::isfinite(a.slack) || !(a.slack >= 0.f) || a.n < 0 || a.n >= (1ll << 31) || !a.mask_dev ||
      !a.summary_dev || (a.n > 0 && (!a.xyz_dev || !a.selected_dev))) {
    set_error("a3d_select_vertices: bad arguments (n=%lld slack=%g rows %s mask %s summary %s)", (long long)a.n, (double)a.slack,
              rows_ok ? "finite" : "NOT finite", a.mask_dev ? "given" : "NULL", a.summary_dev ? "given" : "NULL");
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.summary_dev, 0, sizeof(a3d_select_summary), st));
  if (a.n == 0) return A3D_OK;
  SelectTab t;
  t.xyz = a.xyz_dev, t.n = a.n, t.cam = a.camera, t.slack = a.slack;
  for (int k = 0; k < 9; ++k) t.R[k] = a.rows[k];
  t.mask = a.mask_dev, t.t = a.t_dev, t.selected = a.selected_dev, t.summary = a.summary_dev;
  a3d_section sec;
  memset(&sec, 0, sizeof sec);                 // no section: no plane
  if (a.section) sec = *a.section;
  k_select_vertices<<<capped_grid(a.n, kRegBlock, kRegMaxBlocks), kRegBlock, 0, st>>>(t, sec);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_session_overlay(const a3d_session_overlay_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_session_overlay: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_session_overlay_args& a = *args;
  const bool outputs = a.labels_out_dev || a.colors_out_dev;
  const bool bad_layer = a.n < 0 || a.n >= (1ll << 31) || a.op < A3D_OVERLAY_NONE || a.op > A3D_OVERLAY_ERASE || a.obj < 0 ||
                         a.obj > 255 || !a.summary_dev || (a.n > 0 && (!a.labels_in_dev || !a.manual_on_dev || !a.manual_obj_dev));
  const bool bad_outputs = outputs && (!a.labels_out_dev || !a.colors_out_dev || !a.colors_full_dev || !a.palette_dev ||
                                       a.n_palette < 2 || a.n_palette > 256);
  if (bad_layer || bad_outputs) {
    set_error("a3d_session_overlay: bad arguments (n=%lld op=%d obj=%d palette=%d outputs %s)", (long long)a.n, a.op, a.obj,
              a.n_palette, outputs ? "given" : "absent");
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.summary_dev, 0, sizeof(a3d_overlay_summary), st));
  if (a.n == 0) return A3D_OK;
  k_session_overlay<<<capped_grid(a.n, kRegBlock, kRegMaxBlocks), kRegBlock, 0, st>>>(a);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
