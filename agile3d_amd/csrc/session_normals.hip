// session_normals.hip -- one unoriented surface normal per level-0 voxel of a scan, from the points of its 3 x 3 x 3
// neighbourhood, lifted to the vertices; and the copy of a cloud's coordinates in which the vertices that face away from an
// eye are gone (gfx950).  Two entry points: a3d_estimate_normals, a3d_cull_points -- and a3d_normals_solve, stage B of ONE
// neighbourhood on the host, by the function the kernel calls, for the tests without a GPU.  With them a point cloud is
// lit and culled as a mesh is (a3d_render_shade_lit_points in session.hip is the lit pass).
//
// The reference has no counterpart: its tool shows clouds unlit.  THE RULES are ours, stated in full in
// include/agile3d_hip.h at the entry points and restated in tests/normals_rule.py; in one line each:
//   stage A   X_a = llrint(((double)x_a - origin_a) / quantum); a vertex counts when its row lies in 0..n-1 and |X_a| <= 2^bits;
//             per voxel (CALLER row) cnt, sum[3], mom[6] = the sums of 1, X, (XX, XY, XZ, YY, YZ, ZZ): integer atomics
//   stage B   N, S, M = the integer sums of those words over the voxel and its present neighbours (A3D_TAB_NBR27, both ends
//             through A3D_TAB_ORIGROW); recentred in integers about R = floor(S / N); then ONE sequential double-precision
//             computation: the covariance, 6 cyclic Jacobi sweeps, the column of the smallest diagonal entry, its sign
//   lift      normal_full[i] = normal_qv[inverse_map[i]], zero for a row outside
//   cull      g = (Nx (x - ex) + Ny (y - ey)) + Nz (z - ez) in fp32; BACK hides g > 0, FRONT hides g < 0; hidden = three NaNs
//
// WHY INTEGERS FIRST AND DOUBLES SECOND.  The sums of stage A arrive in whatever order the workgroups run; sums of integers
// do not depend on it, so two calls give the same words, and so does any permutation of the vertices.  Stage B reads only
// those words, and every thread runs a FIXED sequence of individually rounded + - x / sqrt (fp contract off): the result is
// a function of the words alone, and a restatement in numpy float64 scalars gives the same bits.
//
// THE SHAPE.  Stage A: one thread per vertex, grid-stride, ten integer atomics into a STRUCTURE OF ARRAYS (cnt int32 [n],
// nine uint64 [n] planes; two's complement, unsigned adds of signed values): the ten words of a voxel lie in ten planes, so
// that stage B's gather of one word over 27 neighbours reads 27 addresses of ONE plane, near each other.  Stage B: one thread
// per voxel in the INTERNAL (Morton) order -- the 27 neighbours a wave touches lie near each other -- in STAGES without a
// branch between the loads of a stage, as session_grow.hip's sweep learnt: the 27 rows of the table together, the 27 caller
// rows together, then each plane's 27 words together (a missing neighbour reads this row itself and is masked to 0).
// Holding all 270 words at once takes 500 registers (written that way the kernel spilled 1.2 KB a lane); one plane at a time
// takes 54: the loop over the planes is NOT unrolled and parks each sum in the thread's own LDS column.  Then ~600 fp64
// operations a voxel, which gfx950 issues at the full vector rate: the pass is bound by its gathers.
// THE SUMMARY (counted vertices; voxels with and without a valid normal; the error word) is integer sums reduced per
// workgroup -- registers, wave shuffles, LDS -- and ONE atomic per workgroup and counter (none for a zero), from few, fat
// workgroups for the reason recorded at a3d_select_vertices -- in stage A, the lift and the cull.  Stage B is the exception:
// it is bound by the latency of a thread's chain of gathers and fp64 divisions, not by bytes or atomics, and a scene holds
// few voxels per CU (92 k voxels: 360).  With 512-thread workgroups, one per CU, 136 k voxels made 266 workgroups on 256 CUs
// and the last ten ran as a second round: 277 us against 97 us for 92 k (profiles/normals_timing.txt).  Hence 256 threads
// (it holds 169 registers: three waves a SIMD) and up to 1024 workgroups, which a CU takes three at a time.
// No grid barrier, no spin-wait: the stages are launches, ordered by the stream.  The library allocates nothing and does
// not synchronise.
#include "session_solve.h"

namespace a3d {

constexpr int kNrmFat = 1024;                 // stage A, the lift, the cull: few, fat workgroups ...
constexpr int kNrmFatBlocks = 256;            // ... at most one per CU
constexpr int kNrmB = 256;                    // stage B (see above)
constexpr int kNrmBBlocks = 1024;
static_assert(sizeof(a3d_estimate_normals_args) == 168 && sizeof(a3d_normals_summary) == 32, "lib.py: EstimateNormalsArgs, NormalsSummary");

struct NormalsWs {
  int32_t* cnt;                // [n] vertices counted in the voxel (caller row)
  u64* word;                   // [9][n] X, Y, Z, XX, XY, XZ, YY, YZ, ZZ (two's complement)
  float* normal;               // [n][3] stage B's normals, for the lift
  size_t plane;                // elements between two planes of word
  size_t zero_bytes, bytes;    // cnt and word are cleared together
};
static NormalsWs carve_normals(void* base, long long n) {
  NormalsWs w;
  Carver c{base};
  const size_t m = (size_t)(n > 0 ? n : 1);
  w.cnt = (int32_t*)c.take(m * 4);
  w.plane = align256(m * 8) / 8;
  w.word = (u64*)c.take(9 * w.plane * 8);
  w.zero_bytes = c.off;
  w.normal = (float*)c.take(m * 12);
  w.bytes = c.off;
  return w;
}

// ---- stage A: the ten words of every voxel ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNrmFat) void k_normals_moments(const a3d_estimate_normals_args a, const NormalsWs w, const double lim) {
  __shared__ int wave_part[kNrmFat / 64];
  const long long stride = (long long)gridDim.x * kNrmFat;
  int counted = 0, err = 0;                    // (n_full < 2^31: a thread's share fits an int)
  for (long long i = (long long)blockIdx.x * kNrmFat + threadIdx.x; i < a.n_full; i += stride) {
    const long long row = a.inverse_map_dev ? a.inverse_map_dev[i] : i;
    const float x = a.xyz_dev[3 * i], y = a.xyz_dev[3 * i + 1], z = a.xyz_dev[3 * i + 2];
    long long X = 0, Y = 0, Z = 0;
    const bool fx = fixed_point(x, a.origin[0], a.quantum, lim, X), fy = fixed_point(y, a.origin[1], a.quantum, lim, Y),
               fz = fixed_point(z, a.origin[2], a.quantum, lim, Z);
    const bool in_range = fx && fy && fz, inside = row >= 0 && row < a.n;
    if (!inside) err |= A3D_NORMALS_BAD_INDEX;
    if (!in_range) err |= A3D_NORMALS_RANGE;
    if (!(inside && in_range)) continue;
    ++counted;
    atomicAdd(w.cnt + row, 1);
    u64* p = w.word + row;
    atomicAdd(p, (u64)X), atomicAdd(p + w.plane, (u64)Y), atomicAdd(p + 2 * w.plane, (u64)Z);
    atomicAdd(p + 3 * w.plane, (u64)(X * X)), atomicAdd(p + 4 * w.plane, (u64)(X * Y)), atomicAdd(p + 5 * w.plane, (u64)(X * Z));
    atomicAdd(p + 6 * w.plane, (u64)(Y * Y)), atomicAdd(p + 7 * w.plane, (u64)(Y * Z)), atomicAdd(p + 8 * w.plane, (u64)(Z * Z));
  }
  const long long s_counted = block_sum<kNrmFat>(counted, wave_part), s_err_range = block_sum<kNrmFat>(err & A3D_NORMALS_RANGE, wave_part),
                  s_err_index = block_sum<kNrmFat>(err & A3D_NORMALS_BAD_INDEX, wave_part);
  if (threadIdx.x == 0) {
    add_i64(&a.summary_dev->counted, s_counted);
    const int e = (s_err_range ? A3D_NORMALS_RANGE : 0) | (s_err_index ? A3D_NORMALS_BAD_INDEX : 0);
    if (e) atomicOr(&a.summary_dev->err, e);
  }
}

__global__ __launch_bounds__(kNrmB) void k_normals_solve(const a3d_estimate_normals_args a, const NormalsWs w,
                                                         const int32_t* __restrict__ nbr, const int32_t* __restrict__ orig,
                                                         const int n, const int npad) {
  __shared__ int wave_part[kNrmB / 64];
  __shared__ u64 sums[9][kNrmB];               // a thread's nine sums, in its own column (18 KB; nobody else reads them)
  const int stride = gridDim.x * kNrmB;
  int n_valid = 0, n_invalid = 0;
  for (int r = blockIdx.x * kNrmB + threadIdx.x; r < n; r += stride) {
    const int i = orig[r];
    int j[27];
    unsigned present = 0;                      // bit k: the neighbour at offset k is there
    {
      int jr[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) jr[k] = k == 13 ? r : nbr[(size_t)k * npad + r];   // (the centre is this voxel, whatever the table holds)
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        const bool there = (unsigned)jr[k] < (unsigned)n;
        present |= (unsigned)there << k;
        j[k] = orig[there ? jr[k] : r];        // a missing neighbour: this row itself, masked below
      }
    }
    long long N = 0;
    {
      int c[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) c[k] = w.cnt[j[k]];
#pragma unroll
      for (int k = 0; k < 27; ++k) N += (present >> k) & 1 ? c[k] : 0;
    }
    // one plane at a time (NOT unrolled: all nine planes' loads in flight at once would take 500 registers and spill)
#pragma unroll 1
    for (int p = 0; p < 9; ++p) {
      const u64* plane = w.word + (size_t)p * w.plane;
      u64 x[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) x[k] = plane[j[k]];
      u64 sum = 0;
#pragma unroll
      for (int k = 0; k < 27; ++k) sum += (present >> k) & 1 ? x[k] : 0ull;
      sums[p][threadIdx.x] = sum;
    }
    u64 T[9];
#pragma unroll
    for (int p = 0; p < 9; ++p) T[p] = sums[p][threadIdx.x];
    float normal[3], variation;
    const bool valid = nrm_solve(N, T, T + 3, a, normal, variation);
    n_valid += valid, n_invalid += !valid;
    w.normal[3 * (size_t)i] = normal[0], w.normal[3 * (size_t)i + 1] = normal[1], w.normal[3 * (size_t)i + 2] = normal[2];
    if (a.normal_qv_dev)
      a.normal_qv_dev[3 * (size_t)i] = normal[0], a.normal_qv_dev[3 * (size_t)i + 1] = normal[1], a.normal_qv_dev[3 * (size_t)i + 2] = normal[2];
    if (a.variation_qv_dev) a.variation_qv_dev[i] = variation;
    if (a.count_qv_dev) a.count_qv_dev[i] = (int32_t)N;
    if (a.moments_qv_dev) {                    // stage A's own words of THIS voxel
      int64_t* out = a.moments_qv_dev + 10 * (size_t)i;
      out[0] = w.cnt[i];
#pragma unroll
      for (int p = 0; p < 9; ++p) out[1 + p] = (int64_t)w.word[(size_t)p * w.plane + i];
    }
  }
  const long long s_valid = block_sum<kNrmB>(n_valid, wave_part), s_invalid = block_sum<kNrmB>(n_invalid, wave_part);
  if (threadIdx.x == 0) add_i64(&a.summary_dev->valid, s_valid), add_i64(&a.summary_dev->invalid, s_invalid);
}

// ---- the lift: behind a launch boundary (plain loads) --------------------------------------------------------------------------
__global__ __launch_bounds__(kNrmFat) void k_normals_lift(const a3d_estimate_normals_args a, const float* __restrict__ normal) {
  const long long stride = (long long)gridDim.x * kNrmFat;
  for (long long i = (long long)blockIdx.x * kNrmFat + threadIdx.x; i < a.n_full; i += stride) {
    const long long row = a.inverse_map_dev ? a.inverse_map_dev[i] : i;
    float x = 0.f, y = 0.f, z = 0.f;
    if (row >= 0 && row < a.n) x = normal[3 * row], y = normal[3 * row + 1], z = normal[3 * row + 2];
    a.normal_full_dev[3 * i] = x, a.normal_full_dev[3 * i + 1] = y, a.normal_full_dev[3 * i + 2] = z;
  }
}

// ---- culling a cloud ---------------------------------------------------------------------------------------------------------
struct CullTab {
  const float *xyz, *normals;
  float* out;
  uint8_t* hidden;
  int64_t* count;
  long long n;
  float eye[3];
  int mode;
};
__global__ __launch_bounds__(kNrmFat) void k_cull_points(const CullTab t) {
#pragma clang fp contract(off)
  __shared__ int wave_part[kNrmFat / 64];
  const long long stride = (long long)gridDim.x * kNrmFat;
  int n_hidden = 0;
  for (long long i = (long long)blockIdx.x * kNrmFat + threadIdx.x; i < t.n; i += stride) {
    float x = t.xyz[3 * i], y = t.xyz[3 * i + 1], z = t.xyz[3 * i + 2];
    const float nx = t.normals[3 * i], ny = t.normals[3 * i + 1], nz = t.normals[3 * i + 2];
    const float wx = x - t.eye[0], wy = y - t.eye[1], wz = z - t.eye[2];
    const float g = (nx * wx + ny * wy) + nz * wz;
    const bool hide = t.mode == A3D_CULL_BACK ? g > 0.f : g < 0.f;     // (a NaN g fails both: the vertex shows)
    if (hide) x = y = z = __uint_as_float(0x7fc00000u);
    t.out[3 * i] = x, t.out[3 * i + 1] = y, t.out[3 * i + 2] = z;
    if (t.hidden) t.hidden[i] = hide ? 1 : 0;
    n_hidden += hide;
  }
  if (t.count) {                               // (uniform over the launch)
    const long long s = block_sum<kNrmFat>(n_hidden, wave_part);
    if (threadIdx.x == 0) add_i64(t.count, s);
  }
}

}  // namespace a3d

using namespace a3d;

extern "C" size_t a3d_normals_workspace_bytes(int64_t n) {
  if (n < 0 || n > 0x7fffffffll) return 0;
  return carve_normals(nullptr, n).bytes;
}

extern "C" int a3d_estimate_normals(const a3d_estimate_normals_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_estimate_normals: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_estimate_normals_args& a = *args;
  const a3d_scene* s = a.scene;
  const bool bad_scene = !scene_walkable(s, a.n);
  const bool bits_ok = a.bits >= 0 && a.bits <= A3D_MEASURE_MAX_BITS;
  // n_full 2^(2 bits) <= 2^62, in integers (a3d_measure_objects' bound)
  const bool sums_ok = bits_ok && a.n_full >= 0 && a.n_full < (1ll << 31) && a.n_full <= ((1ll << 62) >> (2 * a.bits));
  bool frame_ok = power_of_two(a.quantum);
  for (int k = 0; k < 3; ++k) frame_ok = frame_ok && std::isfinite(a.origin[k]) && (!a.has_viewpoint || std::isfinite(a.viewpoint[k]));
  if (bad_scene || !sums_ok || !frame_ok || (a.n_full > 0 && !a.xyz_dev) || !a.summary_dev || !a.workspace_dev ||
      ((uintptr_t)a.workspace_dev & 255) || a.workspace_bytes < a3d_normals_workspace_bytes(a.n)) {
    set_error("a3d_estimate_normals: bad arguments (scene %s, n=%lld n_full=%lld bits=%d quantum=%g xyz %s summary %s "
              "workspace=%zu; origin and viewpoint must be finite)", s ? "given" : "NULL", (long long)a.n, (long long)a.n_full,
              a.bits, a.quantum, a.xyz_dev ? "given" : "NULL", a.summary_dev ? "given" : "NULL", a.workspace_bytes);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.summary_dev, 0, sizeof(a3d_normals_summary), st));
  const int n = (int)a.n;
  const NormalsWs w = carve_normals(a.workspace_dev, n);
  A3D_HIP_CHECK(hipMemsetAsync(w.cnt, 0, w.zero_bytes, st));
  if (a.n_full > 0) {
    k_normals_moments<<<capped_grid(a.n_full, kNrmFat, kNrmFatBlocks), kNrmFat, 0, st>>>(a, w, std::ldexp(1.0, a.bits));
    A3D_LAUNCH_CHECK();
  }
  if (n > 0) {
    k_normals_solve<<<capped_grid(n, kNrmB, kNrmBBlocks), kNrmB, 0, st>>>(a, w, s->lv[0].nbr27, s->orig_row, n, s->lv[0].npad);
    A3D_LAUNCH_CHECK();
  }
  if (a.n_full > 0 && a.normal_full_dev) {
    k_normals_lift<<<capped_grid(a.n_full, kNrmFat, kNrmFatBlocks), kNrmFat, 0, st>>>(a, w.normal);
    A3D_LAUNCH_CHECK();
  }
  return A3D_OK;
}

extern "C" int a3d_normals_solve(int64_t count, const int64_t* sum3, const int64_t* mom6, const double* origin, double quantum,
                                 const double* viewpoint, float* out5) {
  if (count < 0 || !sum3 || !mom6 || !origin || !out5 || !power_of_two(quantum)) {
    set_error("a3d_normals_solve: bad arguments (count=%lld quantum=%g)", (long long)count, quantum);
    return A3D_ERR_INVALID;
  }
  a3d_estimate_normals_args a = {};
  u64 T[9];
  for (int k = 0; k < 3; ++k) a.origin[k] = origin[k], a.viewpoint[k] = viewpoint ? viewpoint[k] : 0.0, T[k] = (u64)sum3[k];
  for (int k = 0; k < 6; ++k) T[3 + k] = (u64)mom6[k];
  a.quantum = quantum, a.has_viewpoint = viewpoint != nullptr;
  out5[4] = nrm_solve(count, T, T + 3, a, out5, out5[3]) ? 1.f : 0.f;
  return A3D_OK;
}

extern "C" int a3d_cull_points(const float* xyz_dev, const float* normals_dev, int64_t n, const float* eye, int mode,
                               float* xyz_out_dev, uint8_t* hidden_dev, int64_t* count_dev, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n < 0 || n >= (1ll << 31) || (mode != A3D_CULL_BACK && mode != A3D_CULL_FRONT) || !eye || !std::isfinite(eye[0]) ||
      !std::isfinite(eye[1]) || !std::isfinite(eye[2]) || (n > 0 && (!xyz_dev || !normals_dev || !xyz_out_dev)) ||
      ((uintptr_t)count_dev & 7)) {
    set_error("a3d_cull_points: bad arguments (n=%lld mode=%d; a finite eye, A3D_CULL_BACK or A3D_CULL_FRONT, xyz_dev, normals_dev "
              "and xyz_out_dev are needed)", (long long)n, mode);
    return A3D_ERR_INVALID;
  }
  if (count_dev) A3D_HIP_CHECK(hipMemsetAsync(count_dev, 0, sizeof(int64_t), st));
  if (n > 0) {
    CullTab t;
    t.xyz = xyz_dev, t.normals = normals_dev, t.out = xyz_out_dev, t.hidden = hidden_dev, t.count = count_dev, t.n = n, t.mode = mode;
    for (int k = 0; k < 3; ++k) t.eye[k] = eye[k];
    k_cull_points<<<capped_grid(n, kNrmFat, kNrmFatBlocks), kNrmFat, 0, st>>>(t);
    A3D_LAUNCH_CHECK();
  }
  return A3D_OK;
}
