// session_measure.hip -- how big the objects of a labelling are and where they lie (gfx950).  Two entry points:
// a3d_measure_objects (per object id: vertices, voxels, the exact box, first and second moments, covered surface) and
// a3d_object_extents (the second pass of an oriented box: the extent of every object along three axes of its own).
//
// The reference has no counterpart: its tool writes a mask and measures nothing.
// THE RULES (ours, stated in include/agile3d_hip.h at the two entry points) in one line each:
//   moments   X_a = llrint(((double)x_a - origin_a) / quantum); a vertex counts when its label is in range and |X_a| <= 2^bits;
//             sum = the sum of X, mom = the sums of (XX, XY, XZ, YY, YZ, ZZ), all int64
//   box       min / max over the order-preserving uint32 key of the fp32 bits: the total order, -0 below +0
//   area      Q = llrint(|e1 x e2| / area_quantum) in double, no fma contraction, added to the object of each corner
//   extents   p = (a_x*x + a_y*y) + a_z*z in fp32, no fma contraction; min / max by the same key
//
// WHY INTEGERS: sums of integers, minima and maxima do not depend on the order of arrival -- two calls give the same bytes and
// so does any permutation of the vertices.  The bounds under which no int64 sum can overflow are checked on the host before
// anything is launched (header: n 2^(2 bits) <= 2^62; m <= 2^23 with Q <= 2^38).
//
// THE SHAPE of the vertex kernels (k_measure_vertices, k_extents_vertices): a workgroup of kMeasBlock threads owns kMeasChunk
// CONSECUTIVE vertices and keeps all 256 records in LDS (25 600 bytes; 6 144 for the extents).  Labels are coherent in space,
// so a wave's 64 lanes mostly carry ONE label: such a wave folds its lanes with shuffles and lane 0 sends one set of LDS
// atomics -- 64 lanes adding to one LDS address would serialise.  A mixed wave falls back to per-lane LDS atomics.  At the end
// of the chunk thread k sends record k, if it is not empty, to global memory: 64-bit integer adds and unsigned 32-bit min /
// max, which gfx950 has as single instructions in LDS and in global memory (no compare-and-swap loop).
// Within a wave a sum of 64 coordinates fits int32 (64 x 2^20 = 2^26); the products need 64 bits (64 x 2^40).
// Voxels (k_measure_voxels: a histogram) and faces (k_measure_faces) are grid-stride launches of their own with the same
// uniform-wave fold.  The records are prepared by k_measure_init (zeros; lo = key(+inf), hi = key(-inf)) and the keys turned
// back into floats IN PLACE by k_measure_finish: five small launches at most, ordered by the stream.
// The error word collects in a register per thread, is folded per wave and sent with one atomicOr.
#include "session_device.h"

namespace a3d {

constexpr int kMeasBlock = A3D_MEASURE_BLOCK;
constexpr int kMeasChunk = A3D_MEASURE_CHUNK;
constexpr int kMeasIds = 256;
constexpr int kMeasMaxBlocks = 1024;                      // grid-stride launches (voxels, faces)
constexpr unsigned kKeyPosInf = 0x7f800000u ^ 0x80000000u;   // key(+inf)
constexpr unsigned kKeyNegInf = ~0xff800000u;                // key(-inf)
static_assert(kMeasBlock == kMeasIds, "thread k of a workgroup owns record k");
static_assert(kMeasChunk % kMeasBlock == 0, "a chunk is whole rounds of the workgroup");
static_assert(sizeof(a3d_object_moments) == 128, "the record of the header");

// the total order of fp32 bit patterns as an unsigned order: negative values are complemented, the others get the top bit
__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}
__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  return v;
}
// the label every counting lane of the wave carries, or -1 when they carry more than one (`live` is not empty)
__device__ __forceinline__ int wave_label(bool counts, int label, u64 live) {
  const int first = __shfl(label, __ffsll((long long)live) - 1);
  return __all(!counts || label == first) ? first : -1;
}

struct MeasureLds {
  u64 sum[9][kMeasIds];          // X, Y, Z, XX, XY, XZ, YY, YZ, ZZ (two's complement: unsigned adds of signed values)
  unsigned cnt[kMeasIds];
  unsigned lo[3][kMeasIds], hi[3][kMeasIds];
};

__global__ __launch_bounds__(kMeasIds) void k_measure_init(a3d_object_moments* out, int32_t* err, const int n_classes) {
  const int k = threadIdx.x;
  if (k == 0) err[0] = 0;
  if (k >= n_classes) return;
  u64* w = (u64*)(out + k);
#pragma unroll
  for (int j = 0; j < 12; ++j) w[j] = 0;                 // vertices, voxels, sum, mom, area_thirds
  unsigned* lo = (unsigned*)out[k].lo;
  unsigned* hi = (unsigned*)out[k].hi;
#pragma unroll
  for (int c = 0; c < 3; ++c) lo[c] = kKeyPosInf, hi[c] = kKeyNegInf;
  out[k].reserved_[0] = out[k].reserved_[1] = 0;
}

__global__ __launch_bounds__(kMeasIds) void k_measure_finish(a3d_object_moments* out, const int n_classes) {
  const int k = threadIdx.x;
  if (k >= n_classes) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out[k].lo[c] = value_of(((const unsigned*)out[k].lo)[c]);
    out[k].hi[c] = value_of(((const unsigned*)out[k].hi)[c]);
  }
}

__global__ __launch_bounds__(kMeasBlock) void k_measure_vertices(const a3d_measure_args a, const double lim) {
  __shared__ MeasureLds s;
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 9; ++j) s.sum[j][tid] = 0;
  s.cnt[tid] = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) s.lo[c][tid] = kKeyPosInf, s.hi[c][tid] = kKeyNegInf;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kMeasChunk;
  int err = 0;
  for (int it = 0; it < kMeasChunk / kMeasBlock; ++it) {
    const long long first_row = base + (long long)it * kMeasBlock;
    if (first_row >= a.n) break;
    const long long i = first_row + tid;
    bool counts = false;
    int label = 0;
    long long X = 0, Y = 0, Z = 0;
    unsigned kx = 0, ky = 0, kz = 0;
    if (i < a.n) {
      label = a.labels_dev[i];
      const float x = a.xyz_dev[3 * i], y = a.xyz_dev[3 * i + 1], z = a.xyz_dev[3 * i + 2];
      const bool in_label = (unsigned)label < (unsigned)a.n_classes;
      const bool fx = fixed_point(x, a.origin[0], a.quantum, lim, X), fy = fixed_point(y, a.origin[1], a.quantum, lim, Y),
                 fz = fixed_point(z, a.origin[2], a.quantum, lim, Z);
      const bool in_range = fx && fy && fz;
      if (!in_label) err |= A3D_MEASURE_BAD_LABEL;
      if (!in_range) err |= A3D_MEASURE_RANGE;
      counts = in_label && in_range;
      kx = key_of(x), ky = key_of(y), kz = key_of(z);
    }
    const u64 live = __ballot(counts);
    if (!live) continue;
    const int one = wave_label(counts, label, live);
    if (one >= 0) {                                        // one object in the wave: fold, then one set of LDS atomics
      const int cnt = wave_sum(counts ? 1 : 0);
      const int sx = wave_sum(counts ? (int)X : 0), sy = wave_sum(counts ? (int)Y : 0), sz = wave_sum(counts ? (int)Z : 0);
      const long long xx = wave_sum(counts ? X * X : 0ll), xy = wave_sum(counts ? X * Y : 0ll), xz = wave_sum(counts ? X * Z : 0ll);
      const long long yy = wave_sum(counts ? Y * Y : 0ll), yz = wave_sum(counts ? Y * Z : 0ll), zz = wave_sum(counts ? Z * Z : 0ll);
      const unsigned lx = wave_min(counts ? kx : 0xffffffffu), ly = wave_min(counts ? ky : 0xffffffffu),
                     lz = wave_min(counts ? kz : 0xffffffffu);
      const unsigned hx = wave_max(counts ? kx : 0u), hy = wave_max(counts ? ky : 0u), hz = wave_max(counts ? kz : 0u);
      if ((tid & 63) == 0) {
        atomicAdd(&s.cnt[one], (unsigned)cnt);
        atomicAdd(&s.sum[0][one], (u64)(long long)sx), atomicAdd(&s.sum[1][one], (u64)(long long)sy);
        atomicAdd(&s.sum[2][one], (u64)(long long)sz);
        atomicAdd(&s.sum[3][one], (u64)xx), atomicAdd(&s.sum[4][one], (u64)xy), atomicAdd(&s.sum[5][one], (u64)xz);
        atomicAdd(&s.sum[6][one], (u64)yy), atomicAdd(&s.sum[7][one], (u64)yz), atomicAdd(&s.sum[8][one], (u64)zz);
        atomicMin(&s.lo[0][one], lx), atomicMin(&s.lo[1][one], ly), atomicMin(&s.lo[2][one], lz);
        atomicMax(&s.hi[0][one], hx), atomicMax(&s.hi[1][one], hy), atomicMax(&s.hi[2][one], hz);
      }
    } else if (counts) {
      atomicAdd(&s.cnt[label], 1u);
      atomicAdd(&s.sum[0][label], (u64)X), atomicAdd(&s.sum[1][label], (u64)Y), atomicAdd(&s.sum[2][label], (u64)Z);
      atomicAdd(&s.sum[3][label], (u64)(X * X)), atomicAdd(&s.sum[4][label], (u64)(X * Y)), atomicAdd(&s.sum[5][label], (u64)(X * Z));
      atomicAdd(&s.sum[6][label], (u64)(Y * Y)), atomicAdd(&s.sum[7][label], (u64)(Y * Z)), atomicAdd(&s.sum[8][label], (u64)(Z * Z));
      atomicMin(&s.lo[0][label], kx), atomicMin(&s.lo[1][label], ky), atomicMin(&s.lo[2][label], kz);
      atomicMax(&s.hi[0][label], kx), atomicMax(&s.hi[1][label], ky), atomicMax(&s.hi[2][label], kz);
    }
  }
  __syncthreads();
  if (tid < a.n_classes && s.cnt[tid]) {                   // the non-empty records of this chunk
    a3d_object_moments* o = a.out_dev + tid;
    atomicAdd((u64*)&o->vertices, (u64)s.cnt[tid]);
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicAdd((u64*)&o->sum[c], s.sum[c][tid]);
#pragma unroll
    for (int c = 0; c < 6; ++c) atomicAdd((u64*)&o->mom[c], s.sum[3 + c][tid]);
#pragma unroll
    for (int c = 0; c < 3; ++c) atomicMin((unsigned*)&o->lo[c], s.lo[c][tid]), atomicMax((unsigned*)&o->hi[c], s.hi[c][tid]);
  }
  send_error(a.err_dev, err);
}

__global__ __launch_bounds__(kMeasBlock) void k_measure_voxels(const a3d_measure_args a) {
  __shared__ unsigned hist[kMeasIds];
  const int tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  int err = 0;
  const long long stride = (long long)gridDim.x * kMeasBlock;
  for (long long base = (long long)blockIdx.x * kMeasBlock; base < a.n_qv; base += stride) {
    const long long i = base + tid;
    int label = 0;
    bool counts = false;
    if (i < a.n_qv) {
      label = a.labels_qv_dev[i];
      counts = (unsigned)label < (unsigned)a.n_classes;
      if (!counts) err |= A3D_MEASURE_BAD_LABEL;
    }
    const u64 live = __ballot(counts);
    if (!live) continue;
    const int one = wave_label(counts, label, live);
    if (one >= 0) {
      if ((tid & 63) == 0) atomicAdd(&hist[one], (unsigned)__popcll(live));
    } else if (counts) {
      atomicAdd(&hist[label], 1u);
    }
  }
  __syncthreads();
  if (tid < a.n_classes && hist[tid]) atomicAdd((u64*)&a.out_dev[tid].voxels, (u64)hist[tid]);
  send_error(a.err_dev, err);
}

// Q of one face in double, every operation rounded on its own (hipcc contracts to fma by default); false: above the cap or NaN
__device__ __forceinline__ bool face_quanta(const float* __restrict__ xyz, int ia, int ib, int ic, double area_quantum,
                                            long long& Q) {
#pragma clang fp contract(off)
  const double ax = xyz[3 * (size_t)ia], ay = xyz[3 * (size_t)ia + 1], az = xyz[3 * (size_t)ia + 2];
  const double e1x = (double)xyz[3 * (size_t)ib] - ax, e1y = (double)xyz[3 * (size_t)ib + 1] - ay,
               e1z = (double)xyz[3 * (size_t)ib + 2] - az;
  const double e2x = (double)xyz[3 * (size_t)ic] - ax, e2y = (double)xyz[3 * (size_t)ic + 1] - ay,
               e2z = (double)xyz[3 * (size_t)ic + 2] - az;
  const double p0 = e1y * e2z, p1 = e1z * e2y, p2 = e1z * e2x, p3 = e1x * e2z, p4 = e1x * e2y, p5 = e1y * e2x;
  const double nx = p0 - p1, ny = p2 - p3, nz = p4 - p5;
  const double xx = nx * nx, yy = ny * ny, zz = nz * nz;
  const double len = sqrt((xx + yy) + zz);
  const double q = rint(len / area_quantum);
  if (!(q <= (double)A3D_MEASURE_MAX_Q)) return false;
  Q = (long long)q;
  return true;
}

__global__ __launch_bounds__(kMeasBlock) void k_measure_faces(const a3d_measure_args a) {
  __shared__ u64 area[kMeasIds];
  const int tid = threadIdx.x;
  area[tid] = 0;
  __syncthreads();
  int err = 0;
  const unsigned n = (unsigned)a.n, classes = (unsigned)a.n_classes;
  const long long stride = (long long)gridDim.x * kMeasBlock;
  for (long long base = (long long)blockIdx.x * kMeasBlock; base < a.m; base += stride) {
    const long long f = base + tid;
    bool counts = false;
    int la = 0, lb = 0, lc = 0;
    long long Q = 0;
    if (f < a.m) {
      const int ia = a.faces_dev[3 * f], ib = a.faces_dev[3 * f + 1], ic = a.faces_dev[3 * f + 2];
      if ((unsigned)ia < n && (unsigned)ib < n && (unsigned)ic < n) {          // (n < 2^31: a negative index fails as well)
        la = a.labels_dev[ia], lb = a.labels_dev[ib], lc = a.labels_dev[ic];
        if ((unsigned)la >= classes || (unsigned)lb >= classes || (unsigned)lc >= classes) {
          err |= A3D_MEASURE_BAD_LABEL;
        } else if (!face_quanta(a.xyz_dev, ia, ib, ic, a.area_quantum, Q)) {
          err |= A3D_MEASURE_RANGE;
        } else {
          counts = true;
        }
      }
    }
    const u64 live = __ballot(counts);
    if (!live) continue;
    const int one = wave_label(counts, la, live);
    if (__all(!counts || (la == lb && lb == lc)) && one >= 0) {   // every face of the wave inside one object
      const long long q = wave_sum(counts ? Q : 0ll);
      if ((tid & 63) == 0) atomicAdd(&area[one], (u64)(3 * q));
    } else if (counts) {
      atomicAdd(&area[la], (u64)Q), atomicAdd(&area[lb], (u64)Q), atomicAdd(&area[lc], (u64)Q);
    }
  }
  __syncthreads();
  if (tid < a.n_classes && area[tid]) atomicAdd((u64*)&a.out_dev[tid].area_thirds, area[tid]);
  send_error(a.err_dev, err);
}

// ---- extents ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float project(const float* __restrict__ ax, float x, float y, float z) {
#pragma clang fp contract(off)
  const float px = ax[0] * x, py = ax[1] * y, pz = ax[2] * z;
  return (px + py) + pz;
}

__global__ __launch_bounds__(kMeasIds) void k_extents_init(unsigned* out, int32_t* err, const int n_classes) {
  const int k = threadIdx.x;
  if (k == 0) err[0] = 0;
  if (k >= n_classes) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) out[6 * k + 2 * j] = kKeyPosInf, out[6 * k + 2 * j + 1] = kKeyNegInf;
}

__global__ __launch_bounds__(kMeasIds) void k_extents_finish(float* out, const int n_classes) {
  const int k = threadIdx.x;
  if (k >= n_classes) return;
#pragma unroll
  for (int j = 0; j < 6; ++j) out[6 * k + j] = value_of(((const unsigned*)out)[6 * k + j]);
}

__global__ __launch_bounds__(kMeasBlock) void k_extents_vertices(const a3d_extents_args a) {
  __shared__ unsigned lo[3][kMeasIds], hi[3][kMeasIds];
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 3; ++j) lo[j][tid] = 0xffffffffu, hi[j][tid] = 0u;      // (no key is below 0 or above 2^32 - 1)
  __syncthreads();
  const long long base = (long long)blockIdx.x * kMeasChunk;
  int err = 0;
  for (int it = 0; it < kMeasChunk / kMeasBlock; ++it) {
    const long long first_row = base + (long long)it * kMeasBlock;
    if (first_row >= a.n) break;
    const long long i = first_row + tid;
    bool counts = false;
    int label = 0;
    unsigned kmin[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, kmax[3] = {0u, 0u, 0u};
    if (i < a.n) {
      label = a.labels_dev[i];
      const float x = a.xyz_dev[3 * i], y = a.xyz_dev[3 * i + 1], z = a.xyz_dev[3 * i + 2];
      const bool in_label = (unsigned)label < (unsigned)a.n_classes, finite = finite3(x, y, z);
      if (!in_label) err |= A3D_MEASURE_BAD_LABEL;
      if (!finite) err |= A3D_MEASURE_RANGE;
      if (in_label && finite) {
        const float* ax = a.axes_dev + 9 * label;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float p = project(ax + 3 * j, x, y, z);
          if (p != p) {
            err |= A3D_MEASURE_RANGE;
          } else {
            kmin[j] = kmax[j] = key_of(p);
            counts = true;
          }
        }
      }
    }
    const u64 live = __ballot(counts);
    if (!live) continue;
    const int one = wave_label(counts, label, live);
    if (one >= 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const unsigned l = wave_min(kmin[j]), h = wave_max(kmax[j]);
        if ((tid & 63) == 0) atomicMin(&lo[j][one], l), atomicMax(&hi[j][one], h);
      }
    } else if (counts) {
#pragma unroll
      for (int j = 0; j < 3; ++j) atomicMin(&lo[j][label], kmin[j]), atomicMax(&hi[j][label], kmax[j]);
    }
  }
  __syncthreads();
  if (tid < a.n_classes) {
    unsigned* out = (unsigned*)a.out_dev + 6 * tid;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (lo[j][tid] <= hi[j][tid]) atomicMin(out + 2 * j, lo[j][tid]), atomicMax(out + 2 * j + 1, hi[j][tid]);
    }
  }
  send_error(a.err_dev, err);
}

}  // namespace a3d

using namespace a3d;

extern "C" int a3d_measure_objects(const a3d_measure_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_measure_objects: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_measure_args& a = *args;
  const bool counts_ok = a.n_classes >= 1 && a.n_classes <= kMeasIds && a.bits >= 0 && a.bits <= A3D_MEASURE_MAX_BITS &&
                         a.n >= 0 && a.n < (1ll << 31) && a.n_qv >= 0 && a.n_qv < (1ll << 31) && a.m >= 0 &&
                         a.m <= A3D_MEASURE_MAX_FACES;
  // n 2^(2 bits) <= 2^62, in integers: n < 2^31 and 2 bits <= 40, so the product is below 2^71 -- compare the shifted bound
  const bool sums_ok = counts_ok && a.n <= ((1ll << 62) >> (2 * a.bits));
  if (!sums_ok || !a.out_dev || !a.err_dev || ((uintptr_t)a.out_dev & 7) || ((uintptr_t)a.err_dev & 3) ||
      (a.n > 0 && (!a.xyz_dev || !a.labels_dev)) || (a.n_qv > 0 && !a.labels_qv_dev) || (a.m > 0 && !a.faces_dev) ||
      !std::isfinite(a.origin[0]) || !std::isfinite(a.origin[1]) || !std::isfinite(a.origin[2]) || !power_of_two(a.quantum) ||
      (a.m > 0 && !power_of_two(a.area_quantum))) {
    set_error("a3d_measure_objects: bad arguments (n=%lld n_qv=%lld m=%lld classes=%d bits=%d quantum=%g area_quantum=%g)",
              (long long)a.n, (long long)a.n_qv, (long long)a.m, a.n_classes, a.bits, a.quantum, a.area_quantum);
    return A3D_ERR_INVALID;
  }
  k_measure_init<<<1, kMeasIds, 0, st>>>(a.out_dev, a.err_dev, a.n_classes);
  A3D_LAUNCH_CHECK();
  if (a.n > 0) {
    const unsigned grid = (unsigned)((a.n + kMeasChunk - 1) / kMeasChunk);
    k_measure_vertices<<<grid, kMeasBlock, 0, st>>>(a, std::ldexp(1.0, a.bits));
    A3D_LAUNCH_CHECK();
  }
  if (a.n_qv > 0) {
    k_measure_voxels<<<capped_grid(a.n_qv, kMeasBlock, kMeasMaxBlocks), kMeasBlock, 0, st>>>(a);
    A3D_LAUNCH_CHECK();
  }
  if (a.m > 0) {
    k_measure_faces<<<capped_grid(a.m, kMeasBlock, kMeasMaxBlocks), kMeasBlock, 0, st>>>(a);
    A3D_LAUNCH_CHECK();
  }
  k_measure_finish<<<1, kMeasIds, 0, st>>>(a.out_dev, a.n_classes);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_object_extents(const a3d_extents_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_object_extents: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_extents_args& a = *args;
  if (a.n_classes < 1 || a.n_classes > kMeasIds || a.n < 0 || a.n >= (1ll << 31) || !a.out_dev || !a.err_dev || !a.axes_dev ||
      ((uintptr_t)a.out_dev & 3) || ((uintptr_t)a.err_dev & 3) || (a.n > 0 && (!a.xyz_dev || !a.labels_dev))) {
    set_error("a3d_object_extents: bad arguments (n=%lld classes=%d)", (long long)a.n, a.n_classes);
    return A3D_ERR_INVALID;
  }
  k_extents_init<<<1, kMeasIds, 0, st>>>((unsigned*)a.out_dev, a.err_dev, a.n_classes);
  A3D_LAUNCH_CHECK();
  if (a.n > 0) {
    const unsigned grid = (unsigned)((a.n + kMeasChunk - 1) / kMeasChunk);
    k_extents_vertices<<<grid, kMeasBlock, 0, st>>>(a);
    A3D_LAUNCH_CHECK();
  }
  k_extents_finish<<<1, kMeasIds, 0, st>>>(a.out_dev, a.n_classes);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
