// The small helpers every session_*.hip shares, one definition each: wave and workgroup reductions, the 64-bit counter add,
// the fixed-point rule of a3d_measure_objects and a3d_estimate_normals, the finite test, and on the host the grid size, the
// workspace carver, the offsets of a connectivity and the check of a scene's level 0.  A new session file includes this
// header; it does not copy from it.
#pragma once
#include "common.h"

#include <cmath>
#include <cstdlib>

namespace a3d {

typedef unsigned long long u64;

// ---- device ---------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// The sum of v over the workgroup (BLOCK threads), in thread 0 (the other threads' return value is not meant to be used).
// The first loop is wave_sum<int>, written out: through the call hipcc schedules k_cull_points differently.
template <int BLOCK>
__device__ __forceinline__ long long block_sum(int v, int* wave_part) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();                             // (wave_part may still be read from the reduction before)
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < BLOCK / 64; ++w) s += wave_part[w];
  return s;
}
// The maximum of v >= 0 over the workgroup, in thread 0.
template <int BLOCK>
__device__ __forceinline__ int block_max(int v, int* wave_part) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
  __syncthreads();                             // (as in block_sum)
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  int m = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < BLOCK / 64; ++w) m = max(m, wave_part[w]);
  return m;
}
// The error word of a wave: the OR of its lanes, sent by lane 0 with one atomic (none for a zero).
__device__ __forceinline__ void send_error(int32_t* err_dev, int err) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) err |= __shfl_xor(err, o);
  if ((threadIdx.x & 63) == 0 && err) atomicOr(err_dev, err);
}
__device__ __forceinline__ void add_i64(int64_t* dst, long long s) {
  if (s) atomicAdd((u64*)dst, (u64)s);
}
// X = llrint((x - origin) / quantum) when |X| <= lim (= 2^bits); a NaN or an infinity fails the comparison.  THE frame of
// a3d_measure_objects and a3d_estimate_normals: each operation rounded on its own.
__device__ __forceinline__ bool fixed_point(float x, double origin, double quantum, double lim, long long& X) {
#pragma clang fp contract(off)
  const double r = rint(((double)x - origin) / quantum);
  if (!(fabs(r) <= lim)) return false;
  X = (long long)r;
  return true;
}
// THE finite test: a NaN or an infinity has the exponent bits all ones.  One coordinate (is it odd?) and three (are all
// sound?); both spell the test out: with one written through the other hipcc compiles k_extents_vertices or
// k_select_vertices to other code than the one that was measured.
constexpr unsigned kExpBits = 0x7f800000u;
__device__ __forceinline__ bool not_finite(float x) { return (__float_as_uint(x) & kExpBits) == kExpBits; }
__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return (__float_as_uint(x) & kExpBits) != kExpBits && (__float_as_uint(y) & kExpBits) != kExpBits &&
         (__float_as_uint(z) & kExpBits) != kExpBits;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
inline bool power_of_two(double q) {
  int e;
  return std::isfinite(q) && q > 0.0 && std::frexp(q, &e) == 0.5;
}
// workgroups of `block` threads for n items walked grid-stride: ceil(n / block), at least 1, at most cap
inline unsigned capped_grid(long long n, int block, int cap) {
  const long long want = (n + block - 1) / block;
  return (unsigned)(want < 1 ? 1 : want < cap ? want : cap);
}
// Hands out consecutive 256-byte aligned pieces of a workspace; with base == nullptr it only measures (off = the bytes).
struct Carver {
  void* base;
  size_t off = 0;
  void* take(size_t b) {
    void* p = base ? (char*)base + off : nullptr;
    off += align256(b);
    return p;
  }
};
// the offsets a connectivity admits, bit k = offset (k % 3 - 1, (k / 3) % 3 - 1, k / 9 - 1)
inline unsigned offset_mask(int connectivity) {
  unsigned m = 0;
  for (int k = 0; k < 27; ++k) {
    const int l1 = std::abs(k % 3 - 1) + std::abs((k / 3) % 3 - 1) + std::abs(k / 9 - 1);
    if (l1 >= 1 && (connectivity == 26 || (connectivity == 18 && l1 <= 2) || (connectivity == 6 && l1 == 1))) m |= 1u << k;
  }
  return m;
}
// Level 0 of the scene can be walked (the 27-neighbour table, the callers' rows) and has n rows.
inline bool scene_walkable(const a3d_scene* s, long long n) {
  return s && s->lv[0].nbr27 && s->orig_row && s->n0 == s->lv[0].n && n == s->lv[0].n;
}

}  // namespace a3d
