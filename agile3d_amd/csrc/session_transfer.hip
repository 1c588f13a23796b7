// session_transfer.hip -- an index over an ARBITRARY point set and the bulk, exact nearest-point query against it (gfx950):
// what carries labels from the scan a session loaded to another point set, and from another point set into the session.
// Entry points: a3d_point_index_workspace_bytes, a3d_point_index_create, a3d_point_index_destroy, a3d_point_index_nearest.
//
// The reference has no counterpart (its tool labels the vertices it loaded and nothing else).  THE RULE is a3d_nearest_rows'
// with a cutoff, stated in full in include/agile3d_hip.h and restated in tests/transfer_rule.py; in one line:
//   nearest[q] = the FIRST arg-min over the source rows p with finite coordinates of d2 = (dx dx + dy dy) + dz dz (fp32, from
//   the differences, every operation rounded on its own) among the rows with d2 <= r2 = fl32(r * r); -1 when there is none.
//
// THE SHAPE.  Build: one cell key per row (c = floor(fl32(x / cell)) per axis, make_key of common.h; a sentinel above every
// key for a row that is left out), radix.hip's stable sort of (key, row) in its LAUNCH-CHAIN form, then one pass that writes
// the sorted points as float4 (x, y, z, row | last-of-its-cell << 31) -- a cell's points are contiguous and the list ends at
// the flag, so a candidate costs ONE 16-byte load -- and enters (key -> first position) into an open-addressing table
// wherever the sorted key changes (hash64 / hash_lookup of common.h, atomicCAS as scene.hip's).  No scan, no compaction.
// Query: one thread per query walks the 27 cells around the query's cell, a plane of 9 at a time: the 9 table probes are
// issued together, then the 9 first positions, then each list four candidates at a time -- no branch between the loads of a
// stage, as session_grow.hip's sweep and session_normals.hip's stage B learnt.  The minimum is kept as a packed (d2 bits, row)
// key: the result does not depend on the order of the cells, of the lists or of the table.
//
// make_key wraps a cell coordinate modulo 2^21, so the cells -2^20 and +2^20 of an axis share a key and hence a list.  Every
// candidate of a list is tested by the exact rule, so a shared list costs time, never a wrong answer.
//
// WHY 27 CELLS ENCLOSE (DESIGN.md 4.9 has the argument in full): with r <= cell / 2 and r2 a NORMAL fp32 number a match
// has |p - q| <= (cell / 2)(1 + 2^-21) on every axis, and fl32(x / cell) is off by at most 2^-4 + 2^-23 of a cell for a row
// that can be keyed (|c| <= 2^20): the two quotients differ by less than 0.63, their floors by at most 1.  When r2 is NOT a
// normal number (r below 2^-63 or from 2^64 on) that argument does not hold -- an r2 of 0 still accepts d2 == 0, which a
// difference of 2^-75 gives -- and the query walks EVERY sorted point instead: the contract holds, slowly, where no scan lives.
//
// THE SUMMARY is integer sums reduced per workgroup (session_device.h) and ONE atomic per workgroup and counter.  Stages are
// launches; no grid barrier, no spin-wait of this file's own.  The library allocates nothing on the device and does not
// synchronise.
#include "session_device.h"

#include <new>

namespace a3d {

constexpr int kTiFat = 1024;                  // the key pass: few, fat workgroups (one atomic per workgroup and counter) ...
constexpr int kTiFatBlocks = 256;             // ... at most one per CU
constexpr int kTiB = 256;                     // the list pass and the query
constexpr int kTiQueryBlocks = 2048;          // the query: 8 workgroups a CU, grid-stride beyond
constexpr uint64_t kTiLeftOut = 1ull << 63;   // above every make_key(0, ..) (63 bits); sorts behind every cell
constexpr float kTiMaxCell = 1048576.f;       // 2^20
static_assert(sizeof(a3d_transfer_summary) == 40, "lib.py: TransferSummary");

struct TiHead {                               // what the build leaves for every query's summary
  int64_t left_out;                           // source rows with a coordinate that is not finite
  int32_t err;                                // A3D_TRANSFER_UNKEYABLE
  int32_t sort_fail;                          // radix.hip's give-up word (0 or A3D_ERR_HIP)
};

struct TiWs {
  TiHead* head;
  uint64_t *keys_in, *keys;
  int *vals_in, *vals;
  float4* pts;
  uint64_t* hk;
  int* hv;
  void* sort_temp;
  size_t hsize, sort_bytes, bytes;
};
static TiWs carve_index(void* base, long long n) {
  TiWs w;
  Carver c{base};
  const size_t m = (size_t)(n > 0 ? n : 1);
  w.head = (TiHead*)c.take(sizeof(TiHead));
  w.keys_in = (uint64_t*)c.take(m * 8), w.keys = (uint64_t*)c.take(m * 8);
  w.vals_in = (int*)c.take(m * 4), w.vals = (int*)c.take(m * 4);
  w.pts = (float4*)c.take(m * 16);
  w.hsize = 64;
  while (w.hsize < 2 * m) w.hsize <<= 1;      // a power of two >= 2 n (at most 2^32: the mask fits 32 bits)
  w.hk = (uint64_t*)c.take(w.hsize * 8), w.hv = (int*)c.take(w.hsize * 4);
  w.sort_bytes = radix_sort_temp_bytes((int)m);
  w.sort_temp = c.take(w.sort_bytes);
  w.bytes = c.off;
  return w;
}

}  // namespace a3d

struct a3d_point_index {
  long long n;
  float cell;
  const float4* pts;
  const uint64_t* hk;
  const int* hv;
  uint32_t hmask;
  const a3d::TiHead* head;
};

namespace a3d {

// THE cell of a coordinate: floor of the correctly rounded fp32 quotient (build and query share this line)
__device__ __forceinline__ float cell_of(float x, float cell) { return floorf(__fdiv_rn(x, cell)); }

// ---- build ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTiFat) void k_ti_keys(const float* __restrict__ xyz, const long long n, const float cell,
                                                    uint64_t* __restrict__ keys, int* __restrict__ vals, TiHead* head) {
  __shared__ int wave_part[kTiFat / 64];
  const long long stride = (long long)gridDim.x * kTiFat;
  int left = 0, err = 0;                       // (n < 2^31: a thread's share fits an int)
  for (long long i = (long long)blockIdx.x * kTiFat + threadIdx.x; i < n; i += stride) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    uint64_t key = kTiLeftOut;
    if (!finite3(x, y, z)) {
      ++left;
    } else {
      const float cx = cell_of(x, cell), cy = cell_of(y, cell), cz = cell_of(z, cell);
      if (fabsf(cx) <= kTiMaxCell && fabsf(cy) <= kTiMaxCell && fabsf(cz) <= kTiMaxCell)
        key = make_key(0, (int)cx, (int)cy, (int)cz, 0);
      else
        err = A3D_TRANSFER_UNKEYABLE;          // cannot be keyed: flagged, never indexed wrongly
    }
    keys[i] = key, vals[i] = (int)i;
  }
  const long long s_left = block_sum<kTiFat>(left, wave_part), s_err = block_sum<kTiFat>(err, wave_part);
  if (threadIdx.x == 0) {
    add_i64(&head->left_out, s_left);
    if (s_err) atomicOr(&head->err, A3D_TRANSFER_UNKEYABLE);
  }
}

// The sorted points with their rows, and the table: position i is the head of its cell's list where the key changes.
__global__ __launch_bounds__(kTiB) void k_ti_lists(const float* __restrict__ xyz, const int n, const uint64_t* __restrict__ keys,
                                                   const int* __restrict__ vals, float4* __restrict__ pts, uint64_t* hk,
                                                   int* __restrict__ hv, const uint32_t hmask) {
  const int i = blockIdx.x * kTiB + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  const int row = vals[i];
  if (key == kTiLeftOut) {                     // three NaNs fail every d2 <= r2; its own list of one, which no table entry names
    const float nan = __uint_as_float(0x7fc00000u);
    pts[i] = make_float4(nan, nan, nan, __uint_as_float((unsigned)row | 0x80000000u));
    return;
  }
  const bool head = i == 0 || keys[i - 1] != key, last = i + 1 == n || keys[i + 1] != key;
  pts[i] = make_float4(xyz[3 * (size_t)row], xyz[3 * (size_t)row + 1], xyz[3 * (size_t)row + 2],
                       __uint_as_float((unsigned)row | (last ? 0x80000000u : 0u)));
  if (!head) return;
  uint32_t h = hash64(key) & hmask;
  for (uint32_t probe = 0; probe <= hmask; ++probe) {     // (as scene.hip's table; at most n keys in >= 2 n slots)
    const unsigned long long prev = atomicCAS((unsigned long long*)&hk[h], (unsigned long long)kEmptyKey, (unsigned long long)key);
    if (prev == kEmptyKey) {
      hv[h] = i;
      return;
    }
    h = (h + 1) & hmask;
  }
}

// ---- query ----------------------------------------------------------------------------------------------------------------
struct TiQuery {
  a3d_point_index ix;
  const float* q;
  long long m;
  float r2;
  const int32_t* labels_src;
  int32_t fill;
  int32_t* nearest;
  float* d2;
  int32_t* labels;
  a3d_transfer_summary* summary;
};

// one candidate against the best so far: THE rule's arithmetic (contraction off), the packed (d2 bits, row) minimum
__device__ __forceinline__ void ti_candidate(const float4 p, const float qx, const float qy, const float qz, const float r2, u64& best) {
#pragma clang fp contract(off)
  const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  const u64 k = (u64)__float_as_uint(d2) << 32 | (__float_as_uint(p.w) & 0x7fffffffu);
  if (d2 <= r2 && k < best) best = k;          // (d2 >= +0 and never NaN for finite p and q: its bits order as it does)
}

template <bool ALL>
__global__ __launch_bounds__(kTiB) void k_ti_query(const TiQuery t) {
  __shared__ int wave_part[kTiB / 64];
  const a3d_point_index& ix = t.ix;
  const long long stride = (long long)gridDim.x * kTiB;
  const int last_pos = (int)ix.n - 1;
  int n_match = 0, n_miss = 0, n_odd = 0;
  for (long long i = (long long)blockIdx.x * kTiB + threadIdx.x; i < t.m; i += stride) {
    const float qx = t.q[3 * i], qy = t.q[3 * i + 1], qz = t.q[3 * i + 2];
    u64 best = ~0ull;
    const bool sound = finite3(qx, qy, qz);
    if (sound && ALL) {
      for (int pos = 0; pos <= last_pos; ++pos) ti_candidate(ix.pts[pos], qx, qy, qz, t.r2, best);
    } else if (sound) {
      const float ux = cell_of(qx, ix.cell), uy = cell_of(qy, ix.cell), uz = cell_of(qz, ix.cell);
      // a match lies at most one cell from the query's, and no row beyond +-2^20 is in the table
      if (fabsf(ux) <= kTiMaxCell + 1.f && fabsf(uy) <= kTiMaxCell + 1.f && fabsf(uz) <= kTiMaxCell + 1.f) {
        const int cx = (int)ux, cy = (int)uy, cz = (int)uz;
#pragma unroll 1
        for (int dz = -1; dz <= 1; ++dz) {
          uint64_t key[9], got[9];
          uint32_t slot[9];
          int start[9];
          unsigned inside = 0;                 // bit k: the cell lies in the key range
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            const int x = cx + k % 3 - 1, y = cy + k / 3 - 1, z = cz + dz;
            const bool in = abs(x) <= (1 << 20) && abs(y) <= (1 << 20) && abs(z) <= (1 << 20);
            inside |= (unsigned)in << k;
            key[k] = make_key(0, x, y, z, 0);
            slot[k] = hash64(key[k]) & ix.hmask;
          }
#pragma unroll
          for (int k = 0; k < 9; ++k) got[k] = ix.hk[slot[k]];
#pragma unroll
          for (int k = 0; k < 9; ++k) start[k] = ix.hv[slot[k]];       // (an empty slot's word is not looked at)
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            if (!((inside >> k) & 1) || got[k] == kEmptyKey) start[k] = -1;
            else if (got[k] != key[k]) start[k] = hash_lookup(ix.hk, ix.hv, ix.hmask, key[k]);   // the slot is another key's: probe on
          }
#pragma unroll 1
          for (int k = 0; k < 9; ++k) {
            int pos = start[k];
            bool more = pos >= 0;
            while (more) {
              float4 p[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) p[j] = ix.pts[min(pos + j, last_pos)];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                if (more) ti_candidate(p[j], qx, qy, qz, t.r2, best);
                more = more && !(__float_as_uint(p[j].w) >> 31);
              }
              pos += 4;
            }
          }
        }
      }
    }
    const bool hit = best != ~0ull;
    const int row = hit ? (int)(best & 0xffffffffu) : -1;
    t.nearest[i] = row;
    if (t.d2) t.d2[i] = hit ? __uint_as_float((unsigned)(best >> 32)) : __uint_as_float(0x7f800000u);
    if (t.labels) t.labels[i] = hit ? t.labels_src[row] : t.fill;
    n_match += hit, n_miss += sound && !hit, n_odd += !sound;
  }
  const long long s_match = block_sum<kTiB>(n_match, wave_part), s_miss = block_sum<kTiB>(n_miss, wave_part),
                  s_odd = block_sum<kTiB>(n_odd, wave_part);
  if (threadIdx.x == 0) {
    add_i64(&t.summary->matched, s_match), add_i64(&t.summary->unmatched, s_miss), add_i64(&t.summary->nonfinite, s_odd);
    if (blockIdx.x == 0) {                     // what the build found, once
      add_i64(&t.summary->source_left_out, ix.head->left_out);
      const int e = ix.head->err | (ix.head->sort_fail ? A3D_TRANSFER_SORT_FAILED : 0);
      if (e) atomicOr(&t.summary->err, e);
    }
  }
}

}  // namespace a3d

using namespace a3d;

extern "C" size_t a3d_point_index_workspace_bytes(int64_t n) {
  if (n < 0 || n >= (1ll << 31)) return 0;
  return carve_index(nullptr, n).bytes;
}

extern "C" int a3d_point_index_create(const float* xyz_dev, int64_t n, float cell_size, void* workspace_dev, size_t workspace_bytes,
                                      void* stream, a3d_point_index** out) {
  hipStream_t st = (hipStream_t)stream;
  if (out) *out = nullptr;
  if (!out || n < 0 || n >= (1ll << 31) || (n > 0 && !xyz_dev) || !(cell_size > 0.f) || !std::isfinite(cell_size) || !workspace_dev ||
      ((uintptr_t)workspace_dev & 255)) {
    set_error("a3d_point_index_create: bad arguments (n=%lld cell_size=%g xyz %s workspace %s out %s; 0 <= n < 2^31, a finite "
              "cell_size > 0 and a 256-byte aligned workspace are needed)", (long long)n, (double)cell_size,
              xyz_dev ? "given" : "NULL", workspace_dev ? "given" : "NULL", out ? "given" : "NULL");
    return A3D_ERR_INVALID;
  }
  if (workspace_bytes < a3d_point_index_workspace_bytes(n)) {
    set_error("a3d_point_index_create: workspace too small (%zu < %zu)", workspace_bytes, a3d_point_index_workspace_bytes(n));
    return A3D_ERR_WORKSPACE;
  }
  const TiWs w = carve_index(workspace_dev, n);
  A3D_HIP_CHECK(hipMemsetAsync(w.head, 0, sizeof(TiHead), st));
  A3D_HIP_CHECK(hipMemsetAsync(w.hk, 0xff, w.hsize * 8, st));          // kEmptyKey everywhere
  if (n > 0) {
    k_ti_keys<<<capped_grid(n, kTiFat, kTiFatBlocks), kTiFat, 0, st>>>(xyz_dev, n, cell_size, w.keys_in, w.vals_in, w.head);
    A3D_LAUNCH_CHECK();
    RadixPass ps[kRadixMaxPasses];
    const int np = radix_passes(0, 64, ps);    // digits the set's extent does not touch are skipped on the device
    const int rc = radix_sort_pairs(w.sort_temp, w.sort_bytes, w.keys_in, w.keys, w.vals_in, w.vals, (int)n, ps, np, st,
                                    &w.head->sort_fail, false);        // the launch chain: no grid barrier next to other work
    if (rc) return rc;
    k_ti_lists<<<(unsigned)((n + kTiB - 1) / kTiB), kTiB, 0, st>>>(xyz_dev, (int)n, w.keys, w.vals, w.pts, w.hk, w.hv,
                                                                  (uint32_t)(w.hsize - 1));
    A3D_LAUNCH_CHECK();
  }
  a3d_point_index* ix = new (std::nothrow) a3d_point_index;
  if (!ix) {
    set_error("a3d_point_index_create: out of host memory");
    return A3D_ERR_INVALID;
  }
  ix->n = n, ix->cell = cell_size, ix->pts = w.pts, ix->hk = w.hk, ix->hv = w.hv, ix->hmask = (uint32_t)(w.hsize - 1), ix->head = w.head;
  *out = ix;
  return A3D_OK;
}

extern "C" void a3d_point_index_destroy(a3d_point_index* index) { delete index; }

extern "C" int a3d_point_index_nearest(const a3d_point_index* index, const float* queries_dev, int64_t m, float max_distance,
                                       const int32_t* labels_src_dev, int32_t fill, int32_t* nearest_out_dev, float* d2_out_dev,
                                       int32_t* labels_out_dev, a3d_transfer_summary* summary_dev, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!index || m < 0 || m >= (1ll << 31) || (m > 0 && (!queries_dev || !nearest_out_dev)) || !summary_dev ||
      ((uintptr_t)summary_dev & 7) || (labels_out_dev != nullptr) != (labels_src_dev != nullptr)) {
    set_error("a3d_point_index_nearest: bad arguments (index %s, m=%lld queries %s nearest_out %s summary %s labels_src %s "
              "labels_out %s; 0 <= m < 2^31, labels_out is given exactly when labels_src is)", index ? "given" : "NULL",
              (long long)m, queries_dev ? "given" : "NULL", nearest_out_dev ? "given" : "NULL", summary_dev ? "given" : "NULL",
              labels_src_dev ? "given" : "NULL", labels_out_dev ? "given" : "NULL");
    return A3D_ERR_INVALID;
  }
  if (!(max_distance > 0.f && max_distance <= 0.5f * index->cell)) {   // (a NaN fails the first)
    set_error("a3d_point_index_nearest: max_distance=%g must lie in (0, cell_size / 2 = %g]", (double)max_distance,
              0.5 * (double)index->cell);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(summary_dev, 0, sizeof(a3d_transfer_summary), st));
  TiQuery t;
  t.ix = *index, t.q = queries_dev, t.m = m, t.labels_src = labels_src_dev, t.fill = fill, t.nearest = nearest_out_dev,
  t.d2 = d2_out_dev, t.labels = labels_out_dev, t.summary = summary_dev;
  t.r2 = max_distance * max_distance;          // rounded once
  const bool normal = t.r2 >= 1.17549435e-38f && std::isfinite(t.r2);   // else the 27 cells do not enclose: every point is walked
  const unsigned grid = capped_grid(m, kTiB, kTiQueryBlocks);
  if (normal)
    k_ti_query<false><<<grid, kTiB, 0, st>>>(t);
  else
    k_ti_query<true><<<grid, kTiB, 0, st>>>(t);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
