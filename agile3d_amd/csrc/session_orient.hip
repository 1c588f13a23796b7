// session_orient.hip -- one sign for a whole surface: the normals of a3d_estimate_normals oriented consistently by
// propagation from seed voxels over the voxel lattice (gfx950).  Entry points: a3d_orient_normals, and a3d_orient_edge, the
// edge function on the host by the function the kernel calls, for the tests without a GPU.
//
// The reference has no counterpart.  THE RULE (ours, stated in full in include/agile3d_hip.h at the entry point): the nodes
// are the ADMITTED level-0 voxels (a finite normal that is not all zero) in the CALLER's row order; an edge joins two
// admitted neighbours under the connectivity and carries w = 1 + floor(1023 max(1 - |dot|, 0)) in 1 .. 1024 and flip = dot < 0,
// dot in fp32 with every operation rounded on its own; (dist, owner) of a voxel is the lexicographic minimum of (path cost,
// seed row) over the seeds; its parent is the neighbour at the LOWEST slot that explains its dist; its parity is the XOR of
// the flips along the parent chain and of the seed's own flip; the output normal has its sign bits flipped where parity is 1.
//
// THE ADJACENCY is session_grow.hip's: A3D_TAB_NBR27 (int32 [27][npad], internal rows, a missing neighbour is n), both ends
// through A3D_TAB_ORIGROW.  Threads walk the INTERNAL (Morton) order.
// THE EDGE TABLE.  Of the two forms -- every relaxation gathers the neighbours' normals, or one kernel tabulates the 27
// (w, flip) words of every voxel first -- this file TABULATES: k_orient_edges writes edge[k][r] (uint16 [27][n], internal
// row r, slot k): bits 0..10 = w, bit 14 = dot > 0, bit 15 = dot < 0, the whole word 0 where there is no edge (a missing or
// unadmitted end, an offset the connectivity leaves out, slot 13).  A sweep's front then reads 2 bytes a slot instead of 12
// and tests nothing else; the parent and the conflict count read the same words, so the fp32 function runs once per pair
// and end.  It is symmetric bit for bit (products and the two sums commute), so both ends hold the same word.
// PHASE 1 is session_grow.hip's relaxation and its argument for an order-free fixed point, word for word: ONE word
// dist << 32 | owner (none: all ones), 64-bit atomicMin, relaxed agent-scope loads while workgroups write, only the FRONT
// offers (stamp[r] = the sweep that last lowered the voxel), a sweep that lowers anything raises flag[k], and sweep k + 1
// returns at once when flag[k] is clear.  There is no limit on dist here: n <= 2^21 rows and w <= 2^10 keep every path
// cost below 2^31.  The call launches the `sweeps` it is given and k_orient_close records whether the last was quiet.
// RESUME.  The stamps count sweeps from 1 in every call.  k_orient_close leaves (flag[sweeps], sweeps) in the workspace; a
// resumed call first turns the stamps of the last sweep into 0 (the front of its sweep 1) and all others into -1
// (k_orient_restamp: a voxel lowered before the last sweep has spoken since), and starts from the flag that was left.  The
// flag array is never indexed by anything read from the workspace.
// WHY THE PARITY IS NOT IN THE WORD: XOR along a path is not monotone; a transient word of parity 0 that arrived by a path
// which later loses could never be raised again, and the result would depend on the order of arrival.  So PHASE 2 derives
// the parent from the fixed point alone (lowest slot k with owner[u] == owner[v] and dist[u] + w == dist[v]; dist strictly
// decreases along parents, so there is no cycle whatever the state), and PHASE 3 composes (ancestor, parity) by pointer
// jumping: a root holds (itself, 0), every round is a launch that reads one buffer and writes the other (anc << 1 | parity
// in an int32, -1: not reached), ceil(log2 n) rounds; the seed's own flip is XORed in at the end.
// THE NEAREST SEEDS: atomicMin on the bit pattern of d2 (a double >= +0) per component, then atomicMin on the row among
// the rows that hold that d2: minima do not depend on the order of arrival.
// THE FINISH is grow's lift: one streaming pass over the voxels and the vertices by few, fat workgroups, integer counts
// through registers, shuffles and LDS, ONE atomic per workgroup and counter.  The conflicts are counted by a pass of their
// own (it needs every voxel's parity), each edge at its end with the slot above 13.
// No grid barrier, no cooperative launch, no spin-wait: no thread waits for another.  Every stage issues its 26 loads
// together (session_grow.hip measured why).
#include "session_device.h"

namespace a3d {

constexpr int kOrientBlock = 256;
constexpr int kOrientMaxBlocks = 2048;
constexpr int kOrientFat = 1024;
constexpr int kOrientFatBlocks = 256;
constexpr u64 kOrientNone = ~0ull;
constexpr unsigned kEdgeCost = 0x7ffu, kEdgePos = 0x4000u, kEdgeNeg = 0x8000u;
static_assert(sizeof(a3d_orient_normals_args) == 176 && sizeof(a3d_orient_summary) == 64, "lib.py: OrientNormalsArgs, OrientSummary");

// THE edge function of the header: every operation rounded on its own, in the order written.
__host__ __device__ inline void orient_edge(const float a0, const float a1, const float a2, const float b0, const float b1,
                                            const float b2, int& w, float& dot_out) {
#pragma clang fp contract(off)
  const float dot = (a0 * b0 + a1 * b1) + a2 * b2;
  w = 1 + (int)floorf(1023.0f * fmaxf(1.0f - fabsf(dot), 0.0f));
  dot_out = dot;
}

struct OrientWs {
  u64* value;          // [n] dist << 32 | owner at the caller row, kOrientNone: not reached
  int32_t* stamp;      // [n] at the INTERNAL row: the sweep of this call that last lowered the voxel, -1: none
  int32_t* flag;       // [A3D_ORIENT_MAX_SWEEPS + 1] flag[0]: there is a front; flag[k]: sweep k lowered something
  int32_t* meta;       // [2] what k_orient_close left: the last flag, the number of sweeps
  uint8_t* sflip;      // [n] 1 at a seed whose normal is negated first
  uint8_t* parity;     // [n] the result, for the conflict count
  u64* best;           // [n] NEAREST: the least d2 bits per component ...
  int32_t* jump;       // ... [2][n] the pointer-jumping buffers, which live in the same bytes (the seeds are found before)
  int32_t* seedrow;    // [n] NEAREST: the least row among those with the least d2, per component
  uint16_t* edge;      // [27][n]
  size_t bytes;
};
static OrientWs carve_orient(void* base, long long n) {
  OrientWs w;
  Carver c{base};
  const size_t m = (size_t)(n > 0 ? n : 1);
  w.value = (u64*)c.take(m * 8);
  w.stamp = (int32_t*)c.take(m * 4);
  w.flag = (int32_t*)c.take((A3D_ORIENT_MAX_SWEEPS + 1) * sizeof(int32_t));
  w.meta = (int32_t*)c.take(2 * sizeof(int32_t));
  w.sflip = (uint8_t*)c.take(m);
  w.parity = (uint8_t*)c.take(m);
  w.best = (u64*)c.take(m * 8);
  w.jump = (int32_t*)w.best;
  w.seedrow = (int32_t*)c.take(m * 4);
  w.edge = (uint16_t*)c.take(27 * m * 2);
  w.bytes = c.off;
  return w;
}

struct OrientTab {
  const int32_t* nbr;          // [27][npad]
  const int32_t* orig;         // [n]
  int n, npad;
  unsigned mask;
};

__device__ __forceinline__ bool admitted(const float x, const float y, const float z) {
  return finite3(x, y, z) && !(x == 0.0f && y == 0.0f && z == 0.0f);
}
__device__ __forceinline__ u64 word_now(const u64* value, int x) {
  return __hip_atomic_load(value + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The 27 words of every voxel.  Stages: the table's rows, the callers' rows, the normals, the function, the stores.
__global__ __launch_bounds__(kOrientBlock) void k_orient_edges(const float* __restrict__ normal, const OrientTab t,
                                                               uint16_t* __restrict__ edge) {
  const int stride = gridDim.x * kOrientBlock;
  for (int r = blockIdx.x * kOrientBlock + threadIdx.x; r < t.n; r += stride) {
    const int i = t.orig[r];
    const float a0 = normal[3 * (size_t)i], a1 = normal[3 * (size_t)i + 1], a2 = normal[3 * (size_t)i + 2];
    const bool mine = admitted(a0, a1, a2);
    int jr[27], j[27];
    float b[27][3];
#pragma unroll
    for (int k = 0; k < 27; ++k) jr[k] = k == 13 ? t.n : t.nbr[(size_t)k * t.npad + r];
#pragma unroll
    for (int k = 0; k < 27; ++k) j[k] = t.orig[(unsigned)jr[k] < (unsigned)t.n ? jr[k] : r];   // a missing neighbour: this row, masked below
#pragma unroll
    for (int k = 0; k < 27; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) b[k][c] = normal[3 * (size_t)j[k] + c];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      int w;
      float dot;
      orient_edge(a0, a1, a2, b[k][0], b[k][1], b[k][2], w, dot);
      const bool there = mine && ((t.mask >> k) & 1u) && (unsigned)jr[k] < (unsigned)t.n && admitted(b[k][0], b[k][1], b[k][2]);
      const unsigned word = (unsigned)w | (dot > 0.0f ? kEdgePos : 0u) | (dot < 0.0f ? kEdgeNeg : 0u);
      edge[(size_t)k * t.n + r] = (uint16_t)(there ? word : 0u);
    }
  }
}

// NEAREST: the bits of d2 of a candidate row, by the header's sequence of doubles.
__device__ __forceinline__ bool near_candidate(const a3d_orient_normals_args& a, const int i, const int n, int& comp, u64& bits,
                                               int& err) {
#pragma clang fp contract(off)
  comp = a.component_qv_dev[i];
  if (comp >= n) err |= A3D_ORIENT_BAD_COMPONENT;
  const float* nv = a.normal_qv_dev + 3 * (size_t)i;
  const float* p = a.position_qv_dev + 3 * (size_t)i;
  const float p0 = p[0], p1 = p[1], p2 = p[2];
  if ((unsigned)comp >= (unsigned)n || !admitted(nv[0], nv[1], nv[2]) || !finite3(p0, p1, p2)) return false;
  const double dx = (double)p0 - a.viewpoint[0], dy = (double)p1 - a.viewpoint[1], dz = (double)p2 - a.viewpoint[2];
  const double d2 = (dx * dx + dy * dy) + dz * dz;
  bits = (u64)__double_as_longlong(d2);
  return true;
}
__global__ __launch_bounds__(kOrientBlock) void k_orient_near_d2(const a3d_orient_normals_args a, u64* best, const int n) {
  const int stride = gridDim.x * kOrientBlock;
  int err = 0;
  for (int i = blockIdx.x * kOrientBlock + threadIdx.x; i < n; i += stride) {
    int comp;
    u64 bits;
    if (near_candidate(a, i, n, comp, bits, err)) atomicMin(best + comp, bits);
  }
  send_error(&a.summary_dev->err, err);
}
__global__ __launch_bounds__(kOrientBlock) void k_orient_near_row(const a3d_orient_normals_args a, const u64* __restrict__ best,
                                                                  int32_t* seedrow, const int n) {
  const int stride = gridDim.x * kOrientBlock;
  int err = 0;
  for (int i = blockIdx.x * kOrientBlock + threadIdx.x; i < n; i += stride) {
    int comp;
    u64 bits;
    if (near_candidate(a, i, n, comp, bits, err) && bits == best[comp]) atomicMin(seedrow + comp, i);
  }
}

__global__ __launch_bounds__(kOrientBlock) void k_orient_init(const a3d_orient_normals_args a, const OrientTab t, const OrientWs w) {
#pragma clang fp contract(off)
  const int stride = gridDim.x * kOrientBlock;
  bool any = false;
  for (int r = blockIdx.x * kOrientBlock + threadIdx.x; r < t.n; r += stride) {
    const int i = t.orig[r];
    const float* nv = a.normal_qv_dev + 3 * (size_t)i;
    const float n0 = nv[0], n1 = nv[1], n2 = nv[2];
    bool seed = false, flip = false;
    if (admitted(n0, n1, n2)) {
      if (a.mode == A3D_ORIENT_GIVEN) {
        seed = a.seed_qv_dev[i] != 0;
        flip = a.seed_flip_dev && a.seed_flip_dev[i] != 0;
      } else {
        const int comp = a.component_qv_dev[i];
        seed = (unsigned)comp < (unsigned)t.n && w.seedrow[comp] == i;
        if (seed) {
          const float* p = a.position_qv_dev + 3 * (size_t)i;
          const double g = ((double)n0 * (a.viewpoint[0] - (double)p[0]) + (double)n1 * (a.viewpoint[1] - (double)p[1])) +
                           (double)n2 * (a.viewpoint[2] - (double)p[2]);
          flip = g < 0.0;
        }
      }
    }
    w.value[i] = seed ? (u64)i : kOrientNone;                          // (0, i): a seed owns itself
    w.stamp[r] = seed ? 0 : -1;
    w.sflip[i] = seed && flip ? 1 : 0;
    any = any || seed;
  }
  if (any) w.flag[0] = 1;                                              // (every writer stores 1)
}

// A resumed call: the voxels the last sweep of the call before lowered are the front of this call's sweep 1.
__global__ __launch_bounds__(kOrientBlock) void k_orient_restamp(const OrientWs w, const int n) {
  const int last = w.meta[1];
  const int stride = gridDim.x * kOrientBlock;
  for (int r = blockIdx.x * kOrientBlock + threadIdx.x; r < n; r += stride) w.stamp[r] = w.stamp[r] == last ? 0 : -1;
  if (blockIdx.x == 0 && threadIdx.x == 0) w.flag[0] = w.meta[0] != 0;
}

// ONE SWEEP, session_grow.hip's: only the front offers word + w to the neighbours its edge words name.
__global__ __launch_bounds__(kOrientBlock) void k_orient_sweep(const OrientTab t, const uint16_t* __restrict__ edge, u64* value,
                                                               int32_t* stamp, const int32_t* __restrict__ before, int32_t* mine,
                                                               const int sweep) {
  if (*before == 0) return;                                            // the sweep before lowered nothing: the fixed point
  const int stride = gridDim.x * kOrientBlock;
  bool lowered = false;
  for (int r = blockIdx.x * kOrientBlock + threadIdx.x; r < t.n; r += stride) {
    if (__hip_atomic_load(stamp + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < sweep - 1) continue;
    const int i = t.orig[r];
    const u64 cur = word_now(value, i);
    if (cur == kOrientNone) continue;                                  // (a stamped voxel holds a word)
    int jr[27], j[27];
    unsigned e[27];
    u64 cand[27], old[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      if (k == 13) continue;
      jr[k] = t.nbr[(size_t)k * t.npad + r];
      e[k] = edge[(size_t)k * t.n + r];
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      if (k == 13) continue;
      j[k] = t.orig[(unsigned)jr[k] < (unsigned)t.n ? jr[k] : r];     // a missing neighbour: this row itself, masked below
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      if (k == 13) continue;
      const u64 now = word_now(value, j[k]);
      const u64 c = cur + ((u64)(e[k] & kEdgeCost) << 32);
      const bool offer = e[k] != 0 && (unsigned)jr[k] < (unsigned)t.n && c < now;
      cand[k] = offer ? c : kOrientNone;
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      if (k == 13) continue;
      old[k] = 0;                                                      // (nothing is below 0: no offer, nothing lowered)
      if (cand[k] != kOrientNone) old[k] = atomicMin(value + j[k], cand[k]);
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      if (k == 13) continue;
      if (cand[k] < old[k]) {                                          // THIS offer lowered the neighbour: it speaks in the next sweep
        __hip_atomic_store(stamp + jr[k], sweep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lowered = true;
      }
    }
  }
  if (__any(lowered) && (threadIdx.x & 63) == 0) *mine = 1;            // (every writer stores 1)
}

// One thread: was the last sweep quiet?  What a resumed call starts from.  (last == NULL: a scene without rows.)
__global__ void k_orient_close(const int32_t* last, int32_t* meta, a3d_orient_summary* summary, const int sweeps) {
  const int f = last ? *last : 0;
  if (meta) meta[0] = f, meta[1] = sweeps;
  summary->converged = f == 0;
}

// PHASE 2: (ancestor << 1 | parity of the edge to it) per caller row; a root holds (itself, 0); -1: not reached.
__global__ __launch_bounds__(kOrientBlock) void k_orient_parent(const OrientTab t, const uint16_t* __restrict__ edge,
                                                                const u64* __restrict__ value, int32_t* __restrict__ out) {
  const int stride = gridDim.x * kOrientBlock;
  for (int r = blockIdx.x * kOrientBlock + threadIdx.x; r < t.n; r += stride) {
    const int i = t.orig[r];
    const u64 cur = value[i];
    const unsigned owner = (unsigned)(cur & 0xffffffffull), dist = (unsigned)(cur >> 32);
    if (cur == kOrientNone || owner >= (unsigned)t.n) {
      out[i] = -1;
      continue;
    }
    int found = i << 1;                                                // a seed; or, before the fixed point, a voxel nobody explains
    if (dist != 0) {
      int jr[27], j[27];
      unsigned e[27];
      u64 v[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        if (k == 13) continue;
        jr[k] = t.nbr[(size_t)k * t.npad + r];
        e[k] = edge[(size_t)k * t.n + r];
      }
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        if (k == 13) continue;
        j[k] = t.orig[(unsigned)jr[k] < (unsigned)t.n ? jr[k] : r];
      }
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        if (k == 13) continue;
        v[k] = value[j[k]];
      }
#pragma unroll
      for (int k = 26; k >= 0; --k) {                                  // descending: the lowest slot that qualifies is kept
        if (k == 13) continue;
        const bool ok = e[k] != 0 && (unsigned)jr[k] < (unsigned)t.n && v[k] != kOrientNone &&
                        v[k] + ((u64)(e[k] & kEdgeCost) << 32) == cur;  // the same owner and dist[u] + w == dist[v], in one comparison
        if (ok) found = (j[k] << 1) | ((e[k] & kEdgeNeg) ? 1 : 0);
      }
    }
    out[i] = found;
  }
}

// PHASE 3, one round: (anc, p) o (anc', p') = (anc', p ^ p'); a root is (itself, 0), so composing with it changes nothing.
__global__ __launch_bounds__(kOrientBlock) void k_orient_jump(const int32_t* __restrict__ in, int32_t* __restrict__ out, const int n) {
  const int stride = gridDim.x * kOrientBlock;
  for (int i = blockIdx.x * kOrientBlock + threadIdx.x; i < n; i += stride) {
    const int a = in[i];
    int b = a;
    if (a >= 0 && (a >> 1) < n) {
      const int t = in[a >> 1];
      if (t >= 0) b = (t & ~1) | ((a ^ t) & 1);
    }
    out[i] = b;
  }
}

// the parity of a row from its final (root, parity of the path to it) and the root's own flip
__device__ __forceinline__ int parity_of(const int32_t* __restrict__ jump, const uint8_t* __restrict__ sflip, const long long i,
                                         const int n) {
  const int a = jump[i];
  if (a < 0 || (a >> 1) >= n) return 0;
  return (a & 1) ^ (sflip[a >> 1] ? 1 : 0);
}
__device__ __forceinline__ unsigned signed_bits(const float x, const int parity) {
  return __float_as_uint(x) ^ (parity ? 0x80000000u : 0u);
}

// The outputs, the lift, the summary but the conflicts: one streaming pass behind a launch boundary (plain loads).
__global__ __launch_bounds__(kOrientFat) void k_orient_finish(const a3d_orient_normals_args a, const u64* __restrict__ value,
                                                              const int32_t* __restrict__ jump, const uint8_t* __restrict__ sflip,
                                                              uint8_t* __restrict__ parity) {
  __shared__ int wave_part[kOrientFat / 64];
  const long long stride = (long long)gridDim.x * kOrientFat;
  const int n = (int)a.n;
  int n_adm = 0, n_seeds = 0, n_reached = 0, n_flipped = 0, far = 0, bad = 0;
  for (long long i = (long long)blockIdx.x * kOrientFat + threadIdx.x; i < n; i += stride) {
    const float* nv = a.normal_qv_dev + 3 * i;
    const float n0 = nv[0], n1 = nv[1], n2 = nv[2];
    const u64 w = value[i];
    const bool reached = w != kOrientNone && jump[i] >= 0;
    const int d = reached ? (int)(w >> 32) : -1, s = reached ? (int)(w & 0xffffffffull) : -1;
    const int p = reached ? parity_of(jump, sflip, i, n) : 0;
    parity[i] = (uint8_t)p;
    if (a.normal_out_qv_dev) {
      unsigned* o = (unsigned*)a.normal_out_qv_dev + 3 * i;
      o[0] = signed_bits(n0, p), o[1] = signed_bits(n1, p), o[2] = signed_bits(n2, p);
    }
    if (a.flipped_qv_dev) a.flipped_qv_dev[i] = (uint8_t)p;
    if (a.dist_qv_dev) a.dist_qv_dev[i] = d;
    if (a.owner_qv_dev) a.owner_qv_dev[i] = s;
    n_adm += admitted(n0, n1, n2), n_seeds += d == 0, n_reached += d >= 0, n_flipped += p, far = max(far, d);
  }
  for (long long v = (long long)blockIdx.x * kOrientFat + threadIdx.x; v < a.n_full; v += stride) {
    const long long row = a.inverse_map_dev ? a.inverse_map_dev[v] : v;
    unsigned o0 = 0, o1 = 0, o2 = 0;
    if (row < 0 || row >= n) {
      bad = 1;
    } else {
      const int p = value[row] != kOrientNone ? parity_of(jump, sflip, row, n) : 0;
      const float* nv = a.normal_qv_dev + 3 * row;
      o0 = signed_bits(nv[0], p), o1 = signed_bits(nv[1], p), o2 = signed_bits(nv[2], p);
    }
    if (a.normal_full_dev) {
      unsigned* o = (unsigned*)a.normal_full_dev + 3 * v;
      o[0] = o0, o[1] = o1, o[2] = o2;
    }
  }
  const long long s_adm = block_sum<kOrientFat>(n_adm, wave_part), s_seeds = block_sum<kOrientFat>(n_seeds, wave_part);
  const long long s_reached = block_sum<kOrientFat>(n_reached, wave_part), s_flipped = block_sum<kOrientFat>(n_flipped, wave_part);
  const long long s_bad = block_sum<kOrientFat>(bad, wave_part);
  const int m_far = block_max<kOrientFat>(far, wave_part);
  if (threadIdx.x == 0) {
    add_i64(&a.summary_dev->admitted, s_adm);
    add_i64(&a.summary_dev->seeds, s_seeds);
    add_i64(&a.summary_dev->reached, s_reached);
    add_i64(&a.summary_dev->unreached, s_adm - s_reached);             // (a reached row is admitted)
    add_i64(&a.summary_dev->flipped, s_flipped);
    if (m_far > 0) atomicMax(&a.summary_dev->max_dist, m_far);
    if (s_bad) atomicOr(&a.summary_dev->err, A3D_ORIENT_BAD_INDEX);
  }
}

// The edges whose two OUTPUT normals still have dot < 0, each at its end with the slot above 13 (slot 26 - k is the other's).
__global__ __launch_bounds__(kOrientBlock) void k_orient_conflicts(const OrientTab t, const uint16_t* __restrict__ edge,
                                                                   const uint8_t* __restrict__ parity, a3d_orient_summary* summary) {
  __shared__ int wave_part[kOrientBlock / 64];
  const int stride = gridDim.x * kOrientBlock;
  int count = 0;
  for (int r = blockIdx.x * kOrientBlock + threadIdx.x; r < t.n; r += stride) {
    const int mine = parity[t.orig[r]];
    int jr[13];
    unsigned e[13];
    int other[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      jr[k] = t.nbr[(size_t)(k + 14) * t.npad + r];
      e[k] = edge[(size_t)(k + 14) * t.n + r];
    }
#pragma unroll
    for (int k = 0; k < 13; ++k) other[k] = t.orig[(unsigned)jr[k] < (unsigned)t.n ? jr[k] : r];
#pragma unroll
    for (int k = 0; k < 13; ++k) other[k] = parity[other[k]];
#pragma unroll
    for (int k = 0; k < 13; ++k) count += (e[k] & ((mine ^ other[k]) ? kEdgePos : kEdgeNeg)) ? 1 : 0;
  }
  const long long s = block_sum<kOrientBlock>(count, wave_part);
  if (threadIdx.x == 0) add_i64(&summary->conflicts, s);
}

static int jump_rounds(long long n) {
  int rounds = 0;
  while ((1ll << rounds) < n) ++rounds;                                // ceil(log2 n): a parent chain has fewer than n edges
  return rounds;
}

}  // namespace a3d

using namespace a3d;

extern "C" size_t a3d_orient_workspace_bytes(int64_t n) {
  if (n < 0 || n > A3D_ORIENT_MAX_ROWS) return 0;
  return carve_orient(nullptr, n).bytes;
}

extern "C" int a3d_orient_edge(const float* a, const float* b, int32_t* w, int32_t* flip) {
  if (!a || !b || !w || !flip) {
    set_error("a3d_orient_edge: a NULL pointer");
    return A3D_ERR_INVALID;
  }
  int cost;
  float dot;
  orient_edge(a[0], a[1], a[2], b[0], b[1], b[2], cost, dot);
  *w = cost, *flip = dot < 0.0f ? 1 : 0;
  return A3D_OK;
}

extern "C" int a3d_orient_normals(const a3d_orient_normals_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_orient_normals: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_orient_normals_args& a = *args;
  const a3d_scene* s = a.scene;
  const bool bad_scene = !scene_walkable(s, a.n) || a.n > A3D_ORIENT_MAX_ROWS;
  const bool bad_conn = a.connectivity != 6 && a.connectivity != 18 && a.connectivity != 26;
  const bool bad_mode = a.mode != A3D_ORIENT_GIVEN && a.mode != A3D_ORIENT_NEAREST;
  const bool bad_seeds =
      bad_mode || (a.mode == A3D_ORIENT_GIVEN && !a.seed_qv_dev) ||
      (a.mode == A3D_ORIENT_NEAREST && (!a.component_qv_dev || !a.position_qv_dev || !std::isfinite(a.viewpoint[0]) ||
                                        !std::isfinite(a.viewpoint[1]) || !std::isfinite(a.viewpoint[2])));
  if (bad_scene || bad_conn || bad_seeds || a.sweeps < 1 || a.sweeps > A3D_ORIENT_MAX_SWEEPS || (a.resume != 0 && a.resume != 1) ||
      (a.n > 0 && !a.normal_qv_dev) || !a.summary_dev || (a.normal_out_qv_dev && a.normal_out_qv_dev == a.normal_qv_dev) ||
      a.n_full < 0 || a.n_full > 0x7fffffffll || !a.workspace_dev || ((uintptr_t)a.workspace_dev & 255) ||
      a.workspace_bytes < a3d_orient_workspace_bytes(a.n)) {
    set_error("a3d_orient_normals: bad arguments (scene %s, n=%lld connectivity=%d mode=%d sweeps=%d resume=%d normals %s seeds %s "
              "summary %s n_full=%lld workspace=%zu)", s ? "given" : "NULL", (long long)a.n, a.connectivity, a.mode, a.sweeps,
              a.resume, a.normal_qv_dev ? "given" : "NULL", bad_seeds ? "incomplete" : "given", a.summary_dev ? "given" : "NULL",
              (long long)a.n_full, a.workspace_bytes);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.summary_dev, 0, sizeof(a3d_orient_summary), st));
  const int n = (int)a.n;
  const OrientWs w = carve_orient(a.workspace_dev, n);
  if (n > 0) {
    OrientTab t;
    t.nbr = s->lv[0].nbr27, t.orig = s->orig_row, t.n = n, t.npad = s->lv[0].npad;
    t.mask = offset_mask(a.connectivity);
    const unsigned grid = capped_grid(n, kOrientBlock, kOrientMaxBlocks);
    A3D_HIP_CHECK(hipMemsetAsync(w.flag, 0, (A3D_ORIENT_MAX_SWEEPS + 1) * sizeof(int32_t), st));
    if (a.resume) {
      k_orient_restamp<<<grid, kOrientBlock, 0, st>>>(w, n);
      A3D_LAUNCH_CHECK();
    } else {
      k_orient_edges<<<grid, kOrientBlock, 0, st>>>(a.normal_qv_dev, t, w.edge);
      A3D_LAUNCH_CHECK();
      if (a.mode == A3D_ORIENT_NEAREST) {
        A3D_HIP_CHECK(hipMemsetAsync(w.best, 0xff, (size_t)n * 8, st));        // all ones: above every d2
        A3D_HIP_CHECK(hipMemsetAsync(w.seedrow, 0x7f, (size_t)n * 4, st));     // 0x7f7f7f7f: above every row
        k_orient_near_d2<<<grid, kOrientBlock, 0, st>>>(a, w.best, n);
        A3D_LAUNCH_CHECK();
        k_orient_near_row<<<grid, kOrientBlock, 0, st>>>(a, w.best, w.seedrow, n);
        A3D_LAUNCH_CHECK();
      }
      k_orient_init<<<grid, kOrientBlock, 0, st>>>(a, t, w);
      A3D_LAUNCH_CHECK();
    }
    for (int k = 1; k <= a.sweeps; ++k) {
      k_orient_sweep<<<grid, kOrientBlock, 0, st>>>(t, w.edge, w.value, w.stamp, w.flag + k - 1, w.flag + k, k);
      A3D_LAUNCH_CHECK();
    }
    k_orient_close<<<1, 1, 0, st>>>(w.flag + a.sweeps, w.meta, a.summary_dev, a.sweeps);
    A3D_LAUNCH_CHECK();
    int32_t* from = w.jump;
    int32_t* to = w.jump + n;
    k_orient_parent<<<grid, kOrientBlock, 0, st>>>(t, w.edge, w.value, from);
    A3D_LAUNCH_CHECK();
    for (int round = 0; round < jump_rounds(n); ++round) {
      k_orient_jump<<<grid, kOrientBlock, 0, st>>>(from, to, n);
      A3D_LAUNCH_CHECK();
      int32_t* swap = from;
      from = to, to = swap;
    }
    const long long longest = a.n_full > n ? a.n_full : n;
    k_orient_finish<<<capped_grid(longest, kOrientFat, kOrientFatBlocks), kOrientFat, 0, st>>>(a, w.value, from, w.sflip, w.parity);
    A3D_LAUNCH_CHECK();
    k_orient_conflicts<<<grid, kOrientBlock, 0, st>>>(t, w.edge, w.parity, a.summary_dev);
    A3D_LAUNCH_CHECK();
  } else {
    k_orient_close<<<1, 1, 0, st>>>(nullptr, nullptr, a.summary_dev, a.sweeps);
    A3D_LAUNCH_CHECK();
    if (a.n_full > 0) {
      k_orient_finish<<<capped_grid(a.n_full, kOrientFat, kOrientFatBlocks), kOrientFat, 0, st>>>(a, w.value, w.jump, w.sflip, w.parity);
      A3D_LAUNCH_CHECK();
    }
  }
  return A3D_OK;
}
