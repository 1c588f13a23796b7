// session_pieces.hip -- the connected pieces of a labelling on the voxel lattice, the despeckle step that gives a small
// piece to its surroundings, the pieces under a SIMILARITY of normals and colours (smooth patches, the magic wand) and the
// vote that snaps a labelling to such a partition (gfx950).  Entry points: a3d_label_pieces, a3d_absorb_pieces,
// a3d_similar_pieces, a3d_vote_pieces -- and a3d_similar_pair, the pair predicate on the host by the function the kernel
// calls, for the tests without a GPU.
//
// The reference has no counterpart: its tool keeps an arg-max per voxel and never asks where in space a label lies.
// THE RULES (ours, stated in include/agile3d_hip.h at the two entry points):
//   pieces   rows with key >= 0 are joined when they are neighbours under the connectivity (6: |d|1 = 1, 18: |d|1 <= 2, 26:
//            the whole 3^3 table) and hold the same key; a piece is a class of the transitive closure and is named by its
//            SMALLEST CALLER ROW; one record per piece, ascending root: key, voxels, "holds a clicked row", bounding box
//   absorb   ONE simultaneous step on the input labels: a piece of fewer than min_voxels voxels without a clicked row takes
//            the label most of its differently labelled neighbour pairs vote for (ties: the lowest label; no vote: kept)
//
// THE ADJACENCY is the scene's level-0 table A3D_TAB_NBR27 (int32 [27][npad], internal rows, a missing neighbour is n); both
// ends of an entry go through A3D_TAB_ORIGROW, so parent[], the keys and every output are indexed by CALLER row.
//
// UNION-FIND, three launches.  k_pieces_init: parent[i] = i (-1 where key < 0).  k_pieces_hook: one thread per voxel looks at
// the 13 offsets of one half-space (adjacency is symmetric: offset 26 - k is -k, and the other end looks that way) and
// unites the two rows when the keys agree: both walk to their roots, and the LARGER root is linked under the smaller with one
// atomicCAS(parent[large], large, small); a walk shortens the path behind it (atomicMin to the grandparent).
// k_pieces_flatten: every row walks to its root and writes it to piece_qv.
// WHY NO LOOP CAN HANG: parent[x] <= x always (init sets x, a link writes a smaller row), so a walk strictly descends and
// ends after at most n steps; a CAS that fails means another thread LOWERED that parent meanwhile, the sum of all parents
// is bounded below, and the retry walks on from the value the CAS returned.  No thread waits for another: no spin-wait, no
// grid barrier, no cooperative launch.
// WHY THE RESULT IS ORDER-FREE: whatever order the links arrive in, each class ends as one tree whose root was never linked
// under anything; the smallest row m of a class has parent[m] <= m inside the class, so parent[m] = m: the root IS the
// minimum.  piece_qv is therefore a function of the arguments, and so is everything derived from it.
// MEMORY VISIBILITY in the hook kernel: the XCDs' L2s are not coherent for plain accesses.  While other workgroups may be
// writing parent[], it is read with __hip_atomic_load(..., __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) and written with
// atomics only.  A STALE parent is still a member of the same set (parents are only ever replaced by members further down
// the same tree), so a walk over stale values still ends in that set, and a CAS on a row that is no longer a root fails and
// is retried.  The kernels behind a launch boundary (flatten, statistics, records) use plain loads.
//
// THE RECORDS: sizes, boxes and the click flag are integer atomicAdd / atomicMin / atomicMax / atomicOr at the root's slot
// (a wave whose rows all share one root -- the internal order is Morton order, so most do -- folds them with shuffles
// first and sends one atomic each); one block then counts the roots before every row (k_pieces_records, as k_render_scan
// turns counts into offsets), so the list comes out in root order without an atomic append.
// ABSORB: small pieces are numbered by the same one-block scan; votes are integer atomicAdds into votes[small][label].
// Sums of integers, minima and maxima do not depend on the order of arrival: two calls give the same bytes.
//
// SIMILAR PIECES: the same three launches with another edge test.  k_similar_init writes parent[i] = -1 for a row that is
// not ADMISSIBLE (key < 0, or it fails the test against the reference normal / colour); k_similar_hook unites two admissible
// neighbours of one key when sim_normals and sim_feats pass (fp32, one rounding per operation, stated in the header).  Both
// are symmetric bit for bit, so it does not matter that only the end that looks into the half-space evaluates them, and the
// order-free argument above holds unchanged: the classes are a function of the arguments, the root is the minimum.
// The hook issues a stage's loads TOGETHER: 13 table entries, then 13 caller rows, then 13 keys / normals / colours, each
// into registers with constant indices (a missing neighbour reads the thread's own row, so no load hangs on a branch); the
// 13 bits that survive are then united one by one -- that part is a dependent chain by nature.
// VOTE: the eligible pieces (>= min_voxels) are numbered by the one-block scan; votes[slot][label] are integer atomicAdds;
// one thread per eligible root picks the winner, tests the share in int64 and looks through the clicks for one that
// contradicts it.
#include "session_device.h"

#include <cstdlib>

namespace a3d {

constexpr int kPiecesBlock = 256;
constexpr int kPiecesMaxBlocks = 2048;
constexpr int kPiecesScan = 1024;
static_assert(kPiecesBlock == A3D_MAX_CLICKS, "one click per thread of a workgroup");

struct PiecesWs {
  int32_t* size;       // [n] voxels of the piece, at its root's slot (a3d_absorb_pieces reads them)
  int32_t* clicked;    // [n] 1 at the root of a piece that holds a clicked row
  int32_t* lo;         // [3][n]
  int32_t* hi;         // [3][n]
  int32_t* parent;     // [n]
  // a3d_absorb_pieces, behind what a3d_label_pieces left
  int32_t* slot;       // [n] number of the small piece rooted here, -1 elsewhere
  int32_t* newlabel;   // [capacity] the winner of the vote, -1: none
  int32_t* cflag;      // [n] as `clicked`, from a3d_absorb_pieces' own click list; zeroed together with the votes
  int32_t* votes;      // [capacity][n_classes]
  size_t label_bytes, zero_bytes, bytes;
};
// k int32 of a workspace (at least one)
static int32_t* take_ints(Carver& c, size_t k) { return (int32_t*)c.take((k > 0 ? k : 1) * 4); }
static PiecesWs carve_pieces(void* base, long long n, long long capacity, int n_classes) {
  PiecesWs w;
  Carver c{base};
  const size_t m = (size_t)(n > 0 ? n : 1);
  w.size = take_ints(c, m), w.clicked = take_ints(c, m), w.lo = take_ints(c, 3 * m), w.hi = take_ints(c, 3 * m);
  w.parent = take_ints(c, m);
  w.label_bytes = c.off;
  w.slot = take_ints(c, m), w.newlabel = take_ints(c, (size_t)capacity);
  const size_t zero_from = c.off;
  w.cflag = take_ints(c, m), w.votes = take_ints(c, (size_t)capacity * (size_t)n_classes);
  w.zero_bytes = c.off - zero_from;
  w.bytes = c.off;
  return w;
}

struct PiecesTab {
  const int32_t* nbr;        // [27][npad]
  const int32_t* orig;       // [n]
  const int32_t* xyzb;       // [n][4]
  int n, npad;
  unsigned mask;
};

__device__ __forceinline__ int parent_now(const int32_t* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The root of x as far as this thread can see it: a strictly descending walk (parent[x] <= x).  On the way every row passed
// is pointed at its grandparent (path halving) with an atomicMin: a lower ancestor of the same tree, so parents still only
// decrease and still name members of the set; without it the trees of a room-sized piece grow hundreds of links deep.
__device__ __forceinline__ int root_now(int32_t* parent, int x) {
  int p = parent_now(parent, x);
  while (p != x) {
    const int g = parent_now(parent, p);
    if (g != p) atomicMin(parent + x, g);
    x = p, p = g;
  }
  return x;
}
__device__ __forceinline__ void unite(int32_t* parent, int a, int b) {
  for (;;) {
    a = root_now(parent, a), b = root_now(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicCAS(parent + a, a, b);       // the larger root under the smaller
    if (old == a) return;
    a = old;                                           // a was linked meanwhile, to a smaller row of its set: walk on from there
  }
}

__global__ __launch_bounds__(kPiecesBlock) void k_pieces_init(const int32_t* __restrict__ keys, const PiecesWs w, const int n) {
  const int stride = gridDim.x * kPiecesBlock;
  for (int i = blockIdx.x * kPiecesBlock + threadIdx.x; i < n; i += stride) {
    w.parent[i] = keys[i] < 0 ? -1 : i;
    w.size[i] = 0, w.clicked[i] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) w.lo[(size_t)c * n + i] = 0x7fffffff, w.hi[(size_t)c * n + i] = (int32_t)0x80000000;
  }
}

__global__ __launch_bounds__(kPiecesBlock) void k_pieces_hook(const int32_t* __restrict__ keys, const PiecesTab t, int32_t* parent) {
  const int stride = gridDim.x * kPiecesBlock;
  for (int r = blockIdx.x * kPiecesBlock + threadIdx.x; r < t.n; r += stride) {
    const int i = t.orig[r];
    const int key = keys[i];
    if (key < 0) continue;
    for (int k = 0; k < 13; ++k) {
      if (!((t.mask >> k) & 1u)) continue;
      const int jr = t.nbr[(size_t)k * t.npad + r];
      if ((unsigned)jr >= (unsigned)t.n) continue;
      const int j = t.orig[jr];
      if (keys[j] == key) unite(parent, i, j);
    }
  }
}

__global__ __launch_bounds__(kPiecesBlock) void k_pieces_flatten(const int32_t* __restrict__ parent, int32_t* __restrict__ piece_qv,
                                                                 const int n) {
  const int stride = gridDim.x * kPiecesBlock;
  for (int i = blockIdx.x * kPiecesBlock + threadIdx.x; i < n; i += stride) {
    int x = parent[i];
    if (x >= 0)
      for (int p = parent[x]; p != x; p = parent[x]) x = p;
    piece_qv[i] = x;
  }
}

// sizes, boxes, click flags at the root's slot.  One thread per INTERNAL row (consecutive rows are neighbours in space).
__global__ __launch_bounds__(kPiecesBlock) void k_pieces_stats(const a3d_label_pieces_args a, const PiecesTab t, const PiecesWs w) {
  const int n = t.n;
  const int32_t* __restrict__ piece = a.piece_qv_dev;
  if (blockIdx.x == 0 && (int)threadIdx.x < a.n_clicks) {
    const int row = a.click_row[threadIdx.x];
    if ((unsigned)row < (unsigned)n && piece[row] >= 0) atomicOr(w.clicked + piece[row], 1);
  }
  const int stride = gridDim.x * kPiecesBlock;
  for (int base = blockIdx.x * kPiecesBlock; base < n; base += stride) {
    const int r = base + threadIdx.x;
    int root = -1, x = 0, y = 0, z = 0;
    if (r < n) {
      root = piece[t.orig[r]];
      const int4 c = *(const int4*)(t.xyzb + 4 * (size_t)r);
      x = c.x, y = c.y, z = c.z;
    }
    const bool valid = root >= 0;
    const unsigned long long live = __ballot(valid);
    if (!live) continue;
    const int first = __shfl(root, __ffsll((long long)live) - 1);
    if (__all(!valid || root == first)) {              // one piece in the wave: fold, then one atomic each
      int cnt = valid ? 1 : 0;
      int lx = valid ? x : 0x7fffffff, ly = valid ? y : 0x7fffffff, lz = valid ? z : 0x7fffffff;
      int hx = valid ? x : (int)0x80000000, hy = valid ? y : (int)0x80000000, hz = valid ? z : (int)0x80000000;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        lx = min(lx, __shfl_xor(lx, o)), ly = min(ly, __shfl_xor(ly, o)), lz = min(lz, __shfl_xor(lz, o));
        hx = max(hx, __shfl_xor(hx, o)), hy = max(hy, __shfl_xor(hy, o)), hz = max(hz, __shfl_xor(hz, o));
      }
      if ((threadIdx.x & 63) == 0) {
        atomicAdd(w.size + first, cnt);
        atomicMin(w.lo + first, lx), atomicMin(w.lo + (size_t)n + first, ly), atomicMin(w.lo + 2 * (size_t)n + first, lz);
        atomicMax(w.hi + first, hx), atomicMax(w.hi + (size_t)n + first, hy), atomicMax(w.hi + 2 * (size_t)n + first, hz);
      }
    } else if (valid) {
      atomicAdd(w.size + root, 1);
      atomicMin(w.lo + root, x), atomicMin(w.lo + (size_t)n + root, y), atomicMin(w.lo + 2 * (size_t)n + root, z);
      atomicMax(w.hi + root, x), atomicMax(w.hi + (size_t)n + root, y), atomicMax(w.hi + 2 * (size_t)n + root, z);
    }
  }
}

// exclusive prefix sums over the kPiecesScan threads of one block (what k_render_scan does for the tiles' counts)
__device__ __forceinline__ int block_scan_exclusive(int mine, int* part, int* total) {
  part[threadIdx.x] = mine;
  __syncthreads();
  for (int o = 1; o < kPiecesScan; o <<= 1) {
    const int add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  *total = part[kPiecesScan - 1];
  return part[threadIdx.x] - mine;
}

// ONE block: the roots before every row; the first max_out records in root order, the true count
__global__ __launch_bounds__(kPiecesScan) void k_pieces_records(const a3d_label_pieces_args a, const int32_t* __restrict__ keys,
                                                                const PiecesWs w, const int n) {
  __shared__ int part[kPiecesScan];
  const int32_t* __restrict__ piece = a.piece_qv_dev;
  const int per = (n + kPiecesScan - 1) / kPiecesScan;
  const long long lo64 = (long long)threadIdx.x * per;
  const int lo = (int)(lo64 < n ? lo64 : n), hi = (int)(lo64 + per < n ? lo64 + per : n);
  int mine = 0;
  for (int i = lo; i < hi; ++i) mine += piece[i] == i;
  int total;
  int run = block_scan_exclusive(mine, part, &total);
  for (int i = lo; i < hi && run < a.max_out; ++i)
    if (piece[i] == i) {
      a3d_piece rec;
      rec.root = i, rec.key = keys ? keys[i] : 0, rec.voxels = w.size[i], rec.clicked = w.clicked[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) rec.lo[c] = w.lo[(size_t)c * n + i], rec.hi[c] = w.hi[(size_t)c * n + i];
      a.out_dev[run++] = rec;
    }
  if (threadIdx.x == 0) a.n_out_dev[0] = total;
}

__global__ __launch_bounds__(kPiecesBlock) void k_pieces_full(const a3d_label_pieces_args a, const long long n) {
  const long long stride = (long long)gridDim.x * kPiecesBlock;
  for (long long v = (long long)blockIdx.x * kPiecesBlock + threadIdx.x; v < a.n_full; v += stride) {
    const long long src = a.inverse_map_dev ? a.inverse_map_dev[v] : v;
    if (src < 0 || src >= n) {
      atomicOr(a.n_out_dev + 1, 1);                    // reported through the error word; the vertex is left unwritten
      continue;
    }
    a.piece_full_dev[v] = a.piece_qv_dev[src];
  }
}

// ---- absorb ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPiecesBlock) void k_absorb_clicks(const a3d_absorb_pieces_args a, const PiecesWs w, const int n) {
  if ((int)threadIdx.x < a.n_clicks) {
    const int row = a.click_row[threadIdx.x];
    if ((unsigned)row < (unsigned)n) {
      const int root = a.piece_qv_dev[row];
      if ((unsigned)root < (unsigned)n) w.cflag[root] = 1;     // (every writer writes 1)
    }
  }
}

// ONE block: numbers the small pieces in root order; says whether they fit
__global__ __launch_bounds__(kPiecesScan) void k_absorb_scan(const a3d_absorb_pieces_args a, const PiecesWs w, const int n) {
  __shared__ int part[kPiecesScan];
  const int32_t* __restrict__ piece = a.piece_qv_dev;
  const int per = (n + kPiecesScan - 1) / kPiecesScan;
  const long long lo64 = (long long)threadIdx.x * per;
  const int lo = (int)(lo64 < n ? lo64 : n), hi = (int)(lo64 + per < n ? lo64 + per : n);
  int mine = 0;
  for (int i = lo; i < hi; ++i) mine += piece[i] == i && w.size[i] < a.min_voxels && !w.cflag[i];
  int total;
  int run = block_scan_exclusive(mine, part, &total);
  for (int i = lo; i < hi; ++i) w.slot[i] = (piece[i] == i && w.size[i] < a.min_voxels && !w.cflag[i]) ? run++ : -1;
  if (threadIdx.x == 0) {
    a.summary_dev->small_pieces = total;
    if (total > a.capacity) atomicOr(&a.summary_dev->err, A3D_ABSORB_OVERFLOW);
  }
}

__global__ __launch_bounds__(kPiecesBlock) void k_absorb_vote(const a3d_absorb_pieces_args a, const PiecesTab t, const PiecesWs w) {
  if (a.summary_dev->small_pieces > a.capacity) return;
  const int32_t* __restrict__ labels = a.labels_dev;
  const int stride = gridDim.x * kPiecesBlock;
  for (int r = blockIdx.x * kPiecesBlock + threadIdx.x; r < t.n; r += stride) {
    const int i = t.orig[r];
    const int root = a.piece_qv_dev[i];
    if ((unsigned)root >= (unsigned)t.n) continue;
    const int s = w.slot[root];
    if (s < 0) continue;
    const int mine = labels[i];
    for (int k = 0; k < 27; ++k) {
      if (!((t.mask >> k) & 1u)) continue;
      const int jr = t.nbr[(size_t)k * t.npad + r];
      if ((unsigned)jr >= (unsigned)t.n) continue;
      const int other = labels[t.orig[jr]];
      if (other == mine) continue;
      if ((unsigned)other >= (unsigned)a.n_classes) {
        atomicOr(&a.summary_dev->err, A3D_ABSORB_BAD_LABEL);
        continue;
      }
      atomicAdd(w.votes + (size_t)s * a.n_classes + other, 1);
    }
  }
}

__global__ __launch_bounds__(kPiecesBlock) void k_absorb_decide(const a3d_absorb_pieces_args a, const PiecesWs w, const int n) {
  if (a.summary_dev->small_pieces > a.capacity) return;
  const int stride = gridDim.x * kPiecesBlock;
  for (int i = blockIdx.x * kPiecesBlock + threadIdx.x; i < n; i += stride) {
    const int s = w.slot[i];
    if (s < 0) continue;
    const int32_t* v = w.votes + (size_t)s * a.n_classes;
    int best = -1, most = 0;
    for (int c = 0; c < a.n_classes; ++c)
      if (v[c] > most) most = v[c], best = c;           // ties: the lowest label
    w.newlabel[s] = best;
    if (best >= 0) {
      atomicAdd(&a.summary_dev->relabelled_pieces, 1);
      atomicAdd(&a.summary_dev->relabelled_voxels, w.size[i]);
    } else {
      atomicAdd(&a.summary_dev->kept_isolated, 1);
    }
  }
}

__global__ __launch_bounds__(kPiecesBlock) void k_absorb_write(const a3d_absorb_pieces_args a, const PiecesWs w, const int n) {
  if (a.summary_dev->small_pieces > a.capacity) return;
  const int stride = gridDim.x * kPiecesBlock;
  for (int i = blockIdx.x * kPiecesBlock + threadIdx.x; i < n; i += stride) {
    int out = a.labels_dev[i];
    const int root = a.piece_qv_dev[i];
    if ((unsigned)root < (unsigned)n) {
      const int s = w.slot[root];
      if (s >= 0 && w.newlabel[s] >= 0) out = w.newlabel[s];
    }
    a.labels_out_dev[i] = out;
  }
}

// ---- similar pieces -------------------------------------------------------------------------------------------------------
// NSIM and FSIM of the header: every operation rounded on its own, in the order written; a NaN fails the comparison.
__host__ __device__ inline bool sim_normals(const float a0, const float a1, const float a2, const float b0, const float b1,
                                            const float b2, const float c, const int oriented) {
#pragma clang fp contract(off)
  const float dot = (a0 * b0 + a1 * b1) + a2 * b2;
  return (oriented ? dot : fabsf(dot)) >= c;
}
__host__ __device__ inline bool sim_feats(const float a0, const float a1, const float a2, const float b0, const float b1,
                                          const float b2, const float t) {
#pragma clang fp contract(off)
  const float d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2;
  const float q = (d0 * d0 + d1 * d1) + d2 * d2;
  return q <= t;
}

struct SimilarTab {
  const int32_t* keys;       // [n] or NULL: all 0
  const float* normal;       // [n][3] or NULL
  const float* feat;         // [n][3] or NULL
  float cos_min, tol2, ref_cos_min, ref_tol2;
  float ref_normal[3], ref_feat[3];
  int oriented, ref_flags;
};

__global__ __launch_bounds__(kPiecesBlock) void k_similar_init(const SimilarTab s, const PiecesWs w, const int n) {
  const int stride = gridDim.x * kPiecesBlock;
  for (int i = blockIdx.x * kPiecesBlock + threadIdx.x; i < n; i += stride) {
    bool ok = !s.keys || s.keys[i] >= 0;
    if (s.ref_flags & A3D_SIMILAR_REF_NORMAL) {
      const float* a = s.normal + 3 * (size_t)i;
      ok = ok && sim_normals(a[0], a[1], a[2], s.ref_normal[0], s.ref_normal[1], s.ref_normal[2], s.ref_cos_min, s.oriented);
    }
    if (s.ref_flags & A3D_SIMILAR_REF_FEAT) {
      const float* a = s.feat + 3 * (size_t)i;
      ok = ok && sim_feats(a[0], a[1], a[2], s.ref_feat[0], s.ref_feat[1], s.ref_feat[2], s.ref_tol2);
    }
    w.parent[i] = ok ? i : -1;
    w.size[i] = 0, w.clicked[i] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) w.lo[(size_t)c * n + i] = 0x7fffffff, w.hi[(size_t)c * n + i] = (int32_t)0x80000000;
  }
}

template <bool HAS_N, bool HAS_F>
__global__ __launch_bounds__(kPiecesBlock) void k_similar_hook(const SimilarTab s, const PiecesTab t, int32_t* parent) {
  const int stride = gridDim.x * kPiecesBlock;
  for (int r = blockIdx.x * kPiecesBlock + threadIdx.x; r < t.n; r += stride) {
    const int i = t.orig[r];
    if (parent_now(parent, i) < 0) continue;             // not admissible: -1 since k_similar_init, never written again
    int j[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) j[k] = ((t.mask >> k) & 1u) ? t.nbr[(size_t)k * t.npad + r] : t.n;
    unsigned join = 0;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      const bool there = (unsigned)j[k] < (unsigned)t.n;
      join |= (there ? 1u : 0u) << k;
      j[k] = t.orig[there ? j[k] : r];                   // a missing neighbour reads this thread's own row: no load waits on a branch
    }
    if (s.keys) {
      const int key = s.keys[i];
      int kj[13];
#pragma unroll
      for (int k = 0; k < 13; ++k) kj[k] = s.keys[j[k]];
#pragma unroll
      for (int k = 0; k < 13; ++k) join &= ~((kj[k] != key ? 1u : 0u) << k);
    }
    if (s.ref_flags) {                                   // (without a reference, admissible = key >= 0, and the keys are equal)
      int pj[13];
#pragma unroll
      for (int k = 0; k < 13; ++k) pj[k] = parent_now(parent, j[k]);
#pragma unroll
      for (int k = 0; k < 13; ++k) join &= ~((pj[k] < 0 ? 1u : 0u) << k);
    }
    if (HAS_N) {
      const float a0 = s.normal[3 * (size_t)i], a1 = s.normal[3 * (size_t)i + 1], a2 = s.normal[3 * (size_t)i + 2];
      float b[13][3];
#pragma unroll
      for (int k = 0; k < 13; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) b[k][c] = s.normal[3 * (size_t)j[k] + c];
#pragma unroll
      for (int k = 0; k < 13; ++k)
        join &= ~((sim_normals(a0, a1, a2, b[k][0], b[k][1], b[k][2], s.cos_min, s.oriented) ? 0u : 1u) << k);
    }
    if (HAS_F) {
      const float a0 = s.feat[3 * (size_t)i], a1 = s.feat[3 * (size_t)i + 1], a2 = s.feat[3 * (size_t)i + 2];
      float b[13][3];
#pragma unroll
      for (int k = 0; k < 13; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) b[k][c] = s.feat[3 * (size_t)j[k] + c];
#pragma unroll
      for (int k = 0; k < 13; ++k) join &= ~((sim_feats(a0, a1, a2, b[k][0], b[k][1], b[k][2], s.tol2) ? 0u : 1u) << k);
    }
#pragma unroll
    for (int k = 0; k < 13; ++k)
      if ((join >> k) & 1u) unite(parent, i, j[k]);
  }
}

// ---- vote -----------------------------------------------------------------------------------------------------------------
struct VoteWs {
  int32_t* size;       // [n] what the labelling call left at the roots
  int32_t* slot;       // [n] number of the eligible piece rooted here, -1 elsewhere
  int32_t* decision;   // [capacity] the label the piece's voxels take, -1: the piece is left alone
  int32_t* votes;      // [capacity][n_classes]; the slots in use are zeroed by the call
  size_t bytes;
};
static VoteWs carve_vote(void* base, long long n, long long capacity, int n_classes) {
  const PiecesWs p = carve_pieces(base, n, 0, 1);
  VoteWs w;
  Carver c{base, p.label_bytes};                // behind what the labelling call left
  w.size = p.size;
  w.slot = take_ints(c, (size_t)(n > 0 ? n : 1)), w.decision = take_ints(c, (size_t)capacity);
  w.votes = take_ints(c, (size_t)capacity * (size_t)n_classes);
  w.bytes = c.off;
  return w;
}

// ONE block: numbers the eligible pieces in root order; says whether they fit
__global__ __launch_bounds__(kPiecesScan) void k_vote_scan(const a3d_vote_pieces_args a, const VoteWs w, const int n) {
  __shared__ int part[kPiecesScan];
  const int32_t* __restrict__ piece = a.piece_qv_dev;
  const int per = (n + kPiecesScan - 1) / kPiecesScan;
  const long long lo64 = (long long)threadIdx.x * per;
  const int lo = (int)(lo64 < n ? lo64 : n), hi = (int)(lo64 + per < n ? lo64 + per : n);
  int mine = 0;
  for (int i = lo; i < hi; ++i) mine += piece[i] == i && w.size[i] >= a.min_voxels;
  int total;
  int run = block_scan_exclusive(mine, part, &total);
  for (int i = lo; i < hi; ++i) w.slot[i] = (piece[i] == i && w.size[i] >= a.min_voxels) ? run++ : -1;
  if (threadIdx.x == 0) {
    a.summary_dev->eligible_pieces = total;
    if (total > a.capacity) atomicOr(&a.summary_dev->err, A3D_VOTE_OVERFLOW);
  }
}

// zeroes the votes of the slots in use: the cost follows the eligible pieces, not the capacity
__global__ __launch_bounds__(kPiecesBlock) void k_vote_clear(const a3d_vote_pieces_args a, const VoteWs w) {
  const int used = a.summary_dev->eligible_pieces;
  if (used > a.capacity) return;
  const long long words = (long long)used * a.n_classes, stride = (long long)gridDim.x * kPiecesBlock;
  for (long long k = (long long)blockIdx.x * kPiecesBlock + threadIdx.x; k < words; k += stride) w.votes[k] = 0;
}

__global__ __launch_bounds__(kPiecesBlock) void k_vote_count(const a3d_vote_pieces_args a, const VoteWs w, const int n) {
  if (a.summary_dev->eligible_pieces > a.capacity) return;
  const int stride = gridDim.x * kPiecesBlock;
  for (int i = blockIdx.x * kPiecesBlock + threadIdx.x; i < n; i += stride) {
    const int label = a.labels_dev[i];
    if ((unsigned)label >= (unsigned)a.n_classes) {
      atomicOr(&a.summary_dev->err, A3D_VOTE_BAD_LABEL);
      continue;
    }
    const int root = a.piece_qv_dev[i];
    if ((unsigned)root >= (unsigned)n) continue;
    const int s = w.slot[root];
    if (s >= 0) atomicAdd(w.votes + (size_t)s * a.n_classes + label, 1);
  }
}

__global__ __launch_bounds__(kPiecesBlock) void k_vote_decide(const a3d_vote_pieces_args a, const VoteWs w, const int n) {
  if (a.summary_dev->eligible_pieces > a.capacity) return;
  const int stride = gridDim.x * kPiecesBlock;
  for (int i = blockIdx.x * kPiecesBlock + threadIdx.x; i < n; i += stride) {
    const int s = w.slot[i];
    if (s < 0) continue;
    const int32_t* v = w.votes + (size_t)s * a.n_classes;
    int winner = 0, most = v[0], cast = v[0];
    for (int c = 1; c < a.n_classes; ++c) {
      cast += v[c];
      if (v[c] > most) most = v[c], winner = c;          // ties: the lowest label
    }
    const int voxels = w.size[i];
    int decision = -1;
    if (most == voxels) {
      atomicAdd(&a.summary_dev->uniform_pieces, 1);
    } else if ((long long)most * a.share_den < (long long)voxels * a.share_num) {
      atomicAdd(&a.summary_dev->below_share_pieces, 1);
    } else {
      bool blocked = false;
      for (int c = 0; c < a.n_clicks; ++c) {
        const int row = a.click_row[c];
        if ((unsigned)row < (unsigned)n && a.piece_qv_dev[row] == i && a.labels_dev[row] != winner) blocked = true;
      }
      if (blocked) {
        atomicAdd(&a.summary_dev->blocked_pieces, 1);
      } else {
        decision = winner;
        if (cast > most) {
          atomicAdd(&a.summary_dev->relabelled_pieces, 1);
          atomicAdd(&a.summary_dev->relabelled_voxels, cast - most);
        }
      }
    }
    w.decision[s] = decision;
  }
}

__global__ __launch_bounds__(kPiecesBlock) void k_vote_write(const a3d_vote_pieces_args a, const VoteWs w, const int n) {
  if (a.summary_dev->eligible_pieces > a.capacity) return;
  const int stride = gridDim.x * kPiecesBlock;
  for (int i = blockIdx.x * kPiecesBlock + threadIdx.x; i < n; i += stride) {
    int out = a.labels_dev[i];
    const int root = a.piece_qv_dev[i];
    if ((unsigned)root < (unsigned)n && (unsigned)out < (unsigned)a.n_classes) {
      const int s = w.slot[root];
      if (s >= 0 && w.decision[s] >= 0) out = w.decision[s];
    }
    a.labels_out_dev[i] = out;
  }
}

static bool pieces_tab(const a3d_scene* s, long long n, int connectivity, PiecesTab* t) {
  if (!scene_walkable(s, n) || !s->lv[0].xyzb) return false;
  t->nbr = s->lv[0].nbr27, t->orig = s->orig_row, t->xyzb = s->lv[0].xyzb;
  t->n = s->lv[0].n, t->npad = s->lv[0].npad;
  t->mask = offset_mask(connectivity);
  return true;
}

}  // namespace a3d

using namespace a3d;

extern "C" size_t a3d_pieces_workspace_bytes(int64_t n) {
  if (n < 0 || n > 0x7fffffffll) return 0;
  return carve_pieces(nullptr, n, 0, 1).label_bytes;
}

extern "C" size_t a3d_absorb_workspace_bytes(int64_t n, int capacity, int n_classes) {
  if (n < 0 || n > 0x7fffffffll || capacity < 0 || n_classes < 1 || n_classes > 256) return 0;
  return carve_pieces(nullptr, n, capacity, n_classes).bytes;
}

extern "C" int a3d_label_pieces(const a3d_label_pieces_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_label_pieces: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_label_pieces_args& a = *args;
  PiecesTab t;
  const bool bad_conn = a.connectivity != 6 && a.connectivity != 18 && a.connectivity != 26;
  if (bad_conn || !pieces_tab(a.scene, a.n, a.connectivity, &t) || a.n_clicks < 0 || a.n_clicks > A3D_MAX_CLICKS ||
      a.max_out < 0 || a.n_full < 0 || !a.n_out_dev || (a.max_out > 0 && !a.out_dev) ||
      (a.n > 0 && (!a.keys_dev || !a.piece_qv_dev || !a.workspace_dev)) || (a.n_full > 0 && (!a.piece_full_dev || !a.piece_qv_dev)) ||
      ((uintptr_t)a.workspace_dev & 255) || a.workspace_bytes < a3d_pieces_workspace_bytes(a.n)) {
    set_error("a3d_label_pieces: bad arguments (n=%lld connectivity=%d clicks=%d max_out=%d n_full=%lld workspace=%zu)",
              (long long)a.n, a.connectivity, a.n_clicks, a.max_out, (long long)a.n_full, a.workspace_bytes);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.n_out_dev, 0, 2 * sizeof(int32_t), st));
  const int n = t.n;
  if (n > 0) {
    const PiecesWs w = carve_pieces(a.workspace_dev, n, 0, 1);
    const unsigned grid = capped_grid(n, kPiecesBlock, kPiecesMaxBlocks);
    k_pieces_init<<<grid, kPiecesBlock, 0, st>>>(a.keys_dev, w, n);
    A3D_LAUNCH_CHECK();
    k_pieces_hook<<<grid, kPiecesBlock, 0, st>>>(a.keys_dev, t, w.parent);
    A3D_LAUNCH_CHECK();
    k_pieces_flatten<<<grid, kPiecesBlock, 0, st>>>(w.parent, a.piece_qv_dev, n);
    A3D_LAUNCH_CHECK();
    k_pieces_stats<<<grid, kPiecesBlock, 0, st>>>(a, t, w);
    A3D_LAUNCH_CHECK();
    k_pieces_records<<<1, kPiecesScan, 0, st>>>(a, a.keys_dev, w, n);
    A3D_LAUNCH_CHECK();
  }
  if (a.n_full > 0) {
    k_pieces_full<<<capped_grid(a.n_full, kPiecesBlock, kPiecesMaxBlocks), kPiecesBlock, 0, st>>>(a, n);
    A3D_LAUNCH_CHECK();
  }
  return A3D_OK;
}

extern "C" int a3d_absorb_pieces(const a3d_absorb_pieces_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_absorb_pieces: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_absorb_pieces_args& a = *args;
  PiecesTab t;
  const bool bad_conn = a.connectivity != 6 && a.connectivity != 18 && a.connectivity != 26;
  if (bad_conn || !pieces_tab(a.scene, a.n, a.connectivity, &t) || a.n_clicks < 0 || a.n_clicks > A3D_MAX_CLICKS ||
      a.n_classes < 1 || a.n_classes > 256 || a.capacity < 0 || a.min_voxels < 0 || !a.summary_dev ||
      (a.n > 0 && (!a.labels_dev || !a.piece_qv_dev || !a.labels_out_dev || !a.workspace_dev || a.labels_out_dev == a.labels_dev)) ||
      ((uintptr_t)a.workspace_dev & 255) || a.workspace_bytes < a3d_absorb_workspace_bytes(a.n, a.capacity, a.n_classes)) {
    set_error("a3d_absorb_pieces: bad arguments (n=%lld connectivity=%d clicks=%d classes=%d capacity=%d min_voxels=%d "
              "workspace=%zu)", (long long)a.n, a.connectivity, a.n_clicks, a.n_classes, a.capacity, a.min_voxels,
              a.workspace_bytes);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.summary_dev, 0, sizeof(a3d_absorb_summary), st));
  const int n = t.n;
  if (n > 0) {
    const PiecesWs w = carve_pieces(a.workspace_dev, n, a.capacity, a.n_classes);
    A3D_HIP_CHECK(hipMemsetAsync(w.cflag, 0, w.zero_bytes, st));       // the click flags and the votes
    const unsigned grid = capped_grid(n, kPiecesBlock, kPiecesMaxBlocks);
    if (a.n_clicks > 0) {
      k_absorb_clicks<<<1, kPiecesBlock, 0, st>>>(a, w, n);
      A3D_LAUNCH_CHECK();
    }
    k_absorb_scan<<<1, kPiecesScan, 0, st>>>(a, w, n);
    A3D_LAUNCH_CHECK();
    k_absorb_vote<<<grid, kPiecesBlock, 0, st>>>(a, t, w);
    A3D_LAUNCH_CHECK();
    k_absorb_decide<<<grid, kPiecesBlock, 0, st>>>(a, w, n);
    A3D_LAUNCH_CHECK();
    k_absorb_write<<<grid, kPiecesBlock, 0, st>>>(a, w, n);
    A3D_LAUNCH_CHECK();
  }
  return A3D_OK;
}

static bool sim_unit(float c) { return std::isfinite(c) && c >= -1.f && c <= 1.f; }
static bool sim_tol(float t) { return std::isfinite(t) && t >= 0.f; }

extern "C" int a3d_similar_pair(const float* normal_a, const float* normal_b, const float* feat_a, const float* feat_b,
                                float cos_min, float tol2, int oriented) {
  if (!normal_a != !normal_b || !feat_a != !feat_b || (oriented != 0 && oriented != 1)) {
    set_error("a3d_similar_pair: a pointer without its partner, or oriented=%d", oriented);
    return -1;
  }
  bool ok = true;
  if (normal_a) ok = ok && sim_normals(normal_a[0], normal_a[1], normal_a[2], normal_b[0], normal_b[1], normal_b[2], cos_min, oriented);
  if (feat_a) ok = ok && sim_feats(feat_a[0], feat_a[1], feat_a[2], feat_b[0], feat_b[1], feat_b[2], tol2);
  return ok ? 1 : 0;
}

extern "C" int a3d_similar_pieces(const a3d_similar_pieces_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_similar_pieces: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_similar_pieces_args& a = *args;
  PiecesTab t;
  const bool bad_conn = a.connectivity != 6 && a.connectivity != 18 && a.connectivity != 26;
  if (bad_conn || !pieces_tab(a.scene, a.n, a.connectivity, &t) || a.n_clicks < 0 || a.n_clicks > A3D_MAX_CLICKS ||
      a.max_out < 0 || a.n_full < 0 || !a.n_out_dev || (a.max_out > 0 && !a.out_dev) ||
      (a.n > 0 && (!a.piece_qv_dev || !a.workspace_dev)) || (a.n_full > 0 && (!a.piece_full_dev || !a.piece_qv_dev)) ||
      ((uintptr_t)a.workspace_dev & 255) || a.workspace_bytes < a3d_pieces_workspace_bytes(a.n)) {
    set_error("a3d_similar_pieces: bad arguments (n=%lld connectivity=%d clicks=%d max_out=%d n_full=%lld workspace=%zu)",
              (long long)a.n, a.connectivity, a.n_clicks, a.max_out, (long long)a.n_full, a.workspace_bytes);
    return A3D_ERR_INVALID;
  }
  bool ref_ok = !(a.ref_flags & ~(A3D_SIMILAR_REF_NORMAL | A3D_SIMILAR_REF_FEAT)) &&
                !((a.ref_flags & A3D_SIMILAR_REF_NORMAL) && !a.normal_qv_dev) && !((a.ref_flags & A3D_SIMILAR_REF_FEAT) && !a.feat_qv_dev);
  for (int c = 0; c < 3; ++c) ref_ok = ref_ok && std::isfinite(a.ref_normal[c]) && std::isfinite(a.ref_feat[c]);
  if (!ref_ok || !sim_unit(a.cos_min) || !sim_unit(a.ref_cos_min) || !sim_tol(a.tol2) || !sim_tol(a.ref_tol2) ||
      (a.oriented != 0 && a.oriented != 1)) {
    set_error("a3d_similar_pieces: bad thresholds or reference (cos_min=%g tol2=%g ref_cos_min=%g ref_tol2=%g oriented=%d "
              "ref_flags=%d)", a.cos_min, a.tol2, a.ref_cos_min, a.ref_tol2, a.oriented, a.ref_flags);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.n_out_dev, 0, 2 * sizeof(int32_t), st));
  // the kernels behind the hook are a3d_label_pieces' own: they take its argument block
  a3d_label_pieces_args la = {};
  la.scene = a.scene, la.n = a.n, la.keys_dev = a.keys_dev, la.inverse_map_dev = a.inverse_map_dev, la.n_full = a.n_full;
  la.piece_qv_dev = a.piece_qv_dev, la.piece_full_dev = a.piece_full_dev, la.out_dev = a.out_dev, la.n_out_dev = a.n_out_dev;
  la.workspace_dev = a.workspace_dev, la.workspace_bytes = a.workspace_bytes;
  la.connectivity = a.connectivity, la.max_out = a.max_out, la.n_clicks = a.n_clicks;
  for (int c = 0; c < a.n_clicks; ++c) la.click_row[c] = a.click_row[c];
  const int n = t.n;
  if (n > 0) {
    SimilarTab s;
    s.keys = a.keys_dev, s.normal = a.normal_qv_dev, s.feat = a.feat_qv_dev;
    s.cos_min = a.cos_min, s.tol2 = a.tol2, s.ref_cos_min = a.ref_cos_min, s.ref_tol2 = a.ref_tol2;
    for (int c = 0; c < 3; ++c) s.ref_normal[c] = a.ref_normal[c], s.ref_feat[c] = a.ref_feat[c];
    s.oriented = a.oriented, s.ref_flags = a.ref_flags;
    const PiecesWs w = carve_pieces(a.workspace_dev, n, 0, 1);
    const unsigned grid = capped_grid(n, kPiecesBlock, kPiecesMaxBlocks);
    k_similar_init<<<grid, kPiecesBlock, 0, st>>>(s, w, n);
    A3D_LAUNCH_CHECK();
    if (s.normal && s.feat)
      k_similar_hook<true, true><<<grid, kPiecesBlock, 0, st>>>(s, t, w.parent);
    else if (s.normal)
      k_similar_hook<true, false><<<grid, kPiecesBlock, 0, st>>>(s, t, w.parent);
    else if (s.feat)
      k_similar_hook<false, true><<<grid, kPiecesBlock, 0, st>>>(s, t, w.parent);
    else
      k_similar_hook<false, false><<<grid, kPiecesBlock, 0, st>>>(s, t, w.parent);
    A3D_LAUNCH_CHECK();
    k_pieces_flatten<<<grid, kPiecesBlock, 0, st>>>(w.parent, a.piece_qv_dev, n);
    A3D_LAUNCH_CHECK();
    k_pieces_stats<<<grid, kPiecesBlock, 0, st>>>(la, t, w);
    A3D_LAUNCH_CHECK();
    k_pieces_records<<<1, kPiecesScan, 0, st>>>(la, a.keys_dev, w, n);
    A3D_LAUNCH_CHECK();
  }
  if (a.n_full > 0) {
    k_pieces_full<<<capped_grid(a.n_full, kPiecesBlock, kPiecesMaxBlocks), kPiecesBlock, 0, st>>>(la, n);
    A3D_LAUNCH_CHECK();
  }
  return A3D_OK;
}

extern "C" size_t a3d_vote_workspace_bytes(int64_t n, int capacity, int n_classes) {
  if (n < 0 || n > 0x7fffffffll || capacity < 0 || n_classes < 1 || n_classes > 256) return 0;
  return carve_vote(nullptr, n, capacity, n_classes).bytes;
}

extern "C" int a3d_vote_pieces(const a3d_vote_pieces_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_vote_pieces: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_vote_pieces_args& a = *args;
  PiecesTab t;
  if (!pieces_tab(a.scene, a.n, 26, &t) || a.n_clicks < 0 || a.n_clicks > A3D_MAX_CLICKS || a.n_classes < 1 ||
      a.n_classes > 256 || a.capacity < 0 || a.min_voxels < 1 || a.share_num < 1 || a.share_num > a.share_den ||
      a.share_den > 65536 || !a.summary_dev ||
      (a.n > 0 && (!a.labels_dev || !a.piece_qv_dev || !a.labels_out_dev || !a.workspace_dev || a.labels_out_dev == a.labels_dev)) ||
      ((uintptr_t)a.workspace_dev & 255) || a.workspace_bytes < a3d_vote_workspace_bytes(a.n, a.capacity, a.n_classes)) {
    set_error("a3d_vote_pieces: bad arguments (n=%lld clicks=%d classes=%d capacity=%d min_voxels=%d share=%d/%d workspace=%zu)",
              (long long)a.n, a.n_clicks, a.n_classes, a.capacity, a.min_voxels, a.share_num, a.share_den, a.workspace_bytes);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.summary_dev, 0, sizeof(a3d_vote_summary), st));
  const int n = t.n;
  if (n > 0) {
    const VoteWs w = carve_vote(a.workspace_dev, n, a.capacity, a.n_classes);
    const unsigned grid = capped_grid(n, kPiecesBlock, kPiecesMaxBlocks);
    k_vote_scan<<<1, kPiecesScan, 0, st>>>(a, w, n);
    A3D_LAUNCH_CHECK();
    k_vote_clear<<<grid, kPiecesBlock, 0, st>>>(a, w);
    A3D_LAUNCH_CHECK();
    k_vote_count<<<grid, kPiecesBlock, 0, st>>>(a, w, n);
    A3D_LAUNCH_CHECK();
    k_vote_decide<<<grid, kPiecesBlock, 0, st>>>(a, w, n);
    A3D_LAUNCH_CHECK();
    k_vote_write<<<grid, kPiecesBlock, 0, st>>>(a, w, n);
    A3D_LAUNCH_CHECK();
  }
  return A3D_OK;
}
