// session_grow.hip -- a bounded shortest-path distance from a set of seed voxels over the voxel lattice, and which seed is
// nearest (gfx950).  One entry point: a3d_grow_voxels.  It is the primitive under "from here, 30 cm along the surface",
// under growing and shrinking a selection by a margin, and under splitting an object between its clicks.
//
// The reference has no counterpart: its tool selects nothing by distance.  THE RULE (ours, stated in include/agile3d_hip.h at
// the entry point): the nodes are the level-0 voxels in the CALLER's row order; an edge joins two neighbours under the
// connectivity (6 / 18 / 26, the offsets a3d_label_pieces admits) that hold the same key >= 0 and costs cost[|d|1 - 1]; the
// value of a voxel v is the lexicographic minimum of (d, s) over the seeds s with a path to v of cost d <= limit, s = the
// seed's caller row; dist = d, owner = s, both -1 where there is none.
//
// THE ADJACENCY is the scene's level-0 table A3D_TAB_NBR27 (int32 [27][npad], internal rows, a missing neighbour is n); both
// ends of an entry go through A3D_TAB_ORIGROW, so value[], the keys and every output are indexed by CALLER row.  Threads
// walk the INTERNAL (Morton) order: the 26 neighbours a wave touches lie near each other.
//
// ONE WORD.  (dist, owner) is held as dist << 32 | owner (none: all ones) and relaxed with a 64-bit atomicMin; comparing the
// words compares the pairs lexicographically, and adding cost << 32 keeps the owner (dist <= 2^30 and cost <= 2^16: nothing
// carries out of a half).  A RELAXATION of the edge u -> v is atomicMin(word[v], word[u] + cost) when that is within the limit.
// WHY THE RESULT IS ORDER-FREE.  Every word ever written is (the cost of a real walkable path from a seed s within the
// limit, s), so no word is ever below the rule's value T[v].  Words only decrease.  Consider a state in which no relaxation
// lowers anything, and suppose some v holds more than T[v] = (d, s).  Take a cheapest path from s to v and on it the first
// voxel w whose word is above T[w]; it is not s (a seed starts at (0, s), the least any word can be: every cost is >= 1), so
// it has a predecessor u on the path with word[u] = T[u].  T[u] is (d_u, s) with d_u the cost of the path up to u: were
// another seed nearer to u, or as near with a smaller row, it would be nearer to w as well, or as near with a smaller row,
// and the path would not be the one that gives T[w].  Relaxing u -> w would then lower w: a contradiction.  So the fixed
// point of "word[v] = min over walkable neighbours u of (dist[u] + cost, owner[u])" is unique and equal to T, a function of
// the arguments, whatever order the relaxations land in: two calls give the same bytes.
// A SWEEP is one thread per voxel, and only the FRONT works: stamp[r] (at the internal row) is the number of the sweep that
// last lowered the voxel (a seed: 0, nothing yet: -1), and in sweep k a voxel whose stamp is k - 1 -- or already k -- offers
// word + step to its walkable neighbours; where an offer lowers a neighbour (the atomicMin returned more than it offered)
// that neighbour is stamped k.  Every other thread reads its stamp and is done, so a sweep costs what its front costs and
// not what the scene holds.  EVERY LOWERING IS SPOKEN ONCE MORE: a voxel lowered in sweep m has stamp m (or later), so in
// sweep m + 1 it offers its word of then, which is no larger; a voxel lowered again while it speaks is stamped again and
// speaks again.  Hence a sweep that lowers nothing leaves no stamp for the next one and the state is the fixed point: the
// last word of every voxel has been offered to all its neighbours.
// TERMINATION WITHOUT ANYBODY WAITING.  A path of cost <= limit has at most S = limit / min(cost) edges.  After k sweeps
// every word is at most the least (d, s) over the paths of at most k edges: such a path ends in an edge u -> v behind a path of
// at most k - 1 edges, u took its word of the end of sweep k - 1 in some sweep m <= k - 1 (or is a seed, m = 0), and offered
// no more than that to v in sweep m + 1 <= k.  So S sweeps always suffice and the host launches exactly S (<=
// A3D_GROW_MAX_STEPS; the cheapest ADMITTED step counts), never reading the device in mid-call.  Most calls are done long
// before: each sweep raises flag[k] when it lowered anything, and sweep k + 1 reads flag[k] first and returns at once when it
// is clear (flag[k + 1] then stays clear too, and so on down the queue: 1.5 us a launch).  No grid barrier, no cooperative
// launch, no spin-wait: no thread waits for another.
// A SWEEP MAY RELAX CHAOTICALLY: reading a neighbour's newer word only helps, and a stale one is merely larger (the atomicMin
// decides, not the read before it, which only spares the atomics that cannot win).
// MEMORY VISIBILITY (as session_pieces.hip explains for parent[]): the XCDs' L2s are not coherent for plain accesses.  While
// other workgroups may be writing them, value[] and stamp[] are read with __hip_atomic_load(..., __ATOMIC_RELAXED,
// __HIP_MEMORY_SCOPE_AGENT) and written with atomics only (a stamp that is read stale is k - 1 or less where it is k: the
// voxel then speaks in sweep k + 1, as it must anyway).  The kernels behind a launch boundary (the lift) use plain loads.
// WHAT WAS MEASURED (profiles/grow_timing.txt, one MI355X): a sweep in which every voxel PULLED from its 26 neighbours, one
// loop with a test and a `continue` per load, took 20 us on 80 k voxels; so did the first pushing sweep written the same
// way, though nearly all its threads read one int: the front's threads ran 26 chains of dependent loads one after the other.
// The sweep below issues each stage's 26 loads together and takes 10 - 12 us.  Iterating a workgroup over its own rows
// 4 / 8 / 16 times per launch (the pulling sweep) cut the launches that did work to a quarter and less but made each as much
// dearer: 1.6 x slower at 5 steps, within 10 % at 100.  Not kept.
//
// SEEDS FROM VERTICES are scattered into a byte per voxel with a plain store of the constant 1: every writer stores the same
// value, so the race is benign.  So are the stores of 1 that raise a flag.
// THE LIFT AND THE SUMMARY are one streaming pass over the voxels and then the vertices: it decodes the words into dist_qv /
// owner_qv, writes selected_full / dist_full, and reduces the counts as the region kernels do -- registers, wave shuffles,
// LDS, ONE 64-bit atomic per workgroup and counter (none for a zero).  Few, fat workgroups (1024 threads, at most one per
// CU) for the reason recorded at a3d_select_vertices: the atomics of a call land on the same few addresses and are served one
// after the other.  Sums of integers and maxima do not depend on the order of arrival.
#include "session_device.h"

namespace a3d {

constexpr int kGrowBlock = 256;
constexpr int kGrowMaxBlocks = 2048;
constexpr int kGrowFat = 1024;                // the lift: FEW, FAT workgroups (see above) ...
constexpr int kGrowFatBlocks = 256;           // ... one per CU
constexpr unsigned long long kGrowNone = ~0ull;
static_assert(sizeof(a3d_grow_voxels_args) == 136 && sizeof(a3d_grow_summary) == 32, "lib.py: GrowVoxelsArgs, GrowSummary");

struct GrowWs {
  unsigned long long* value;   // [n] dist << 32 | owner at the caller row, kGrowNone: not reached
  uint8_t* seed;               // [n] 1 where a seed vertex lies in the voxel
  int32_t* flag;               // [A3D_GROW_MAX_STEPS + 1] flag[0]: there is a seed; flag[k]: sweep k lowered something
  int32_t* stamp;              // [n] at the INTERNAL row: the sweep that last lowered the voxel (a seed: 0), -1: none yet
  size_t zero_bytes, bytes;    // seed and flag are cleared together
};
static GrowWs carve_grow(void* base, long long n) {
  GrowWs w;
  Carver c{base};
  const size_t m = (size_t)(n > 0 ? n : 1);
  w.value = (unsigned long long*)c.take(m * 8);
  const size_t zero_from = c.off;
  w.seed = (uint8_t*)c.take(m);
  w.flag = (int32_t*)c.take((A3D_GROW_MAX_STEPS + 1) * sizeof(int32_t));
  w.zero_bytes = c.off - zero_from;
  w.stamp = (int32_t*)c.take(m * 4);
  w.bytes = c.off;
  return w;
}

struct GrowTab {
  const int32_t* nbr;          // [27][npad]
  const int32_t* orig;         // [n]
  int n, npad;
  int cost[3];
  int limit;
};

__device__ __forceinline__ unsigned long long value_now(const unsigned long long* value, int x) {
  return __hip_atomic_load(value + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// seed vertices -> a byte per voxel (every writer stores 1); an index outside the rows is ignored (the lift reports it)
__global__ __launch_bounds__(kGrowFat) void k_grow_scatter(const a3d_grow_voxels_args a, uint8_t* seed) {
  const long long stride = (long long)gridDim.x * kGrowFat;
  for (long long v = (long long)blockIdx.x * kGrowFat + threadIdx.x; v < a.n_full; v += stride) {
    if (a.seed_full_dev[v] == 0) continue;
    const long long row = a.inverse_map_dev ? a.inverse_map_dev[v] : v;
    if (row >= 0 && row < a.n) seed[row] = 1;
  }
}

__global__ __launch_bounds__(kGrowBlock) void k_grow_init(const int32_t* __restrict__ keys, const uint8_t* __restrict__ seed_qv,
                                                          const int32_t* __restrict__ orig, const GrowWs w, const int n) {
  const int stride = gridDim.x * kGrowBlock;
  bool any = false;
  for (int r = blockIdx.x * kGrowBlock + threadIdx.x; r < n; r += stride) {
    const int i = orig[r];
    const bool seed = (keys ? keys[i] : 0) >= 0 && ((seed_qv && seed_qv[i] != 0) || w.seed[i] != 0);
    w.value[i] = seed ? (unsigned long long)i : kGrowNone;             // (0, i): a seed owns itself
    w.stamp[r] = seed ? 0 : -1;
    any = any || seed;
  }
  if (any) w.flag[0] = 1;                                              // (every writer stores 1)
}

// ONE SWEEP.  Only the voxels lowered in the sweep before (or already in this one) do anything: each offers word + step to
// its walkable neighbours.  L1MAX = 1 / 2 / 3 for connectivity 6 / 18 / 26 and KEYS are compile-time, and the body is written
// in STAGES without a branch between the loads of a stage (the rows of the table, the callers' rows, the keys and the words,
// the atomics), so that a thread has all 26 of a stage in flight at once: written as one loop with a `continue` per test, the
// 26 dependent chains ran one after the other and a sweep over 80 k voxels took 20 us whatever it did (profiles/grow_timing.txt).
template <int L1MAX, bool KEYS>
__global__ __launch_bounds__(kGrowBlock) void k_grow_sweep(const int32_t* __restrict__ keys, const GrowTab t,
                                                           unsigned long long* value, int32_t* stamp,
                                                           const int32_t* __restrict__ before, int32_t* mine, const int sweep) {
  if (*before == 0) return;                                            // the sweep before lowered nothing: the fixed point
  const int stride = gridDim.x * kGrowBlock;
  const unsigned long long limit = (unsigned long long)(unsigned)t.limit;
  bool lowered = false;
  for (int r = blockIdx.x * kGrowBlock + threadIdx.x; r < t.n; r += stride) {
    if (__hip_atomic_load(stamp + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < sweep - 1) continue;
    const int i = t.orig[r];
    const int key = KEYS ? keys[i] : 0;
    const unsigned long long cur = value_now(value, i);
    if (cur == kGrowNone) continue;                                    // (a stamped voxel holds a word)
    int jr[27], j[27];
    unsigned long long cand[27], old[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      const int l1 = (k % 3 != 1) + ((k / 3) % 3 != 1) + (k / 9 != 1);
      if (l1 == 0 || l1 > L1MAX) continue;                             // (folded at compile time)
      jr[k] = t.nbr[(size_t)k * t.npad + r];
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      const int l1 = (k % 3 != 1) + ((k / 3) % 3 != 1) + (k / 9 != 1);
      if (l1 == 0 || l1 > L1MAX) continue;
      j[k] = t.orig[(unsigned)jr[k] < (unsigned)t.n ? jr[k] : r];     // a missing neighbour: this row itself, masked below
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      const int l1 = (k % 3 != 1) + ((k / 3) % 3 != 1) + (k / 9 != 1);
      if (l1 == 0 || l1 > L1MAX) continue;
      const int other = KEYS ? keys[j[k]] : 0;
      const unsigned long long now = value_now(value, j[k]);
      const unsigned long long c = cur + ((unsigned long long)(unsigned)t.cost[l1 - 1] << 32);
      const bool offer = (unsigned)jr[k] < (unsigned)t.n && other == key && (c >> 32) <= limit && c < now;
      cand[k] = offer ? c : kGrowNone;
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      const int l1 = (k % 3 != 1) + ((k / 3) % 3 != 1) + (k / 9 != 1);
      if (l1 == 0 || l1 > L1MAX) continue;
      old[k] = 0;                                                      // (nothing is below 0: no offer, nothing lowered)
      if (cand[k] != kGrowNone) old[k] = atomicMin(value + j[k], cand[k]);
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      const int l1 = (k % 3 != 1) + ((k / 3) % 3 != 1) + (k / 9 != 1);
      if (l1 == 0 || l1 > L1MAX) continue;
      if (cand[k] < old[k]) {                                          // THIS offer lowered the neighbour: it speaks in the next sweep
        __hip_atomic_store(stamp + jr[k], sweep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (every writer of this sweep stores it)
        lowered = true;
      }
    }
  }
  if (__any(lowered) && (threadIdx.x & 63) == 0) *mine = 1;            // (every writer stores 1)
}

// The words decoded, the lift, the summary: one streaming pass, behind a launch boundary (plain loads).
__global__ __launch_bounds__(kGrowFat) void k_grow_lift(const a3d_grow_voxels_args a, const unsigned long long* __restrict__ value) {
  __shared__ int wave_part[kGrowFat / 64];
  const long long stride = (long long)gridDim.x * kGrowFat;
  int n_seeds = 0, n_reached = 0, n_selected = 0, far = 0, bad = 0;    // (n, n_full < 2^31: a thread's share fits an int)
  for (long long i = (long long)blockIdx.x * kGrowFat + threadIdx.x; i < a.n; i += stride) {
    const unsigned long long w = value[i];
    const int d = w == kGrowNone ? -1 : (int)(w >> 32), s = w == kGrowNone ? -1 : (int)(w & 0xffffffffull);
    if (a.dist_qv_dev) a.dist_qv_dev[i] = d;
    if (a.owner_qv_dev) a.owner_qv_dev[i] = s;
    n_seeds += d == 0, n_reached += d >= 0, far = max(far, d);         // (dist 0 is a seed's alone: every cost is >= 1)
  }
  for (long long v = (long long)blockIdx.x * kGrowFat + threadIdx.x; v < a.n_full; v += stride) {
    const long long row = a.inverse_map_dev ? a.inverse_map_dev[v] : v;
    int d = -1;
    if (row < 0 || row >= a.n) {
      bad = 1;
    } else {
      const unsigned long long w = value[row];
      if (w != kGrowNone) d = (int)(w >> 32);
    }
    if (a.selected_full_dev) a.selected_full_dev[v] = d >= 0 ? 1 : 0;
    if (a.dist_full_dev) a.dist_full_dev[v] = d;
    n_selected += d >= 0;
  }
  const long long s_seeds = block_sum<kGrowFat>(n_seeds, wave_part), s_reached = block_sum<kGrowFat>(n_reached, wave_part);
  const long long s_selected = block_sum<kGrowFat>(n_selected, wave_part), s_bad = block_sum<kGrowFat>(bad, wave_part);
  const int m_far = block_max<kGrowFat>(far, wave_part);
  if (threadIdx.x == 0) {
    add_i64(&a.summary_dev->seeds, s_seeds);
    add_i64(&a.summary_dev->reached, s_reached);
    add_i64(&a.summary_dev->selected, s_selected);
    if (m_far > 0) atomicMax(&a.summary_dev->max_dist, m_far);
    if (s_bad) atomicOr(&a.summary_dev->err, A3D_GROW_BAD_INDEX);
  }
}

}  // namespace a3d

using namespace a3d;

extern "C" size_t a3d_grow_workspace_bytes(int64_t n) {
  if (n < 0 || n > 0x7fffffffll) return 0;
  return carve_grow(nullptr, n).bytes;
}

extern "C" int a3d_grow_voxels(const a3d_grow_voxels_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_grow_voxels: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_grow_voxels_args& a = *args;
  const a3d_scene* s = a.scene;
  const bool bad_scene = !scene_walkable(s, a.n);
  const bool bad_conn = a.connectivity != 6 && a.connectivity != 18 && a.connectivity != 26;
  int cheapest = 65536;
  bool bad_cost = false;
  for (int c = 0; c < 3; ++c) {
    bad_cost = bad_cost || a.cost[c] < 1 || a.cost[c] > 65536;
    if (a.cost[c] < cheapest) cheapest = a.cost[c];
  }
  const bool bad_limit = a.limit < 0 || a.limit > (1 << 30) || (!bad_cost && a.limit / cheapest > A3D_GROW_MAX_STEPS);
  if (bad_scene || bad_conn || bad_cost || bad_limit || (!a.seed_qv_dev && !a.seed_full_dev) || !a.summary_dev || a.n_full < 0 ||
      a.n_full > 0x7fffffffll || (a.n > 0 && !a.workspace_dev) || ((uintptr_t)a.workspace_dev & 255) ||
      a.workspace_bytes < a3d_grow_workspace_bytes(a.n)) {
    set_error("a3d_grow_voxels: bad arguments (scene %s, n=%lld connectivity=%d cost=%d,%d,%d limit=%d seeds %s summary %s "
              "n_full=%lld workspace=%zu)", s ? "given" : "NULL", (long long)a.n, a.connectivity, a.cost[0], a.cost[1], a.cost[2],
              a.limit, a.seed_qv_dev || a.seed_full_dev ? "given" : "absent", a.summary_dev ? "given" : "NULL",
              (long long)a.n_full, a.workspace_bytes);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.summary_dev, 0, sizeof(a3d_grow_summary), st));
  const int n = (int)a.n;
  GrowWs w = carve_grow(a.workspace_dev, n);
  if (n > 0) {
    A3D_HIP_CHECK(hipMemsetAsync(w.seed, 0, w.zero_bytes, st));        // the seed bytes and the flags
    if (a.seed_full_dev && a.n_full > 0) {
      k_grow_scatter<<<capped_grid(a.n_full, kGrowFat, kGrowFatBlocks), kGrowFat, 0, st>>>(a, w.seed);
      A3D_LAUNCH_CHECK();
    }
    const unsigned grid = capped_grid(n, kGrowBlock, kGrowMaxBlocks);
    k_grow_init<<<grid, kGrowBlock, 0, st>>>(a.keys_dev, a.seed_qv_dev, s->orig_row, w, n);
    A3D_LAUNCH_CHECK();
    GrowTab t;
    t.nbr = s->lv[0].nbr27, t.orig = s->orig_row, t.n = n, t.npad = s->lv[0].npad;
    for (int c = 0; c < 3; ++c) t.cost[c] = a.cost[c];
    t.limit = a.limit;
    // a cost no admitted offset uses does not shorten the bound: S counts the edges of the cheapest ADMITTED offset
    int admitted = a.cost[0];
    if (a.connectivity >= 18 && a.cost[1] < admitted) admitted = a.cost[1];
    if (a.connectivity == 26 && a.cost[2] < admitted) admitted = a.cost[2];
    const int sweeps = a.limit / admitted;                             // <= limit / min(cost) <= A3D_GROW_MAX_STEPS
    const bool with_keys = a.keys_dev != nullptr;
    for (int k = 1; k <= sweeps; ++k) {
#define A3D_GROW_SWEEP(L1MAX, KEYS) \
  k_grow_sweep<L1MAX, KEYS><<<grid, kGrowBlock, 0, st>>>(a.keys_dev, t, w.value, w.stamp, w.flag + k - 1, w.flag + k, k)
      if (a.connectivity == 6) {
        if (with_keys) A3D_GROW_SWEEP(1, true); else A3D_GROW_SWEEP(1, false);
      } else if (a.connectivity == 18) {
        if (with_keys) A3D_GROW_SWEEP(2, true); else A3D_GROW_SWEEP(2, false);
      } else {
        if (with_keys) A3D_GROW_SWEEP(3, true); else A3D_GROW_SWEEP(3, false);
      }
#undef A3D_GROW_SWEEP
      A3D_LAUNCH_CHECK();
    }
  }
  if (n > 0 || a.n_full > 0) {
    const long long longest = a.n_full > n ? a.n_full : n;
    k_grow_lift<<<capped_grid(longest, kGrowFat, kGrowFatBlocks), kGrowFat, 0, st>>>(a, w.value);
    A3D_LAUNCH_CHECK();
  }
  return A3D_OK;
}
