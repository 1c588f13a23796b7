// session_planes.hip -- the few global planes a scan is made of (floor, ceiling, walls, table tops), their equations and the
// voxels on each (gfx950).  Entry points: a3d_planes_workspace_bytes, a3d_find_planes.
//
// The reference has no counterpart.  THE RULE is stated in full in include/agile3d_hip.h and restated in tests/planes_rule.py;
// in short: every admitted row votes for ONE bin of a Hough array H[axis][iu][iv][k] -- the direction cell found by exact
// comparisons against dyadic boundaries, the offset bin by an integer dot product with the HOST's table of cell-centre
// directions and a floor division; INTEGER atomics, so the votes have no order.  Then rounds: the peak of the votes smoothed
// over the offset only (a packed 64-bit atomic max of (score, ~bin): the highest score, of equals the lowest bin), the integer
// sums of the seeds, the solve of a3d_estimate_normals (session_solve.h), two refits from the integer sums of the inliers, the
// final inlier pass, and either a record (the inliers leave H and the remaining rows) or a spent round (the seeds leave).
// Every test a row passes or fails is exact (int64, or doubles that hold exact products), every sum over rows is of integers,
// and the double arithmetic that is left runs in ONE thread in a fixed order: two calls give the same bytes.
//
// THE SHAPE.  Stages are launches, ordered by the stream: no grid barrier, no spin-wait.  A round is ten launches -- k_peak,
// k_plane_sums (seeds), k_plane_step, three times k_plane_sums (inliers) + k_plane_step, k_plane_assign -- and the host
// enqueues 2 max_planes rounds without reading anything back: PlaneState.done, set by k_plane_step, turns what follows into
// no-ops.  The row kernels walk the rows grid-stride from few, fat workgroups (256 x 256: one per CU), because each ends in
// ONE 64-bit atomic per workgroup and value (ten values in k_plane_sums); k_plane_step is one thread: a solve is ~600 fp64
// operations, and a round has four.  Per row the workspace keeps its bin (-1: not admitted, or removed) and its fixed-point
// position (three int32: |X| <= 2^20), so a pass reads 16 bytes a row and the normal only where the bin says "remaining".
// The library allocates nothing and does not synchronise.
#include "session_solve.h"

namespace a3d {

constexpr int kPlG = A3D_PLANES_GRID, kPlD = A3D_PLANES_BINS, kPlCells = 3 * kPlG * kPlG;
constexpr int kPlBinsAll = kPlCells * kPlD;   // 786432 votes: 3 MB
constexpr int kPlB = 256;                     // every kernel's workgroup
constexpr int kPlRowBlocks = 256;             // the row kernels: at most one workgroup per CU
constexpr int kPlPeakBlocks = 1024;           // k_peak
constexpr int kPlMaxRounds = 2 * A3D_PLANES_MAX;
constexpr long long kPlMaxUnits = 1ll << 44;  // bin_width, dist_tol
static_assert(sizeof(a3d_plane) == 136 && sizeof(a3d_planes_summary) == 48 && sizeof(a3d_planes_out) == 2224 &&
              sizeof(a3d_find_planes_args) == 168, "lib.py: Plane, PlanesSummary, PlanesOut, FindPlanesArgs");

struct PlaneState {
  u64 peak[kPlMaxRounds];      // per round: score << 32 | ~bin
  u64 sums[10];                // cnt, X, Y, Z, XX, XY, XZ, YY, YZ, ZZ of the pass just run (two's complement)
  long long off;               // the fit: N . X = off
  int N[3];
  float normal[3];
  int done;                    // the call has ended: every later launch returns at once
  int valid;                   // the round's current fit is one
  int bin, score;              // the round's peak
  int assign;                  // round + 1 whose k_plane_assign is due
  int record;                  // ... 1: the inliers become plane `id`, 0: the seeds are spent
  int id;
};

struct PlanesWs {
  int32_t* bin;                // [n]
  int32_t* X;                  // [n][3]
  int32_t* H;                  // [kPlBinsAll]
  PlaneState* state;
  size_t zero_bytes, bytes;    // H and state are cleared together
};
static PlanesWs carve_planes(void* base, long long n) {
  PlanesWs w;
  Carver c{base};
  const size_t m = (size_t)(n > 0 ? n : 1);
  w.H = (int32_t*)c.take((size_t)kPlBinsAll * 4);
  w.state = (PlaneState*)c.take(sizeof(PlaneState));
  w.zero_bytes = c.off;
  w.bin = (int32_t*)c.take(m * 4);
  w.X = (int32_t*)c.take(m * 12);
  w.bytes = c.off;
  return w;
}

// The sum of v over the workgroup, in thread 0 (session_device.h's block_sum for 64-bit values).
__device__ __forceinline__ long long block_sum64(long long v, long long* wave_part) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kPlB / 64; ++w) s += wave_part[w];
  return s;
}

// iu of the header: the number of boundaries t_j = (j - G/2) / (G/2), j = 1..G-1, with nb >= t_j * na (exact in double)
__device__ __forceinline__ int direction_index(const double nb, const double na) {
#pragma clang fp contract(off)
  int iu = 0;
#pragma unroll
  for (int j = 1; j < kPlG; ++j) iu += nb >= ((double)(j - kPlG / 2) * (2.0 / kPlG)) * na;
  return iu;
}

// ---- votes ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlB) void k_plane_vote(const a3d_find_planes_args a, const PlanesWs w, const double lim) {
  __shared__ int wave_part[kPlB / 64];
  const long long stride = (long long)gridDim.x * kPlB;
  int admitted = 0, out[5] = {0, 0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * kPlB + threadIdx.x; i < a.n; i += stride) {
    a.plane_qv_dev[i] = -1;
    int bin = -1, reason = -1;
    long long X[3] = {0, 0, 0};
    if (a.candidate_dev && a.candidate_dev[i] == 0) {
      reason = A3D_PLANES_OUT_CANDIDATE;
    } else {
      float v[3] = {a.normal_dev[3 * i], a.normal_dev[3 * i + 1], a.normal_dev[3 * i + 2]};
      const float p[3] = {a.pos_dev[3 * i], a.pos_dev[3 * i + 1], a.pos_dev[3 * i + 2]};
      if (!(finite3(v[0], v[1], v[2]) && finite3(p[0], p[1], p[2]))) {
        reason = A3D_PLANES_OUT_NONFINITE;
      } else if (v[0] == 0.f && v[1] == 0.f && v[2] == 0.f) {
        reason = A3D_PLANES_OUT_ZERO;
      } else {
        const bool f0 = fixed_point(p[0], a.origin[0], a.quantum, lim, X[0]), f1 = fixed_point(p[1], a.origin[1], a.quantum, lim, X[1]),
                   f2 = fixed_point(p[2], a.origin[2], a.quantum, lim, X[2]);
        if (!(f0 && f1 && f2)) {
          reason = A3D_PLANES_OUT_FRAME;
        } else {
          int ax = 0;
          if (fabsf(v[1]) > fabsf(v[ax])) ax = 1;
          if (fabsf(v[2]) > fabsf(v[ax])) ax = 2;
          const float sign = v[ax] < 0.f ? -1.f : 1.f;
          const double na = (double)(sign * v[ax]), nb = (double)(sign * v[(ax + 1) % 3]), nc = (double)(sign * v[(ax + 2) % 3]);
          const int cell = (ax * kPlG + direction_index(nb, na)) * kPlG + direction_index(nc, na);
          const int32_t* C = a.table_dev + 3 * cell;
          const long long d = (long long)C[0] * X[0] + (long long)C[1] * X[1] + (long long)C[2] * X[2];
          long long q = d / a.bin_width;
          if (d % a.bin_width < 0) --q;        // floor
          const long long k = q + kPlD / 2;
          if (k < 0 || k >= kPlD)
            reason = A3D_PLANES_OUT_BINS;
          else
            bin = cell * kPlD + (int)k;
        }
      }
    }
    w.bin[i] = bin;
    w.X[3 * i] = (int32_t)X[0], w.X[3 * i + 1] = (int32_t)X[1], w.X[3 * i + 2] = (int32_t)X[2];
    if (bin >= 0) {
      atomicAdd(w.H + bin, 1);
      ++admitted;
    } else {
#pragma unroll
      for (int r = 0; r < 5; ++r) out[r] += reason == r;
    }
  }
  a3d_planes_summary* s = &a.out_dev->summary;
  const long long s_adm = block_sum<kPlB>(admitted, wave_part);
  if (threadIdx.x == 0 && s_adm) atomicAdd(&s->admitted, (int)s_adm);
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const long long s_out = block_sum<kPlB>(out[r], wave_part);
    if (threadIdx.x == 0 && s_out) atomicAdd(&s->left_out[r], (int)s_out);
  }
}

// ---- the peak -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlB) void k_plane_peak(const int32_t* __restrict__ H, PlaneState* st, const int round) {
  __shared__ u64 wave_best[kPlB / 64];
  if (st->done) return;
  u64 best = 0;
  const int stride = gridDim.x * kPlB;
  for (int b = blockIdx.x * kPlB + threadIdx.x; b < kPlBinsAll; b += stride) {
    const int k = b & (kPlD - 1);
    const int below = k > 0 ? H[b - 1] : 0, above = k < kPlD - 1 ? H[b + 1] : 0;
    const u64 key = (u64)(unsigned)(below + H[b] + above) << 32 | (u64)(~(unsigned)b);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const u64 other = __shfl_xor(best, o);
    best = other > best ? other : best;
  }
  if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int wv = 1; wv < kPlB / 64; ++wv) best = wave_best[wv] > best ? wave_best[wv] : best;
    atomicMax(&st->peak[round], best);
  }
}

// ---- which rows a pass means ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_seed(const int bin, const int peak_bin) {
  return bin >= 0 && bin / kPlD == peak_bin / kPlD && bin - peak_bin >= -1 && bin - peak_bin <= 1;
}
struct PlaneFit {
  double n[3], cos_min;
  long long N[3], off, tol;
};
__device__ __forceinline__ PlaneFit load_fit(const PlaneState* st, const a3d_find_planes_args& a) {
  PlaneFit f;
#pragma unroll
  for (int k = 0; k < 3; ++k) f.n[k] = (double)st->normal[k], f.N[k] = st->N[k];
  f.off = st->off, f.tol = a.dist_tol, f.cos_min = a.cos_min;
  return f;
}
__device__ __forceinline__ bool is_inlier(const PlaneFit& f, const int bin, const float* __restrict__ v, const int32_t* __restrict__ X) {
#pragma clang fp contract(off)
  if (bin < 0) return false;
  const double dot = (f.n[0] * (double)v[0] + f.n[1] * (double)v[1]) + f.n[2] * (double)v[2];
  const long long e = (f.N[0] * X[0] + f.N[1] * X[1] + f.N[2] * X[2]) - f.off;
  return fabs(dot) >= f.cos_min && (e < 0 ? -e : e) <= f.tol;
}

// the integer sums of the seeds (seeds != 0) or of the current fit's inliers, into st->sums
__global__ __launch_bounds__(kPlB) void k_plane_sums(const a3d_find_planes_args a, const PlanesWs w, const int round, const int seeds,
                                                     const int stop) {
  __shared__ long long wave_part[kPlB / 64];
  PlaneState* st = w.state;
  if (st->done) return;
  int peak_bin = 0;
  PlaneFit f = {};
  if (seeds) {
    const u64 peak = st->peak[round];
    if ((int)(peak >> 32) < stop) return;       // (k_plane_step ends the call)
    peak_bin = (int)~(unsigned)peak;
  } else {
    if (!st->valid) return;
    f = load_fit(st, a);
  }
  long long acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const long long stride = (long long)gridDim.x * kPlB;
  for (long long i = (long long)blockIdx.x * kPlB + threadIdx.x; i < a.n; i += stride) {
    const int bin = w.bin[i];
    if (bin < 0) continue;
    const int32_t* Xi = w.X + 3 * i;
    if (!(seeds ? is_seed(bin, peak_bin) : is_inlier(f, bin, a.normal_dev + 3 * i, Xi))) continue;
    const long long X = Xi[0], Y = Xi[1], Z = Xi[2];
    acc[0] += 1, acc[1] += X, acc[2] += Y, acc[3] += Z;
    acc[4] += X * X, acc[5] += X * Y, acc[6] += X * Z, acc[7] += Y * Y, acc[8] += Y * Z, acc[9] += Z * Z;
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const long long s = block_sum64(acc[k], wave_part);
    if (threadIdx.x == 0 && s) atomicAdd(&st->sums[k], (u64)s);
  }
}

// ---- one thread between the passes: the stop test, the fits, the record -----------------------------------------------------
__device__ inline long long floor_div(const long long x, const long long y) {      // y > 0
  long long q = x / y;
  if (x % y < 0) --q;
  return q;
}

// stage 0: after the seeds' sums; 1, 2: after an inlier pass (a refit); 3: after the final inlier pass (record or spent)
__global__ __launch_bounds__(64) void k_plane_step(const a3d_find_planes_args a, PlaneState* st, const int round, const int stage,
                                                   const int stop) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0 || st->done) return;
  a3d_planes_summary* sum = &a.out_dev->summary;
  if (stage == 0) {
    const u64 peak = st->peak[round];
    if ((int)(peak >> 32) < stop) {
      st->done = 1;
      return;
    }
    st->score = (int)(peak >> 32), st->bin = (int)~(unsigned)peak, st->valid = 1;
  }
  u64 T[10];
  for (int k = 0; k < 10; ++k) T[k] = st->sums[k], st->sums[k] = 0;
  const long long cnt = (long long)T[0];
  if (stage < 3) {
    if (!st->valid) return;
    float normal[3], variation;
    const a3d_estimate_normals_args none = {};   // no viewpoint: the canonical sign
    if (!nrm_solve(cnt, T + 1, T + 4, none, normal, variation)) {
      st->valid = 0;
      return;
    }
    long long N[3], NR = 0, Ns = 0;
    for (int k = 0; k < 3; ++k) {
      N[k] = llrint((double)normal[k] * 1048576.0);
      const long long S = (long long)T[1 + k], R = floor_div(S, cnt);
      NR += N[k] * R, Ns += N[k] * (S - cnt * R);
      st->normal[k] = normal[k], st->N[k] = (int)N[k];
    }
    st->off = NR + floor_div(Ns, cnt);
    return;
  }
  // the end of the round
  const bool record = st->valid && cnt >= a.min_voxels;
  st->assign = round + 1, st->record = record, st->id = sum->n_planes;
  sum->rounds += 1;
  if (!record) {
    sum->spent += 1;
    return;
  }
  a3d_plane* p = &a.out_dev->plane[sum->n_planes];
  const long long off = st->off;
  const __int128 N0 = st->N[0], N1 = st->N[1], N2 = st->N[2];
  const __int128 S0 = (long long)T[1], S1 = (long long)T[2], S2 = (long long)T[3];
  const __int128 Mxx = (long long)T[4], Mxy = (long long)T[5], Mxz = (long long)T[6], Myy = (long long)T[7], Myz = (long long)T[8],
                 Mzz = (long long)T[9];
  const __int128 NS = N0 * S0 + N1 * S1 + N2 * S2;
  const __int128 NMN = N0 * N0 * Mxx + N1 * N1 * Myy + N2 * N2 * Mzz + 2 * (N0 * N1 * Mxy + N0 * N2 * Mxz + N1 * N2 * Myz);
  const __int128 E = NMN - 2 * (__int128)off * NS + (__int128)cnt * off * off;      // the sum of (N . X - off)^2: >= 0
  const u64 hi = (u64)((unsigned __int128)E >> 64), lo = (u64)E;
  const double Ed = (double)hi * 18446744073709551616.0 + (double)lo;
  const double unit = a.quantum * (1.0 / 1048576.0);
  double n[3];
  for (int k = 0; k < 3; ++k) n[k] = (double)st->normal[k], p->normal[k] = st->normal[k], p->N[k] = st->N[k];
  p->offset = (float)(((n[0] * a.origin[0] + n[1] * a.origin[1]) + n[2] * a.origin[2]) + (double)off * unit);
  p->rms = (float)(sqrt(Ed / (double)cnt) * unit);
  p->inliers = (int)cnt, p->score = st->score, p->round = round, p->bin = st->bin;
  p->count = cnt, p->off = off;
  for (int k = 0; k < 3; ++k) p->sum[k] = (long long)T[1 + k];
  for (int k = 0; k < 6; ++k) p->mom[k] = (long long)T[4 + k];
  sum->n_planes += 1;
  if (sum->n_planes >= a.max_planes) st->done = 1;
}

// the round's rows leave: the inliers with their plane's id, or the seeds with nothing
__global__ __launch_bounds__(kPlB) void k_plane_assign(const a3d_find_planes_args a, const PlanesWs w, const int round) {
  const PlaneState* st = w.state;
  if (st->assign != round + 1) return;
  const int record = st->record, id = st->id, peak_bin = st->bin;
  const PlaneFit f = load_fit(st, a);
  const long long stride = (long long)gridDim.x * kPlB;
  for (long long i = (long long)blockIdx.x * kPlB + threadIdx.x; i < a.n; i += stride) {
    const int bin = w.bin[i];
    if (bin < 0) continue;
    if (!(record ? is_inlier(f, bin, a.normal_dev + 3 * i, w.X + 3 * i) : is_seed(bin, peak_bin))) continue;
    if (record) a.plane_qv_dev[i] = id;
    atomicSub(w.H + bin, 1);
    w.bin[i] = -1;
  }
}

// plane_full[j] = plane_qv[inverse_map[j]]; an index outside 0 .. n-1 is flagged and not followed
__global__ __launch_bounds__(kPlB) void k_plane_lift(const a3d_find_planes_args a) {
  const long long stride = (long long)gridDim.x * kPlB;
  int err = 0;
  for (long long j = (long long)blockIdx.x * kPlB + threadIdx.x; j < a.n_full; j += stride) {
    const long long v = a.inverse_map_dev[j];
    if (v < 0 || v >= a.n) {
      err = A3D_PLANES_BAD_INDEX;
      continue;
    }
    a.plane_full_dev[j] = a.plane_qv_dev[v];
  }
  send_error(&a.out_dev->summary.err, err);
}

}  // namespace a3d

using namespace a3d;

extern "C" size_t a3d_planes_workspace_bytes(int64_t n) {
  if (n < 0 || n > 0x7fffffffll) return 0;
  return carve_planes(nullptr, n).bytes;
}

extern "C" int a3d_find_planes(const a3d_find_planes_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_find_planes: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_find_planes_args& a = *args;
  const bool bits_ok = a.bits >= 0 && a.bits <= A3D_MEASURE_MAX_BITS;
  const bool sums_ok = bits_ok && a.n >= 0 && a.n < (1ll << 31) && a.n <= ((1ll << 62) >> (2 * a.bits));
  bool frame_ok = power_of_two(a.quantum);
  for (int k = 0; k < 3; ++k) frame_ok = frame_ok && std::isfinite(a.origin[k]);
  const bool lift = a.inverse_map_dev != nullptr;
  const bool settings_ok = a.bin_width >= 1 && a.bin_width <= kPlMaxUnits && a.dist_tol >= 0 && a.dist_tol <= kPlMaxUnits &&
                           a.cos_min >= 0.0 && a.cos_min <= 1.0 && a.min_voxels >= 1 && a.max_planes >= 1 &&
                           a.max_planes <= A3D_PLANES_MAX;                     // (a NaN cos_min fails the first comparison)
  const bool lift_ok = a.n_full >= 0 && a.n_full < (1ll << 31) &&
                       (lift ? a.n_full == 0 || a.plane_full_dev != nullptr : a.n_full == 0 && !a.plane_full_dev);
  if (!sums_ok || !frame_ok || !settings_ok || !lift_ok || (a.n > 0 && (!a.normal_dev || !a.pos_dev || !a.plane_qv_dev)) ||
      !a.table_dev || !a.out_dev || ((uintptr_t)a.out_dev & 7) || !a.workspace_dev || ((uintptr_t)a.workspace_dev & 255) ||
      a.workspace_bytes < a3d_planes_workspace_bytes(a.n)) {
    set_error("a3d_find_planes: bad arguments (n=%lld n_full=%lld bits=%d quantum=%g bin_width=%lld dist_tol=%lld cos_min=%g "
              "min_voxels=%d max_planes=%d normal %s pos %s table %s plane_qv %s inverse_map %s plane_full %s out %s workspace=%zu; a "
              "finite origin, 1 <= bin_width and 0 <= dist_tol <= 2^44, cos_min in [0, 1], min_voxels >= 1, 1 <= max_planes <= %d, "
              "out 8-byte aligned, plane_full and n_full exactly with inverse_map are needed)", (long long)a.n, (long long)a.n_full,
              a.bits, a.quantum, (long long)a.bin_width, (long long)a.dist_tol, a.cos_min, a.min_voxels, a.max_planes,
              a.normal_dev ? "given" : "NULL", a.pos_dev ? "given" : "NULL", a.table_dev ? "given" : "NULL",
              a.plane_qv_dev ? "given" : "NULL", lift ? "given" : "NULL", a.plane_full_dev ? "given" : "NULL",
              a.out_dev ? "given" : "NULL", a.workspace_bytes, A3D_PLANES_MAX);
    return A3D_ERR_INVALID;
  }
  const PlanesWs w = carve_planes(a.workspace_dev, a.n);
  A3D_HIP_CHECK(hipMemsetAsync(a.out_dev, 0, sizeof(a3d_planes_out), st));
  A3D_HIP_CHECK(hipMemsetAsync(w.H, 0, w.zero_bytes, st));
  if (a.n > 0) {
    const unsigned rows = capped_grid(a.n, kPlB, kPlRowBlocks);
    const int stop = a.min_voxels / 4 > 3 ? a.min_voxels / 4 : 3;
    k_plane_vote<<<rows, kPlB, 0, st>>>(a, w, std::ldexp(1.0, a.bits));
    A3D_LAUNCH_CHECK();
    for (int round = 0; round < 2 * a.max_planes; ++round) {
      k_plane_peak<<<capped_grid(kPlBinsAll, kPlB, kPlPeakBlocks), kPlB, 0, st>>>(w.H, w.state, round);
      A3D_LAUNCH_CHECK();
      for (int stage = 0; stage < 4; ++stage) {
        k_plane_sums<<<rows, kPlB, 0, st>>>(a, w, round, stage == 0, stop);
        A3D_LAUNCH_CHECK();
        k_plane_step<<<1, 64, 0, st>>>(a, w.state, round, stage, stop);
        A3D_LAUNCH_CHECK();
      }
      k_plane_assign<<<rows, kPlB, 0, st>>>(a, w, round);
      A3D_LAUNCH_CHECK();
    }
  }
  if (lift && a.n_full > 0) {
    k_plane_lift<<<capped_grid(a.n_full, kPlB, kPlRowBlocks), kPlB, 0, st>>>(a);
    A3D_LAUNCH_CHECK();
  }
  return A3D_OK;
}
