// session.hip -- the headless interactive session around forward_mask: exact nearest rows, ray picking (vertices of a point
// cloud, surfaces of a triangle mesh) and the full-resolution paint pass (gfx950).
//
// Replaces (reference file:line):
//   find_nearest (torch.cdist over all voxel rows, again over all vertices)   interactive_tool/utils.py:27-29, gui.py:273-274
//   "render a depth image and unproject" (Open3D's renderer)                  gui.py:247-271   -> k_pick_ray (point clouds) and
//                                                                             k_pick_mesh (triangle meshes), rules of OURS
//   pred[inverse_map], get_colors, the click cubes                            interactive_segmentation_user.py:83-84,125-140, gui.py:276-298,327
//
// All four are streaming passes over 12-byte rows, memory bound, no MFMA.  Nothing here uses an atomic on a result: every
// search is a minimum over a packed integer key whose order is total (distance bits, then row), reduced per wave with
// shuffles, per workgroup through LDS, and over the workgroups by ONE second-stage block -- the result does not depend on
// the order in which workgroups finish.  The tables of a call (sources, queries, ray) travel by value in the kernel
// arguments; the library allocates nothing, the caller brings a3d_session_workspace_bytes() of scratch.
//
// THE PICK RULE (ours: the reference delegates picking to Open3D's depth render).  Ray (o, d), |d| = 1, radius r: among the
// points p with t = (p - o) . d > 0 and |(p - o) - t d| <= r the one with the smallest t; ties -> the smaller perpendicular
// distance, then the lower index; none -> -1 ("clicked on nothing", gui.py:265).
//
// THE MESH PICK RULE (ours as well).  Ray (o, d), faces int32 [m][3] into the same vertex rows: the first SURFACE the ray
// meets -- among the faces the ray crosses at a finite t > 0 the one with the smallest t, ties -> the lower face index; none
// -> -1.  Faces are double-sided, edges inclusive.  The crossing test is the watertight one of Woop, Benthin and Wald
// ("Watertight Ray/Triangle Intersection", JCGT 2013): vertices translated by the origin, axes permuted so that the ray's
// dominant axis is z, sheared so that the ray becomes the z axis, then the three 2-D edge functions of the sheared x/y.  An
// edge function is f(P, Q) = Qx Py - Qy Px of ITS two endpoints only; with every product and the difference rounded on its
// own (no fma) f(P, Q) = -f(Q, P) exactly, so two faces that share an edge see the ray on opposite sides of it or both on
// it, never both outside: no ray passes between them.  A function that comes out exactly 0 is recomputed in double (exact
// products, one rounding), as in the paper.  Skipped, never an error: det == 0, a repeated index, a NaN, an index outside
// [0, n) (which also sets bit 0 of the result's flags).
#include "common.h"

namespace a3d {

constexpr int kSesBlock = 256;
constexpr int kSesMaxBlocks = 256;            // first-stage workgroups per source (one per CU; they walk the rows grid-stride)
constexpr int kSesQT = 8;                     // queries a first-stage thread serves (its keys stay in registers)
constexpr unsigned long long kNoKey = ~0ull;

// THE distance of every stage and every caller of this file: (x-qx)^2 + (y-qy)^2 + (z-qz)^2 in fp32 from the differences,
// the squares added in x, y, z order.  Contraction to fma is NOT allowed (hipcc contracts by default): each product and sum is
// rounded on its own, so the value is the one a plain fp32 restatement (numpy float32, one operation at a time) gives, bit
// for bit, and does not depend on how the compiler schedules the surrounding loop.
__device__ __forceinline__ float ses_dist2(float x, float y, float z, float qx, float qy, float qz) {
#pragma clang fp contract(off)
  const float dx = x - qx, dy = y - qy, dz = z - qz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return (xx + yy) + zz;
}
// bits of a non-negative float order like the float: (bits << 32) | row is smallest for the smallest distance, lowest row
__device__ __forceinline__ unsigned long long ses_key(float d2, unsigned row) {
  return ((unsigned long long)__float_as_uint(d2) << 32) | row;
}
__device__ __forceinline__ unsigned long long ses_wave_min(unsigned long long k) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(k, o);
    k = other < k ? other : k;
  }
  return k;
}
// the 96-bit key of the pick: (t bits, perpendicular distance^2 bits), then the row
struct PickKey {
  unsigned long long a;
  unsigned row;
};
__device__ __forceinline__ PickKey pick_min(const PickKey x, const PickKey y) {
  return (y.a < x.a || (y.a == x.a && y.row < x.row)) ? y : x;
}
__device__ __forceinline__ PickKey pick_wave_min(PickKey k) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    PickKey other;
    other.a = __shfl_xor(k.a, o);
    other.row = __shfl_xor(k.row, o);
    k = pick_min(k, other);
  }
  return k;
}

// ---- nearest rows: m queries against up to A3D_NEAREST_MAX_SOURCES row sets in one launch pair -----------------------------
struct NearestTab {
  int n_src, m;
  const float* xyz[A3D_NEAREST_MAX_SOURCES];
  long long n[A3D_NEAREST_MAX_SOURCES];
  int32_t* out[A3D_NEAREST_MAX_SOURCES];
  int n_blocks[A3D_NEAREST_MAX_SOURCES];      // first-stage workgroups that serve this source (the grid is sized for the largest)
  float q[A3D_NEAREST_MAX_QUERIES * 3];
};
// partial[(source * MAX_QUERIES + query) * kSesMaxBlocks + workgroup]
__global__ __launch_bounds__(kSesBlock) void k_nearest_rows(const NearestTab t, unsigned long long* __restrict__ partial) {
  const int s = blockIdx.y, q0 = blockIdx.z * kSesQT;
  if ((int)blockIdx.x >= t.n_blocks[s]) return;   // a workgroup beyond this source's share: nothing to read, nothing the finish reads
  const float* __restrict__ xyz = t.xyz[s];
  const long long n = t.n[s];
  float qx[kSesQT], qy[kSesQT], qz[kSesQT];
  unsigned long long best[kSesQT];
#pragma unroll
  for (int u = 0; u < kSesQT; ++u) {
    const int q = min(q0 + u, t.m - 1);       // (a tile's spare slots repeat the last query; they are not written)
    qx[u] = t.q[3 * q], qy[u] = t.q[3 * q + 1], qz[u] = t.q[3 * q + 2];
    best[u] = kNoKey;
  }
  const long long stride = (long long)t.n_blocks[s] * kSesBlock;   // this source's workgroups walk its rows between them
  for (long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x; i < n; i += stride) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];   // a wave reads 768 contiguous bytes
#pragma unroll
    for (int u = 0; u < kSesQT; ++u) {
      const unsigned long long k = ses_key(ses_dist2(x, y, z, qx[u], qy[u], qz[u]), (unsigned)i);
      best[u] = k < best[u] ? k : best[u];
    }
  }
  __shared__ unsigned long long sm[kSesBlock / 64][kSesQT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int u = 0; u < kSesQT; ++u) {
    const unsigned long long k = ses_wave_min(best[u]);
    if (lane == 0) sm[wv][u] = k;
  }
  __syncthreads();
  if (threadIdx.x < kSesQT && q0 + (int)threadIdx.x < t.m) {
    unsigned long long k = sm[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kSesBlock / 64; ++w) k = sm[w][threadIdx.x] < k ? sm[w][threadIdx.x] : k;
    partial[((size_t)s * A3D_NEAREST_MAX_QUERIES + q0 + threadIdx.x) * kSesMaxBlocks + blockIdx.x] = k;
  }
}
// second stage, one block: wave w folds the workgroups' keys of the (source, query) pairs w, w + 4, ...
__global__ __launch_bounds__(kSesBlock) void k_nearest_finish(const NearestTab t, const unsigned long long* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int p = wv; p < t.n_src * t.m; p += kSesBlock / 64) {
    const int s = p / t.m, q = p - s * t.m;
    const int n_blocks = t.n_blocks[s];
    const unsigned long long* row = partial + ((size_t)s * A3D_NEAREST_MAX_QUERIES + q) * kSesMaxBlocks;
    unsigned long long k = kNoKey;
    for (int j = lane; j < n_blocks; j += 64) k = row[j] < k ? row[j] : k;
    k = ses_wave_min(k);
    if (lane == 0) t.out[s][q] = k == kNoKey ? -1 : (int32_t)(unsigned)(k & 0xffffffffu);
  }
}

// ---- ray pick ------------------------------------------------------------------------------------------------------------
struct PickTab {
  const float* xyz;
  long long n;
  float o[3], d[3];
  float r2;
  a3d_pick_result* out;
};
__global__ __launch_bounds__(kSesBlock) void k_pick_ray(const PickTab t, unsigned long long* __restrict__ part_a,
                                                        unsigned* __restrict__ part_row) {
  const float* __restrict__ xyz = t.xyz;
  PickKey best;
  best.a = kNoKey, best.row = 0xffffffffu;
  const long long stride = (long long)gridDim.x * kSesBlock;
  for (long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x; i < t.n; i += stride) {
#pragma clang fp contract(off)
    const float vx = xyz[3 * i] - t.o[0], vy = xyz[3 * i + 1] - t.o[1], vz = xyz[3 * i + 2] - t.o[2];
    const float tt = (vx * t.d[0] + vy * t.d[1]) + vz * t.d[2];
    const float px = vx - tt * t.d[0], py = vy - tt * t.d[1], pz = vz - tt * t.d[2];
    const float p2 = (px * px + py * py) + pz * pz;
    if (tt > 0.f && p2 <= t.r2) {              // (NaN fails both tests)
      PickKey k;
      k.a = ((unsigned long long)__float_as_uint(tt) << 32) | __float_as_uint(p2);
      k.row = (unsigned)i;
      best = pick_min(best, k);
    }
  }
  best = pick_wave_min(best);
  __shared__ unsigned long long sa[kSesBlock / 64];
  __shared__ unsigned sr[kSesBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) sa[wv] = best.a, sr[wv] = best.row;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kSesBlock / 64; ++w) {
      PickKey k;
      k.a = sa[w], k.row = sr[w];
      best = pick_min(best, k);
    }
    part_a[blockIdx.x] = best.a;
    part_row[blockIdx.x] = best.row;
  }
}
__global__ __launch_bounds__(64) void k_pick_finish(const PickTab t, const unsigned long long* __restrict__ part_a,
                                                    const unsigned* __restrict__ part_row, int n_blocks) {
  PickKey best;
  best.a = kNoKey, best.row = 0xffffffffu;
  for (int j = threadIdx.x; j < n_blocks; j += 64) {
    PickKey k;
    k.a = part_a[j], k.row = part_row[j];
    best = pick_min(best, k);
  }
  best = pick_wave_min(best);
  if (threadIdx.x == 0) {
    a3d_pick_result r;
    r.index = -1, r.x = r.y = r.z = 0.f;
    if (best.a != kNoKey) {
      r.index = (int32_t)best.row;
      r.x = t.xyz[3 * (size_t)best.row], r.y = t.xyz[3 * (size_t)best.row + 1], r.z = t.xyz[3 * (size_t)best.row + 2];
    }
    *t.out = r;
  }
}

// ---- mesh pick: the first face a ray crosses -------------------------------------------------------------------------------
struct MeshTab {
  const float* xyz;
  long long n;
  const int32_t* faces;
  long long m;
  float o[3];
  float sx, sy, sz;                           // the shear: d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz] (fp32, computed on the host)
  int kx, ky, kz;                             // the permutation: kz = the ray's dominant axis, kx / ky swapped when d[kz] < 0
  a3d_pick_mesh_result* out;
};
struct MeshFace {
  float U, V, W, det, t;                      // edge functions opposite vertex 0, 1, 2; their sum; the ray parameter
};
// THE crossing test of both stages.  Returns 0 = no hit, 1 = hit (f filled), 2 = an index outside [0, n).  Every product,
// sum and difference is rounded on its own (contraction off), in the order written: a numpy float32 restatement gives the
// same bits.
__device__ __forceinline__ int ses_face(const MeshTab& t, long long i, MeshFace& f, int32_t& i0, int32_t& i1, int32_t& i2) {
#pragma clang fp contract(off)
  i0 = t.faces[3 * i], i1 = t.faces[3 * i + 1], i2 = t.faces[3 * i + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= t.n || i1 >= t.n || i2 >= t.n) return 2;
  if (i0 == i1 || i1 == i2 || i0 == i2) return 0;
  const float* __restrict__ pa = t.xyz + 3 * (size_t)i0;
  const float* __restrict__ pb = t.xyz + 3 * (size_t)i1;
  const float* __restrict__ pc = t.xyz + 3 * (size_t)i2;
  const float a[3] = {pa[0] - t.o[0], pa[1] - t.o[1], pa[2] - t.o[2]};
  const float b[3] = {pb[0] - t.o[0], pb[1] - t.o[1], pb[2] - t.o[2]};
  const float c[3] = {pc[0] - t.o[0], pc[1] - t.o[1], pc[2] - t.o[2]};
  const float akz = t.kz == 0 ? a[0] : t.kz == 1 ? a[1] : a[2], akx = t.kx == 0 ? a[0] : t.kx == 1 ? a[1] : a[2],
              aky = t.ky == 0 ? a[0] : t.ky == 1 ? a[1] : a[2];
  const float bkz = t.kz == 0 ? b[0] : t.kz == 1 ? b[1] : b[2], bkx = t.kx == 0 ? b[0] : t.kx == 1 ? b[1] : b[2],
              bky = t.ky == 0 ? b[0] : t.ky == 1 ? b[1] : b[2];
  const float ckz = t.kz == 0 ? c[0] : t.kz == 1 ? c[1] : c[2], ckx = t.kx == 0 ? c[0] : t.kx == 1 ? c[1] : c[2],
              cky = t.ky == 0 ? c[0] : t.ky == 1 ? c[1] : c[2];
  const float ax = akx - t.sx * akz, ay = aky - t.sy * akz;
  const float bx = bkx - t.sx * bkz, by = bky - t.sy * bkz;
  const float cx = ckx - t.sx * ckz, cy = cky - t.sy * ckz;
  float U = cx * by - cy * bx;                // f(B, C)
  float V = ax * cy - ay * cx;                // f(C, A)
  float W = bx * ay - by * ax;                // f(A, B)
  if (U == 0.f || V == 0.f || W == 0.f) {     // on an edge as far as fp32 can tell: products of floats are exact in double
    U = (float)((double)cx * (double)by - (double)cy * (double)bx);
    V = (float)((double)ax * (double)cy - (double)ay * (double)cx);
    W = (float)((double)bx * (double)ay - (double)by * (double)ax);
  }
  if ((U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f)) return 0;   // (edges inclusive, both windings)
  const float det = (U + V) + W;
  if (det == 0.f) return 0;
  const float az = t.sz * akz, bz = t.sz * bkz, cz = t.sz * ckz;
  const float T = (U * az + V * bz) + W * cz;
  const float tt = T / det;
  if (!(tt > 0.f && tt < __builtin_inff())) return 0;   // (NaN fails the first test)
  f.U = U, f.V = V, f.W = W, f.det = det, f.t = tt;
  return 1;
}
__global__ __launch_bounds__(kSesBlock) void k_pick_mesh(const MeshTab t, unsigned long long* __restrict__ part_key,
                                                         unsigned* __restrict__ part_flag) {
  unsigned long long best = kNoKey;
  int bad = 0;
  const long long stride = (long long)gridDim.x * kSesBlock;
  for (long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x; i < t.m; i += stride) {
    MeshFace f;
    int32_t i0, i1, i2;
    const int r = ses_face(t, i, f, i0, i1, i2);
    if (r == 1) {
      const unsigned long long k = ses_key(f.t, (unsigned)i);   // t > 0: its bits order like t
      best = k < best ? k : best;
    }
    bad |= r == 2;
  }
  best = ses_wave_min(best);
  __shared__ unsigned long long sk[kSesBlock / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) sk[wv] = best;
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    for (int w = 1; w < kSesBlock / 64; ++w) best = sk[w] < best ? sk[w] : best;
    part_key[blockIdx.x] = best;
    part_flag[blockIdx.x] = bad ? 1u : 0u;
  }
}
__global__ __launch_bounds__(64) void k_pick_mesh_finish(const MeshTab t, const unsigned long long* __restrict__ part_key,
                                                         const unsigned* __restrict__ part_flag, int n_blocks) {
  unsigned long long best = kNoKey;
  int bad = 0;
  for (int j = threadIdx.x; j < n_blocks; j += 64) {
    best = part_key[j] < best ? part_key[j] : best;
    bad |= part_flag[j] != 0;
  }
  best = ses_wave_min(best);
  bad = __any(bad);
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
    a3d_pick_mesh_result r;
    r.face = -1, r.flags = bad ? 1 : 0, r.t = 0.f, r.x = r.y = r.z = 0.f, r.u = r.v = 0.f;
    MeshFace f;
    int32_t i0, i1, i2;
    if (best != kNoKey && ses_face(t, (long long)(best & 0xffffffffu), f, i0, i1, i2) == 1) {   // (the first stage's bits again)
      const float* pa = t.xyz + 3 * (size_t)i0;
      const float* pb = t.xyz + 3 * (size_t)i1;
      const float* pc = t.xyz + 3 * (size_t)i2;
      const float u = f.V / f.det, v = f.W / f.det, w = (1.f - u) - v;
      r.face = (int32_t)(best & 0xffffffffu), r.t = f.t, r.u = u, r.v = v;
      r.x = (w * pa[0] + u * pb[0]) + v * pc[0];
      r.y = (w * pa[1] + u * pb[1]) + v * pc[1];
      r.z = (w * pa[2] + u * pb[2]) + v * pc[2];
    }
    *t.out = r;
  }
}

// ---- paint: labels, colours and click cubes of every full-resolution vertex in one pass -----------------------------------
__global__ __launch_bounds__(kSesBlock) void k_session_paint(const a3d_session_paint_args a) {
  __shared__ float pal[256 * 3];
  __shared__ float cube[A3D_MAX_CLICKS * 6];
  for (int i = threadIdx.x; i < a.n_palette * 3; i += kSesBlock) pal[i] = a.palette_dev[i];
  for (int i = threadIdx.x; i < a.n_cubes * 6; i += kSesBlock) cube[i] = a.cubes_dev[i];
  __syncthreads();
  const long long stride = (long long)gridDim.x * kSesBlock;
  for (long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x; i < a.n_full; i += stride) {
    const long long src = a.inverse_map_dev ? a.inverse_map_dev[i] : i;
    if (src < 0 || src >= a.n_qv) {
      atomicOr(a.err_dev, 1);                  // reported through the flag (the call's results are refused by the caller)
      continue;
    }
    const int lab = a.labels_qv_dev[src];
    a.label_full_dev[i] = lab;
    float r = a.colors_full_dev[3 * i], g = a.colors_full_dev[3 * i + 1], b = a.colors_full_dev[3 * i + 2];
    if (lab < 0) atomicOr(a.err_dev, 2);
    if (lab > 0) {
      const int e = lab < a.n_palette ? lab : 1 + (lab - 1) % (a.n_palette - 1);   // ids beyond the table wrap over 1..n-1
      r = pal[3 * e], g = pal[3 * e + 1], b = pal[3 * e + 2];
    }
    if (a.n_cubes) {
      const float x = a.xyz_full_dev[3 * i], y = a.xyz_full_dev[3 * i + 1], z = a.xyz_full_dev[3 * i + 2];
      for (int c = a.n_cubes - 1; c >= 0; --c) {      // later clicks win: the first hit from the back
        const float* q = cube + 6 * c;
        if (fabsf(x - q[0]) < a.cube_size && fabsf(y - q[1]) < a.cube_size && fabsf(z - q[2]) < a.cube_size) {
          r = q[3], g = q[4], b = q[5];
          break;
        }
      }
    }
    a.colors_out_dev[3 * i] = r, a.colors_out_dev[3 * i + 1] = g, a.colors_out_dev[3 * i + 2] = b;
  }
}

struct SesWs {
  unsigned long long* near_part;
  unsigned long long* pick_a;
  unsigned* pick_row;
  unsigned long long* mesh_key;
  unsigned* mesh_flag;
  size_t bytes;
};
static SesWs carve_session(void* base) {
  SesWs w;
  size_t off = 0;
  auto take = [&](size_t b) {
    void* p = base ? (char*)base + off : nullptr;
    off += align256(b);
    return p;
  };
  w.near_part = (unsigned long long*)take((size_t)A3D_NEAREST_MAX_SOURCES * A3D_NEAREST_MAX_QUERIES * kSesMaxBlocks * 8);
  w.pick_a = (unsigned long long*)take((size_t)kSesMaxBlocks * 8);
  w.pick_row = (unsigned*)take((size_t)kSesMaxBlocks * 4);
  w.mesh_key = (unsigned long long*)take((size_t)kSesMaxBlocks * 8);
  w.mesh_flag = (unsigned*)take((size_t)kSesMaxBlocks * 4);
  w.bytes = off;
  return w;
}
static int ses_blocks(long long n) {
  const long long want = (n + kSesBlock - 1) / kSesBlock;
  return (int)(want < 1 ? 1 : want > kSesMaxBlocks ? kSesMaxBlocks : want);
}
static bool ses_ws_ok(const void* ws, size_t bytes, const char* what) {
  if (!ws || ((uintptr_t)ws & 255) || bytes < carve_session(nullptr).bytes) {
    set_error("%s: workspace too small or misaligned (a3d_session_workspace_bytes, 256-byte aligned)", what);
    return false;
  }
  return true;
}

}  // namespace a3d

using namespace a3d;

extern "C" size_t a3d_session_workspace_bytes(void) { return carve_session(nullptr).bytes; }

extern "C" int a3d_nearest_rows(const a3d_nearest_source* sources, int n_sources, const float* queries, int m,
                                void* workspace_dev, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!sources || n_sources < 1 || n_sources > A3D_NEAREST_MAX_SOURCES || !queries || m < 1 || m > A3D_NEAREST_MAX_QUERIES) {
    set_error("a3d_nearest_rows: 1..%d sources, 1..%d queries per call", A3D_NEAREST_MAX_SOURCES, A3D_NEAREST_MAX_QUERIES);
    return A3D_ERR_INVALID;
  }
  if (!ses_ws_ok(workspace_dev, workspace_bytes, "a3d_nearest_rows")) return A3D_ERR_WORKSPACE;
  NearestTab t;
  memset(&t, 0, sizeof(t));
  t.n_src = n_sources, t.m = m;
  long long n_max = 0;
  for (int s = 0; s < n_sources; ++s) {
    const a3d_nearest_source& sp = sources[s];
    if (sp.n < 0 || sp.n >= (1ll << 31) || (sp.n && !sp.xyz_dev) || !sp.rows_out_dev) {
      set_error("a3d_nearest_rows: source %d: bad arguments (n=%lld)", s, (long long)sp.n);
      return A3D_ERR_INVALID;
    }
    t.xyz[s] = sp.xyz_dev, t.n[s] = sp.n, t.out[s] = sp.rows_out_dev;
    t.n_blocks[s] = ses_blocks(sp.n);
    n_max = sp.n > n_max ? sp.n : n_max;
  }
  memcpy(t.q, queries, (size_t)m * 3 * sizeof(float));
  const SesWs w = carve_session(workspace_dev);
  const int nb = ses_blocks(n_max);
  k_nearest_rows<<<dim3(nb, n_sources, (m + kSesQT - 1) / kSesQT), kSesBlock, 0, st>>>(t, w.near_part);
  A3D_LAUNCH_CHECK();
  k_nearest_finish<<<1, kSesBlock, 0, st>>>(t, w.near_part);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_pick_ray(const float* xyz_dev, int64_t n, const float* origin, const float* direction, float radius,
                            a3d_pick_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n < 0 || n >= (1ll << 31) || (n && !xyz_dev) || !origin || !direction || !result_dev || !(radius >= 0.f)) {
    set_error("a3d_pick_ray: bad arguments (n=%lld radius=%g)", (long long)n, (double)radius);
    return A3D_ERR_INVALID;
  }
  const double len2 = (double)direction[0] * direction[0] + (double)direction[1] * direction[1] + (double)direction[2] * direction[2];
  if (!(len2 > 0.999 && len2 < 1.001)) {
    set_error("a3d_pick_ray: the direction must be a unit vector (|d|^2 = %g)", len2);
    return A3D_ERR_INVALID;
  }
  if (!ses_ws_ok(workspace_dev, workspace_bytes, "a3d_pick_ray")) return A3D_ERR_WORKSPACE;
  PickTab t;
  t.xyz = xyz_dev, t.n = n;
  for (int k = 0; k < 3; ++k) t.o[k] = origin[k], t.d[k] = direction[k];
  t.r2 = radius * radius;
  t.out = result_dev;
  const SesWs w = carve_session(workspace_dev);
  const int nb = ses_blocks(n);
  k_pick_ray<<<nb, kSesBlock, 0, st>>>(t, w.pick_a, w.pick_row);
  A3D_LAUNCH_CHECK();
  k_pick_finish<<<1, 64, 0, st>>>(t, w.pick_a, w.pick_row, nb);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_pick_mesh(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m, const float* origin,
                             const float* direction, a3d_pick_mesh_result* result_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n < 0 || n >= (1ll << 31) || m < 0 || m >= (1ll << 31) || (n && !xyz_dev) || (m && !faces_dev) || !origin || !direction ||
      !result_dev) {
    set_error("a3d_pick_mesh: bad arguments (n=%lld m=%lld)", (long long)n, (long long)m);
    return A3D_ERR_INVALID;
  }
  const double len2 = (double)direction[0] * direction[0] + (double)direction[1] * direction[1] + (double)direction[2] * direction[2];
  if (!(len2 > 0.999 && len2 < 1.001)) {
    set_error("a3d_pick_mesh: the direction must be a unit vector (|d|^2 = %g)", len2);
    return A3D_ERR_INVALID;
  }
  if (!ses_ws_ok(workspace_dev, workspace_bytes, "a3d_pick_mesh")) return A3D_ERR_WORKSPACE;
  MeshTab t;
  t.xyz = xyz_dev, t.n = n, t.faces = faces_dev, t.m = m;
  for (int k = 0; k < 3; ++k) t.o[k] = origin[k];
  int kz = 0;                                  // the dominant axis (the first of equals)
  if (fabsf(direction[1]) > fabsf(direction[kz])) kz = 1;
  if (fabsf(direction[2]) > fabsf(direction[kz])) kz = 2;
  int kx = (kz + 1) % 3, ky = (kx + 1) % 3;
  if (direction[kz] < 0.f) {                   // keep the winding
    const int s = kx;
    kx = ky, ky = s;
  }
  t.kx = kx, t.ky = ky, t.kz = kz;
  t.sx = direction[kx] / direction[kz], t.sy = direction[ky] / direction[kz], t.sz = 1.f / direction[kz];
  t.out = result_dev;
  const SesWs w = carve_session(workspace_dev);
  const int nb = ses_blocks(m);
  k_pick_mesh<<<nb, kSesBlock, 0, st>>>(t, w.mesh_key, w.mesh_flag);
  A3D_LAUNCH_CHECK();
  k_pick_mesh_finish<<<1, 64, 0, st>>>(t, w.mesh_key, w.mesh_flag, nb);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_session_paint(const a3d_session_paint_args* args, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!args) {
    set_error("a3d_session_paint: no arguments");
    return A3D_ERR_INVALID;
  }
  const a3d_session_paint_args& a = *args;
  if (a.n_full < 0 || a.n_qv < 0 || a.n_palette < 2 || a.n_palette > 256 || a.n_cubes < 0 || a.n_cubes > A3D_MAX_CLICKS ||
      !a.palette_dev || !a.err_dev || (a.n_cubes && (!a.cubes_dev || !a.xyz_full_dev)) ||
      (a.n_full && (!a.labels_qv_dev || !a.colors_full_dev || !a.label_full_dev || !a.colors_out_dev))) {
    set_error("a3d_session_paint: bad arguments (n_full=%lld palette=%d cubes=%d)", (long long)a.n_full, a.n_palette, a.n_cubes);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a.err_dev, 0, sizeof(int32_t), st));
  if (a.n_full == 0) return A3D_OK;
  const long long want = (a.n_full + kSesBlock - 1) / kSesBlock;
  k_session_paint<<<(unsigned)(want < 2048 ? want : 2048), kSesBlock, 0, st>>>(a);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
