// session.hip -- the headless interactive session around forward_mask: exact nearest rows, ray picking (vertices of a point
// cloud, surfaces of a triangle mesh), the rendered view (per pixel what the picks return) and the full-resolution paint
// pass (gfx950).
//
// Replaces (reference file:line):
//   find_nearest (torch.cdist over all voxel rows, again over all vertices)   interactive_tool/utils.py:27-29, gui.py:273-274
//   "render a depth image and unproject" (Open3D's renderer)                  gui.py:247-271   -> k_pick_ray (point clouds) and
//                                                                             k_pick_mesh (triangle meshes), rules of OURS
//   pred[inverse_map], get_colors, the click cubes                            interactive_segmentation_user.py:83-84,125-140, gui.py:276-298,327
//
// The searches and the paint are streaming passes over 12-byte rows, memory bound, no MFMA; the rendered view bins primitives
// to screen tiles and is bound by its exact tests (see "the rendered view" below).  Nothing here uses an atomic on a result: every
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
//
// THE SECTION RULE (ours; the header states it in full).  Planes (n, c) keep the side n . p >= c; a mesh may also drop the
// faces that turn their back (or their front) to the ray.  On a mesh a section cuts the RAY, not the faces: the planes
// become one interval [t_lo, t_hi] per ray (ses_section_ray) and a crossing counts iff its t lies in it, so faces that share
// an edge still classify every ray consistently.  On a cloud a vertex shows iff it lies on the kept side of every plane.  The
// section is a template parameter of the kernels that test primitives: NoSection is the code the entry points without a
// section have always run, and the binning of the rendered view does not know about sections at all.
#include "session_device.h"                   // Carver, capped_grid
#include "session_rules.h"                    // ses_pixel_ray, ses_keeps(a3d_section): shared with session_region.hip

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

// ---- the section --------------------------------------------------------------------------------------------------------------
struct NoSection {};                          // no section: every overload below folds to nothing
struct RayCut {                               // a section as ONE ray of a mesh sees it
  float t_lo, t_hi;                           // crossings count for t_lo <= t <= t_hi ...
  int empty;                                  // ... unless the ray runs parallel to a plane on its cut side
  int cull;
};
// THE interval of a ray (o, d) under the planes of s: on the host for a3d_pick_mesh_section's one ray and for
// a3d_section_ray, per pixel in the rendered view.  Every operation rounded on its own, in the order written; the divisions
// are correctly rounded on both sides: the same bits.  The maximum and the minimum are written as a comparison, not as fmaxf /
// fminf: a NaN quotient leaves the bound as it is, as with those, and where both are zeros of either sign the bound stays
// -- fmaxf(+0, -0) may return either zero, and host, device and numpy need not agree on which.
__host__ __device__ inline void ses_section_ray(const a3d_section& s, const float* o, const float* d, RayCut& c) {
#pragma clang fp contract(off)
  c.t_lo = 0.f, c.t_hi = __builtin_inff(), c.empty = 0, c.cull = s.cull;
  for (int k = 0; k < s.n_planes; ++k) {
    const float nx = s.planes[k][0], ny = s.planes[k][1], nz = s.planes[k][2], cc = s.planes[k][3];
    const float den = (nx * d[0] + ny * d[1]) + nz * d[2];
    const float so = (nx * o[0] + ny * o[1]) + nz * o[2];
    if (den > 0.f) {
      const float q = (cc - so) / den;
      c.t_lo = q > c.t_lo ? q : c.t_lo;
    } else if (den < 0.f) {
      const float q = (cc - so) / den;
      c.t_hi = q < c.t_hi ? q : c.t_hi;
    } else if (!(so >= cc)) {                 // (a NaN den lands here as well)
      c.empty = 1;
    }
  }
}
__host__ __device__ inline NoSection ses_ray_cut(const NoSection&, const float*, const float*) { return NoSection{}; }
__host__ __device__ inline RayCut ses_ray_cut(const a3d_section& s, const float* o, const float* d) {
  RayCut c;
  ses_section_ray(s, o, d, c);
  return c;
}
// Whether a crossing the face test accepted counts: t inside the interval, both ends inclusive, and the facing.  The shear
// keeps the winding, so det = (U + V) + W > 0 iff the vertices appear counter-clockwise from the origin: a FRONT face
// (g . d < 0 for g = (b - a) x (c - a)); det < 0: a back face; det == 0 never gets here.
__device__ __forceinline__ bool ses_counts(const NoSection&, float, float) { return true; }
__device__ __forceinline__ bool ses_counts(const RayCut& c, float t, float det) {
  if (c.empty || !(t >= c.t_lo && t <= c.t_hi)) return false;
  return !((c.cull == A3D_CULL_BACK && det < 0.f) || (c.cull == A3D_CULL_FRONT && det > 0.f));
}
// Whether a cloud's vertex shows: ses_keeps(a3d_section) of session_rules.h; without a section every vertex does.
__device__ __forceinline__ bool ses_keeps(const NoSection&, float, float, float) { return true; }

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
// THE point test of the pick and of the rendered view: point (x, y, z), row i, against the ray (o, d), |d| = 1, and r^2.
// Every operation rounded on its own, in the order written.  Folds a passing point's key into best.
__device__ __forceinline__ void ses_point(const float* o, const float* d, float r2, float x, float y, float z, unsigned i,
                                          PickKey& best) {
#pragma clang fp contract(off)
  const float vx = x - o[0], vy = y - o[1], vz = z - o[2];
  const float tt = (vx * d[0] + vy * d[1]) + vz * d[2];
  const float px = vx - tt * d[0], py = vy - tt * d[1], pz = vz - tt * d[2];
  const float p2 = (px * px + py * py) + pz * pz;
  if (tt > 0.f && p2 <= r2) {                  // (NaN fails both tests)
    PickKey k;
    k.a = ((unsigned long long)__float_as_uint(tt) << 32) | __float_as_uint(p2);
    k.row = i;
    best = pick_min(best, k);
  }
}
template <class S>                            // NoSection or a3d_section
__global__ __launch_bounds__(kSesBlock) void k_pick_ray(const PickTab t, unsigned long long* __restrict__ part_a,
                                                        unsigned* __restrict__ part_row, const S sec) {
  const float* __restrict__ xyz = t.xyz;
  PickKey best;
  best.a = kNoKey, best.row = 0xffffffffu;
  const long long stride = (long long)gridDim.x * kSesBlock;
  for (long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x; i < t.n; i += stride) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (ses_keeps(sec, x, y, z)) ses_point(t.o, t.d, t.r2, x, y, z, (unsigned)i, best);
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
struct RayShear {                             // a ray as the crossing test sees it
  float o[3];
  float sx, sy, sz;                           // the shear: d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz] (fp32)
  int kx, ky, kz;                             // the permutation: kz = the ray's dominant axis, kx / ky swapped when d[kz] < 0
};
// THE derivation of shear and permutation from a unit direction: on the host for a3d_pick_mesh's one ray, per pixel in the
// rendered view (three correctly rounded fp32 divisions: the same bits on both sides).
__host__ __device__ inline void ses_shear(const float* d, RayShear& r) {
  int kz = 0;                                  // the dominant axis (the first of equals)
  if (fabsf(d[1]) > fabsf(d[kz])) kz = 1;
  if (fabsf(d[2]) > fabsf(d[kz])) kz = 2;
  int kx = (kz + 1) % 3, ky = (kx + 1) % 3;
  if (d[kz] < 0.f) {                           // keep the winding
    const int s = kx;
    kx = ky, ky = s;
  }
  r.kx = kx, r.ky = ky, r.kz = kz;
  r.sx = d[kx] / d[kz], r.sy = d[ky] / d[kz], r.sz = 1.f / d[kz];
}
struct MeshTab {
  const float* xyz;
  long long n;
  const int32_t* faces;
  long long m;
  RayShear r;
  a3d_pick_mesh_result* out;
};
struct MeshFace {
  float U, V, W, det, t;                      // edge functions opposite vertex 0, 1, 2; their sum; the ray parameter
};
// THE crossing test of both stages.  Returns 0 = no hit, 1 = hit (f filled), 2 = an index outside [0, n).  Every product,
// sum and difference is rounded on its own (contraction off), in the order written: a numpy float32 restatement gives the
// same bits.
// ses_face_test: the arithmetic, on three vertices wherever they lie (global memory, or LDS in the rendered view);
// ses_face: the index checks in front of it.
__device__ __forceinline__ int ses_face_test(const RayShear& t, const float* pa, const float* pb, const float* pc, MeshFace& f) {
#pragma clang fp contract(off)
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
__device__ __forceinline__ int ses_face(const MeshTab& t, long long i, MeshFace& f, int32_t& i0, int32_t& i1, int32_t& i2) {
  i0 = t.faces[3 * i], i1 = t.faces[3 * i + 1], i2 = t.faces[3 * i + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= t.n || i1 >= t.n || i2 >= t.n) return 2;
  if (i0 == i1 || i1 == i2 || i0 == i2) return 0;
  return ses_face_test(t.r, t.xyz + 3 * (size_t)i0, t.xyz + 3 * (size_t)i1, t.xyz + 3 * (size_t)i2, f);
}
template <class S>                            // NoSection or RayCut (the host derived it from the call's one ray)
__global__ __launch_bounds__(kSesBlock) void k_pick_mesh(const MeshTab t, unsigned long long* __restrict__ part_key,
                                                         unsigned* __restrict__ part_flag, const S cut) {
  unsigned long long best = kNoKey;
  int bad = 0;
  const long long stride = (long long)gridDim.x * kSesBlock;
  for (long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x; i < t.m; i += stride) {
    MeshFace f;
    int32_t i0, i1, i2;
    const int r = ses_face(t, i, f, i0, i1, i2);
    if (r == 1 && ses_counts(cut, f.t, f.det)) {
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
// (The finish needs no section: the first stage chose the face, the finish only evaluates it again.)
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
  Carver c{base};
  w.near_part = (unsigned long long*)c.take((size_t)A3D_NEAREST_MAX_SOURCES * A3D_NEAREST_MAX_QUERIES * kSesMaxBlocks * 8);
  w.pick_a = (unsigned long long*)c.take((size_t)kSesMaxBlocks * 8);
  w.pick_row = (unsigned*)c.take((size_t)kSesMaxBlocks * 4);
  w.mesh_key = (unsigned long long*)c.take((size_t)kSesMaxBlocks * 8);
  w.mesh_flag = (unsigned*)c.take((size_t)kSesMaxBlocks * 4);
  w.bytes = c.off;
  return w;
}
// n rows behind a pointer: a count that fits the kernels' 32-bit row ids, and rows to read unless there are none
static bool ses_rows_ok(long long n, const void* rows) { return n >= 0 && n < (1ll << 31) && (!n || rows); }
static bool ses_unit_direction(const char* what, const float* d) {
  const double len2 = (double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2];
  if (!(len2 > 0.999 && len2 < 1.001)) {
    set_error("%s: the direction must be a unit vector (|d|^2 = %g)", what, len2);
    return false;
  }
  return true;
}
static bool ses_ws_ok(const void* ws, size_t bytes, const char* what) {
  if (!ws || ((uintptr_t)ws & 255) || bytes < carve_session(nullptr).bytes) {
    set_error("%s: workspace too small or misaligned (a3d_session_workspace_bytes, 256-byte aligned)", what);
    return false;
  }
  return true;
}

// ---- the rendered view: per pixel what the picks above return for the ray through the pixel's centre -----------------------
// Three passes around one exclusive scan.  (1) k_render_bin: per primitive a conservative rectangle of tiles (render_rect_*),
// kept in the workspace, its tiles counted; a primitive without a bound joins the everywhere-list.  (2) k_render_scan: one
// block turns the counts into offsets and decides whether the pairs fit.  (3) k_render_fill: the rectangles again, ids into
// the tiles' lists.  (4) k_render_tile_*: one workgroup per tile, one thread per pixel; the everywhere-list and the tile's
// list pass through LDS in chunks of 256 primitives (vertices staged once per workgroup, then read by all 256 pixels at the
// same address: a broadcast), every thread keeps its packed minimum in registers.  The minimum is order-free, so the order
// in which the atomics of (3) fill a list does not reach the image.
constexpr int kTile = A3D_RENDER_TILE;
constexpr int kTilePixels = kTile * kTile;    // = the workgroup of the tile pass = the chunk staged in LDS
constexpr int kMaxRectTiles = 256;            // a bound of more tiles: the primitive goes to the everywhere-list
constexpr double kU = 5.9604644775390625e-8;  // 2^-24, unit roundoff of fp32

struct RenderCam {
  a3d_camera c;
  double inv[9];                              // rows of [du dv d00]^-1: p -> (a, b, c), screen position (a / c, b / c)
  double na, nb, nc;                          // the rows' norms
  double dmax;                                // >= |d00 + u du + v dv| for every pixel
  int tiles_x, tiles_y;
};
struct RenderWs {
  unsigned* tile_count;                       // [tiles]       pairs of each tile; zeroed by the call
  unsigned* tile_fill;                        // [tiles]       fill cursors; zeroed by the call
  unsigned* every_count;                      // [1] (+ padding to 256 bytes); zeroed by the call
  unsigned* tile_offset;                      // [tiles]
  int4* rect;                                 // [n_primitives] tile rectangle tx0, ty0, tx1, ty1 (tx1 < tx0: none)
  unsigned* every;                            // [n_primitives]
  unsigned* pairs;                            // [pair_capacity]
  size_t zero_bytes, bytes;
};
static RenderWs carve_render(void* base, long long n_prim, int width, int height, long long cap) {
  RenderWs w;
  Carver c{base};
  const size_t tiles = (size_t)((width + kTile - 1) / kTile) * ((height + kTile - 1) / kTile);
  w.tile_count = (unsigned*)c.take(tiles * 4);
  w.tile_fill = (unsigned*)c.take(tiles * 4);
  w.every_count = (unsigned*)c.take(4);
  w.zero_bytes = c.off;
  w.tile_offset = (unsigned*)c.take(tiles * 4);
  w.rect = (int4*)c.take((size_t)(n_prim > 0 ? n_prim : 1) * 16);
  w.every = (unsigned*)c.take((size_t)(n_prim > 0 ? n_prim : 1) * 4);
  w.pairs = (unsigned*)c.take((size_t)(cap > 0 ? cap : 1) * 4);
  w.bytes = c.off;
  return w;
}

// ---- the bound (tests/test_render_host.py restates it in numpy and holds it against the exact tests) ------
// Screen positions are continuous pixel coordinates in which pixel (i, j)'s ray is the point (i, j).  A rectangle
// [x0, x1] x [y0, y1] of them becomes the tiles of the pixels floor(x0) .. ceil(x1), clamped to the image.
// Returns 0 = no pixel can pass, 1 = rect filled, 2 = no bound (everywhere).
__device__ __forceinline__ int render_rect_tiles(const RenderCam& cam, double x0, double x1, double y0, double y1, int4& rect) {
  if (!(x0 <= x1 && y0 <= y1)) return 2;      // (a NaN)
  const double w1 = cam.c.width - 1, h1 = cam.c.height - 1;
  if (x1 < 0. || y1 < 0. || x0 > w1 || y0 > h1) return 0;
  const int px0 = (int)floor(fmax(x0, 0.)), px1 = (int)ceil(fmin(x1, w1));
  const int py0 = (int)floor(fmax(y0, 0.)), py1 = (int)ceil(fmin(y1, h1));
  rect.x = px0 / kTile, rect.y = py0 / kTile, rect.z = px1 / kTile, rect.w = py1 / kTile;
  if ((rect.z - rect.x + 1) * (rect.w - rect.y + 1) > kMaxRectTiles) return 2;
  return 1;
}
// A face with vertices A, B, C (fp32).  With p = vertex - o in double: R = the largest |coordinate| of the three p, g = the
// distance from the origin to their bounding box.  A pixel's test passes only if its ray meets the triangle of the sheared
// fp32 vertices, which lie within eta = 32 u R of the true ones (ray rounding included); the hit point q has |q| >= g - eta,
// and q = c D(u, v) with |D| <= dmax, so c >= c_lo = 0.98 g / dmax.  g <= R / 1024: no bound.  The triangle is clipped to
// c >= c_lo, its remaining corners projected, and the rectangle grown by what eta can move a corner at depth c_lo.
__device__ __forceinline__ int render_rect_face(const RenderCam& cam, const float* A, const float* B, const float* C, int4& rect) {
  double p[3][3];
  double R = 0., g2 = 0.;
  for (int k = 0; k < 3; ++k) {
    p[0][k] = (double)A[k] - (double)cam.c.o[k], p[1][k] = (double)B[k] - (double)cam.c.o[k], p[2][k] = (double)C[k] - (double)cam.c.o[k];
    if (p[0][k] != p[0][k] || p[1][k] != p[1][k] || p[2][k] != p[2][k]) return 0;   // a NaN vertex: the exact test never passes
    const double lo = fmin(p[0][k], fmin(p[1][k], p[2][k])), hi = fmax(p[0][k], fmax(p[1][k], p[2][k]));
    R = fmax(R, fmax(fabs(lo), fabs(hi)));
    const double gap = fmax(0., fmax(lo, -hi));
    g2 += gap * gap;
  }
  const double g = sqrt(g2);
  if (!(R < 1e30) || !(g > R * (1. / 1024.))) return 2;
  const double c_lo = 0.98 * g / cam.dmax, eta = 32. * kU * R;
  double a[3], b[3], c[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = cam.inv[0] * p[k][0] + cam.inv[1] * p[k][1] + cam.inv[2] * p[k][2];
    b[k] = cam.inv[3] * p[k][0] + cam.inv[4] * p[k][1] + cam.inv[5] * p[k][2];
    c[k] = cam.inv[6] * p[k][0] + cam.inv[7] * p[k][1] + cam.inv[8] * p[k][2];
  }
  double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
  for (int k = 0; k < 3; ++k) {
    const int j = k == 2 ? 0 : k + 1;
    if (c[k] >= c_lo) {
      const double x = a[k] / c[k], y = b[k] / c[k];
      x0 = fmin(x0, x), x1 = fmax(x1, x), y0 = fmin(y0, y), y1 = fmax(y1, y);
    }
    if ((c[k] >= c_lo) != (c[j] >= c_lo)) {   // the edge k -> j crosses the plane c = c_lo
      const double s = (c_lo - c[k]) / (c[j] - c[k]);
      const double x = (a[k] + s * (a[j] - a[k])) / c_lo, y = (b[k] + s * (b[j] - b[k])) / c_lo;
      x0 = fmin(x0, x), x1 = fmax(x1, x), y0 = fmin(y0, y), y1 = fmax(y1, y);
    }
  }
  if (x0 > x1) return 0;                       // wholly behind c = c_lo
  const double mx = 1. / 128. + (cam.na + 8192. * cam.nc) * eta / c_lo, my = 1. / 128. + (cam.nb + 8192. * cam.nc) * eta / c_lo;
  return render_rect_tiles(cam, x0 - mx, x1 + mx, y0 - my, y1 + my, rect);
}
// A point P with radius r.  The fp32 test admits rays within r_eff = r (1 + 2^-10) + 128 u (|p| + r) of it.  |p| <= r_eff
// (1 + 2^-10): no bound.  Else the ray's closest point q to P lies in the ball, at |q| >= t0 = sqrt(|p|^2 - r_eff^2), so its
// c >= 0.98 t0 / dmax; the ball lies in the box (a +- r_eff na, b +- r_eff nb, c +- r_eff nc) of the camera's coordinates.
__device__ __forceinline__ int render_rect_point(const RenderCam& cam, const float* P, double r, int4& rect) {
  double p[3], n2 = 0.;
  for (int k = 0; k < 3; ++k) {
    p[k] = (double)P[k] - (double)cam.c.o[k];
    n2 += p[k] * p[k];
  }
  if (!(n2 < 1e60)) return 0;                  // NaN or infinite: the exact test never passes
  const double len = sqrt(n2);
  const double reff = r * (1. + 1. / 1024.) + 128. * kU * (len + r);
  if (!(len > reff * (1. + 1. / 1024.))) return 2;
  const double t0 = sqrt(n2 - reff * reff);
  const double a = cam.inv[0] * p[0] + cam.inv[1] * p[1] + cam.inv[2] * p[2];
  const double b = cam.inv[3] * p[0] + cam.inv[4] * p[1] + cam.inv[5] * p[2];
  const double c = cam.inv[6] * p[0] + cam.inv[7] * p[1] + cam.inv[8] * p[2];
  const double ha = reff * cam.na, hb = reff * cam.nb, hc = reff * cam.nc;
  const double c_lo = fmax(c - hc, 0.98 * t0 / cam.dmax), c_hi = c + hc;
  if (!(c_hi >= c_lo)) return 0;               // behind the camera
  const double x0 = fmin((a - ha) / c_lo, (a - ha) / c_hi), x1 = fmax((a + ha) / c_lo, (a + ha) / c_hi);
  const double y0 = fmin((b - hb) / c_lo, (b - hb) / c_hi), y1 = fmax((b + hb) / c_lo, (b + hb) / c_hi);
  return render_rect_tiles(cam, x0 - 1. / 128., x1 + 1. / 128., y0 - 1. / 128., y1 + 1. / 128., rect);
}

struct RenderTab {
  RenderCam cam;
  const float* xyz;
  long long n;
  const int32_t* faces;                       // a mesh's faces (may be NULL when m == 0)
  int mesh;                                   // 1: faces of a mesh, 0: points of a cloud
  long long m;                                // primitives: faces of a mesh, points of a cloud
  float r2;
  double radius;
  a3d_render_out out;
  long long cap;
};
__global__ __launch_bounds__(kSesBlock) void k_render_bin(const RenderTab t, const RenderWs w) {
  const long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x;
  if (i >= t.m) return;
  int4 rect = make_int4(1, 0, 0, 0);
  int r = 0;
  if (t.mesh) {
    const int32_t i0 = t.faces[3 * i], i1 = t.faces[3 * i + 1], i2 = t.faces[3 * i + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= t.n || i1 >= t.n || i2 >= t.n)
      atomicOr(&t.out.header_dev->flags, A3D_RENDER_BAD_INDEX);
    else if (i0 != i1 && i1 != i2 && i0 != i2)
      r = render_rect_face(t.cam, t.xyz + 3 * (size_t)i0, t.xyz + 3 * (size_t)i1, t.xyz + 3 * (size_t)i2, rect);
  } else {
    r = render_rect_point(t.cam, t.xyz + 3 * (size_t)i, t.radius, rect);
  }
  if (r == 2) w.every[atomicAdd(w.every_count, 1u)] = (unsigned)i;   // (at most one entry per primitive: < m)
  if (r != 1) rect = make_int4(1, 0, 0, 0);
  w.rect[i] = rect;
  for (int ty = rect.y; ty <= rect.w; ++ty)
    for (int tx = rect.x; tx <= rect.z; ++tx) atomicAdd(w.tile_count + ty * t.cam.tiles_x + tx, 1u);
}
// one block: exclusive scan of the tiles' counts (each thread a run of consecutive tiles), the verdict into the header
__global__ __launch_bounds__(1024) void k_render_scan(const RenderTab t, const RenderWs w) {
  const int tiles = t.cam.tiles_x * t.cam.tiles_y;
  const int per = (tiles + 1023) / 1024;
  const int lo = min((int)threadIdx.x * per, tiles), hi = min(lo + per, tiles);
  unsigned long long sum = 0;
  for (int k = lo; k < hi; ++k) sum += w.tile_count[k];
  __shared__ unsigned long long part[1024];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0ull;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  const unsigned long long total = part[1023];
  unsigned long long run = part[threadIdx.x] - sum;
  if (total <= (unsigned long long)t.cap)     // (else the offsets are not used: no list is filled)
    for (int k = lo; k < hi; ++k) {
      w.tile_offset[k] = (unsigned)run;
      run += w.tile_count[k];
    }
  if (threadIdx.x == 0) {
    a3d_render_header* h = t.out.header_dev;
    h->pairs_needed = (int64_t)total;
    h->n_everywhere = (int32_t)*w.every_count;
    if (total > (unsigned long long)t.cap) atomicOr(&h->flags, A3D_RENDER_OVERFLOW);
  }
}
__global__ __launch_bounds__(kSesBlock) void k_render_fill(const RenderTab t, const RenderWs w) {
  if (t.out.header_dev->flags & A3D_RENDER_OVERFLOW) return;
  const long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x;
  if (i >= t.m) return;
  const int4 rect = w.rect[i];
  for (int ty = rect.y; ty <= rect.w; ++ty)
    for (int tx = rect.x; tx <= rect.z; ++tx) {
      const int tile = ty * t.cam.tiles_x + tx;
      const unsigned long long pos = (unsigned long long)w.tile_offset[tile] + atomicAdd(w.tile_fill + tile, 1u);
      if (pos < (unsigned long long)t.cap) w.pairs[pos] = (unsigned)i;   // (always: the counts are those of k_render_bin)
    }
}
// The lists of a tile: the everywhere-list, then its own.  Entry e of the two, laid end to end.
__device__ __forceinline__ unsigned render_list_entry(const RenderWs& w, unsigned n_every, unsigned offset, unsigned e) {
  return e < n_every ? w.every[e] : w.pairs[offset + (e - n_every)];
}
// What a thread of the tile pass (workgroup = tile blockIdx.x) starts from.  render_tile_pixel: its pixel and the pixel's
// ray; returns whether the pixel lies inside the image (a thread outside still stages primitives).  render_tile_lists: the
// length of the everywhere-list, of both lists, and the offset of the tile's own.
__device__ __forceinline__ bool render_tile_pixel(const RenderTab& t, int& px, int& py, float* d) {
  const int tile = blockIdx.x;
  px = (tile % t.cam.tiles_x) * kTile + (threadIdx.x & (kTile - 1));
  py = (tile / t.cam.tiles_x) * kTile + (threadIdx.x >> 4);
  const bool live = px < t.cam.c.width && py < t.cam.c.height;
  ses_pixel_ray(t.cam.c, live ? px : 0, live ? py : 0, d);
  return live;
}
struct TileLists {
  unsigned n_every, total, offset;
};
__device__ __forceinline__ TileLists render_tile_lists(const RenderWs& w) {
  const int tile = blockIdx.x;
  const unsigned n_every = *w.every_count;
  return {n_every, n_every + w.tile_count[tile], w.tile_offset[tile]};
}
template <class S>                            // NoSection or a3d_section
__global__ __launch_bounds__(kTilePixels) void k_render_tile_mesh(const RenderTab t, const RenderWs w, const S sec) {
  if (t.out.header_dev->flags & A3D_RENDER_OVERFLOW) return;
  __shared__ float vtx[kTilePixels][9];
  __shared__ unsigned ids[kTilePixels];
  int px, py;
  float d[3];
  const bool live = render_tile_pixel(t, px, py, d);
  RayShear ray;
  ray.o[0] = t.cam.c.o[0], ray.o[1] = t.cam.c.o[1], ray.o[2] = t.cam.c.o[2];
  ses_shear(d, ray);
  const auto cut = ses_ray_cut(sec, ray.o, d);  // the pixel's interval, as a3d_pick_mesh_section derives it for this ray
  const auto [n_every, total, offset] = render_tile_lists(w);
  unsigned long long best = kNoKey;
  for (unsigned base = 0; base < total; base += kTilePixels) {
    const unsigned cnt = min((unsigned)kTilePixels, total - base);
    __syncthreads();
    if (threadIdx.x < cnt) {                   // (only faces whose indices k_render_bin found in range and distinct are listed)
      const unsigned f = render_list_entry(w, n_every, offset, base + threadIdx.x);
      ids[threadIdx.x] = f;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float* p = t.xyz + 3 * (size_t)t.faces[3 * (size_t)f + k];
        vtx[threadIdx.x][3 * k] = p[0], vtx[threadIdx.x][3 * k + 1] = p[1], vtx[threadIdx.x][3 * k + 2] = p[2];
      }
    }
    __syncthreads();
    if (live)
      for (unsigned k = 0; k < cnt; ++k) {
        MeshFace f;
        if (ses_face_test(ray, vtx[k], vtx[k] + 3, vtx[k] + 6, f) == 1 && ses_counts(cut, f.t, f.det)) {
          const unsigned long long key = ses_key(f.t, ids[k]);
          best = key < best ? key : best;
        }
      }
  }
  if (!live) return;
  const size_t at = (size_t)py * t.cam.c.width + px;
  int32_t face = -1;
  float tt = __builtin_inff(), u = 0.f, v = 0.f;
  if (best != kNoKey) {
    face = (int32_t)(unsigned)(best & 0xffffffffu);
    tt = __uint_as_float((unsigned)(best >> 32));
    if (t.out.u_dev || t.out.v_dev) {          // (the bits of the list pass again, as in k_pick_mesh_finish)
      MeshTab mt;
      mt.xyz = t.xyz, mt.n = t.n, mt.faces = t.faces, mt.m = t.m, mt.r = ray, mt.out = nullptr;
      MeshFace f;
      int32_t i0, i1, i2;
      if (ses_face(mt, face, f, i0, i1, i2) == 1) u = f.V / f.det, v = f.W / f.det;
    }
  }
  t.out.id_dev[at] = face;
  t.out.t_dev[at] = tt;
  if (t.out.u_dev) t.out.u_dev[at] = u;
  if (t.out.v_dev) t.out.v_dev[at] = v;
}
template <class S>                            // NoSection or a3d_section
__global__ __launch_bounds__(kTilePixels) void k_render_tile_points(const RenderTab t, const RenderWs w, const S sec) {
  if (t.out.header_dev->flags & A3D_RENDER_OVERFLOW) return;
  __shared__ float pts[kTilePixels][3];
  __shared__ unsigned ids[kTilePixels];
  int px, py;
  float d[3];
  const bool live = render_tile_pixel(t, px, py, d);
  const float o[3] = {t.cam.c.o[0], t.cam.c.o[1], t.cam.c.o[2]};
  const auto [n_every, total, offset] = render_tile_lists(w);
  PickKey best;
  best.a = kNoKey, best.row = 0xffffffffu;
  for (unsigned base = 0; base < total; base += kTilePixels) {
    const unsigned cnt = min((unsigned)kTilePixels, total - base);
    __syncthreads();
    if (threadIdx.x < cnt) {
      const unsigned i = render_list_entry(w, n_every, offset, base + threadIdx.x);
      ids[threadIdx.x] = i;
      const float* p = t.xyz + 3 * (size_t)i;
      // a vertex the section cuts away is staged as a NaN, which ses_point passes for no ray: the vertex rule does not depend
      // on the view, so the thread that stages a vertex decides it once for the tile's 256 pixels
      pts[threadIdx.x][0] = ses_keeps(sec, p[0], p[1], p[2]) ? p[0] : __builtin_nanf("");
      pts[threadIdx.x][1] = p[1], pts[threadIdx.x][2] = p[2];
    }
    __syncthreads();
    if (live)
      for (unsigned k = 0; k < cnt; ++k) ses_point(o, d, t.r2, pts[k][0], pts[k][1], pts[k][2], ids[k], best);
  }
  if (!live) return;
  const size_t at = (size_t)py * t.cam.c.width + px;
  const bool hit = best.a != kNoKey;
  t.out.id_dev[at] = hit ? (int32_t)best.row : -1;
  t.out.t_dev[at] = hit ? __uint_as_float((unsigned)(best.a >> 32)) : __builtin_inff();
}

struct ShadeTab {
  const int32_t* id;
  const float *u, *v;
  const int32_t* faces;
  long long m, n;
  const float* colors;
  float bg[3];
  uint8_t* rgb;
  long long pixels;
};
static ShadeTab shade_tab(const int32_t* id, const float* u, const float* v, const int32_t* faces, long long m,
                          const float* colors, long long n, const float* background, uint8_t* rgb, long long pixels) {
  ShadeTab t;
  t.id = id, t.u = u, t.v = v, t.faces = faces, t.m = m, t.n = n, t.colors = colors, t.rgb = rgb, t.pixels = pixels;
  for (int k = 0; k < 3; ++k) t.bg[k] = background[k];
  return t;
}
__device__ __forceinline__ uint8_t shade_q(float c) { return (uint8_t)(fminf(fmaxf(c, 0.f), 1.f) * 255.f + 0.5f); }
// THE base colour of pixel i, for the flat pass and the two shaded ones: the background, the vertex's colour (no faces) or
// the face's interpolated one.  false: the pixel shows the background (id -1, or an id / a face's index outside its table).
// On a mesh hit f holds the face's three vertices and u, v, wgt the pixel's weights.
__device__ __forceinline__ bool shade_base(const ShadeTab& t, long long i, float* c, int32_t* f, float& u, float& v, float& wgt) {
#pragma clang fp contract(off)
  const int32_t id = t.id[i];
  c[0] = t.bg[0], c[1] = t.bg[1], c[2] = t.bg[2];
  if (!t.faces) {
    if (!(id >= 0 && id < t.n)) return false;
    for (int k = 0; k < 3; ++k) c[k] = t.colors[3 * (size_t)id + k];
    return true;
  }
  if (!(id >= 0 && id < t.m)) return false;
  f[0] = t.faces[3 * (size_t)id], f[1] = t.faces[3 * (size_t)id + 1], f[2] = t.faces[3 * (size_t)id + 2];
  if (!(f[0] >= 0 && f[1] >= 0 && f[2] >= 0 && f[0] < t.n && f[1] < t.n && f[2] < t.n)) return false;
  u = t.u[i], v = t.v[i], wgt = (1.f - u) - v;
  for (int k = 0; k < 3; ++k)
    c[k] = (wgt * t.colors[3 * (size_t)f[0] + k] + u * t.colors[3 * (size_t)f[1] + k]) + v * t.colors[3 * (size_t)f[2] + k];
  return true;
}
__global__ __launch_bounds__(kSesBlock) void k_render_shade(const ShadeTab t) {
  const long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x;
  if (i >= t.pixels) return;
  float c[3], u, v, wgt;
  int32_t f[3];
  shade_base(t, i, c, f, u, v, wgt);
  t.rgb[3 * i] = shade_q(c[0]), t.rgb[3 * i + 1] = shade_q(c[1]), t.rgb[3 * i + 2] = shade_q(c[2]);
}

// ---- lit shading (meshes): a double-sided light at the camera ---------------------------------------------------------------
// THE RULE (ours; the header states it in full): base colour as above; the interpolated normal Nn = (w N0 + u N1) + v N2, the
// pixel's unit ray d; k0 = min(|Nn . d| / |Nn|, 1), or 1 where |Nn|^2 is 0 or not finite; k = ambient + (1 - ambient) k0; each
// channel c k.  Every operation rounded on its own, in the order written.
struct LitTab {
  ShadeTab s;                                 // (s.faces is NULL only in k_render_shade_lit_points)
  const float* normals;
  a3d_camera cam;
  float ambient;
};
__global__ __launch_bounds__(kSesBlock) void k_render_shade_lit(const LitTab t) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x;
  if (i >= t.s.pixels) return;
  float c[3], u, v, wgt;
  int32_t f[3];
  if (shade_base(t.s, i, c, f, u, v, wgt)) {
    const float *n0 = t.normals + 3 * (size_t)f[0], *n1 = t.normals + 3 * (size_t)f[1], *n2 = t.normals + 3 * (size_t)f[2];
    const float nx = (wgt * n0[0] + u * n1[0]) + v * n2[0];
    const float ny = (wgt * n0[1] + u * n1[1]) + v * n2[1];
    const float nz = (wgt * n0[2] + u * n1[2]) + v * n2[2];
    const float l2 = (nx * nx + ny * ny) + nz * nz;
    float k0 = 1.f;
    if (l2 > 0.f && l2 < __builtin_inff()) {
      float d[3];
      ses_pixel_ray(t.cam, (int)(i % t.cam.width), (int)(i / t.cam.width), d);
      const float dot = (nx * d[0] + ny * d[1]) + nz * d[2];
      k0 = fminf(fabsf(dot) / sqrtf(l2), 1.f);
    }
    const float k = t.ambient + (1.f - t.ambient) * k0;
    c[0] = c[0] * k, c[1] = c[1] * k, c[2] = c[2] * k;
  }
  t.s.rgb[3 * i] = shade_q(c[0]), t.s.rgb[3 * i + 1] = shade_q(c[1]), t.s.rgb[3 * i + 2] = shade_q(c[2]);
}

// ---- lit shading (point clouds with estimated normals): the same light, the pixel's vertex in place of the corners -----------
// THE RULE: base colour as above (s.faces is NULL: ids are vertices); N = the vertex's normal as it is stored; the rest is
// k_render_shade_lit's, operation for operation.  A zero normal (a voxel without a valid one) leaves the colour unshaded.
__global__ __launch_bounds__(kSesBlock) void k_render_shade_lit_points(const LitTab t) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x;
  if (i >= t.s.pixels) return;
  float c[3], u, v, wgt;
  int32_t f[3];
  if (shade_base(t.s, i, c, f, u, v, wgt)) {
    const float* nn = t.normals + 3 * (size_t)t.s.id[i];
    const float nx = nn[0], ny = nn[1], nz = nn[2];
    const float l2 = (nx * nx + ny * ny) + nz * nz;
    float k0 = 1.f;
    if (l2 > 0.f && l2 < __builtin_inff()) {
      float d[3];
      ses_pixel_ray(t.cam, (int)(i % t.cam.width), (int)(i / t.cam.width), d);
      const float dot = (nx * d[0] + ny * d[1]) + nz * d[2];
      k0 = fminf(fabsf(dot) / sqrtf(l2), 1.f);
    }
    const float k = t.ambient + (1.f - t.ambient) * k0;
    c[0] = c[0] * k, c[1] = c[1] * k, c[2] = c[2] * k;
  }
  t.s.rgb[3 * i] = shade_q(c[0]), t.s.rgb[3 * i + 1] = shade_q(c[1]), t.s.rgb[3 * i + 2] = shade_q(c[2]);
}

// ---- depth shading (point clouds have no normals): a pixel darkens by how far it lies behind its four neighbours -----------
// THE RULE: s = (((0 + r(left)) + r(right)) + r(up)) + r(down), r(q) = max(t_p - t_q, 0) / t_p for a neighbour inside the
// image that shows something (id >= 0), else 0; k = 1 / (1 + strength s); each channel c k.
struct DepthTab {
  ShadeTab s;
  const float* t;
  int width, height;
  float strength;
};
__global__ __launch_bounds__(kSesBlock) void k_render_shade_depth(const DepthTab t) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x;
  if (i >= t.s.pixels) return;
  float c[3], u, v, wgt;
  int32_t f[3];
  if (shade_base(t.s, i, c, f, u, v, wgt)) {
    const int px = (int)(i % t.width), py = (int)(i / t.width);
    const float tp = t.t[i];
    const long long q[4] = {i - 1, i + 1, i - t.width, i + t.width};
    const bool in[4] = {px > 0, px + 1 < t.width, py > 0, py + 1 < t.height};
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float r = 0.f;
      if (in[j] && t.s.id[q[j]] >= 0) r = fmaxf(tp - t.t[q[j]], 0.f) / tp;
      s = s + r;
    }
    const float k = 1.f / (1.f + t.strength * s);
    c[0] = c[0] * k, c[1] = c[1] * k, c[2] = c[2] * k;
  }
  t.s.rgb[3 * i] = shade_q(c[0]), t.s.rgb[3 * i + 1] = shade_q(c[1]), t.s.rgb[3 * i + 2] = shade_q(c[2]);
}

// ---- vertex normals: area-weighted sums of the incident faces' normals, in the order of the vertex's corner list -----------
// One thread per vertex walks ITS list (offsets / corners, CSR, ascending by face then corner), so the sum is the sequential
// one of the rule: no atomics, the same bits on every call.  A face's g = e1 x e2 is computed from the face alone, so the
// three vertices of a face add the same three numbers.  A list entry outside [0, 3m) or a range outside the list is skipped,
// never followed.
struct NormalTab {
  const float* xyz;
  long long n;
  const int32_t* faces;
  long long m;
  const int64_t* offsets;
  const int32_t* corners;
  float* out;
};
__global__ __launch_bounds__(kSesBlock) void k_vertex_normals(const NormalTab t) {
#pragma clang fp contract(off)
  const long long vtx = (long long)blockIdx.x * kSesBlock + threadIdx.x;
  if (vtx >= t.n) return;
  const long long lo = max((long long)t.offsets[vtx], 0ll), hi = min((long long)t.offsets[vtx + 1], 3 * t.m);
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (long long e = lo; e < hi; ++e) {
    const int32_t corner = t.corners[e];
    if (corner < 0 || corner >= 3 * t.m) continue;
    const long long face = corner / 3;
    const int32_t a = t.faces[3 * face], b = t.faces[3 * face + 1], c = t.faces[3 * face + 2];
    if (a < 0 || b < 0 || c < 0 || a >= t.n || b >= t.n || c >= t.n) continue;
    const float *pa = t.xyz + 3 * (size_t)a, *pb = t.xyz + 3 * (size_t)b, *pc = t.xyz + 3 * (size_t)c;
    const float e1x = pb[0] - pa[0], e1y = pb[1] - pa[1], e1z = pb[2] - pa[2];
    const float e2x = pc[0] - pa[0], e2y = pc[1] - pa[1], e2z = pc[2] - pa[2];
    const float gx = e1y * e2z - e1z * e2y, gy = e1z * e2x - e1x * e2z, gz = e1x * e2y - e1y * e2x;
    const float inf = __builtin_inff();
    if (!(fabsf(gx) < inf && fabsf(gy) < inf && fabsf(gz) < inf)) continue;   // (NaN fails the tests)
    sx = sx + gx, sy = sy + gy, sz = sz + gz;
  }
  const float l2 = (sx * sx + sy * sy) + sz * sz;
  float nx = 0.f, ny = 0.f, nz = 0.f;
  if (l2 > 0.f && l2 < __builtin_inff()) {
    const float len = sqrtf(l2);
    nx = sx / len, ny = sy / len, nz = sz / len;
  }
  t.out[3 * vtx] = nx, t.out[3 * vtx + 1] = ny, t.out[3 * vtx + 2] = nz;
}

// ---- the annotation in the view: the label image, object outlines and click markers (rules of ours; the header states them) --
// Both are per-pixel passes: no atomics, no workspace, two calls give the same bytes.
//
// THE LABEL RULE: a cloud's pixel shows its vertex's label; a mesh's pixel the label of its face's HEAVIEST corner, with
// w = (1 - u) - v: corner 0 if w >= u && w >= v, else corner 1 if u >= v, else corner 2 (ties -> the lower corner; NaN weights
// fail every test and end at corner 2).  -1 where shade_base shows the background.  Label values pass through unchecked.
struct LabelTab {
  const int32_t* id;
  const float *u, *v;
  const int32_t* faces;
  long long m, n;
  const int32_t* labels;
  int32_t* out;
  long long pixels;
};
__global__ __launch_bounds__(kSesBlock) void k_render_labels(const LabelTab t) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x;
  if (i >= t.pixels) return;
  const int32_t id = t.id[i];
  int32_t lab = -1;
  if (!t.faces) {
    if (id >= 0 && id < t.n) lab = t.labels[id];
  } else if (id >= 0 && id < t.m) {
    const int32_t f0 = t.faces[3 * (size_t)id], f1 = t.faces[3 * (size_t)id + 1], f2 = t.faces[3 * (size_t)id + 2];
    if (f0 >= 0 && f1 >= 0 && f2 >= 0 && f0 < t.n && f1 < t.n && f2 < t.n) {
      const float u = t.u[i], v = t.v[i], w = (1.f - u) - v;
      lab = t.labels[(w >= u && w >= v) ? f0 : (u >= v ? f1 : f2)];
    }
  }
  t.out[i] = lab;
}

// THE ANNOTATION RULE, per pixel p = (px, py), in this order: (1) the bytes of rgb_in; (2) if outlines are on and L_p >= 1 and
// a 4-neighbour INSIDE the image has a label != L_p: the outline colour; (3) for every marker k in table order with
// d2 = dx*dx + dy*dy (dx = (float)px - x_k, dy = (float)py - y_k), d2 <= radius^2 and t_k - t_p <= depth_slack: the marker's
// colour if d2 <= inner_radius^2, else the border colour -- the last covering marker wins.  A row with a NaN field covers
// nothing: the staging below turns its x into NaN, so its first comparison fails.  Colours are quantised as shade_q does,
// the product and the sum rounded on their own.
// The table is staged into LDS once per workgroup, one field per array: in the loop every lane reads the same address
// (a broadcast), and a pixel that no marker covers touches x, y and t only.  A pixel reads its own colour before it writes
// it and reads its neighbours from the label image, so rgb_out may be rgb_in.
static_assert(kSesBlock >= A3D_MAX_CLICKS, "k_render_annotate stages one marker per thread");
struct AnnotTab {
  const uint8_t* in;
  const int32_t* label;
  const float* t;
  const float* markers;
  int n_markers, outlines;
  float r2, i2, slack;
  float outline[3], border[3];
  uint8_t* out;
  int width, height;
  long long pixels;
};
__device__ __forceinline__ uint8_t annot_q(float c) {
#pragma clang fp contract(off)
  const float s = fminf(fmaxf(c, 0.f), 1.f) * 255.f;
  return (uint8_t)(s + 0.5f);
}
__global__ __launch_bounds__(kSesBlock) void k_render_annotate(const AnnotTab a) {
#pragma clang fp contract(off)
  __shared__ float mx[A3D_MAX_CLICKS], my[A3D_MAX_CLICKS], mt[A3D_MAX_CLICKS], mc[A3D_MAX_CLICKS][3];
  if ((int)threadIdx.x < a.n_markers) {
    const float* row = a.markers + 6 * (size_t)threadIdx.x;
    float f[6];
    bool nan = false;
#pragma unroll
    for (int j = 0; j < 6; ++j) f[j] = row[j], nan |= f[j] != f[j];
    mx[threadIdx.x] = nan ? __builtin_nanf("") : f[0], my[threadIdx.x] = f[1], mt[threadIdx.x] = f[2];
    mc[threadIdx.x][0] = f[3], mc[threadIdx.x][1] = f[4], mc[threadIdx.x][2] = f[5];
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * kSesBlock + threadIdx.x;
  if (i >= a.pixels) return;
  const int px = (int)((unsigned)i % (unsigned)a.width), py = (int)((unsigned)i / (unsigned)a.width);   // (pixels <= 4096^2)
  uint8_t c0 = a.in[3 * i], c1 = a.in[3 * i + 1], c2 = a.in[3 * i + 2];
  if (a.outlines) {
    const int32_t lab = a.label[i];
    if (lab >= 1) {
      const bool edge = (px > 0 && a.label[i - 1] != lab) || (px + 1 < a.width && a.label[i + 1] != lab) ||
                        (py > 0 && a.label[i - a.width] != lab) || (py + 1 < a.height && a.label[i + a.width] != lab);
      if (edge) c0 = annot_q(a.outline[0]), c1 = annot_q(a.outline[1]), c2 = annot_q(a.outline[2]);
    }
  }
  if (a.n_markers) {
    const float fx = (float)px, fy = (float)py, tp = a.t[i];
    int hit = -1;
    bool inner = false;
    for (int k = 0; k < a.n_markers; ++k) {
      const float dx = fx - mx[k], dy = fy - my[k];
      const float xx = dx * dx, yy = dy * dy;
      const float d2 = xx + yy;
      const float behind = mt[k] - tp;
      const bool cover = (d2 <= a.r2) & (behind <= a.slack);        // (no short circuit: the loop stays free of branches)
      hit = cover ? k : hit, inner = cover ? d2 <= a.i2 : inner;
    }
    if (hit >= 0) {
      c0 = annot_q(inner ? mc[hit][0] : a.border[0]);
      c1 = annot_q(inner ? mc[hit][1] : a.border[1]);
      c2 = annot_q(inner ? mc[hit][2] : a.border[2]);
    }
  }
  a.out[3 * i] = c0, a.out[3 * i + 1] = c1, a.out[3 * i + 2] = c2;
}

// Host: what the bound needs from a camera, in double.  false: a camera the renders refuse.
static bool render_camera(const a3d_camera* c, RenderCam& r) {
  if (!c || c->width < 1 || c->height < 1 || c->width > A3D_RENDER_MAX_SIZE || c->height > A3D_RENDER_MAX_SIZE) return false;
  double M[9];                                 // columns du, dv, d00
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(c->o[k]) || !std::isfinite(c->d00[k]) || !std::isfinite(c->du[k]) || !std::isfinite(c->dv[k])) return false;
    M[3 * k] = c->du[k], M[3 * k + 1] = c->dv[k], M[3 * k + 2] = c->d00[k];
  }
  const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
  const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
  double scale = 1.;
  for (int col = 0; col < 3; ++col) scale *= std::sqrt(M[col] * M[col] + M[3 + col] * M[3 + col] + M[6 + col] * M[6 + col]);
  if (!(std::fabs(det) > 1e-9 * scale)) return false;   // (du, dv, d00 close to one plane: no camera)
  r.c = *c;
  r.inv[0] = c00 / det, r.inv[1] = (M[2] * M[7] - M[1] * M[8]) / det, r.inv[2] = (M[1] * M[5] - M[2] * M[4]) / det;
  r.inv[3] = c01 / det, r.inv[4] = (M[0] * M[8] - M[2] * M[6]) / det, r.inv[5] = (M[2] * M[3] - M[0] * M[5]) / det;
  r.inv[6] = c02 / det, r.inv[7] = (M[1] * M[6] - M[0] * M[7]) / det, r.inv[8] = (M[0] * M[4] - M[1] * M[3]) / det;
  r.na = std::sqrt(r.inv[0] * r.inv[0] + r.inv[1] * r.inv[1] + r.inv[2] * r.inv[2]);
  r.nb = std::sqrt(r.inv[3] * r.inv[3] + r.inv[4] * r.inv[4] + r.inv[5] * r.inv[5]);
  r.nc = std::sqrt(r.inv[6] * r.inv[6] + r.inv[7] * r.inv[7] + r.inv[8] * r.inv[8]);
  double dmax = 0.;                            // |D| is convex in (u, v): its maximum over the image is at a corner
  for (int corner = 0; corner < 4; ++corner) {
    const double u = (corner & 1) ? c->width - 1 : 0, v = (corner & 2) ? c->height - 1 : 0;
    double s = 0.;
    for (int k = 0; k < 3; ++k) {
      const double x = c->d00[k] + u * c->du[k] + v * c->dv[k];
      s += x * x;
    }
    dmax = std::fmax(dmax, std::sqrt(s));
  }
  r.dmax = dmax * (1. + 1e-6);                 // (the fp32 direction's own rounding)
  r.tiles_x = (c->width + kTile - 1) / kTile, r.tiles_y = (c->height + kTile - 1) / kTile;
  return true;
}
// The section of a call as the kernels take it: NULL for none -- also for one without planes and culling, which then runs
// the very code of the entry points that take no section.
static const a3d_section* section_active(const a3d_section* s) { return s && (s->n_planes || s->cull) ? s : nullptr; }
// false (error set): a section the header refuses.  Host arithmetic only; runs before anything else of a call.
static bool section_ok(const char* what, const a3d_section* s, bool mesh) {
  if (!s) return true;
  if (s->n_planes < 0 || s->n_planes > A3D_SECTION_MAX_PLANES) {
    set_error("%s: section: n_planes = %d, 0..%d planes", what, s->n_planes, A3D_SECTION_MAX_PLANES);
    return false;
  }
  if (s->cull < A3D_CULL_NONE || s->cull > A3D_CULL_FRONT || (!mesh && s->cull != A3D_CULL_NONE)) {
    set_error("%s: section: cull = %d (0 none, 1 back, 2 front; a point cloud has no faces to cull: 0)", what, s->cull);
    return false;
  }
  for (int k = 0; k < s->n_planes; ++k) {
    const float* p = s->planes[k];
    const double n2 = (double)p[0] * p[0] + (double)p[1] * p[1] + (double)p[2] * p[2];
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]) || !std::isfinite(p[3]) || !(n2 >= 0.5 && n2 <= 2.)) {
      set_error("%s: section: plane %d must be finite with 0.5 <= |n|^2 <= 2 (|n|^2 = %g)", what, k, n2);
      return false;
    }
  }
  return true;
}
static int render_run(const char* what, RenderTab& t, const a3d_camera* camera, const a3d_render_out* out, void* ws,
                      size_t ws_bytes, hipStream_t st, const a3d_section* sec) {
  if (!out || !out->id_dev || !out->t_dev || !out->header_dev) {
    set_error("%s: id_dev, t_dev and header_dev are needed", what);
    return A3D_ERR_INVALID;
  }
  if (!render_camera(camera, t.cam)) {
    set_error("%s: bad camera (1..%d pixels each way; o, d00, du, dv finite, d00, du, dv linearly independent)", what,
              A3D_RENDER_MAX_SIZE);
    return A3D_ERR_INVALID;
  }
  if (!ws || ((uintptr_t)ws & 255) || ws_bytes < carve_render(nullptr, t.m, camera->width, camera->height, 0).bytes) {
    set_error("%s: workspace too small or misaligned (a3d_render_workspace_bytes, 256-byte aligned)", what);
    return A3D_ERR_WORKSPACE;
  }
  // the pairs the workspace has room for: what is left behind the fixed tables
  const size_t fixed = carve_render(nullptr, t.m, camera->width, camera->height, 0).bytes - 256;
  t.cap = (long long)((ws_bytes - fixed) / 4);
  if (t.cap > 0xffffffffll) t.cap = 0xffffffffll;
  t.out = *out;
  const RenderWs w = carve_render(ws, t.m, camera->width, camera->height, t.cap);
  A3D_HIP_CHECK(hipMemsetAsync(ws, 0, w.zero_bytes, st));
  A3D_HIP_CHECK(hipMemsetAsync(out->header_dev, 0, sizeof(a3d_render_header), st));
  const unsigned blocks = (unsigned)((t.m + kSesBlock - 1) / kSesBlock);
  if (blocks) {
    k_render_bin<<<blocks, kSesBlock, 0, st>>>(t, w);
    A3D_LAUNCH_CHECK();
  }
  k_render_scan<<<1, 1024, 0, st>>>(t, w);
  A3D_LAUNCH_CHECK();
  if (blocks) {
    k_render_fill<<<blocks, kSesBlock, 0, st>>>(t, w);
    A3D_LAUNCH_CHECK();
  }
  const unsigned tiles = (unsigned)(t.cam.tiles_x * t.cam.tiles_y);
  sec = section_active(sec);
  if (t.mesh && sec)
    k_render_tile_mesh<a3d_section><<<tiles, kTilePixels, 0, st>>>(t, w, *sec);
  else if (t.mesh)
    k_render_tile_mesh<NoSection><<<tiles, kTilePixels, 0, st>>>(t, w, NoSection{});
  else if (sec)
    k_render_tile_points<a3d_section><<<tiles, kTilePixels, 0, st>>>(t, w, *sec);
  else
    k_render_tile_points<NoSection><<<tiles, kTilePixels, 0, st>>>(t, w, NoSection{});
  A3D_LAUNCH_CHECK();
  return A3D_OK;
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
    if (!ses_rows_ok(sp.n, sp.xyz_dev) || !sp.rows_out_dev) {
      set_error("a3d_nearest_rows: source %d: bad arguments (n=%lld)", s, (long long)sp.n);
      return A3D_ERR_INVALID;
    }
    t.xyz[s] = sp.xyz_dev, t.n[s] = sp.n, t.out[s] = sp.rows_out_dev;
    t.n_blocks[s] = (int)capped_grid(sp.n, kSesBlock, kSesMaxBlocks);
    n_max = sp.n > n_max ? sp.n : n_max;
  }
  memcpy(t.q, queries, (size_t)m * 3 * sizeof(float));
  const SesWs w = carve_session(workspace_dev);
  const int nb = (int)capped_grid(n_max, kSesBlock, kSesMaxBlocks);
  k_nearest_rows<<<dim3(nb, n_sources, (m + kSesQT - 1) / kSesQT), kSesBlock, 0, st>>>(t, w.near_part);
  A3D_LAUNCH_CHECK();
  k_nearest_finish<<<1, kSesBlock, 0, st>>>(t, w.near_part);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

// Both a3d_pick_ray (sec NULL) and a3d_pick_ray_section.
static int pick_ray_run(const char* what, const float* xyz_dev, int64_t n, const float* origin, const float* direction,
                        float radius, const a3d_section* sec, a3d_pick_result* result_dev, void* workspace_dev,
                        size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!section_ok(what, sec, false)) return A3D_ERR_INVALID;
  if (!ses_rows_ok(n, xyz_dev) || !origin || !direction || !result_dev || !(radius >= 0.f)) {
    set_error("%s: bad arguments (n=%lld radius=%g)", what, (long long)n, (double)radius);
    return A3D_ERR_INVALID;
  }
  if (!ses_unit_direction(what, direction)) return A3D_ERR_INVALID;
  if (!ses_ws_ok(workspace_dev, workspace_bytes, what)) return A3D_ERR_WORKSPACE;
  PickTab t;
  t.xyz = xyz_dev, t.n = n;
  for (int k = 0; k < 3; ++k) t.o[k] = origin[k], t.d[k] = direction[k];
  t.r2 = radius * radius;
  t.out = result_dev;
  const SesWs w = carve_session(workspace_dev);
  const int nb = (int)capped_grid(n, kSesBlock, kSesMaxBlocks);
  sec = section_active(sec);
  if (sec)
    k_pick_ray<a3d_section><<<nb, kSesBlock, 0, st>>>(t, w.pick_a, w.pick_row, *sec);
  else
    k_pick_ray<NoSection><<<nb, kSesBlock, 0, st>>>(t, w.pick_a, w.pick_row, NoSection{});
  A3D_LAUNCH_CHECK();
  k_pick_finish<<<1, 64, 0, st>>>(t, w.pick_a, w.pick_row, nb);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
extern "C" int a3d_pick_ray(const float* xyz_dev, int64_t n, const float* origin, const float* direction, float radius,
                            a3d_pick_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return pick_ray_run("a3d_pick_ray", xyz_dev, n, origin, direction, radius, nullptr, result_dev, workspace_dev,
                      workspace_bytes, stream);
}
extern "C" int a3d_pick_ray_section(const float* xyz_dev, int64_t n, const float* origin, const float* direction, float radius,
                                    const a3d_section* section, a3d_pick_result* result_dev, void* workspace_dev,
                                    size_t workspace_bytes, void* stream) {
  return pick_ray_run("a3d_pick_ray_section", xyz_dev, n, origin, direction, radius, section, result_dev, workspace_dev,
                      workspace_bytes, stream);
}

// Both a3d_pick_mesh (sec NULL) and a3d_pick_mesh_section.
static int pick_mesh_run(const char* what, const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m,
                         const float* origin, const float* direction, const a3d_section* sec, a3d_pick_mesh_result* result_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!section_ok(what, sec, true)) return A3D_ERR_INVALID;
  if (!ses_rows_ok(n, xyz_dev) || !ses_rows_ok(m, faces_dev) || !origin || !direction || !result_dev) {
    set_error("%s: bad arguments (n=%lld m=%lld)", what, (long long)n, (long long)m);
    return A3D_ERR_INVALID;
  }
  if (!ses_unit_direction(what, direction)) return A3D_ERR_INVALID;
  if (!ses_ws_ok(workspace_dev, workspace_bytes, what)) return A3D_ERR_WORKSPACE;
  MeshTab t;
  t.xyz = xyz_dev, t.n = n, t.faces = faces_dev, t.m = m;
  for (int k = 0; k < 3; ++k) t.r.o[k] = origin[k];
  ses_shear(direction, t.r);
  t.out = result_dev;
  const SesWs w = carve_session(workspace_dev);
  const int nb = (int)capped_grid(m, kSesBlock, kSesMaxBlocks);
  sec = section_active(sec);
  if (sec)                                     // the ray's interval, here on the host: what a pixel of the view derives for the same ray
    k_pick_mesh<RayCut><<<nb, kSesBlock, 0, st>>>(t, w.mesh_key, w.mesh_flag, ses_ray_cut(*sec, t.r.o, direction));
  else
    k_pick_mesh<NoSection><<<nb, kSesBlock, 0, st>>>(t, w.mesh_key, w.mesh_flag, NoSection{});
  A3D_LAUNCH_CHECK();
  k_pick_mesh_finish<<<1, 64, 0, st>>>(t, w.mesh_key, w.mesh_flag, nb);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
extern "C" int a3d_pick_mesh(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m, const float* origin,
                             const float* direction, a3d_pick_mesh_result* result_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream) {
  return pick_mesh_run("a3d_pick_mesh", xyz_dev, n, faces_dev, m, origin, direction, nullptr, result_dev, workspace_dev,
                       workspace_bytes, stream);
}
extern "C" int a3d_pick_mesh_section(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m, const float* origin,
                                     const float* direction, const a3d_section* section, a3d_pick_mesh_result* result_dev,
                                     void* workspace_dev, size_t workspace_bytes, void* stream) {
  return pick_mesh_run("a3d_pick_mesh_section", xyz_dev, n, faces_dev, m, origin, direction, section, result_dev, workspace_dev,
                       workspace_bytes, stream);
}
extern "C" int a3d_section_ray(const a3d_section* section, const float* origin, const float* direction, float* out3) {
  if (!section_ok("a3d_section_ray", section, true)) return A3D_ERR_INVALID;
  if (!origin || !direction || !out3) {
    set_error("a3d_section_ray: origin, direction and out3 are needed");
    return A3D_ERR_INVALID;
  }
  a3d_section none;
  none.n_planes = 0, none.cull = A3D_CULL_NONE;
  const RayCut c = ses_ray_cut(section ? *section : none, origin, direction);
  out3[0] = c.t_lo, out3[1] = c.t_hi, out3[2] = c.empty ? 1.f : 0.f;
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
  k_session_paint<<<capped_grid(a.n_full, kSesBlock, 2048), kSesBlock, 0, st>>>(a);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" size_t a3d_render_workspace_bytes(int64_t n_primitives, int width, int height, int64_t pair_capacity) {
  if (n_primitives < 0 || pair_capacity < 0 || width < 1 || height < 1 || width > A3D_RENDER_MAX_SIZE || height > A3D_RENDER_MAX_SIZE)
    return 0;
  return carve_render(nullptr, n_primitives, width, height, pair_capacity).bytes;
}

extern "C" int a3d_render_camera_bounds(const a3d_camera* camera, double* out13) {
  RenderCam r;
  if (!out13 || !render_camera(camera, r)) {
    set_error("a3d_render_camera_bounds: bad camera");
    return A3D_ERR_INVALID;
  }
  for (int k = 0; k < 9; ++k) out13[k] = r.inv[k];
  out13[9] = r.na, out13[10] = r.nb, out13[11] = r.nc, out13[12] = r.dmax;
  return A3D_OK;
}

// Both a3d_render_mesh (sec NULL) and a3d_render_mesh_section.
static int render_mesh_run(const char* what, const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m,
                           const a3d_camera* camera, const a3d_section* sec, const a3d_render_out* out, void* workspace_dev,
                           size_t workspace_bytes, void* stream) {
  if (!section_ok(what, sec, true)) return A3D_ERR_INVALID;
  if (!ses_rows_ok(n, xyz_dev) || !ses_rows_ok(m, faces_dev)) {
    set_error("%s: bad arguments (n=%lld m=%lld)", what, (long long)n, (long long)m);
    return A3D_ERR_INVALID;
  }
  RenderTab t;
  memset(&t, 0, sizeof(t));
  t.xyz = xyz_dev, t.n = n, t.faces = faces_dev, t.mesh = 1, t.m = m;
  return render_run(what, t, camera, out, workspace_dev, workspace_bytes, (hipStream_t)stream, sec);
}
extern "C" int a3d_render_mesh(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m, const a3d_camera* camera,
                               const a3d_render_out* out, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return render_mesh_run("a3d_render_mesh", xyz_dev, n, faces_dev, m, camera, nullptr, out, workspace_dev, workspace_bytes, stream);
}
extern "C" int a3d_render_mesh_section(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m,
                                       const a3d_camera* camera, const a3d_section* section, const a3d_render_out* out,
                                       void* workspace_dev, size_t workspace_bytes, void* stream) {
  return render_mesh_run("a3d_render_mesh_section", xyz_dev, n, faces_dev, m, camera, section, out, workspace_dev,
                         workspace_bytes, stream);
}

// Both a3d_render_points (sec NULL) and a3d_render_points_section.
static int render_points_run(const char* what, const float* xyz_dev, int64_t n, float radius, const a3d_camera* camera,
                             const a3d_section* sec, const a3d_render_out* out, void* workspace_dev, size_t workspace_bytes,
                             void* stream) {
  if (!section_ok(what, sec, false)) return A3D_ERR_INVALID;
  if (!ses_rows_ok(n, xyz_dev) || !(radius >= 0.f) || !std::isfinite(radius)) {
    set_error("%s: bad arguments (n=%lld radius=%g)", what, (long long)n, (double)radius);
    return A3D_ERR_INVALID;
  }
  RenderTab t;
  memset(&t, 0, sizeof(t));
  t.xyz = xyz_dev, t.n = n, t.faces = nullptr, t.mesh = 0, t.m = n;
  t.r2 = radius * radius, t.radius = radius;
  return render_run(what, t, camera, out, workspace_dev, workspace_bytes, (hipStream_t)stream, sec);
}
extern "C" int a3d_render_points(const float* xyz_dev, int64_t n, float radius, const a3d_camera* camera,
                                 const a3d_render_out* out, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return render_points_run("a3d_render_points", xyz_dev, n, radius, camera, nullptr, out, workspace_dev, workspace_bytes, stream);
}
extern "C" int a3d_render_points_section(const float* xyz_dev, int64_t n, float radius, const a3d_camera* camera,
                                         const a3d_section* section, const a3d_render_out* out, void* workspace_dev,
                                         size_t workspace_bytes, void* stream) {
  return render_points_run("a3d_render_points_section", xyz_dev, n, radius, camera, section, out, workspace_dev, workspace_bytes,
                           stream);
}

extern "C" int a3d_render_shade(const int32_t* id_dev, const float* u_dev, const float* v_dev, const int32_t* faces_dev, int64_t m,
                                const float* colors_dev, int64_t n, const float* background, uint8_t* rgb_dev, int width,
                                int height, void* stream) {
  if (!id_dev || !rgb_dev || !background || width < 1 || height < 1 || width > A3D_RENDER_MAX_SIZE || height > A3D_RENDER_MAX_SIZE ||
      n < 0 || m < 0 || (n && !colors_dev) || (faces_dev && (!u_dev || !v_dev))) {
    set_error("a3d_render_shade: bad arguments (%d x %d, n=%lld m=%lld; a mesh needs u_dev and v_dev)", width, height,
              (long long)n, (long long)m);
    return A3D_ERR_INVALID;
  }
  const ShadeTab t = shade_tab(id_dev, u_dev, v_dev, faces_dev, m, colors_dev, n, background, rgb_dev, (long long)width * height);
  k_render_shade<<<(unsigned)((t.pixels + kSesBlock - 1) / kSesBlock), kSesBlock, 0, (hipStream_t)stream>>>(t);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_render_shade_lit(const int32_t* id_dev, const float* u_dev, const float* v_dev, const int32_t* faces_dev,
                                    int64_t m, const float* colors_dev, int64_t n, const float* normals_dev,
                                    const a3d_camera* camera, float ambient, const float* background, uint8_t* rgb_dev,
                                    void* stream) {
  RenderCam rc;
  if (!id_dev || !u_dev || !v_dev || !rgb_dev || !background || n < 0 || m < 0 || (m && !faces_dev) ||
      (n && (!colors_dev || !normals_dev)) || !(ambient >= 0.f && ambient <= 1.f) || !render_camera(camera, rc)) {
    set_error("a3d_render_shade_lit: bad arguments (n=%lld m=%lld ambient=%g; u_dev, v_dev, normals_dev and a camera the "
              "renders accept are needed, ambient in [0, 1])", (long long)n, (long long)m, (double)ambient);
    return A3D_ERR_INVALID;
  }
  LitTab t;
  t.s = shade_tab(id_dev, u_dev, v_dev, faces_dev, m, colors_dev, n, background, rgb_dev, (long long)camera->width * camera->height);
  t.normals = normals_dev, t.cam = *camera, t.ambient = ambient;
  const unsigned blocks = (unsigned)((t.s.pixels + kSesBlock - 1) / kSesBlock);
  if (m == 0) {                                // no face: no id is good.  The flat pass as a cloud without vertices: all background
    t.s.faces = nullptr, t.s.n = 0;
    k_render_shade<<<blocks, kSesBlock, 0, (hipStream_t)stream>>>(t.s);
  } else {
    k_render_shade_lit<<<blocks, kSesBlock, 0, (hipStream_t)stream>>>(t);
  }
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_render_shade_lit_points(const int32_t* id_dev, const float* colors_dev, int64_t n, const float* normals_dev,
                                           const a3d_camera* camera, float ambient, const float* background, uint8_t* rgb_dev,
                                           void* stream) {
  RenderCam rc;
  if (!id_dev || !rgb_dev || !background || n < 0 || (n && (!colors_dev || !normals_dev)) || !(ambient >= 0.f && ambient <= 1.f) ||
      !render_camera(camera, rc)) {
    set_error("a3d_render_shade_lit_points: bad arguments (n=%lld ambient=%g; colors_dev, normals_dev and a camera the renders "
              "accept are needed, ambient in [0, 1])", (long long)n, (double)ambient);
    return A3D_ERR_INVALID;
  }
  LitTab t;
  t.s = shade_tab(id_dev, nullptr, nullptr, nullptr, 0, colors_dev, n, background, rgb_dev, (long long)camera->width * camera->height);
  t.normals = normals_dev, t.cam = *camera, t.ambient = ambient;
  k_render_shade_lit_points<<<(unsigned)((t.s.pixels + kSesBlock - 1) / kSesBlock), kSesBlock, 0, (hipStream_t)stream>>>(t);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_render_shade_depth(const int32_t* id_dev, const float* t_dev, const float* u_dev, const float* v_dev,
                                      const int32_t* faces_dev, int64_t m, const float* colors_dev, int64_t n, float strength,
                                      const float* background, uint8_t* rgb_dev, int width, int height, void* stream) {
  if (!id_dev || !t_dev || !rgb_dev || !background || width < 1 || height < 1 || width > A3D_RENDER_MAX_SIZE ||
      height > A3D_RENDER_MAX_SIZE || n < 0 || m < 0 || (n && !colors_dev) || (faces_dev && (!u_dev || !v_dev)) ||
      !(strength >= 0.f) || !std::isfinite(strength)) {
    set_error("a3d_render_shade_depth: bad arguments (%d x %d, n=%lld m=%lld strength=%g; a mesh needs u_dev and v_dev)", width,
              height, (long long)n, (long long)m, (double)strength);
    return A3D_ERR_INVALID;
  }
  DepthTab t;
  t.s = shade_tab(id_dev, u_dev, v_dev, faces_dev, m, colors_dev, n, background, rgb_dev, (long long)width * height);
  t.t = t_dev, t.width = width, t.height = height, t.strength = strength;
  k_render_shade_depth<<<(unsigned)((t.s.pixels + kSesBlock - 1) / kSesBlock), kSesBlock, 0, (hipStream_t)stream>>>(t);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_vertex_normals(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m, const int64_t* offsets_dev,
                                  const int32_t* corners_dev, float* normals_out_dev, void* stream) {
  if (!ses_rows_ok(n, xyz_dev) || m < 0 || 3 * m >= (1ll << 31) || (n && (!offsets_dev || !normals_out_dev)) ||
      (m && (!faces_dev || !corners_dev))) {
    set_error("a3d_vertex_normals: bad arguments (n=%lld m=%lld; 3 m must fit int32)", (long long)n, (long long)m);
    return A3D_ERR_INVALID;
  }
  if (n == 0) return A3D_OK;
  NormalTab t;
  t.xyz = xyz_dev, t.n = n, t.faces = faces_dev, t.m = m, t.offsets = offsets_dev, t.corners = corners_dev, t.out = normals_out_dev;
  k_vertex_normals<<<(unsigned)((n + kSesBlock - 1) / kSesBlock), kSesBlock, 0, (hipStream_t)stream>>>(t);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_render_labels(const int32_t* id_dev, const float* u_dev, const float* v_dev, const int32_t* faces_dev, int64_t m,
                                 const int32_t* labels_dev, int64_t n, int32_t* label_out_dev, int width, int height,
                                 void* stream) {
  if (!id_dev || !label_out_dev || width < 1 || height < 1 || width > A3D_RENDER_MAX_SIZE || height > A3D_RENDER_MAX_SIZE ||
      n < 0 || m < 0 || (n && !labels_dev) || (faces_dev && (!u_dev || !v_dev))) {
    set_error("a3d_render_labels: bad arguments (%d x %d, n=%lld m=%lld; a mesh needs u_dev and v_dev)", width, height,
              (long long)n, (long long)m);
    return A3D_ERR_INVALID;
  }
  LabelTab t;
  t.id = id_dev, t.u = u_dev, t.v = v_dev, t.faces = faces_dev, t.m = m, t.n = n, t.labels = labels_dev, t.out = label_out_dev;
  t.pixels = (long long)width * height;
  k_render_labels<<<(unsigned)((t.pixels + kSesBlock - 1) / kSesBlock), kSesBlock, 0, (hipStream_t)stream>>>(t);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_render_annotate(const uint8_t* rgb_in_dev, const int32_t* label_dev, const float* t_dev,
                                   const float* markers_dev, int n_markers, float radius, float inner_radius, float depth_slack,
                                   const float* outline, const float* border, uint8_t* rgb_out_dev, int width, int height,
                                   void* stream) {
  const bool sizes = width >= 1 && height >= 1 && width <= A3D_RENDER_MAX_SIZE && height <= A3D_RENDER_MAX_SIZE;
  const size_t bytes = sizes ? (size_t)3 * width * height : 0;
  const uintptr_t in = (uintptr_t)rgb_in_dev, out = (uintptr_t)rgb_out_dev;
  if (!sizes || !rgb_in_dev || !rgb_out_dev || !t_dev || !border || (outline && !label_dev) || n_markers < 0 ||
      n_markers > A3D_MAX_CLICKS || (n_markers && !markers_dev) || !std::isfinite(radius) || !std::isfinite(inner_radius) ||
      !(inner_radius >= 0.f && radius >= inner_radius) || !std::isfinite(depth_slack) || !(depth_slack >= 0.f) ||
      (in != out && in < out + bytes && out < in + bytes)) {
    set_error("a3d_render_annotate: bad arguments (%d x %d, markers=%d radius=%g inner_radius=%g depth_slack=%g; at most %d "
              "markers, radius >= inner_radius >= 0, depth_slack >= 0, outlines need label_dev, rgb_out_dev is rgb_in_dev or "
              "apart from it)", width, height, n_markers, (double)radius, (double)inner_radius, (double)depth_slack,
              A3D_MAX_CLICKS);
    return A3D_ERR_INVALID;
  }
  AnnotTab a;
  a.in = rgb_in_dev, a.label = label_dev, a.t = t_dev, a.markers = markers_dev, a.n_markers = n_markers, a.outlines = outline ? 1 : 0;
  a.r2 = radius * radius, a.i2 = inner_radius * inner_radius, a.slack = depth_slack;
  for (int k = 0; k < 3; ++k) a.outline[k] = outline ? outline[k] : 0.f, a.border[k] = border[k];
  a.out = rgb_out_dev, a.width = width, a.height = height, a.pixels = (long long)width * height;
  k_render_annotate<<<(unsigned)((a.pixels + kSesBlock - 1) / kSesBlock), kSesBlock, 0, (hipStream_t)stream>>>(a);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}
