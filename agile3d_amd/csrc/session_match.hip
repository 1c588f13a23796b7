// session_match.hip -- query by example on the backbone's features (gfx950): one prototype per example class, and per voxel
// the best prototype under a cosine threshold.  Entry points: a3d_feature_prototypes, a3d_feature_match.
//
// The reference has no counterpart (its tool never looks at the backbone's output again after the decoder).  THE RULE is stated
// in full in include/agile3d_hip.h and restated in tests/match_rule.py; in short:
//   prototypes: every channel of an example row in fixed point (session_device.h's fixed_point, origin 0, quantum 2^-20, |X| <=
//   2^40), INTEGER sums per class -- no order, no rounding; the division by the count is the host's (view.prototype_table).
//   match: nn, pp_c and dot_c in double with ONE accumulator each, channels ascending; the products of two fp32 values are exact
//   in double, so fma and mul + add give the same bits and only the ORDER of the additions matters -- hence no split across
//   lanes and no matrix cores.  Prototype c passes when dot_c > 0 and dot_c dot_c >= c2 (nn pp_c); the best is found by ONE
//   scan over c ascending with a division-free comparison (a new prototype replaces the best so far only when it is strictly
//   better: ties go to the lower index).  The comparison of rounded products need not be transitive, so the scan's ORDER is
//   part of the rule and one thread walks all prototypes of its voxel.
//
// THE SHAPE.  k_proto_sums: a wave per row, two channels per lane (one 512-byte coalesced load), the row's verdict by a wave
// vote; partial sums of the first 32 classes in LDS (64-bit LDS atomics), flushed with one 64-bit global atomic per non-zero
// entry and workgroup -- the classes beyond go to global atomics directly.  Rows of class -1 are not read at all.
// k_feature_match: a workgroup of ONE wave owns a tile of 64 rows, staged through LDS by coalesced 16-byte loads and read back
// one row per lane (row stride 65 floats: no bank conflict either way); the prototypes are staged as doubles, 16 at a time,
// channel-major, so that a step of the channel loop reads one float of the row and 16 broadcast doubles and issues 16
// independent fmas -- one accumulator per prototype, sixteen prototypes in flight.  The running best (index, dot, dot^2, pp) is
// carried in registers across the chunks of 16.  k_match_lift gathers through the inverse map.
//
// THE SUMMARIES are integer sums reduced per workgroup (session_device.h) and ONE atomic per workgroup and counter.  Stages are
// launches; no grid barrier, no spin-wait.  The library allocates nothing on the device and does not synchronise.
#include "session_device.h"

namespace a3d {

constexpr int kMC = A3D_MATCH_CHANNELS;
constexpr int kMpB = 256;                     // k_proto_sums: four waves, a row each ...
constexpr int kMpWaves = kMpB / 64;
constexpr int kMpBlocks = 1024;               // ... at most four workgroups a CU (32 KB of LDS each)
constexpr int kMpLdsClasses = 32;             // classes whose partial sums live in LDS
constexpr int kMmRows = 64;                   // k_feature_match: the tile = the workgroup = one wave
constexpr int kMmStride = kMmRows + 1;        // floats between two channels of the tile
constexpr int kMmChunk = A3D_MATCH_CHUNK;     // prototypes staged at a time
constexpr int kMmBlocks = 768;                // three workgroups a CU (50 KB of LDS each)
constexpr int kMlB = 256;                     // k_match_lift
constexpr int kMlBlocks = 2048;
static_assert(kMC == 128 && kMmChunk == 16, "the staging loops are written for 128 channels and chunks of 16");
static_assert(sizeof(a3d_prototypes_summary) == 24, "lib.py: PrototypesSummary");
static_assert(sizeof(a3d_match_summary) == 2064, "lib.py: MatchSummary");

// ---- prototypes -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMpB) void k_proto_sums(const float* __restrict__ feats, const int32_t* __restrict__ classes,
                                                     const long long n, const int n_classes, const double quantum, const double lim,
                                                     int64_t* sums, int32_t* count, a3d_prototypes_summary* summary) {
  __shared__ u64 part[kMpLdsClasses * kMC];
  __shared__ int cnt[A3D_MATCH_MAX_PROTOTYPES];
  __shared__ int wave_part[kMpWaves];
  for (int i = threadIdx.x; i < kMpLdsClasses * kMC; i += kMpB) part[i] = 0;
  for (int i = threadIdx.x; i < A3D_MATCH_MAX_PROTOTYPES; i += kMpB) cnt[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long stride = (long long)gridDim.x * kMpWaves;
  int used = 0, left = 0, err = 0;             // lane 0 counts for its wave (n < 2^22: an int)
  for (long long r = (long long)blockIdx.x * kMpWaves + wave; r < n; r += stride) {
    const int c = __builtin_amdgcn_readfirstlane(classes[r]);
    if (c == -1) continue;
    if (c < -1 || c >= n_classes) {
      err = A3D_MATCH_BAD_CLASS;
      continue;
    }
    const float2 f = ((const float2*)(feats + r * kMC))[lane];
    long long x0 = 0, x1 = 0;
    const bool ok0 = fixed_point(f.x, 0.0, quantum, lim, x0), ok1 = fixed_point(f.y, 0.0, quantum, lim, x1);
    if (!__all(ok0 && ok1)) {                  // one channel out of range or not finite: the row is left out as a whole
      left += lane == 0;
      continue;
    }
    if (c < kMpLdsClasses) {
      if (x0) atomicAdd(&part[c * kMC + 2 * lane], (u64)x0);
      if (x1) atomicAdd(&part[c * kMC + 2 * lane + 1], (u64)x1);
    } else {
      add_i64(&sums[(size_t)c * kMC + 2 * lane], x0), add_i64(&sums[(size_t)c * kMC + 2 * lane + 1], x1);
    }
    if (lane == 0) atomicAdd(&cnt[c], 1);
    used += lane == 0;
  }
  __syncthreads();
  const int in_lds = (n_classes < kMpLdsClasses ? n_classes : kMpLdsClasses) * kMC;
  for (int i = threadIdx.x; i < in_lds; i += kMpB) add_i64(&sums[i], (long long)part[i]);
  for (int i = threadIdx.x; i < n_classes; i += kMpB)
    if (cnt[i]) atomicAdd(&count[i], cnt[i]);
  const long long s_used = block_sum<kMpB>(used, wave_part), s_left = block_sum<kMpB>(left, wave_part);
  if (threadIdx.x == 0) add_i64(&summary->examples, s_used), add_i64(&summary->examples_left_out, s_left);
  send_error(&summary->err, err);
}

// ---- match ----------------------------------------------------------------------------------------------------------------
struct MatchK {
  const float* feats;
  long long n;
  const float* protos;
  const int32_t* proto_class;
  const uint8_t* candidate;
  int k;
  double c2;
  int32_t* match_qv;
  int32_t* best_qv;
  float* score_qv;
  a3d_match_summary* summary;
};

// The running state of one voxel's scan: the best prototype overall and the best among the passing ones.
struct MatchScan {
  int best = -1, match = -1, match_class = -1;
  double b_dot = 0.0, b_d2 = 0.0, b_pp = 1.0, m_d2 = 0.0, m_pp = 1.0;
};

// THE step of the scan: prototype c (0 < pp < +inf) with its dot product against the state.  Every product rounded on its own.
__device__ __forceinline__ void scan_step(MatchScan& s, const int c, const int cls, const double dot, const double pp,
                                          const double nn, const double c2) {
#pragma clang fp contract(off)
  const double d2 = dot * dot;
  bool beats = s.best < 0;
  if (!beats) {
    const int sa = (dot > 0.0) - (dot < 0.0), sb = (s.b_dot > 0.0) - (s.b_dot < 0.0);
    const double l = d2 * s.b_pp, r = s.b_d2 * pp;
    beats = sa != sb ? sa > sb : sa > 0 ? l > r : sa < 0 ? l < r : false;
  }
  if (beats) s.best = c, s.b_dot = dot, s.b_d2 = d2, s.b_pp = pp;
  if (dot > 0.0 && d2 >= c2 * (nn * pp) && (s.match < 0 || d2 * s.m_pp > s.m_d2 * pp))
    s.match = c, s.match_class = cls, s.m_d2 = d2, s.m_pp = pp;
}

__global__ __launch_bounds__(kMmRows) void k_feature_match(const MatchK a) {
  __shared__ float tile[kMC * kMmStride];      // tile[i * 65 + r]: channel i of row r
  __shared__ double protos[kMC * kMmChunk];    // protos[i * 16 + c]: channel i of the chunk's prototype c, 0 beyond k
  __shared__ double pp_s[kMmChunk];
  __shared__ int class_s[kMmChunk];
  __shared__ int hist[A3D_MATCH_MAX_PROTOTYPES];
  __shared__ int wave_part[1];
  const int t = threadIdx.x;
  for (int i = t; i < A3D_MATCH_MAX_PROTOTYPES; i += kMmRows) hist[i] = 0;
  const long long tiles = (a.n + kMmRows - 1) / kMmRows;
  const int chunks = (a.k + kMmChunk - 1) / kMmChunk;
  bool staged = false;                         // with one chunk the prototypes are staged once a workgroup
  int n_odd = 0, err = 0;
  for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
    const long long row0 = tl * kMmRows;
    __syncthreads();                           // (the tile before is read)
#pragma unroll 4
    for (int j = 0; j < 32; ++j) {             // 8 rows x 128 bytes a step: whole cache lines, and 32 distinct banks a half wave
      const int q = (t & 7) + 8 * (j & 3), r = (t >> 3) + 8 * (j >> 2);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row0 + r < a.n) v = ((const float4*)(a.feats + (row0 + r) * kMC))[q];
      float* dst = &tile[4 * q * kMmStride + r];
      dst[0] = v.x, dst[kMmStride] = v.y, dst[2 * kMmStride] = v.z, dst[3 * kMmStride] = v.w;
    }
    __syncthreads();
    const long long row = row0 + t;
    const bool live = row < a.n;
    double nn = 0.0;
    bool odd = false;
    for (int i = 0; i < kMC; ++i) {
      const float f = tile[i * kMmStride + t];
      odd |= not_finite(f);
      nn = fma((double)f, (double)f, nn);
    }
    n_odd += live && odd;
    const bool can = live && !odd && nn > 0.0 && (!a.candidate || a.candidate[row] != 0);
    MatchScan s;
    for (int ch = 0; ch < chunks; ++ch) {
      if (!(staged && chunks == 1)) {
        __syncthreads();                       // (the chunk before is read)
        for (int e = 0; e < kMC * kMmChunk / kMmRows; ++e) {
          const int idx = t + kMmRows * e, c = idx & (kMmChunk - 1), i = idx >> 4, pc = ch * kMmChunk + c;   // (LDS word idx)
          protos[idx] = pc < a.k ? (double)a.protos[(size_t)pc * kMC + i] : 0.0;
        }
        __syncthreads();
        if (t < kMmChunk) {
          const int pc = ch * kMmChunk + t;
          double pp = 0.0;
          for (int i = 0; i < kMC; ++i) pp = fma(protos[i * kMmChunk + t], protos[i * kMmChunk + t], pp);
          const int cls = pc < a.k ? a.proto_class[pc] : -1;
          pp_s[t] = pp, class_s[t] = cls;
          if (pc < a.k && !(pp < INFINITY)) err |= A3D_MATCH_BAD_PROTOTYPE;     // (a NaN fails the comparison too)
          if (pc < a.k && (cls < 0 || cls >= A3D_MATCH_MAX_PROTOTYPES)) err |= A3D_MATCH_BAD_CLASS;
        }
        __syncthreads();
        staged = true;
      }
      double acc[kMmChunk];
#pragma unroll
      for (int c = 0; c < kMmChunk; ++c) acc[c] = 0.0;
      for (int i = 0; i < kMC; ++i) {
        const double f = (double)tile[i * kMmStride + t];
#pragma unroll
        for (int c = 0; c < kMmChunk; ++c) acc[c] = fma(f, protos[i * kMmChunk + c], acc[c]);
      }
      const int kc = a.k - ch * kMmChunk;
      if (can) {
#pragma unroll
        for (int c = 0; c < kMmChunk; ++c) {
          const double pp = pp_s[c];
          if (c < kc && pp > 0.0 && pp < INFINITY) scan_step(s, ch * kMmChunk + c, class_s[c], acc[c], pp, nn, a.c2);
        }
      }
    }
    if (live) {
      a.match_qv[row] = s.match < 0 ? -1 : s.match_class;
      a.best_qv[row] = s.best;
      a.score_qv[row] = s.best < 0 ? 0.f : (float)(s.b_dot / sqrt(nn * s.b_pp));
      if (s.match >= 0 && s.match_class >= 0 && s.match_class < A3D_MATCH_MAX_PROTOTYPES) atomicAdd(&hist[s.match_class], 1);
    }
  }
  __syncthreads();
  for (int i = t; i < A3D_MATCH_MAX_PROTOTYPES; i += kMmRows) add_i64(&a.summary->matched[i], hist[i]);
  const long long s_odd = block_sum<kMmRows>(n_odd, wave_part);
  if (t == 0) add_i64(&a.summary->rows_nonfinite, s_odd);
  send_error(&a.summary->err, err);
}

// match_full[j] = match_qv[inverse_map[j]], score_full likewise; an index outside 0 .. n-1 is flagged and not followed.
__global__ __launch_bounds__(kMlB) void k_match_lift(const int64_t* __restrict__ inverse_map, const long long n_full, const long long n,
                                                     const int32_t* __restrict__ match_qv, const float* __restrict__ score_qv,
                                                     int32_t* __restrict__ match_full, float* __restrict__ score_full, int32_t* err_dev) {
  const long long stride = (long long)gridDim.x * kMlB;
  int err = 0;
  for (long long j = (long long)blockIdx.x * kMlB + threadIdx.x; j < n_full; j += stride) {
    const long long v = inverse_map[j];
    if (v < 0 || v >= n) {
      err = A3D_MATCH_BAD_INDEX;
      continue;
    }
    match_full[j] = match_qv[v], score_full[j] = score_qv[v];
  }
  send_error(err_dev, err);
}

}  // namespace a3d

using namespace a3d;

extern "C" int a3d_feature_prototypes(const a3d_feature_prototypes_args* a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!a || a->n < 0 || a->n >= A3D_MATCH_MAX_EXAMPLE_ROWS || a->n_classes < 1 || a->n_classes > A3D_MATCH_MAX_PROTOTYPES ||
      (a->n > 0 && (!a->feats_dev || !a->classes_dev)) || ((uintptr_t)a->feats_dev & 15) || !a->sums_dev || !a->count_dev ||
      !a->summary_dev || ((uintptr_t)a->sums_dev & 7) || ((uintptr_t)a->summary_dev & 7)) {
    if (!a)
      set_error("a3d_feature_prototypes: no arguments");
    else
      set_error("a3d_feature_prototypes: bad arguments (n=%lld n_classes=%d feats %s classes %s sums %s count %s summary %s; 0 <= n "
                "< 2^22, 1 <= n_classes <= %d, feats 16-byte and sums and summary 8-byte aligned are needed)", (long long)a->n,
                a->n_classes, a->feats_dev ? "given" : "NULL", a->classes_dev ? "given" : "NULL", a->sums_dev ? "given" : "NULL",
                a->count_dev ? "given" : "NULL", a->summary_dev ? "given" : "NULL", A3D_MATCH_MAX_PROTOTYPES);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a->sums_dev, 0, (size_t)a->n_classes * kMC * sizeof(int64_t), st));
  A3D_HIP_CHECK(hipMemsetAsync(a->count_dev, 0, (size_t)a->n_classes * sizeof(int32_t), st));
  A3D_HIP_CHECK(hipMemsetAsync(a->summary_dev, 0, sizeof(a3d_prototypes_summary), st));
  if (a->n == 0) return A3D_OK;
  const double quantum = std::ldexp(1.0, -A3D_MATCH_QUANTUM_BITS), lim = std::ldexp(1.0, A3D_MATCH_FIXED_BITS);
  k_proto_sums<<<capped_grid(a->n, kMpWaves, kMpBlocks), kMpB, 0, st>>>(a->feats_dev, a->classes_dev, a->n, a->n_classes, quantum, lim,
                                                                     a->sums_dev, a->count_dev, a->summary_dev);
  A3D_LAUNCH_CHECK();
  return A3D_OK;
}

extern "C" int a3d_feature_match(const a3d_feature_match_args* a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!a) {
    set_error("a3d_feature_match: no arguments");
    return A3D_ERR_INVALID;
  }
  const bool lift = a->inverse_map_dev != nullptr;
  if (a->n < 0 || a->n >= (1ll << 31) || a->k < 1 || a->k > A3D_MATCH_MAX_PROTOTYPES || !a->protos_dev || !a->proto_class_dev ||
      (a->n > 0 && (!a->feats_dev || !a->match_qv_dev || !a->best_qv_dev || !a->score_qv_dev)) || ((uintptr_t)a->feats_dev & 15) ||
      !a->summary_dev || ((uintptr_t)a->summary_dev & 7) || a->n_full < 0 || a->n_full >= (1ll << 31) || (!lift && a->n_full != 0) ||
      (lift ? a->n_full > 0 && (!a->match_full_dev || !a->score_full_dev) : a->match_full_dev || a->score_full_dev)) {
    set_error("a3d_feature_match: bad arguments (n=%lld k=%d n_full=%lld feats %s protos %s proto_class %s match_qv %s best_qv %s "
              "score_qv %s summary %s inverse_map %s match_full %s score_full %s; 0 <= n, n_full < 2^31, 1 <= k <= %d, feats "
              "16-byte and summary 8-byte aligned, match_full, score_full and n_full exactly with inverse_map are needed)",
              (long long)a->n, a->k, (long long)a->n_full, a->feats_dev ? "given" : "NULL", a->protos_dev ? "given" : "NULL",
              a->proto_class_dev ? "given" : "NULL", a->match_qv_dev ? "given" : "NULL", a->best_qv_dev ? "given" : "NULL",
              a->score_qv_dev ? "given" : "NULL", a->summary_dev ? "given" : "NULL", lift ? "given" : "NULL",
              a->match_full_dev ? "given" : "NULL", a->score_full_dev ? "given" : "NULL", A3D_MATCH_MAX_PROTOTYPES);
    return A3D_ERR_INVALID;
  }
  if (!(a->cos_min >= 0.0 && a->cos_min <= 1.0)) {                     // (a NaN fails the first)
    set_error("a3d_feature_match: cos_min=%g must lie in [0, 1]", a->cos_min);
    return A3D_ERR_INVALID;
  }
  A3D_HIP_CHECK(hipMemsetAsync(a->summary_dev, 0, sizeof(a3d_match_summary), st));
  if (a->n > 0) {
    MatchK m;
    m.feats = a->feats_dev, m.n = a->n, m.protos = a->protos_dev, m.proto_class = a->proto_class_dev, m.candidate = a->candidate_dev;
    m.k = a->k, m.match_qv = a->match_qv_dev, m.best_qv = a->best_qv_dev, m.score_qv = a->score_qv_dev, m.summary = a->summary_dev;
    m.c2 = a->cos_min * a->cos_min;            // rounded once
    k_feature_match<<<capped_grid(a->n, kMmRows, kMmBlocks), kMmRows, 0, st>>>(m);
    A3D_LAUNCH_CHECK();
  }
  if (lift && a->n_full > 0) {
    k_match_lift<<<capped_grid(a->n_full, kMlB, kMlBlocks), kMlB, 0, st>>>(a->inverse_map_dev, a->n_full, a->n, a->match_qv_dev,
                                                                         a->score_qv_dev, a->match_full_dev, a->score_full_dev,
                                                                         &a->summary_dev->err);
    A3D_LAUNCH_CHECK();
  }
  return A3D_OK;
}
