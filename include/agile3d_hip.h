/*
 * agile3d_hip.h -- C ABI of libagile3d_hip.so (MI355X / gfx950).
 *
 * The reference (ywyue/AGILE3D) is pure Python and has no FFI of its own: its hot path
 * calls MinkowskiEngine (third-party C++/CUDA) and torch.nn.  This header is the boundary a
 * maintainer would bind instead (ctypes stub in INTEGRATION.md).  Every entry point cites the
 * reference interface it replaces (paths relative to the reference repository).
 *
 * Conventions
 *   - every pointer named *_dev is a DEVICE pointer owned by the caller; the library never
 *     allocates device memory: callers pass workspaces sized by the *_workspace_bytes queries.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - all feature matrices are row-major fp32; coordinates are int32 (batch, x, y, z).
 *   - return value: 0 = ok, negative = error (a3d_last_error() gives the text; thread-local).
 *   - no exceptions cross the ABI; a scene/program handle is not thread-safe, distinct
 *     handles are independent.
 */
#ifndef AGILE3D_HIP_H
#define AGILE3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define A3D_OK                 0
#define A3D_ERR_INVALID       -1   /* bad argument */
#define A3D_ERR_HIP           -2   /* HIP runtime error */
#define A3D_ERR_COORD_RANGE   -3   /* |xyz| >= 2^17 or batch index > 1022 */
#define A3D_ERR_DUPLICATE     -4   /* duplicate voxel coordinates */
#define A3D_ERR_WORKSPACE     -5   /* workspace too small */
#define A3D_ERR_UNSUPPORTED   -6   /* shape outside what the kernels are built for */

#define A3D_NUM_LEVELS 5           /* tensor strides 1,2,4,8,16 (res16unet.py:222-295) */

/* Version of this interface: bumped whenever a struct grows or a buffer contract changes (2: a3d_op's fused-head fields, the
 * third block of a3d_decoder_sample::kv0_dev + kv0_blocks; 3: a3d_conv_wgrad needs a3d_scene_build_wgrad_lists; 4: the hyper-parameters of a3d_adamw_step and a3d_adamw_step_multi are doubles).  A host binding compares it with the header it was written
 * against before the first call (agile3d_amd/lib.py does). */
#define A3D_ABI_VERSION 4
int         a3d_version(void);
const char* a3d_last_error(void);
/* plain hipMemcpy device->host (+ stream sync); lets non-torch hosts and tests read tables */
int         a3d_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optional kernel timing (bench.py's live roofline numbers).  While enabled, every launch of the
 * kernels listed below is bracketed by a hipEvent pair on the launch stream.
 * ------------------------------------------------------------------------------------------ */
enum {
  A3D_PROF_SPCONV = 0,      /* k_conv_sk / k_conv_deep / k_conv_wl (3^3 / 2^3 s2 / transposed / small 1x1) */
  A3D_PROF_SPLITK = 1,      /* retired (the split-K reduction launches of round 1)          */
  A3D_PROF_STEM = 2,        /* 5^3 stem                                                  */
  A3D_PROF_C2S = 3,         /* click-to-scene attention                                  */
  A3D_PROF_QUERY = 4,       /* query-side chain (one workgroup)                          */
  A3D_PROF_S2C = 5,         /* scene-to-click attention                                  */
  A3D_PROF_LNMASK = 6,      /* LayerNorm + mask head                                     */
  A3D_PROF_POSENC = 7,      /* Fourier position encoding                                 */
  A3D_PROF_SCENE_SORT = 8,  /* keys + radix sort + level compaction                      */
  A3D_PROF_SCENE_TABLES = 9,/* hash, neighbour tables, row clustering                    */
  A3D_PROF_CLICKS = 10,     /* click simulator (error clusters + nearest outside point)  */
  A3D_PROF_DENSE = 11       /* k_dense: N-point nn.Linear / 1x1 conv (no gather)          */
};
typedef struct {
  int32_t id, bn, kernel_volume, cin, cout, n_out, table, level, ksplit;
  float   ms;
} a3d_prof_entry;
int a3d_profile_enable(int on);
int a3d_profile_read(a3d_prof_entry* out, int max_entries);   /* returns #entries, clears */

/* ------------------------------------------------------------------------------------------
 * Scene = the coordinate manager.
 * Replaces: ME.SparseTensor(coordinates=, features=, device=) (engine.py:47-51,
 * eval_multi_obj.py:94-98) and the coordinate manager every ME layer consults implicitly
 * (voxel hash, stride-2 coordinate sets, kernel maps for 3^3 / 5^3 / 2^3-stride-2 kernels).
 * Rows of level 0 keep the caller's order at the API surface; internally every level is
 * re-ordered (Morton super-tiles, rows clustered by neighbour pattern) -- see DESIGN.md.
 * ------------------------------------------------------------------------------------------ */
typedef struct a3d_scene a3d_scene;

/* Stable ascending sort of (uint64 key, int32 value) pairs by the key bits [bit_begin, bit_end): the LSD radix sort the
 * scene build uses for its three sorts (csrc/radix.hip; replaces the sorts MinkowskiEngine's coordinate manager runs
 * inside `ME.SparseTensor(...)` / `MinkowskiConvolution` kernel-map construction, reference models/agile3d.py:163-170).
 * Exposed for the tests (a stand-alone call: up to 128 k pairs as ONE launch with grid barriers, so not next to another
 * barrier kernel of the process).  keys_in / vals_in are only read. */
size_t  a3d_sort_pairs_workspace_bytes(int64_t n);
int     a3d_sort_pairs_u64(const uint64_t* keys_in_dev, const int32_t* vals_in_dev, int64_t n, int bit_begin, int bit_end,
                           uint64_t* keys_out_dev, int32_t* vals_out_dev, void* workspace_dev, size_t workspace_bytes,
                           void* stream);

/* a3d_scene_create synchronises `stream` once (the level sizes come back to the host).  It may be called from several host
 * threads / on several streams at once: a scene-sized input (<= 128 k voxels) runs its first sort and the level compaction as
 * ONE launch each with grid barriers inside, but only when no other call of the process is between its first launch and that
 * synchronisation (a process-wide counter); every other case uses launch chains whose workgroups wait only for workgroups
 * that already run.  A3D_SORT_ONE_LAUNCH=0 keeps the chains everywhere. */
size_t  a3d_scene_workspace_bytes(int64_t n_voxels);
int     a3d_scene_create(const int32_t* coords4_dev, int64_t n_voxels,
                         void* workspace_dev, size_t workspace_bytes,
                         void* stream, a3d_scene** out);
void    a3d_scene_destroy(a3d_scene* s);
int64_t a3d_scene_level_size(const a3d_scene* s, int level);
/* batch samples are contiguous row ranges in ascending batch order (ME.utils.batched_coordinates,
 * datasets/InterMultiObj3DSegDataset.py:129); returns their number B and writes the first row of
 * sample i to starts_out[i] (i < max_out); sample i ends where sample i+1 starts (the last at n). */
int     a3d_scene_batch_ranges(const a3d_scene* s, int64_t* starts_out, int max_out);
/* Level-0 voxel lookup structure chosen by a3d_scene_create: returns 1 and the (x, y, z) cell counts when the batch's
 * bounding box was small enough for a dense voxel -> row grid (at most 64 cells per voxel), 0 when the hash table is
 * used (results are identical; A3D_GRID=0 in the environment forces the hash table). */
int     a3d_scene_grid_dims(const a3d_scene* s, int dims_out[3]);

/* read-only views of the scene tables (device pointers valid while the workspace lives) */
enum {
  A3D_TAB_XYZB      = 0,  /* int32 [n][4]  (x,y,z,batch) in level units, internal row order       */
  A3D_TAB_NBR27     = 1,  /* int32 [27][npad]  3^3 neighbour rows, missing -> n (the zero row)    */
  A3D_TAB_GMASK27   = 2,  /* uint32 [npad/16]  offsets present in each 16-row group               */
  A3D_TAB_CHILD8    = 3,  /* int32 [8][npad(level+1)] rows of `level` under each coarse row       */
  A3D_TAB_GMASKDOWN = 4,  /* uint32 [npad(level+1)/16]                                            */
  A3D_TAB_UP8       = 5,  /* int32 [8][npad] parent row (level+1) of virtual row v at its slot    */
  A3D_TAB_GMASKUP   = 6,  /* uint32 [npad/16]                                                     */
  A3D_TAB_UPROWS    = 7,  /* int32 [npad] virtual row -> row of `level`                           */
  A3D_TAB_ORIGROW   = 8,  /* int32 [n0]   internal level-0 row -> caller's row                    */
  /* 9: retired (tile order of the former dynamic tile queue) */
  A3D_TAB_PRE27     = 10, /* int32 [npad/64+1] (tile, offset) pairs of the 3^3 map before each 64-row tile */
  A3D_TAB_PREDOWN   = 11, /* int32 [npad(level+1)/64+1] same for the stride-2 map                       */
  A3D_TAB_PREUP     = 12  /* int32 [npad/64+1] same for the transposed map                              */
};
int a3d_scene_table(const a3d_scene* s, int level, int which, const void** ptr_dev, int64_t* count);

/* ------------------------------------------------------------------------------------------
 * Backbone program.
 * Replaces: Res16UNetBase.forward (models/res16unet.py:222-295), BasicBlock.forward
 * (models/modules/resnet_block.py:48-64), ME.MinkowskiConvolution / ConvolutionTranspose /
 * BatchNorm / ReLU / cat, and lin_squeeze_head (models/agile3d.py:43-45,179).
 * The host describes the network as a list of ops over numbered activation buffers (the
 * topology stays where the reference keeps it: in the host language); the library runs it.
 * ------------------------------------------------------------------------------------------ */
enum {
  A3D_OP_STEM   = 0,  /* 5^3 (or 3^3) conv, Cin=3, input = caller features          (res16unet.py:225) */
  A3D_OP_CONV3  = 1,  /* 3^3 stride-1 conv on `level_in`                           (resnet_block.py:24-43) */
  A3D_OP_DOWN   = 2,  /* 2^3 stride-2 conv level_in -> level_in+1                  (res16unet.py:229,...) */
  A3D_OP_UP     = 3,  /* 2^3 stride-2 transposed conv level_in -> level_in-1       (res16unet.py:253,...) */
  A3D_OP_LINEAR = 4   /* 1x1 conv                                                  (resnet.py:108-123)   */
};
#define A3D_BUF_NONE       -1
#define A3D_BUF_EXT_OUT    -2   /* out: caller's [n0][cout] matrix, rows in the CALLER's order */

typedef struct {
  int32_t level;       /* rows = a3d_scene_level_size(level) + 1 (last row = zeros) */
  int32_t channels;    /* row stride in floats */
} a3d_buf_desc;

typedef struct {
  int32_t kind;
  int32_t level_in;
  int32_t cin, cout;
  int32_t in_buf,  in_coff;    /* input  = columns [in_coff, in_coff+cin)   of buffer in_buf  */
  int32_t out_buf, out_coff;   /* output = columns [out_coff, out_coff+cout) of buffer out_buf */
  int32_t res_buf, res_coff;   /* residual added before the ReLU, or A3D_BUF_NONE             */
  int32_t relu;
  int32_t kernel_volume;       /* 125 / 27 / 8 / 1 */
  const float* w_dev;          /* weights packed by a3d_pack_conv_weight (STEM: raw [K][3][32]) */
  const float* scale_dev;      /* [cout] folded BatchNorm scale, or NULL (=1)                   */
  const float* shift_dev;      /* [cout] folded BatchNorm shift / bias, or NULL (=0)            */
  /* CONV3 only, proj_cin > 0: the block's residual projection fused into this conv (BasicBlock.downsample: 1x1 conv +
   * BatchNorm on the BLOCK INPUT, resnet_block.py:59-61; models/resnet.py:108-123) -- out = act(conv3(in) + proj_in W1x1 +
   * shift).  w_dev then holds the 27 offsets' packed weights followed by the packed 1x1 weight [proj_cin][cout], BOTH with
   * their BatchNorm scale already multiplied in (scale_dev = NULL), shift_dev the sum of the two shifts; proj_in = columns
   * [proj_coff, proj_coff + proj_cin) of buffer proj_buf (same level).  proj_cin = 0: no projection. */
  int32_t proj_buf, proj_coff, proj_cin, reserved_;
  /* head_cout > 0 (a level-0 op whose output has <= 128 columns): a 1x1 layer applied to this op's OUTPUT rows as a second
   * GEMM in the same kernel's epilogue -- lin_squeeze_head behind block8's last conv (models/agile3d.py:43-45,179): the
   * workgroup holds complete output rows, so ext_out[caller row][0 .. head_cout) = out_row @ head_w + head_bias is
   * written without reading the rows back.  head_w_dev: packed [1][cout][head_cout] (a3d_pack_conv_weight), head_bias_dev
   * [head_cout] or NULL; the result goes to a3d_program_run's ext_out (rows in the CALLER's order).  Shapes without a fused
   * build run the 1x1 layer as its own launch (same arithmetic). */
  const float* head_w_dev;
  const float* head_bias_dev;
  int32_t head_cout, reserved2_;
} a3d_op;

/* W[K][cin][cout] (ME layout, models/modules/common.py:137-155) -> MFMA B-fragment order */
int a3d_pack_conv_weight(const float* w_dev, int kernel_volume, int cin, int cout,
                         float* packed_dev, void* stream);
/* floats the packed form of a [kernel_volume][cin][cout] weight occupies: kernel_volume * cin * cout (the packing only
 * reorders).  Size `packed_dev` of a3d_pack_conv_weight with it. */
size_t a3d_conv_weight_packed_floats(int kernel_volume, int cin, int cout);

size_t a3d_program_workspace_bytes(const a3d_scene* s, const a3d_buf_desc* bufs, int n_bufs,
                                   const a3d_op* ops, int n_ops);
/* byte offset of activation buffer i inside the program workspace (for aux feature maps) */
size_t a3d_program_buffer_offset(const a3d_scene* s, const a3d_buf_desc* bufs, int n_bufs, int i);
int    a3d_program_run(const a3d_scene* s, const a3d_buf_desc* bufs, int n_bufs,
                       const a3d_op* ops, int n_ops,
                       const float* feats3_dev,     /* [n0][3] caller order (STEM input)   */
                       float* ext_out_dev, int ext_out_ld,
                       void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the sparse convolutions (first part): what MinkowskiEngine's autograd
 * computes for `losses.backward()` (engine.py:137-150) through conv / conv_tr (models/modules/common.py:125-188).
 * dL/dx needs no entry point of its own: it is a3d_program_run on the transposed kernel map with transposed weights
 * (3^3: W'[k] = W[26-k]^T, same op; stride 2 <-> transposed with W_s^T; 1x1: W^T) -- agile3d_amd/backward.py.
 * a3d_conv_wgrad: dW[k][ci][co] = sum over the pairs (r_in, r_out) of offset k of x[r_in][ci] * dy[r_out][co];
 * kind / level_in as in the op struct: A3D_OP_CONV3 / DOWN / UP / LINEAR, x [n_in][ldx], dy [n_out][ldy] in the scene's
 * internal row order, channels multiples of 32, dw_dev [K][cin][cout] (ME layout).  Deterministic (fixed summation
 * order).
 * a3d_scene_build_wgrad_lists: once per scene before the first a3d_conv_wgrad on it (the 3^3 / stride-2 / transposed kinds
 * refuse without it): for every kernel map of the scene and every offset k, the 16-position groups that have offset k, so
 * that the kernel's work items are equal cuts of these lists instead of equal cuts of the rows.  The workspace
 * (a3d_scene_wgrad_lists_bytes) must live as long as the scene is used for weight gradients.  The call does not synchronise:
 * the list lengths travel to a pinned host buffer behind an event, and the first a3d_conv_wgrad /
 * a3d_conv_wgrad_workspace_bytes on the scene waits for them (the launch plans are made on the host).
 * ------------------------------------------------------------------------------------------ */
size_t a3d_scene_wgrad_lists_bytes(const a3d_scene* s);
int    a3d_scene_build_wgrad_lists(a3d_scene* s, void* workspace_dev, size_t workspace_bytes, void* stream);
size_t a3d_conv_wgrad_workspace_bytes(const a3d_scene* s, int kind, int level_in, int cin, int cout);
int    a3d_conv_wgrad(const a3d_scene* s, int kind, int level_in, const float* x_dev, int ldx,
                      const float* dy_dev, int ldy, int cin, int cout, float* dw_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* One sparse convolution on the caller's own buffers -- the forward AND (on the transposed map, see above) the input
 * gradient of the training tapes, which keep every activation; the inference path runs whole programs instead.
 *   y[n_out (+1)][ldy] = conv(x[n_in + 1][ldx]; w_packed)      no BatchNorm / ReLU / residual
 * x carries the zero row (row n_in all zeros: what a missing neighbour gathers); with y_zero_row != 0 row n_out of y is
 * written as zeros (the zero row of the next layer).  Deterministic.  Workspace: a3d_conv_apply_workspace_bytes. */
size_t a3d_conv_apply_workspace_bytes(const a3d_scene* s, int kind, int level_in, int cin, int cout);
int    a3d_conv_apply(const a3d_scene* s, int kind, int level_in, const float* x_dev, int ldx, int cin,
                      const float* w_packed_dev, int cout, float* y_dev, int ldy, int y_zero_row,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same convolution with what the training tapes need on top (round 5):
 *   a3d_conv_apply_acc: y = conv(x) + res  -- res_dev [n_out][ldr] may be y itself: a gradient accumulated IN the conv's
 *     epilogue (the input-gradient convs of a node with several consumers: no separate add pass);
 *     state_dev: a3d_conv_state_bytes() bytes ZEROED by the caller (the kernel's hand-off ticket and flags; one block per
 *     conv of an iteration, cleared with one memset for all of them) or NULL (cleared here, one memset per call).
 *   a3d_conv_bn_train_forward: conv -> BatchNorm on the statistics of THIS batch (+ res)(ReLU), the block of
 *     BasicBlock.forward (resnet_block.py:48-64) in training mode: raw_dev [n_out][ld_raw] = the conv's output (kept for
 *     the backward), y_dev as a3d_bn_train_forward's.  The batch statistics come out of the conv kernel's epilogue (per
 *     64-row tile: column sums and squared deviations from the tile mean, merged in fp64 in a fixed order), so the raw
 *     output is not read again for them. */
size_t a3d_conv_state_bytes(void);
/* Small levels (a layer with a few stages of work per CU: levels 2-4 of one scene; res16unet.py:89-147,242-259) run on
 * k_conv_deep -- static (tile, column block, part) workgroups, both operands by LDS-DMA three stages ahead, a cut tile
 * finished by its last arriver -- instead of the stream-K kernel.  mode 1 (default; A3D_CONV_DEEP in the environment) uses it
 * where its cost model prefers it, 0 never; mode < 0 only queries; mode >= 16 forces a geometry (tuning only: bn / 32 |
 * ch / 32 << 4 | parts << 8 | two-slot ring << 19, tools/conv_bench.py --sweep).  Returns the mode in force before the call.  Workspaces
 * sized under one mode stay valid under the other (the launch falls back to the stream-K kernel when the slab is short). */
int    a3d_conv_deep_mode(int mode);
int    a3d_conv_apply_acc(const a3d_scene* s, int kind, int level_in, const float* x_dev, int ldx, int cin,
                          const float* w_packed_dev, int cout, float* y_dev, int ldy, int y_zero_row,
                          const float* res_dev, int ldr, void* state_dev, void* workspace_dev, size_t workspace_bytes,
                          void* stream);
/*   a3d_conv_dgrad_bn: the input-gradient conv (kind / level_in of the BACKWARD op, i.e. the transposed map) whose result
 *     completes dL/dy of a BatchNorm(+ReLU) unit's output y [n_out][ldy]: g = (conv(x) (+ g when acc)) masked by y > 0 is
 *     written to g_dev (row n_out zeroed) and sums_dev [2][cout] (fp64) = sum g, sum g xhat with xhat = (raw - mean) rstd come
 *     out of the conv kernel's epilogue -- what a3d_bn_backward_apply needs (with relu = 0: g is masked already), without a
 *     pass over dy, y and raw for the sums.  Workspace: a3d_conv_bn_train_workspace_bytes of the same op. */
int    a3d_conv_dgrad_bn(const a3d_scene* s, int kind, int level_in, const float* x_dev, int ldx, int cin,
                         const float* w_packed_dev, int cout, float* g_dev, int ldg, int acc, const float* y_dev, int ldy,
                         const float* raw_dev, int ld_raw, const float* mean_dev, const float* rstd_dev, int relu,
                         double* sums_dev, void* state_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
size_t a3d_conv_bn_train_workspace_bytes(const a3d_scene* s, int kind, int level_in, int cin, int cout);
int    a3d_conv_bn_train_forward(const a3d_scene* s, int kind, int level_in, const float* x_dev, int ldx, int cin,
                                 const float* w_packed_dev, int cout, float* raw_dev, int ld_raw,
                                 const float* gamma_dev, const float* beta_dev, float eps, const float* res_dev, int ldr,
                                 int relu, float* y_dev, int ldy, int y_zero_row, float* save_mean_dev,
                                 float* save_rstd_dev, float* running_mean_dev, float* running_var_dev, float momentum,
                                 void* state_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* weight gradient of the input convolution conv0p1s1 (5^3 or 3^3, 3 -> 32; res16unet.py:225): feats3_dev in the
 * caller's row order as for a3d_program_run, dy_dev [n0][lddy >= 32] in internal row order, dw_dev [K][3][32] */
size_t a3d_stem_wgrad_workspace_bytes(int kernel_volume);
/* the size that also lets a3d_stem_wgrad run its matrix-core path (round 5: dW as one [384 x 32] MFMA accumulator per wave,
 * voxels walked in Morton order against Morton-ordered colours kept behind the partials; dense level-0 grid, 5^3 only) --
 * with the smaller workspace above the per-offset kernel runs */
size_t a3d_stem_wgrad_scene_workspace_bytes(const a3d_scene* s, int kernel_volume);
int    a3d_stem_wgrad(const a3d_scene* s, const float* feats3_dev, const float* dy_dev, int lddy, int kernel_volume,
                      float* dw_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* BatchNorm in training mode over the [n][C] rows (ME.MinkowskiBatchNorm = nn.BatchNorm1d over the rows of the whole
 * batch, models/modules/common.py:22), with the residual add and ReLU of BasicBlock.forward (resnet_block.py:48-64):
 *   forward : y = relu?((x - mean) * rstd * gamma + beta (+ res)); mean / rstd of THIS batch are saved for the
 *             backward; running statistics (optional) are updated like torch (momentum, unbiased variance);
 *             y_zero_row != 0: y has n + 1 rows and row n is written as zeros (what a missing neighbour gathers)
 *   backward: g = dy masked by (y > 0) when relu; dres (optional) = g; dbeta = sum g; dgamma = sum g * xhat;
 *             dx = gamma * rstd * (g - dbeta / n - xhat * dgamma / n); zero_row != 0: dx (and dres) have n + 1 rows,
 *             row n written as zeros
 * C a multiple of 32 that divides 768 (32 .. 384), leading dimensions multiples of 4.  Deterministic. */
size_t a3d_bn_workspace_bytes(int64_t n, int C);
int    a3d_bn_train_forward(const float* x_dev, int ldx, int64_t n, int C, const float* gamma_dev,
                            const float* beta_dev, float eps, const float* res_dev, int ldr, int relu,
                            float* y_dev, int ldy, float* save_mean_dev, float* save_rstd_dev,
                            float* running_mean_dev, float* running_var_dev, float momentum, int y_zero_row,
                            void* workspace_dev, size_t workspace_bytes, void* stream);
int    a3d_bn_train_backward(const float* x_dev, int ldx, const float* y_dev, int ldy, const float* dy_dev, int lddy,
                             int64_t n, int C, const float* gamma_dev, const float* save_mean_dev,
                             const float* save_rstd_dev, int relu, float* dx_dev, int lddx, float* dres_dev,
                             int lddres, float* dgamma_dev, float* dbeta_dev, int zero_row,
                             void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same BatchNorm in pieces, for statistics that span the data-parallel ranks (SyncBN; the reference normalises over
 * all rows of the batch on ONE device, models/modules/common.py:20-22 -- with one scene per rank the strict equivalent
 * exchanges [2C+1] numbers per layer).  The caller combines the per-rank numbers between the calls
 * (agile3d_amd/backward.py: all_gather + Chan's parallel variance for the forward, all_reduce for the backward).
 *   a3d_bn_local_stats    : stats[0..C) = mean of THIS call's rows, stats[C..2C) = sum (x - that mean)^2   (fp64)
 *   a3d_bn_apply          : y = relu?((x - mean) rstd gamma + beta (+ res)) with the GIVEN mean / rstd
 *   a3d_bn_backward_sums  : sums[0..C) = sum g, sums[C..2C) = sum g xhat over THIS call's rows (fp64), g = dy (y > 0)
 *   a3d_bn_backward_apply : dx from the GLOBAL sums / row count; dgamma, dbeta = the LOCAL sums (they are averaged over
 *                           the ranks with every other parameter gradient afterwards, as DDP + SyncBatchNorm do) */
int    a3d_bn_local_stats(const float* x_dev, int ldx, int64_t n, int C, double* stats_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream);
int    a3d_bn_apply(const float* x_dev, int ldx, int64_t n, int C, const float* gamma_dev, const float* beta_dev,
                    const float* mean_dev, const float* rstd_dev, const float* res_dev, int ldr, int relu,
                    float* y_dev, int ldy, int y_zero_row, void* stream);
int    a3d_bn_backward_sums(const float* x_dev, int ldx, const float* y_dev, int ldy, const float* dy_dev, int lddy,
                            int64_t n, int C, const float* mean_dev, const float* rstd_dev, int relu,
                            double* sums_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int    a3d_bn_backward_apply(const float* x_dev, int ldx, const float* y_dev, int ldy, const float* dy_dev, int lddy,
                             int64_t n, int C, const float* gamma_dev, const float* mean_dev, const float* rstd_dev,
                             int relu, const double* global_sums_dev, int64_t n_global, const double* local_sums_dev,
                             float* dx_dev, int lddx, float* dres_dev, int lddres, float* dgamma_dev,
                             float* dbeta_dev, int zero_row, void* stream);
/* out[c] = sum over rows of x[i][c] (bias gradient of lin_squeeze_head, agile3d.py:43-45); workspace as above */
int    a3d_column_sums(const float* x_dev, int ldx, int64_t n, int C, float* out_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream);

/* nn.LayerNorm over the channels of every row (the decoder's norms: attention_block.py:38,98,155; agile3d.py:137),
 * forward and backward (C a multiple of 64, <= 512; dx has the layout of x; workspace: a3d_bn_workspace_bytes(n, C)) */
int    a3d_layernorm_forward(const float* x_dev, int ldx, int64_t n, int C, const float* gamma_dev,
                             const float* beta_dev, float eps, float* y_dev, int ldy, void* stream);
int    a3d_layernorm_backward(const float* x_dev, int ldx, const float* dy_dev, int lddy, int64_t n, int C,
                              const float* gamma_dev, float eps, float* dx_dev, float* dgamma_dev, float* dbeta_dev,
                              void* workspace_dev, size_t workspace_bytes, void* stream);
/* dW [cin][cout] = x^T dy for row-major [n][ld] matrices: weight gradient of the decoder's nn.Linear layers (the input
 * gradient dy W^T is a3d_linear with the transposed weight) */
size_t a3d_linear_wgrad_workspace_bytes(int64_t n, int cin, int cout);
int    a3d_linear_wgrad(const float* x_dev, int ldx, const float* dy_dev, int ldy, int64_t n, int cin, int cout,
                        float* dw_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same gradient written where the caller accumulates it (what autograd's AccumulateGrad does for an nn.Linear of
 * attention_block.py / agile3d.py:51-55): dW as [cin][cout] (transposed = 0) or [cout][cin] (transposed = 1: nn.Linear.weight's
 * layout; a row slice of nn.MultiheadAttention's packed in_proj_weight is such a block at an offset) with leading dimension
 * ld_dw, assigned (accumulate = 0) or added; db_dev != NULL: the bias gradient, the column sums of dy, from the same pass over
 * dy, assigned or added (db_accumulate) */
size_t a3d_linear_wgrad_into_workspace_bytes(int64_t n, int cin, int cout);
int    a3d_linear_wgrad_into(const float* x_dev, int ldx, const float* dy_dev, int ldy, int64_t n, int cin, int cout,
                             float* dw_dev, int ld_dw, int transposed, int accumulate, float* db_dev, int db_accumulate,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/* Attention and mask-head primitives with their backward (training path of the decoder; the inference path uses the
 * fused kernels behind a3d_decoder_forward).  nn.MultiheadAttention (attention_block.py) = scores -> softmax -> apply
 * on [heads, Lq, Lk]; q / k / v are row-major [L][H*dh].  mask_dev: uint8 [Lq][Lk], non-zero = blocked (-inf).
 *   a3d_attn_scores        S[h][i][j] = scale * sum_d q[i][h*dh+d] k[j][h*dh+d]
 *   a3d_softmax_rows       in place over the last dimension of [rows][L]
 *   a3d_softmax_rows_backward   dP <- P * (dP - sum_j P dP)
 *   a3d_attn_apply         transposed = 0: O[i][c] = scale * sum_j P[h(c)][i][j] V[j][c];  1: O[j][c] = scale * sum_i P[h(c)][i][j] V[i][c]
 *   a3d_group_max(_backward)    per-object max over an object's queries (agile3d.py:353-360) and its gradient routing */
int a3d_attn_scores(const float* q_dev, const float* k_dev, int64_t Lq, int64_t Lk, int H, int dh, float scale,
                    const unsigned char* mask_dev, float* S_dev, void* stream);
int a3d_softmax_rows(float* S_dev, int64_t rows, int64_t L, void* stream);
int a3d_softmax_rows_backward(const float* P_dev, float* dP_dev, int64_t rows, int64_t L, void* stream);
/* the same over the MIDDLE dimension of [H][Lq][Lk] (scores kept transposed: scene-to-click attention stores
 * [head][query][point] so that the 80 k-long point index is the fastest one everywhere) */
int a3d_softmax_cols(float* S_dev, int H, int64_t Lq, int64_t Lk, void* stream);
int a3d_softmax_cols_backward(const float* P_dev, float* dP_dev, int H, int64_t Lq, int64_t Lk, void* stream);
size_t a3d_attn_apply_workspace_bytes(int64_t Lq, int64_t Lk, int H, int dh, int transposed);
int a3d_attn_apply(const float* P_dev, const float* V_dev, int64_t Lq, int64_t Lk, int H, int dh, int transposed,
                   float scale, float* O_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
int a3d_group_max(const float* lq_dev, int64_t N, int Q, const int32_t* qbeg_dev, const int32_t* qend_dev, int G,
                  float* out_dev, int32_t* arg_dev, void* stream);
int a3d_group_max_backward(const float* dout_dev, const int32_t* arg_dev, int64_t N, int Q, int G, float* dlq_dev,
                           void* stream);
/* The attention mask of the NEXT decoder layer from this layer's mask logits (agile3d.py:362-383: `attn_mask` of the
 * click-to-scene attention; not differentiated): label[n] = first arg-max over the G = 1 + K logits of point n,
 * mask[q][n] = (label[n] != group_of_query[q]) && (some point carries group_of_query[q])  -- uint8 [Q][N], non-zero = blocked;
 * the second term is the reference's "a query that would be blocked everywhere is blocked nowhere" (agile3d.py:369,375). */
size_t a3d_next_layer_mask_workspace_bytes(int64_t N, int G);
int a3d_next_layer_mask(const float* logits_dev, int64_t N, int G, const int32_t* group_of_query_dev, int Q,
                        unsigned char* mask_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same attention in the flash formulation, for the two attentions of a decoder layer that have the N points on one
 * side (attention_block.py:86-98 as called at agile3d.py:283-290 and :305-312; 8 heads x 16 channels fixed): nothing of
 * size [heads, Lq, Lk] is written; the forward pass keeps the softmax statistics (row maximum, row sum), the backward
 * pass recomputes the probabilities tile by tile from them.  q_scaled = q / sqrt(16) (the caller scales: exact), so
 * dL/dq = dq_scaled / 4.  mask_dev: uint8 [Lq][Lk], non-zero = blocked, or NULL.
 *   click-to-scene (few queries, Lk = N keys):  o [Lq][128], stats [2][8][Lq] (max, sum)
 *   scene-to-click (Lq = N queries, few keys):  o [Lq][128], stats [Lq][8][2]
 * Reductions over the N points (dq of click-to-scene; dk, dv of scene-to-click) are per-chunk partial sums added in
 * chunk order by a second kernel: results are bit-identical run to run. */
size_t a3d_flash_c2s_workspace_bytes(int64_t Lq, int64_t Lk);
int a3d_flash_c2s_forward(const float* q_scaled_dev, const float* k_dev, const float* v_dev, const unsigned char* mask_dev,
                          int64_t Lq, int64_t Lk, float* o_dev, float* stats_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream);
int a3d_flash_c2s_backward(const float* q_scaled_dev, const float* k_dev, const float* v_dev, const unsigned char* mask_dev,
                           int64_t Lq, int64_t Lk, const float* o_dev, const float* stats_dev, const float* d_o_dev,
                           float* dq_scaled_dev, float* dk_dev, float* dv_dev, void* workspace_dev, size_t workspace_bytes,
                           void* stream);
size_t a3d_flash_s2c_workspace_bytes(int64_t Lq, int64_t Lk);
int a3d_flash_s2c_forward(const float* q_scaled_dev, const float* k_dev, const float* v_dev, int64_t Lq, int64_t Lk,
                          float* o_dev, float* stats_dev, void* stream);
int a3d_flash_s2c_backward(const float* q_scaled_dev, const float* k_dev, const float* v_dev, int64_t Lq, int64_t Lk,
                           const float* o_dev, const float* stats_dev, const float* d_o_dev, float* dq_scaled_dev,
                           float* dk_dev, float* dv_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Dropout of the training decoder (nn.Dropout / nn.MultiheadAttention(dropout=p) of attention_block.py in training mode):
 * every mask is regenerated where it is used from a counter-based RNG (Philox4x32-10, key = seed), nothing of the shape
 * of an attention is stored.  Element (h, i, j) of site `site_code` (= 8 * decoder pass + site) of batch
 * sample `sample` is kept iff word (j & 3) of philox({j >> 2, h * rows + i, sample, site_code}, seed) >= floor(p 2^32);
 * a kept value is scaled by 1 / (1 - p) (fp32).  0 <= p < 1. */
typedef struct a3d_dropout {
  uint64_t seed;
  float p;
  int32_t sample;
  int32_t site_code;
  int32_t reserved_;
} a3d_dropout;
/* the keep mask itself, uint8 [heads][rows][cols] (1 = kept): for tests; the hot path never writes a mask */
int a3d_dropout_mask(uint64_t seed, int sample, int site_code, float p, int heads, int64_t rows, int64_t cols,
                     unsigned char* out_dev, void* stream);
/* the flash attentions with dropout on the probabilities that multiply V (the softmax statistics stay those of the
 * undropped scores; the backward regenerates the mask: dS = P (Z dP - D), dV = (P Z)^T dO, D = rowsum(dO o O) of the
 * dropped output); rows of the site = the attention's queries, columns = its keys.  Workspaces as without dropout. */
int a3d_flash_c2s_forward_dropout(const float* q_scaled_dev, const float* k_dev, const float* v_dev,
                                  const unsigned char* mask_dev, int64_t Lq, int64_t Lk, float* o_dev, float* stats_dev,
                                  void* workspace_dev, size_t workspace_bytes, a3d_dropout drop, void* stream);
int a3d_flash_c2s_backward_dropout(const float* q_scaled_dev, const float* k_dev, const float* v_dev,
                                   const unsigned char* mask_dev, int64_t Lq, int64_t Lk, const float* o_dev,
                                   const float* stats_dev, const float* d_o_dev, float* dq_scaled_dev, float* dk_dev,
                                   float* dv_dev, void* workspace_dev, size_t workspace_bytes, a3d_dropout drop,
                                   void* stream);
int a3d_flash_s2c_forward_dropout(const float* q_scaled_dev, const float* k_dev, const float* v_dev, int64_t Lq,
                                  int64_t Lk, float* o_dev, float* stats_dev, a3d_dropout drop, void* stream);
int a3d_flash_s2c_backward_dropout(const float* q_scaled_dev, const float* k_dev, const float* v_dev, int64_t Lq,
                                   int64_t Lk, const float* o_dev, const float* stats_dev, const float* d_o_dev,
                                   float* dq_scaled_dev, float* dk_dev, float* dv_dev, void* workspace_dev,
                                   size_t workspace_bytes, a3d_dropout drop, void* stream);
/* the materialised path (a3d_attn_scores / softmax / apply): out = Z o P for P [H][Lq][Lk] (transposed = 0) or stored as
 * [H][Lk][Lq] (transposed = 1; the site's rows are still the Lq queries), in place allowed.  Forward: applied to the
 * softmax output before a3d_attn_apply; backward: to dP before the softmax backward (dV from the dropped P). */
int a3d_attn_dropout(const float* P_dev, int H, int64_t Lq, int64_t Lk, int transposed, float* out_dev, a3d_dropout drop,
                     void* stream);
/* row-wise sites on [rows][cols] (heads = 1), one batch sample's rows:
 *   forward:  y = res + Z o f(x), f = relu (relu != 0) or the identity; res_dev may be NULL (then y = Z o f(x))
 *   backward: dx = Z o dy o (x_pre > 0 if x_pre_dev != NULL) */
int a3d_dropout_rows_forward(const float* x_dev, const float* res_dev, float* y_dev, int64_t rows, int cols, int relu,
                             a3d_dropout drop, void* stream);
int a3d_dropout_rows_backward(const float* dy_dev, const float* x_pre_dev, float* dx_dev, int64_t rows, int cols,
                              a3d_dropout drop, void* stream);

/* Optimiser step of the reference's training loop: torch.optim.AdamW(lr, weight_decay) (main.py:125-127) after
 * clip_grad_norm_(parameters, max_norm) (engine.py:145-150).  a3d_sum_squares returns sum g^2 of one tensor to the
 * host (the caller adds the tensors, clip coefficient = min(1, max_norm / (sqrt(total) + 1e-6))); a3d_adamw_step is
 * torch's single-tensor AdamW update with the gradient read multiplied by grad_scale (the clip coefficient);
 * step counts from 1.  The hyper-parameters are doubles, as torch holds them: 1 - lr * weight_decay, 1 - beta1,
 * 1 - beta2 and the bias corrections are formed in double on the host and rounded to fp32 once ((float)(1 - 0.999)
 * is 0.001f; 1.f - 0.999f is 1.3e-5 away from it, which every element of exp_avg_sq would carry). */
size_t a3d_sum_squares_workspace_bytes(void);
int    a3d_sum_squares(const float* g_dev, int64_t n, double* out_host, void* workspace_dev, size_t workspace_bytes,
                       void* stream);
/* the same, added to *acc_dev (device double, zeroed by the caller) without a host synchronisation */
int    a3d_sum_squares_accumulate(const float* g_dev, int64_t n, double* acc_dev, void* workspace_dev,
                                  size_t workspace_bytes, void* stream);
int    a3d_adamw_step(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n,
                      int step, double lr, double beta1, double beta2, double eps, double weight_decay,
                      double grad_scale, void* stream);

/* The same two operations over ALL parameter tensors in one launch each (a training step updates 268 tensors).  The
 * caller uploads a table of a3d_mt_tensor entries, one per tensor in any fixed order: chunk0 = number of
 * A3D_MT_CHUNK-element chunks of the tensors before it, bias1 = 1 - beta1^step, bias2_sqrt = sqrt(1 - beta2^step) of
 * THAT tensor's step count (torch.optim.AdamW's per-parameter state['step']).  a3d_sum_squares_multi writes
 * sum over all tensors of sum g^2 to *out_dev (fp64, deterministic); a3d_adamw_step_multi = a3d_adamw_step on every
 * entry (bit-identical results when bias1 and bias2_sqrt are (float) of the doubles above: one device function does
 * the update for both). */
#define A3D_MT_CHUNK 4096
typedef struct a3d_mt_tensor {
  float* p; const float* g; float* m; float* v;
  int64_t n;
  int32_t chunk0;
  float bias1, bias2_sqrt;
  int32_t pad_;
} a3d_mt_tensor;
size_t a3d_mt_workspace_bytes(int64_t n_chunks);
int    a3d_sum_squares_multi(const a3d_mt_tensor* table_dev, int n_tensors, int64_t n_chunks, double* out_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);
int    a3d_adamw_step_multi(const a3d_mt_tensor* table_dev, int n_tensors, int64_t n_chunks, double lr, double beta1,
                            double beta2, double eps, double weight_decay, double grad_scale, void* stream);

/* Many conv weights packed by ONE launch (a training iteration repacks both orientations of every sparse-conv kernel
 * after the optimiser step: ~230 a3d_pack_conv_weight calls plus the transposes / flips / slices feeding them).  Job i
 * writes the packed [K][cin][cout] weight to dst, reading
 *   transposed = 0:  W[k][ci][co]      = src[k][ci][co]                         (src is [K][cin][cout])
 *   transposed = 1:  W[k][ci][co]      = src[flip ? K-1-k : k][c0 + co][ci]     (src is [K][src_cin][cin]: the weight of
 *                                        the input-gradient conv, output channels = the slice [c0, c0 + cout) of src's inputs)
 * chunk0 = number of A3D_MT_CHUNK-element chunks of the jobs before it (as a3d_mt_tensor); dst holds K * cin * cout floats
 * (the same layout as a3d_pack_conv_weight's). */
typedef struct a3d_pack_job {
  const float* src;
  float* dst;
  int32_t K, cin, cout;
  int32_t src_cin, src_cout;
  int32_t transposed, flip, c0;
  int32_t chunk0;
  int32_t pad_;
} a3d_pack_job;
int a3d_pack_conv_weights_multi(const a3d_pack_job* table_dev, int n_jobs, int64_t n_chunks, void* stream);

/* Dense row-major GEMM: out[n][cout] = act(((in (+ in_add))[n][cin] @ W) * scale + shift + res).
 * Replaces the nn.Linear / in_proj pieces of nn.MultiheadAttention that run over all N points
 * (models/modules/attention_block.py:91-94; `in_add` is the position encoding the reference adds to
 * its queries / keys before projecting them, attention_block.py:25-26,88-90).  96/128 -> 96/128
 * channels run on a dedicated HBM-bound kernel (k_dense); other shapes fall back to the sparse-conv
 * kernel with kernel volume 1 (no in_add there; the workspace arguments are not used: whole tiles are assigned
 * statically, pass NULL / 0). */
int a3d_linear(const float* in_dev, int ldi, const float* in_add_dev, int ldi_add,
               int64_t n, int cin, int cout,
               const float* w_packed_dev, const float* scale_dev, const float* shift_dev,
               const float* res_dev, int ldr, int relu, float* out_dev, int ldo,
               void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Position encoding.
 * Replaces: Agile3d.get_pos_encs (models/agile3d.py:141-161) ->
 * PositionEmbeddingCoordsSine.get_fourier_embeddings (models/position_embedding.py:123-152).
 * minmax_dev receives [min_x,min_y,min_z,max_x,max_y,max_z] of the sample.
 * ------------------------------------------------------------------------------------------ */
int a3d_posenc_fourier(const float* xyz_dev, int64_t n, const float* gauss_B_dev /*[3][64]*/,
                       float* minmax_dev /*[6]*/, float* out_dev /*[n][128]*/,
                       void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same for every sample of a batch in three launches: rows [starts_host[b], starts_host[b+1]) of xyz_dev / out_dev
 * belong to sample b (1..64 samples, each with its own min / max: agile3d.py:141-161 loops over the batch);
 * minmax_dev is [n_samples][6].  Bit-identical to a3d_posenc_fourier per sample. */
size_t a3d_posenc_batch_workspace_bytes(int n_samples);
int a3d_posenc_fourier_batch(const float* xyz_dev, const int64_t* starts_host, int n_samples,
                             const float* gauss_B_dev /*[3][64]*/, float* minmax_dev /*[n_samples][6]*/,
                             float* out_dev /*[N][128]*/, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Every position encoding of the reference (--positional_encoding_type, --normalize_pos_enc; selected in
 * models/agile3d.py:57-69) behind one pair of entry points shaped like the two above.  Channel layout of a row:
 *   A3D_POSENC_FOURIER  get_fourier_embeddings (position_embedding.py:123-152): p = (2 pi u) @ gauss_B,
 *                       [sin p (64), cos p (64)].  table_dev = gauss_B [3][64].
 *   A3D_POSENC_SINE     get_sine_embeddings (:75-121): 64 interleaved (sin, cos) pairs of one argument each, x owns
 *                       pairs 0..21 (44 channels), y 22..42, z 43..63 (42 each); argument of pair k of an axis with
 *                       cdim channels = 2 pi u / 10000^(2k / cdim).  No parameter: table_dev is ignored (NULL).
 *   A3D_POSENC_LEGACY   PositionalEncoding3D(128) (:179-208): per axis [sin(x f_j) (22), cos(x f_j) (22)], the three
 *                       axes side by side cut to 128 channels.  table_dev = the model's inv_freq buffer [22] (the
 *                       loaded one: a checkpoint's buffer is honoured).
 * u is the coordinate shifted and scaled to [0, 1] by the sample's own min / max when `normalize` != 0 (FOURIER, SINE),
 * the raw coordinate when it is 0; LEGACY always takes the raw coordinate and ignores `normalize`.  Where no min / max
 * is needed the reduction is skipped: minmax_dev and the workspace are not touched and may be NULL / 0.  out_dev must
 * be 16-byte aligned.  a3d_posenc_fourier[_batch] above are these two at (FOURIER, normalize = 1), without that alignment.
 * a3d_posenc_batch: bit-identical to a3d_posenc per sample; workspace of a3d_posenc_batch_workspace_bytes. */
#define A3D_POSENC_FOURIER 0
#define A3D_POSENC_SINE 1
#define A3D_POSENC_LEGACY 2
int a3d_posenc(int kind, int normalize, const float* xyz_dev, int64_t n, const float* table_dev,
               float* minmax_dev /*[6]*/, float* out_dev /*[n][128]*/, void* workspace_dev, size_t workspace_bytes,
               void* stream);
int a3d_posenc_batch(int kind, int normalize, const float* xyz_dev, const int64_t* starts_host, int n_samples,
                     const float* table_dev, float* minmax_dev /*[n_samples][6]*/, float* out_dev /*[N][128]*/,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Click-query decoder.
 * Replaces: Agile3d.forward_mask + mask_module (models/agile3d.py:183-384) and the post-norm
 * CrossAttentionLayer / SelfAttentionLayer / FFNLayer (models/modules/attention_block.py).
 * One call = one batch sample, all `n_layers` decoder iterations.
 * ------------------------------------------------------------------------------------------ */
#define A3D_MAX_QUERIES 256       /* clicks + learned background queries of one sample */
#define A3D_MAX_DEC_LAYERS 8

typedef struct {
  /* nn.MultiheadAttention / LayerNorm / Linear parameters in torch layout (row-major [out][in]):
   *   *_in_w = in_proj_weight [384][128] (rows 0..127 q, 128..255 k, 256..383 v),
   *   *_out_w = out_proj.weight [128][128], ffn_w1 = linear1.weight [dim_ff][128],
   *   ffn_w2 = linear2.weight [128][dim_ff]. */
  const float *c2s_in_w, *c2s_in_b, *c2s_out_w, *c2s_out_b, *c2s_norm_w, *c2s_norm_b;
  const float *c2c_in_w, *c2c_in_b, *c2c_out_w, *c2c_out_b, *c2c_norm_w, *c2c_norm_b;
  const float *ffn_w1, *ffn_b1, *ffn_w2, *ffn_b2, *ffn_norm_w, *ffn_norm_b;
  const float *s2c_in_w, *s2c_in_b, *s2c_out_w, *s2c_out_b, *s2c_norm_w, *s2c_norm_b;
  /* the [128][128] blocks that multiply all N points (c2s Wk, Wv; s2c Wq, Wo), as W^T packed by
   * a3d_pack_conv_weight(kernel_volume=1) */
  const float *c2s_wk_packed, *c2s_wv_packed, *s2c_wq_packed, *s2c_wo_packed;
  /* every matrix the QUERY side of the layer multiplies by (c2s out_proj, c2c in/out_proj, s2c k/v rows, c2s q rows,
   * FFN), in MFMA fragment order, made by a3d_decoder_pack_query_weights(w, layer, ...): a wave's weight load is 1 KB
   * contiguous instead of 64 B of each of 16 rows (35 -> 140 GB/s into one CU, tools/qload_ubench.hip).  REQUIRED since
   * round 4 (the kernel that read the torch-layout matrices is gone): with NULL here or in
   * a3d_decoder_weights::mask_pack the decoder entry points fail with A3D_ERR_INVALID. */
  const float* query_pack;
} a3d_decoder_layer;

typedef struct {
  int32_t n_layers;
  int32_t n_bg_queries;                 /* learned background queries (agile3d.py:47-48) */
  int32_t dim_ff;
  a3d_decoder_layer layers[A3D_MAX_DEC_LAYERS];
  const float *decoder_norm_w, *decoder_norm_b;
  const float *mask_w0, *mask_b0, *mask_w2, *mask_b2;     /* mask_embed_head.{0,2} */
  const float *bg_query_feat, *bg_query_pos;              /* [n_bg][128] */
  const float *gauss_B;                                   /* [3][64] */
  const float *time_table;                                /* [200][128] PositionalEncoding1D */
  const float *mask_pack;                                 /* mask_w0, mask_w2 in fragment order (layer = -1 below); required */
} a3d_decoder_weights;

/* Fragment-order copies of the query-side matrices of one decoder layer (layer >= 0: a3d_decoder_query_pack_floats(dim_ff)
 * floats) or of the mask head (layer = -1: a3d_decoder_mask_pack_floats()), read from the torch-layout pointers of `w`.
 * Re-run after the parameters change. */
size_t a3d_decoder_query_pack_floats(int32_t dim_ff);
size_t a3d_decoder_mask_pack_floats(void);
int a3d_decoder_pack_query_weights(const a3d_decoder_weights* w, int32_t layer, float* out_dev, void* stream);

size_t a3d_decoder_workspace_bytes(int64_t n, int n_queries);

/* One batch sample of forward_mask (agile3d.py:192: the reference loops `for b in range(batch_size)`).  Fields as in
 * a3d_decoder_forward; every sample brings its own workspace (a3d_decoder_workspace_bytes(n, n_clicks + n_bg)). */
typedef struct a3d_decoder_sample {
  const float* feats128_dev;            /* [n][128] rows of this sample */
  const float* posenc_dev;              /* [n][128] */
  int64_t n;
  const int32_t *click_row, *click_obj, *click_time;   /* HOST arrays, see below */
  int32_t n_clicks, n_objects;
  float* logits_dev;                    /* n_layers x [n][1 + n_objects] */
  void* workspace_dev;
  size_t workspace_bytes;
  /* Per-scene cache of the click-independent part of a pass (eval_multi_obj.py:112-160 runs ~100 passes per scene on
   * the same backbone output): the key / value projections of the FIRST layer's click-to-scene attention depend on
   * the scene only (agile3d.py:283-290 with src = pcd_features).  kv0_dev: [3][n][128] floats owned by the caller
   * (keys, values, and -- round 5 -- the first layer's scene-to-click QUERIES (feats + pos) Wq^T + bq, agile3d.py:305-312, which
   * depend on the scene only as well);
   * kv0_state 0 = not used, 1 = computed into kv0_dev by this call and used, 2 = valid from an earlier call with the same
   * features, position encodings and weights.  With the cache the first layer's attention reads K / V instead of
   * projecting them inside the fused kernel (39 instead of 75 us at 80 k points). */
  float* kv0_dev;
  int32_t kv0_state;
  int32_t kv0_blocks;                   /* [n][128] blocks kv0_dev holds: the library refuses a cache of fewer than 3 */
} a3d_decoder_sample;
/* All samples of a batch in one call: per decoder layer the three wide kernels are launched once for the whole batch
 * (samples with the same padded query count share the launches); results per sample equal a3d_decoder_forward's up to
 * the summation order of the click-to-scene partials. */
int    a3d_decoder_forward_batch(const a3d_decoder_weights* w, const a3d_decoder_sample* samples, int n_samples,
                                 void* stream);
/* click arrays are HOST arrays, object-major as the reference builds its queries
 * (agile3d.py:249-264): all clicks of object 1, ..., object K, then background clicks.
 * click_obj[i] in 0..K (0 = background), click_row = row of the sample, click_time < 200.
 * logits_dev: n_layers matrices [n][1+K]; the LAST is 'pred_masks', the others 'aux_outputs'. */
int    a3d_decoder_forward(const a3d_decoder_weights* w,
                           const float* feats128_dev, const float* xyz_dev,
                           const float* posenc_dev, const float* minmax_dev,
                           int64_t n,
                           const int32_t* click_row, const int32_t* click_obj,
                           const int32_t* click_time, int n_clicks, int n_objects,
                           float* logits_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The interactive loop around forward_mask.
 * Replaces: `p.argmax(-1)` + "update prediction with sparse gt" (eval_multi_obj.py:119-134),
 * mean_iou_scene (utils/seg.py:44-59), get_simulated_clicks + measure_error_size +
 * get_next_click_coo_torch (utils/seg.py:93-239) and loss_weights (utils/seg.py:62-70).
 * Labels and predictions are int32 object ids in 0..255 (0 = background).
 * ------------------------------------------------------------------------------------------ */
#define A3D_MAX_CLICKS 256

/* pred[i] = argmax_c logits[i][c] (first maximum), then pred[click_row[k]] = click_obj[k] in the
 * given order; click arrays are HOST arrays. */
int    a3d_argmax_labels(const float* logits_dev, int64_t n, int n_classes,
                         const int32_t* click_row, const int32_t* click_obj, int n_clicks,
                         int32_t* pred_dev, void* stream);

/* The same for every sample of a round in TWO launches (arg-max of all samples; their click lists): the loop over the samples
 * of eval_multi_obj.py:119-134 / engine.py:96-101 was two launches PER SAMPLE.  click_row / click_obj are HOST arrays;
 * workspace_dev (a3d_argmax_labels_batch_workspace_bytes, >= 16-byte aligned) takes the device copy of the click lists. */
typedef struct a3d_argmax_sample {
  const float*   logits_dev;   /* [n][n_classes] */
  int64_t        n;
  int32_t        n_classes;
  int32_t        n_clicks;     /* <= A3D_MAX_CLICKS */
  const int32_t* click_row;    /* host */
  const int32_t* click_obj;    /* host */
  int32_t*       pred_dev;     /* [n] */
} a3d_argmax_sample;
#define A3D_MAX_ROUND_SAMPLES 64
size_t a3d_argmax_labels_batch_workspace_bytes(int n_samples);
int    a3d_argmax_labels_batch(const a3d_argmax_sample* samples, int n_samples, void* workspace_dev, size_t workspace_bytes,
                               void* stream);

/* counts_dev: int64 [3][n_ids] + 1 trailing int64 (non-zero = an inverse_map entry was out of
 * range): [0][id] = |pred==id & label==id|, [1][id] = |pred==id|, [2][id] = |label==id| over the
 * n_full points i, with pred taken at inverse_map_dev[i] (NULL = identity).  IoU(id) =
 * [0]/([1]+[2]-[0]). */
int    a3d_iou_counts(const int32_t* pred_dev, int64_t n_pred, const int64_t* inverse_map_dev,
                      const int32_t* labels_dev, int64_t n_full, int n_ids,
                      int64_t* counts_dev, void* stream);
/* a3d_iou_counts of every sample of a round in one launch + one clear: counts_all_dev = [n_samples][3 n_ids + 1] int64,
 * sample i's block as a3d_iou_counts lays it out. */
typedef struct a3d_iou_sample {
  const int32_t* pred_dev;
  int64_t        n_pred;
  const int64_t* inverse_map_dev;   /* or NULL */
  const int32_t* labels_dev;
  int64_t        n_full;
} a3d_iou_sample;
int    a3d_iou_counts_batch(const a3d_iou_sample* samples, int n_samples, int n_ids, int64_t* counts_all_dev, void* stream);

/* One entry per error cluster (cluster id = 96*label + 11*pred over the wrongly labelled points,
 * utils/seg.py:186): `row` is the cluster point farthest from every point outside the cluster
 * (lowest row on ties), `error_size` that distance -- the next simulated click and the key the
 * reference sorts clusters by.  Entries come out in ascending cluster id (torch.unique order). */
typedef struct {
  int32_t cluster_id, row, label, pred;
  float   error_size;
} a3d_click_cluster;
size_t a3d_click_workspace_bytes(int64_t n);
/* *n_out_dev = number of clusters (may exceed max_out: only max_out are written), -1 if a label or
 * prediction was outside 0..255.  The search is exact: only a cluster's largest distance and its first
 * arg-max are ever used, so wrong points are first bounded from above against every 16th point, each
 * cluster's best candidate is measured exactly (a lower bound of the cluster's maximum), and only the
 * points whose upper bound reaches it go through the pass over all points (clicks.hip). */
int    a3d_click_clusters(const float* xyz_dev, const int32_t* pred_dev, const int32_t* labels_dev,
                          int64_t n, a3d_click_cluster* out_dev, int max_out, int32_t* n_out_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same for up to 64 samples in ONE set of launches (the samples of a training click round, engine.py:103-116, or of a
 * lock-step evaluation round, eval_multi_obj.py:162-166): every kernel takes the samples from a device table, so a round
 * issues ~15 launches whatever the batch size instead of ~12 per sample.  Results per sample are those of
 * a3d_click_clusters; every sample brings its own workspace (a3d_click_workspace_bytes(n)). */
typedef struct a3d_click_sample {
  const float*   xyz_dev;          /* [n][3] */
  const int32_t *pred_dev, *labels_dev;   /* [n] object ids 0..255 */
  int64_t        n;
  a3d_click_cluster* out_dev;      /* max_out records */
  int32_t*       n_out_dev;
  int32_t        max_out;
  void*          workspace_dev;
  size_t         workspace_bytes;
  /* optional: a spatial order of the sample's points and its inverse (a3d_click_spatial_order; the coordinates of a scene do
   * not change over its rounds).  With it the first bounding stage looks at a row's neighbours in that order instead of a
   * sparse sample of all points: far tighter upper bounds where predictions are wrong nearly everywhere.  Any permutation of
   * 0..n-1 is VALID (the bounds stay bounds, the search stays exact); both NULL = the sampled stage. */
  const int32_t *order_dev, *inv_dev;
} a3d_click_sample;
int    a3d_click_clusters_batch(const a3d_click_sample* samples, int n_samples, void* stream);
/* order_dev[s] = row of the s-th point in Morton order of the coordinates (2^16 cells per axis over the bounding box),
 * inv_dev[row] = s.  No reference counterpart: an index the search above may use (utils/seg.py:157-171 has none). */
size_t a3d_click_spatial_order_workspace_bytes(int64_t n);
int    a3d_click_spatial_order(const float* xyz_dev, int64_t n, int32_t* order_dev, int32_t* inv_dev, void* workspace_dev,
                               size_t workspace_bytes, void* stream);

/* weights[i] = alpha + (beta-alpha) * (1 - min(d_i, tita)/tita), d_i = distance of point i to the
 * nearest clicked point; click_row is a HOST array. */
int    a3d_click_loss_weights(const float* xyz_dev, int64_t n, const int32_t* click_row, int n_clicks,
                              float tita, float alpha, float beta, float* weights_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * The headless interactive session (csrc/session.hip; agile3d_amd/session.py).
 * Replaces what surrounds the two model calls of interactive_tool/: find_nearest (utils.py:27-29: one
 * torch.cdist over all voxel rows and one over all vertices per click), the depth-image pick of gui.py:247-271,
 * and pred[inverse_map] + get_colors + the click cubes (interactive_segmentation_user.py:83-84,125-140,
 * gui.py:276-298,327).  a3d_nearest_rows, a3d_pick_ray and a3d_pick_mesh take one scratch buffer of a fixed size (256-byte aligned).
 * All write their first-stage results into it: two calls that share a workspace must be ordered (the same stream, or
 * an event between them); calls on different streams that may overlap each bring their own workspace.
 * ------------------------------------------------------------------------------------------ */
#define A3D_NEAREST_MAX_QUERIES 64
#define A3D_NEAREST_MAX_SOURCES 4
size_t a3d_session_workspace_bytes(void);

/* For each of the m query points (HOST array [m][3]) and each source: rows_out_dev[q] = the FIRST arg-min over the
 * source's rows of (x-qx)^2 + (y-qy)^2 + (z-qz)^2, evaluated in fp32 from the differences, squares added in x, y, z
 * order, every operation rounded on its own (no fma contraction) -- exact, unlike the |a|^2+|b|^2-2ab form torch.cdist
 * takes for one query row, which loses the nearest row on scenes far from the origin.  Ties -> the
 * lowest row; -1 for an empty source.  Deterministic: a minimum over packed (distance bits, row) keys.  One launch pair
 * serves all sources (a click searches the voxel rows and the full-resolution vertices).  n < 2^31 rows per source.
 * Coordinates and queries are expected to be finite; the call does not check them.  A row whose distance is NaN orders
 * behind every finite distance (its key holds the NaN's bits) and is returned only if the source has no other row. */
typedef struct a3d_nearest_source {
  const float* xyz_dev;        /* [n][3] */
  int64_t      n;
  int32_t*     rows_out_dev;   /* [m] */
} a3d_nearest_source;
int    a3d_nearest_rows(const a3d_nearest_source* sources, int n_sources, const float* queries, int m,
                        void* workspace_dev, size_t workspace_bytes, void* stream);

/* The headless stand-in for "render a depth image and unproject".  The rule is this library's (the reference leaves
 * picking to Open3D's renderer): origin o, UNIT direction d (HOST arrays of 3), radius r; among the points p with
 * t = (p-o).d > 0 and perpendicular distance |(p-o) - t d| <= r the one with the smallest t, ties -> the smaller
 * perpendicular distance, then the lower index.  result_dev: its index and coordinates; index -1 = the ray meets no
 * point ("clicked on nothing", gui.py:265). */
typedef struct a3d_pick_result {
  int32_t index;
  float   x, y, z;
} a3d_pick_result;
int    a3d_pick_ray(const float* xyz_dev, int64_t n, const float* origin, const float* direction, float radius,
                    a3d_pick_result* result_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same stand-in for a TRIANGLE MESH: the first surface the ray meets.  faces_dev: int32 [m][3] indices into the same
 * xyz_dev rows [n][3] (no second copy of the vertices); origin o, UNIT direction d (HOST arrays of 3).  The rule is this
 * library's: among the faces the ray crosses at a finite t > 0 the one with the smallest t, ties -> the lower face index.
 * Faces are double-sided and their edges inclusive; the crossing test is the watertight one of Woop, Benthin and Wald
 * (JCGT 2013) evaluated in fp32 without fma contraction, an edge function that is exactly 0 recomputed in double: two
 * faces that share an edge classify every ray consistently, so no ray passes between them.  Skipped, never an error:
 * faces with det == 0, a repeated index, a NaN coordinate, or an index outside 0..n-1 -- the last also sets bit 0 of
 * flags.  m == 0 is valid.  result_dev: face -1 = the ray meets no surface; else t, the barycentric weights u (of the
 * face's second vertex) and v (of its third; the first has 1 - u - v) and the hit point x, y, z = that combination of the
 * face's three vertices in fp32 -- a point of the triangle, not o + t d.  Takes the session workspace like a3d_pick_ray. */
typedef struct a3d_pick_mesh_result {
  int32_t face;
  int32_t flags;
  float   t;
  float   x, y, z;
  float   u, v;
} a3d_pick_mesh_result;
int    a3d_pick_mesh(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m, const float* origin,
                     const float* direction, a3d_pick_mesh_result* result_dev, void* workspace_dev,
                     size_t workspace_bytes, void* stream);

/* One pass over the n_full full-resolution vertices: label_full[i] = labels_qv[inverse_map[i]] (labels_qv = what
 * a3d_argmax_labels wrote, clicked rows already overwritten; inverse_map NULL = identity), colour = the palette entry of
 * a label > 0 (labels >= n_palette wrap over entries 1..n_palette-1; entry 0 is unused) or the vertex's own colour for
 * label 0, then the click cubes: a vertex whose three fp32 |coordinate differences| to cube c's centre are all < cube_size
 * takes that cube's colour, the LAST such cube winning.  *err_dev (int32, cleared by the call): bit 0 = an inverse_map
 * entry outside 0..n_qv-1 (that vertex is left unwritten), bit 1 = a negative label. */
typedef struct a3d_session_paint_args {
  const int32_t* labels_qv_dev;     /* [n_qv] */
  int64_t        n_qv;
  const int64_t* inverse_map_dev;   /* [n_full] or NULL */
  int64_t        n_full;
  const float*   xyz_full_dev;      /* [n_full][3]; read only when n_cubes > 0 */
  const float*   colors_full_dev;   /* [n_full][3] */
  const float*   palette_dev;       /* [n_palette][3], 2 <= n_palette <= 256 */
  const float*   cubes_dev;         /* [n_cubes][6]: centre x, y, z, colour r, g, b; n_cubes <= A3D_MAX_CLICKS */
  int32_t        n_palette;
  int32_t        n_cubes;
  float          cube_size;
  int32_t        reserved_;
  int32_t*       label_full_dev;    /* out [n_full] int32 */
  float*         colors_out_dev;    /* out [n_full][3] */
  int32_t*       err_dev;
} a3d_session_paint_args;
int    a3d_session_paint(const a3d_session_paint_args* args, void* stream);

/* What an EDIT of the session's click list (undo, redo, remove, restore from a file) rebuilds on the device
 * (csrc/session_edit.hip).  The rule is this library's: the reference cannot take a click back (gui.py:283-287 is a TODO).
 * Two independent halves in one launch; a half whose count is 0 is absent and its pointers are not looked at.
 *   RELABEL (n_full > 0): the relabelled ground truth of a click list.  instances_dev[k - 1] is the instance id object k
 *     stands for (the session: the original label of the voxel under the EARLIEST click of k); 0 <= n_objects <= 255.
 *         new_labels[i] = the largest k in 1..n_objects with instances[k - 1] == labels_ori[i], else 0
 *     Ids compare as plain int32: 0, negative and large ids are values like any other.  Where two objects stand for the
 *     same instance the HIGHER id wins -- in a list grown by clicks alone objects are created in id order, so this is the
 *     reference's "the object created last wins" (gui.py:318-319).  new_labels_dev == labels_ori_dev is allowed.
 *   REMAP (n_labels > 0): labels[i] = lut[labels[i]], in place, lut the old -> new object ids after a removal (identity, or
 *     removed id -> 0 and every id above it one down) or their inverse.  A value outside 0..255 becomes 0 and sets bit 0 of
 *     *err_dev (int32, cleared by the call whenever it is given).  labels_dev must not overlap the relabel's arrays.
 * Streaming passes over 4-byte rows, no workspace, no atomic but the flag's: the result depends on the arguments alone.
 * A count < 0, n_objects outside 0..255, or a count > 0 with one of its pointers NULL: A3D_ERR_INVALID, nothing launched. */
typedef struct a3d_session_edit_args {
  const int32_t* labels_ori_dev;    /* [n_full] the scene's instance ids */
  const int32_t* instances_dev;     /* [n_objects] on the DEVICE (gathered there, no host round trip); NULL if n_objects == 0 */
  int32_t*       new_labels_dev;    /* out [n_full] */
  int64_t        n_full;
  int32_t*       labels_dev;        /* in/out [n_labels] */
  int64_t        n_labels;
  int32_t*       err_dev;           /* needed when n_labels > 0 */
  int32_t        n_objects;
  int32_t        reserved_;
  uint8_t        lut[256];
} a3d_session_edit_args;
int    a3d_session_edit(const a3d_session_edit_args* args, void* stream);

/* How SURE the last inference is, and where a next click should look (csrc/session_guide.hip).  The rule is this library's:
 * the reference keeps the arg-max of forward_mask's logits and drops the logits (interactive_segmentation_user.py:78-81).
 * Two independent halves, one launch each; a half whose count is 0 is absent.
 *   VOXELS (n_qv > 0), over logits [n_qv][n_classes] fp32 row-major, 2 <= n_classes <= 256, n_qv < 2^31; every row is written:
 *     label  = the FIRST maximum of the row: scan from column 0, replace on `>` (what a3d_argmax_labels writes)
 *     runner = the first maximum among the OTHER columns, by the same scan
 *     margin = logits[label] - logits[runner], one fp32 subtraction; >= 0 unless it is NaN
 *     then the clicks click_row[k] / click_obj[k], k = 0..n_clicks-1 in order (the last entry of a row wins; a row outside
 *     0..n_qv-1 is ignored, as a3d_argmax_labels ignores it): label = runner = click_obj[k], margin = +inf
 *     want   = runner where margin < threshold (strictly: the row is CONTESTED), else label
 *     A row whose margin is NaN (a NaN logit, or two infinities of one sign) sets bit 0 of the summary's err; its label and
 *     runner are what the two scans leave (columns in 0..n_classes-1) and it is not contested.
 *     Fed to a3d_click_clusters as pred = label, labels = want, the contested rows become its "error" clusters: one per
 *     (runner, label) pair, each with the row farthest from everything outside it -- the deepest point of the region.
 *   SUMMARY (always written; cleared by the call): voxels[l] = rows whose label is l, contested[l] = contested rows among
 *     them; least_key = the COMPLEMENT of the minimum over the rows with a FINITE margin of (margin bits << 32 | row) --
 *     the smallest margin, ties to the lowest row -- and 0, the cleared record, when no row has one (~0 holds row -1);
 *     err as above.  Integer sums and a maximum: identical from run to run.
 *   VERTICES (n_full > 0): src = inverse_map[i] (NULL = identity).  src outside 0..n_qv-1 sets bit 1 of err and leaves
 *     vertex i unwritten.  Else margin_full[i] = margin[src] and, per channel,
 *         colour = base * s + doubt * (1 - s),   s = (x < 1 ? x : 1),   x = margin[src] * (1 / full_margin)
 *     in fp32, every operation (the reciprocal, x, both products, the difference, the sum) rounded on its own, no fma
 *     contraction.  base = the palette entry of label[src] > 0 with a3d_session_paint's wrap, the vertex's own colour
 *     otherwise.  A margin >= full_margin gives exactly base, a margin of 0 exactly doubt; a NaN margin counts as sure.
 *     No click cubes: a3d_render_annotate draws the clicks.
 * A3D_ERR_INVALID with nothing launched: n_classes outside 2..256, a negative count, n_qv >= 2^31, n_clicks >
 * A3D_MAX_CLICKS, threshold or full_margin not finite or <= 0, no summary_dev, a half with a count > 0 and one of its
 * pointers NULL (the vertices need labels_qv_dev and margin_qv_dev too, and 2 <= n_palette <= 256).  click_obj is not
 * checked against n_classes: the session's clicks are its objects. */
typedef struct a3d_session_guide_summary {
  int32_t  voxels[256];
  int32_t  contested[256];
  uint64_t least_key;               /* ~((margin bits << 32) | row); 0 = no row with a finite margin */
  int32_t  err;                     /* bit 0 = a NaN margin, bit 1 = an inverse_map entry out of range */
  int32_t  reserved_;
} a3d_session_guide_summary;
typedef struct a3d_session_guide_args {
  const float*   logits_dev;        /* [n_qv][n_classes] */
  int64_t        n_qv;
  const int64_t* inverse_map_dev;   /* [n_full] or NULL */
  int64_t        n_full;
  const float*   colors_full_dev;   /* [n_full][3] */
  const float*   palette_dev;       /* [n_palette][3] */
  int32_t*       labels_qv_dev;     /* out [n_qv] */
  int32_t*       runner_qv_dev;     /* out [n_qv] */
  float*         margin_qv_dev;     /* out [n_qv] */
  int32_t*       want_qv_dev;       /* out [n_qv] */
  float*         margin_full_dev;   /* out [n_full] */
  float*         colors_out_dev;    /* out [n_full][3] */
  a3d_session_guide_summary* summary_dev;
  int32_t        n_classes;
  int32_t        n_palette;
  int32_t        n_clicks;
  float          threshold;
  float          full_margin;
  float          doubt[3];
  int32_t        click_row[A3D_MAX_CLICKS];
  uint8_t        click_obj[A3D_MAX_CLICKS];
} a3d_session_guide_args;
int    a3d_session_guide(const a3d_session_guide_args* args, void* stream);

/* WHERE IN SPACE a label lies: the connected pieces of a keyed voxel set, and the despeckle step (csrc/session_pieces.hip).
 * The rules are this library's: the reference keeps an arg-max per voxel and has no notion of a piece.  The adjacency is the
 * scene's own level-0 table A3D_TAB_NBR27, both ends translated through A3D_TAB_ORIGROW: nothing is hashed or built again.
 *
 * a3d_label_pieces.  scene: level 0 = the voxels, n = its size (a3d_scene_level_size(scene, 0)); keys_dev int32 [n] in the
 * CALLER's row order; connectivity 6, 18 or 26; up to A3D_MAX_CLICKS clicked rows by value (a row outside 0..n-1 is
 * ignored); optionally inverse_map_dev int64 [n_full] (NULL = identity) with n_full > 0.
 *   A row with key < 0 belongs to no piece.
 *   Two rows are JOINED when both hold:
 *     - they are neighbours under the connectivity, where 6 means |d|1 = 1, 18 means |d|1 <= 2, and 26 means all of the 3^3
 *       table (d = the difference of their voxel coordinates; the scene's table already keeps batch samples apart);
 *     - they have the same key.
 *   A PIECE is a class of the transitive closure.
 *   piece_qv[i] is the SMALLEST CALLER ROW of i's piece, or -1 for a row that belongs to none.
 *   piece_full[v] = piece_qv[inverse_map[v]].  An index outside 0..n-1 sets bit 0 of the error word n_out_dev[1] and leaves
 *   the vertex unwritten, as a3d_session_guide does.
 *   RECORDS: one a3d_piece per piece, in ASCENDING root row: the root row, the key, the number of voxels, clicked = 1 when
 *   the piece holds a clicked row (else 0), and the inclusive bounding box lo[3], hi[3] in voxel coordinates (A3D_TAB_XYZB).
 *   n_out_dev is int32 [2], cleared by the call: n_out_dev[0] = the TRUE number of pieces (it may exceed max_out: only the
 *   first max_out records, in root order, are written -- as a3d_click_clusters reports), n_out_dev[1] = the error word.
 *   Everything is integer; the result does not depend on the order in which workgroups run: two calls give the same bytes.
 *   How: union-find over parent[] indexed by caller row -- init, hook (one thread per voxel, the 13 offsets of one
 *   half-space, the larger root linked under the smaller with atomicCAS), flatten.  Parents only decrease and no thread waits
 *   for another: every loop ends on its own (no spin-wait, no grid barrier), at any graph diameter.
 *   The workspace (a3d_pieces_workspace_bytes(n), 256-byte aligned) holds, behind the call, the sizes of the pieces at their
 *   roots' slots: a3d_absorb_pieces reads them there.  The library allocates nothing and does not synchronise.
 *   A3D_ERR_INVALID with nothing launched: no scene, n != the scene's level-0 size, a connectivity other than 6 / 18 / 26,
 *   n_clicks outside 0..A3D_MAX_CLICKS, max_out < 0, n_full < 0, no n_out_dev, a needed pointer NULL (out_dev when max_out >
 *   0, piece_full_dev when n_full > 0), a workspace that is too small or misaligned.
 *
 * a3d_absorb_pieces -- despeckle.  labels_dev int32 [n] in 0..n_classes-1 (n_classes <= 256); piece_qv_dev = what
 * a3d_label_pieces wrote for keys = these labels under the SAME connectivity, and workspace_dev = the workspace of that call
 * (it holds the sizes), now of at least a3d_absorb_workspace_bytes(n, capacity, n_classes) bytes; min_voxels; the clicked
 * rows; capacity = the number of small pieces the call has room for (the caller's choice).
 * The rule is ONE simultaneous step on the INPUT labels:
 *   A piece is SMALL when it has fewer than min_voxels voxels and holds no clicked row.
 *   Consider every voxel i of a small piece and every present neighbour j under the connectivity with label[j] != label[i].
 *   Each such pair gives one vote to label[j].
 *   The piece takes the label with the most votes.  Ties go to the lowest label.
 *   A piece with no vote keeps its label.  Such a piece is isolated in space.
 *   Nothing else changes.
 * labels_out_dev int32 [n] may not alias labels_dev.  The summary (cleared by the call): small pieces, relabelled pieces,
 * relabelled voxels, kept-isolated pieces, and the error word: A3D_ABSORB_OVERFLOW = there are more small pieces than
 * `capacity`: NOTHING is written to labels_out and small_pieces is the capacity needed (call again with that much, as with
 * a3d_render_header::pairs_needed); A3D_ABSORB_BAD_LABEL = a neighbour's label outside 0..n_classes-1 (its vote is dropped).
 * Votes are integer atomics: the result is order-free.  A3D_ERR_INVALID as above, and for n_classes outside 1..256,
 * capacity < 0, min_voxels < 0, no summary_dev, labels_out_dev == labels_dev. */
typedef struct a3d_piece {
  int32_t root, key, voxels, clicked;
  int32_t lo[3], hi[3];
} a3d_piece;                       /* 40 bytes */
typedef struct a3d_label_pieces_args {
  const a3d_scene* scene;
  int64_t        n;
  const int32_t* keys_dev;          /* [n] caller's row order */
  const int64_t* inverse_map_dev;   /* [n_full] or NULL */
  int64_t        n_full;
  int32_t*       piece_qv_dev;      /* out [n] */
  int32_t*       piece_full_dev;    /* out [n_full] */
  a3d_piece*     out_dev;           /* out: max_out records */
  int32_t*       n_out_dev;         /* out int32 [2]: the true count, the error word */
  void*          workspace_dev;
  size_t         workspace_bytes;
  int32_t        connectivity;
  int32_t        max_out;
  int32_t        n_clicks;
  int32_t        reserved_;
  int32_t        click_row[A3D_MAX_CLICKS];
} a3d_label_pieces_args;
size_t a3d_pieces_workspace_bytes(int64_t n);
int    a3d_label_pieces(const a3d_label_pieces_args* args, void* stream);

#define A3D_ABSORB_OVERFLOW  1
#define A3D_ABSORB_BAD_LABEL 2
typedef struct a3d_absorb_summary {
  int32_t small_pieces;             /* also the capacity needed when A3D_ABSORB_OVERFLOW is set */
  int32_t relabelled_pieces;
  int32_t relabelled_voxels;
  int32_t kept_isolated;
  int32_t err;
  int32_t reserved_[3];
} a3d_absorb_summary;              /* 32 bytes */
typedef struct a3d_absorb_pieces_args {
  const a3d_scene* scene;
  int64_t        n;
  const int32_t* labels_dev;        /* [n] */
  const int32_t* piece_qv_dev;      /* [n] a3d_label_pieces' of these labels */
  int32_t*       labels_out_dev;    /* out [n] */
  a3d_absorb_summary* summary_dev;
  void*          workspace_dev;     /* the workspace a3d_label_pieces used */
  size_t         workspace_bytes;
  int32_t        min_voxels;
  int32_t        connectivity;
  int32_t        n_classes;
  int32_t        capacity;
  int32_t        n_clicks;
  int32_t        reserved_;
  int32_t        click_row[A3D_MAX_CLICKS];
} a3d_absorb_pieces_args;
size_t a3d_absorb_workspace_bytes(int64_t n, int capacity, int n_classes);
int    a3d_absorb_pieces(const a3d_absorb_pieces_args* args, void* stream);

/* WHICH VOXELS BELONG TO ONE SURFACE: connected components under a pairwise SIMILARITY of normals and colours, and the vote
 * that snaps a labelling to such a partition (csrc/session_pieces.hip).  The rules are this library's: the reference's tool
 * has neither a magic wand nor a snap.  Adjacency, record list, capacity protocol and workspace are a3d_label_pieces' and
 * a3d_absorb_pieces'.
 *
 * a3d_similar_pieces.  Everything a3d_label_pieces takes -- keys_dev may be NULL here: every key is 0 -- and
 * normal_qv_dev fp32 [n][3] or NULL, feat_qv_dev fp32 [n][3] or NULL (the colours the backbone was fed), both in the CALLER's
 * row order; by value cos_min, tol2, oriented, ref_flags, ref_normal[3], ref_cos_min, ref_feat[3], ref_tol2.
 *   THE PREDICATES are fp32, every operation rounded on its own (fp contract off), in the order written:
 *     NSIM(a, b, c):  dot = (a0*b0 + a1*b1) + a2*b2;  passes iff (oriented ? dot : fabsf(dot)) >= c.
 *     FSIM(a, b, t):  d_k = a_k - b_k;  q = (d0*d0 + d1*d1) + d2*d2;  passes iff q <= t.
 *   A comparison with a NaN fails.  There is NO special case for a zero normal: its dot is 0, so with cos_min > 0 such a
 *   voxel joins nobody.
 *   A row is ADMISSIBLE iff its key is >= 0, and with A3D_SIMILAR_REF_NORMAL set NSIM(normal[i], ref_normal, ref_cos_min),
 *   and with A3D_SIMILAR_REF_FEAT set FSIM(feat[i], ref_feat, ref_tol2).  A row that is not admissible belongs to no piece
 *   (piece_qv = -1).
 *   Two admissible rows are JOINED iff they are neighbours under the connectivity (a3d_label_pieces' offsets, never across
 *   batch samples), hold the same key, NSIM(normal[i], normal[j], cos_min) when normal_qv_dev is given, and
 *   FSIM(feat[i], feat[j], tol2) when feat_qv_dev is given.
 *   Both predicates are SYMMETRIC BIT FOR BIT: products commute, and a - b and b - a have equal squares.  It therefore does
 *   not matter which end of an edge evaluates them: the components are a function of the arguments, and by a3d_label_pieces'
 *   argument (the root of a class is its smallest row) so is every output.  Two calls give the same bytes.
 *   A PIECE is a class of the transitive closure of "joined" -- a CHAIN: along a smoothly turning surface the two ends of a
 *   piece may differ by far more than the threshold; the reference test bounds every member against one value instead.
 *   piece_qv, piece_full, the records in ascending root order, n_out_dev and the workspace contents (of
 *   a3d_pieces_workspace_bytes(n) bytes; a3d_vote_pieces and a3d_absorb_pieces read the sizes there) are exactly as
 *   a3d_label_pieces defines them.  With neither array and ref_flags == 0 the call writes the bytes a3d_label_pieces writes.
 *   A3D_ERR_INVALID with nothing launched: everything a3d_label_pieces refuses (but keys_dev may be NULL); cos_min or
 *   ref_cos_min not finite or outside [-1, 1]; tol2 or ref_tol2 not finite or < 0; a ref_flags bit without its array; bits
 *   other than 0 and 1; a reference value that is not finite; oriented other than 0 or 1.
 *
 * a3d_similar_pair -- the pair predicate on the host, by the function the kernel calls (no GPU): 1 when
 * (normal_a == NULL || NSIM(normal_a, normal_b, cos_min)) && (feat_a == NULL || FSIM(feat_a, feat_b, tol2)), else 0.  A pair
 * of pointers is given or left out together.  The admissibility test is the same function with the reference as `b`.
 * -1 for a pointer without its partner or oriented other than 0 or 1.  The thresholds are NOT range-checked here.
 *
 * a3d_vote_pieces -- snap a labelling to a partition.  labels_dev int32 [n] in 0..n_classes-1 (n_classes <= 256);
 * piece_qv_dev = ANY partition a3d_label_pieces or a3d_similar_pieces wrote for this scene, and workspace_dev = the workspace
 * of that call (it holds the sizes at the roots), now of at least a3d_vote_workspace_bytes(n, capacity, n_classes) bytes -- or
 * a buffer of that size whose first a3d_pieces_workspace_bytes(n) bytes are a copy of that workspace, taken after the call;
 * min_voxels >= 1; share_num, share_den with 1 <= num <= den <= 65536; the clicked rows; capacity = the number of eligible
 * pieces the call has room for.
 * The rule is ONE simultaneous step on the INPUT labels, all integers:
 *   A piece is ELIGIBLE when it has >= min_voxels voxels.
 *   votes[l] = the number of its voxels with label l.  A label outside 0..n_classes-1 sets A3D_VOTE_BAD_LABEL; such a voxel
 *   casts no vote and keeps its label.
 *   The WINNER is the label with the most votes.  Ties go to the lowest label.
 *   The piece PASSES iff votes[winner] * share_den >= voxels * share_num (int64).
 *   It is BLOCKED when it holds a clicked row whose label differs from the winner: the snap never contradicts a click.  A
 *   clicked row outside 0..n-1 is ignored.
 *   A piece that is eligible, passes and is not blocked gives every one of its voxels (with a label in range) the winner.
 *   Everything else is copied unchanged, rows with no piece included.
 * labels_out_dev int32 [n] may not alias labels_dev.  The summary (cleared by the call) sorts every eligible piece into at
 * most one class, tested in this order: UNIFORM (every voxel already holds the winner), BELOW SHARE (does not pass), BLOCKED,
 * RELABELLED (at least one voxel changed); relabelled_voxels counts the voxels that changed.  (An eligible piece whose only
 * other voxels hold labels out of range falls in none of the four.)  A3D_VOTE_OVERFLOW = there are more eligible pieces than
 * `capacity`: NOTHING is written to labels_out and eligible_pieces is the capacity needed.  The eligible pieces are numbered
 * by a3d_absorb_pieces' one-block scan, votes are integer atomics: two calls give the same bytes.
 * A3D_ERR_INVALID with nothing launched: no scene, n != the scene's level-0 size, n_clicks outside 0..A3D_MAX_CLICKS,
 * n_classes outside 1..256, capacity < 0, min_voxels < 1, share_num / share_den outside 1 <= num <= den <= 65536, no
 * summary_dev, a needed pointer NULL, labels_out_dev == labels_dev, a workspace that is too small or misaligned. */
#define A3D_SIMILAR_REF_NORMAL 1
#define A3D_SIMILAR_REF_FEAT   2
typedef struct a3d_similar_pieces_args {
  const a3d_scene* scene;
  int64_t        n;
  const int32_t* keys_dev;          /* [n] caller's row order, or NULL: all 0 */
  const int64_t* inverse_map_dev;   /* [n_full] or NULL */
  int64_t        n_full;
  int32_t*       piece_qv_dev;      /* out [n] */
  int32_t*       piece_full_dev;    /* out [n_full] */
  a3d_piece*     out_dev;           /* out: max_out records */
  int32_t*       n_out_dev;         /* out int32 [2]: the true count, the error word */
  void*          workspace_dev;
  size_t         workspace_bytes;
  const float*   normal_qv_dev;     /* [n][3] or NULL */
  const float*   feat_qv_dev;       /* [n][3] or NULL */
  float          cos_min;
  float          tol2;
  int32_t        oriented;
  int32_t        ref_flags;
  float          ref_normal[3];
  float          ref_cos_min;
  float          ref_feat[3];
  float          ref_tol2;
  int32_t        connectivity;
  int32_t        max_out;
  int32_t        n_clicks;
  int32_t        reserved_;
  int32_t        click_row[A3D_MAX_CLICKS];
} a3d_similar_pieces_args;
int    a3d_similar_pieces(const a3d_similar_pieces_args* args, void* stream);
int    a3d_similar_pair(const float* normal_a, const float* normal_b, const float* feat_a, const float* feat_b, float cos_min,
                        float tol2, int oriented);

#define A3D_VOTE_OVERFLOW  1
#define A3D_VOTE_BAD_LABEL 2
typedef struct a3d_vote_summary {
  int32_t eligible_pieces;          /* also the capacity needed when A3D_VOTE_OVERFLOW is set */
  int32_t uniform_pieces;
  int32_t relabelled_pieces;
  int32_t relabelled_voxels;
  int32_t blocked_pieces;
  int32_t below_share_pieces;
  int32_t err;
  int32_t reserved_;
} a3d_vote_summary;                /* 32 bytes */
typedef struct a3d_vote_pieces_args {
  const a3d_scene* scene;
  int64_t        n;
  const int32_t* labels_dev;        /* [n] */
  const int32_t* piece_qv_dev;      /* [n] a partition a3d_label_pieces / a3d_similar_pieces wrote */
  int32_t*       labels_out_dev;    /* out [n] */
  a3d_vote_summary* summary_dev;
  void*          workspace_dev;     /* the workspace of the call that wrote piece_qv */
  size_t         workspace_bytes;
  int32_t        min_voxels;
  int32_t        n_classes;
  int32_t        capacity;
  int32_t        share_num;
  int32_t        share_den;
  int32_t        n_clicks;
  int32_t        click_row[A3D_MAX_CLICKS];
} a3d_vote_pieces_args;
size_t a3d_vote_workspace_bytes(int64_t n, int capacity, int n_classes);
int    a3d_vote_pieces(const a3d_vote_pieces_args* args, void* stream);

/* HOW FAR ALONG THE SURFACE: a bounded shortest-path distance from a set of seed voxels over the same adjacency, and which
 * seed is nearest (csrc/session_grow.hip).  The rule is this library's: the reference's tool selects nothing by distance.
 * a3d_label_pieces answers "what is connected at all"; this answers "what is connected within a distance, and how far".
 *
 * a3d_grow_voxels.  The graph's NODES are the level-0 voxels of `scene`, n = its size, in the CALLER's row order.
 *   CONNECTIVITY 6, 18 or 26 with exactly the offsets a3d_label_pieces admits; the neighbours are the scene's (A3D_TAB_NBR27,
 *   both ends through A3D_TAB_ORIGROW), so never across batch samples.
 *   KEYS: keys_dev int32 [n], or NULL = every voxel has key 0.  A voxel with key < 0 cannot be walked on.  An edge is
 *   WALKABLE only when both ends hold the SAME key (a3d_label_pieces' convention: all zeros = walk anywhere, a 0 / -1 mask =
 *   walk inside a region, the labels = stay inside one object).
 *   STEP COST: cost[0], cost[1], cost[2] for the face, edge and corner offsets (|d|1 = 1, 2, 3), each in 1 .. 65536.
 *   LIMIT: 0 .. 2^30, with limit / min(cost) <= A3D_GROW_MAX_STEPS: a path within the limit has at most that many edges.
 *   A larger limit is refused: "everything connected" is what a3d_label_pieces is for.
 *   SEEDS: a voxel is a seed when its key is >= 0 and either seed_qv_dev[row] != 0 (uint8 [n], optional), or some vertex i
 *   has seed_full_dev[i] != 0 and inverse_map_dev[i] == row (uint8 [n_full] and int64 [n_full], optional; a NULL map is the
 *   identity).  At least one of the two seed arrays must be given.
 *   THE VALUE of a voxel v is the LEXICOGRAPHIC MINIMUM, over the seeds s with a walkable path to v of total cost
 *   d <= limit, of the pair (d, s), s being the seed's caller row: dist[v] = d, owner[v] = s; both are -1 when there is no
 *   such seed.  A seed has dist 0 and owns itself.  Everything is an integer: there is no tolerance anywhere.
 *   LIFTING (n_full > 0): for vertex i, row = inverse_map[i]; selected_full[i] = dist[row] >= 0 (uint8 0 / 1) and
 *   dist_full[i] = dist[row].  For an index outside 0..n-1: 0 / -1, and A3D_GROW_BAD_INDEX is set in the summary's err; a
 *   seed vertex with such an index is ignored (and sets the same bit).
 *   OUTPUTS, all optional but the summary: dist_qv_dev int32 [n], owner_qv_dev int32 [n], selected_full_dev uint8 [n_full],
 *   dist_full_dev int32 [n_full].  The summary (cleared by the call): seeds, reached voxels (dist >= 0, the seeds
 *   included), selected vertices, the largest dist reached (0 when nothing is), the error word.  Integer sums and maxima
 *   only, one atomic per workgroup and counter.
 *   How: (dist, owner) is ONE 64-bit word dist << 32 | owner, relaxed with a 64-bit atomicMin until nothing changes: the
 *   fixed point of value[v] = min over walkable neighbours u of (dist[u] + cost, owner[u]) is the value above, in whatever
 *   order the relaxations land, so two calls give the same bytes in every output.  In a sweep the voxels lowered in the
 *   sweep before offer their word to their neighbours; at most limit / min(cost) sweeps are launched; each raises a device
 *   flag when it lowered anything, and a sweep whose predecessor's flag is clear returns at once.  The host reads nothing
 *   in mid-call; no thread waits for another (no grid barrier, no spin-wait).
 *   The workspace: a3d_grow_workspace_bytes(n) bytes, 256-byte aligned.  The library allocates nothing and does not
 *   synchronise.
 *   A3D_ERR_INVALID with nothing launched and nothing written: no arguments, no scene, n != the scene's level-0 size, a
 *   connectivity other than 6 / 18 / 26, a cost outside 1 .. 65536, a limit outside 0 .. 2^30 or beyond
 *   A3D_GROW_MAX_STEPS steps, neither seed array, no summary_dev, n_full < 0, n > 0 without a workspace, a workspace that is
 *   too small or misaligned. */
#define A3D_GROW_MAX_STEPS 1024
#define A3D_GROW_BAD_INDEX 1
typedef struct a3d_grow_summary {
  int64_t seeds;
  int64_t reached;                  /* voxels with dist >= 0 */
  int64_t selected;                 /* vertices with selected_full = 1 */
  int32_t max_dist;
  int32_t err;                      /* A3D_GROW_BAD_INDEX */
} a3d_grow_summary;                /* 32 bytes */
typedef struct a3d_grow_voxels_args {
  const a3d_scene* scene;
  int64_t        n;
  const int32_t* keys_dev;          /* [n] caller's row order, or NULL: all 0 */
  const uint8_t* seed_qv_dev;       /* [n] or NULL */
  const uint8_t* seed_full_dev;     /* [n_full] or NULL */
  const int64_t* inverse_map_dev;   /* [n_full] or NULL: identity */
  int64_t        n_full;
  int32_t*       dist_qv_dev;       /* out [n] or NULL */
  int32_t*       owner_qv_dev;      /* out [n] or NULL */
  uint8_t*       selected_full_dev; /* out [n_full] or NULL */
  int32_t*       dist_full_dev;     /* out [n_full] or NULL */
  a3d_grow_summary* summary_dev;
  void*          workspace_dev;
  size_t         workspace_bytes;
  int32_t        connectivity;
  int32_t        limit;
  int32_t        cost[3];           /* face, edge, corner */
  int32_t        reserved_;
} a3d_grow_voxels_args;
size_t a3d_grow_workspace_bytes(int64_t n);
int    a3d_grow_voxels(const a3d_grow_voxels_args* args, void* stream);

/* HOW BIG an object is and where it lies: one record per object id of a labelling (csrc/session_measure.hip).  The rules are
 * this library's: the reference exports a mask and measures nothing.  Everything accumulated is an INTEGER (counts, sums of
 * fixed-point coordinates, minima and maxima of order-preserving keys), so a result does not depend on the order in which
 * workgroups run: two calls give the same bytes, and so does any permutation of the vertices (with their labels).
 *
 * a3d_measure_objects.  xyz_dev fp32 [n][3], labels_dev int32 [n], object ids 0..n_classes-1, 1 <= n_classes <= 256;
 * optionally labels_qv_dev int32 [n_qv] (NULL with n_qv = 0: none) and faces_dev int32 [m][3] (NULL with m = 0: a cloud).
 * out_dev: n_classes records a3d_object_moments, 8-byte aligned; err_dev: int32 [1].  Both are cleared by the call.
 * Record k:
 *   vertices, voxels   how many entries of labels / labels_qv equal k -- for `vertices`, among the vertices that COUNT (below).
 *   lo[3], hi[3]       the exact axis-aligned box of the vertices that count, fp32.  Coordinates are compared by the total
 *                      order of their IEEE bit patterns: -0 lies below +0.  An object without a vertex has lo = +inf, hi = -inf.
 *                      (How: key = bits ^ (bits >> 31 ? 0xffffffff : 0x80000000) orders like the value; integer min / max.)
 *   sum[3], mom[6]     first and second moments in FIXED POINT: X_a = llrint(((double)x_a - origin[a]) / quantum), round half
 *                      to even; sum[a] = the sum of X_a; mom = the sums of (XX, XY, XZ, YY, YZ, ZZ).  origin (doubles, finite)
 *                      and quantum (a double, a positive power of two) are passed by value.
 *   A vertex COUNTS when its label lies in 0..n_classes-1 and |X_a| <= 2^bits on every axis (0 <= bits <= 20, by value).
 *   Else it contributes to nothing: a label outside sets A3D_MEASURE_BAD_LABEL, a coordinate outside -- or one that is not
 *   finite -- sets A3D_MEASURE_RANGE (a vertex can set both).
 *   OVERFLOW BOUND: |X_a X_b| <= 2^(2 bits), so no sum can leave int64 while n * 2^(2 bits) <= 2^62; the call refuses any
 *   other n (bits = 20: n <= 2^22 vertices; bits = 16: n <= 2^30), and n, n_qv >= 2^31.
 *   area_thirds        the surface the object covers on the mesh.  For every face (a, b, c), in double, every operation rounded
 *                      on its own (no fma contraction) and in this order:
 *                          e1 = b - a;  e2 = c - a
 *                          nx = e1y*e2z - e1z*e2y;  ny = e1z*e2x - e1x*e2z;  nz = e1x*e2y - e1y*e2x
 *                          len = sqrt((nx*nx + ny*ny) + nz*nz);  Q = llrint(len / area_quantum)
 *                      (len = twice the face's area; divide and sqrt correctly rounded).  Q is added to the object of EACH of
 *                      the three corners: the object's area is area_thirds * area_quantum / 6, and the areas of all objects sum
 *                      EXACTLY to the sum of Q over the counted faces, times area_quantum / 2.  area_quantum: a positive power
 *                      of two, by value (suggested: quantum^2 * 2^8; needed only when m > 0).
 *   A face with a corner index outside 0..n-1 is skipped silently (as the renders skip it); one with a corner whose label
 *   lies outside is skipped and sets A3D_MEASURE_BAD_LABEL; one with len / area_quantum above A3D_MEASURE_MAX_Q = 2^38, or
 *   not a number, is skipped and sets A3D_MEASURE_RANGE.  Coordinates play no other part: a corner outside the fixed-point
 *   range still carries its face.
 *   OVERFLOW BOUND: an object receives at most 3 Q per face, so area_thirds <= 3 m 2^38 < 2^63 while m <= A3D_MEASURE_MAX_FACES
 *   = 2^23; the call refuses a larger m.  (With the suggested area_quantum and bits = 20 a face as large as the scene's box has
 *   Q < 2^36.)
 *   A voxel label outside 0..n_classes-1 sets A3D_MEASURE_BAD_LABEL and is not counted.
 *   How: a workgroup of A3D_MEASURE_BLOCK threads owns A3D_MEASURE_CHUNK consecutive vertices and keeps the 256 records in LDS;
 *   a wave whose lanes carry one label -- labels are coherent in space, so most do -- folds its lanes with shuffles and
 *   updates LDS once, a mixed wave falls back to per-lane LDS atomics; the non-empty records then go to out_dev with integer
 *   atomics (add, unsigned min / max: no compare-and-swap loop).  Voxels and faces are launches of their own, shaped alike.
 *   The library allocates nothing and does not synchronise.
 *   A3D_ERR_INVALID with nothing launched and nothing written: no arguments, n_classes outside 1..256, bits outside 0..20, n, n_qv
 *   or m negative or beyond the bounds above, out_dev or err_dev NULL, out_dev not 8-byte aligned, a needed input NULL (xyz_dev,
 *   labels_dev when n > 0; labels_qv_dev when n_qv > 0; faces_dev when m > 0), an origin that is not finite, a quantum (or, with
 *   m > 0, an area_quantum) that is not a positive power of two.
 *
 * a3d_object_extents -- the second pass, for oriented boxes.  axes_dev fp32 [n_classes][3][3]: three axes per object (row j of
 * object k = axis j).  For every vertex whose label k lies in range and whose coordinates are finite, and every axis j, in fp32,
 * every operation rounded on its own:  p = (a_x*x + a_y*y) + a_z*z.  out_dev fp32 [n_classes][3][2] = (min, max) of p per
 * (object, axis), by the same total order of bit patterns; an object without a vertex has (+inf, -inf).  err_dev int32 [1]: a
 * label outside sets A3D_MEASURE_BAD_LABEL; a coordinate that is not finite sets A3D_MEASURE_RANGE and the vertex is skipped;
 * a projection that is NaN (axes that are not finite) sets A3D_MEASURE_RANGE and is skipped.  Both outputs are cleared by the
 * call; the same kernel shape; A3D_ERR_INVALID as above (n_classes, n, NULL pointers; out_dev 4-byte aligned). */
#define A3D_MEASURE_RANGE     1
#define A3D_MEASURE_BAD_LABEL 2
#define A3D_MEASURE_MAX_BITS  20
#define A3D_MEASURE_MAX_Q     (1ll << 38)
#define A3D_MEASURE_MAX_FACES (1ll << 23)
#define A3D_MEASURE_BLOCK     256
#define A3D_MEASURE_CHUNK     1024
typedef struct a3d_object_moments {
  int64_t vertices, voxels;
  int64_t sum[3];                   /* X, Y, Z */
  int64_t mom[6];                   /* XX, XY, XZ, YY, YZ, ZZ */
  int64_t area_thirds;
  float   lo[3], hi[3];
  int32_t reserved_[2];
} a3d_object_moments;              /* 128 bytes */
typedef struct a3d_measure_args {
  const float*   xyz_dev;           /* [n][3] */
  const int32_t* labels_dev;        /* [n] */
  int64_t        n;
  const int32_t* labels_qv_dev;     /* [n_qv] or NULL */
  int64_t        n_qv;
  const int32_t* faces_dev;         /* [m][3] or NULL */
  int64_t        m;
  a3d_object_moments* out_dev;      /* out [n_classes] */
  int32_t*       err_dev;           /* out int32 [1] */
  double         origin[3];
  double         quantum;
  double         area_quantum;
  int32_t        n_classes;
  int32_t        bits;
} a3d_measure_args;
int    a3d_measure_objects(const a3d_measure_args* args, void* stream);

typedef struct a3d_extents_args {
  const float*   xyz_dev;           /* [n][3] */
  const int32_t* labels_dev;        /* [n] */
  int64_t        n;
  const float*   axes_dev;          /* [n_classes][3][3] */
  float*         out_dev;           /* out [n_classes][3][2] */
  int32_t*       err_dev;           /* out int32 [1] */
  int32_t        n_classes;
  int32_t        reserved_;
} a3d_extents_args;
int    a3d_object_extents(const a3d_extents_args* args, void* stream);

/* WHICH WAY THE SURFACE FACES: one unoriented normal per level-0 voxel, from the points of its 3 x 3 x 3 neighbourhood, lifted
 * to the vertices (csrc/session_normals.hip).  With it a point cloud is lit (a3d_render_shade_lit_points) and culled
 * (a3d_cull_points) as a mesh is.  The rule is this library's: the reference shows clouds unlit.  Two stages: the first is
 * INTEGER, so that the order in which workgroups run cannot matter; the second is ONE SEQUENTIAL double-precision
 * computation per voxel, every operation rounded on its own (no fma contraction), using only + - x / sqrt (all correctly
 * rounded) in the order written: a restatement in float64 scalars gives the same bits (tests/normals_rule.py).
 *
 * a3d_estimate_normals.  scene, n = its level-0 size (rows in the CALLER's order); xyz_dev fp32 [n_full][3];
 * inverse_map_dev int64 [n_full], NULL = the identity; origin (doubles, finite), quantum (a positive power of two) and bits
 * (0..20) by value, a3d_measure_objects' fixed-point frame; optionally viewpoint (doubles, finite) with has_viewpoint != 0.
 *   STAGE A, per vertex i: row = inverse_map[i];  X_a = llrint(((double)x_a - origin[a]) / quantum), round half to even.
 *   The vertex COUNTS when 0 <= row < n and |X_a| <= 2^bits on every axis.  Else it contributes nothing: a row outside sets
 *   A3D_NORMALS_BAD_INDEX, a coordinate outside -- or one that is not finite -- sets A3D_NORMALS_RANGE (a vertex can set
 *   both).  Per voxel (caller row), over the vertices that count: cnt (int32), sum[3] = the sums of X_a, mom[6] = the sums of
 *   (XX, XY, XZ, YY, YZ, ZZ), int64, by integer atomics.
 *   OVERFLOW BOUND, a3d_measure_objects': no sum can leave int64 while n_full * 2^(2 bits) <= 2^62; the call refuses any
 *   other n_full, and n_full >= 2^31.
 *   STAGE B, per voxel: the NEIGHBOURHOOD is the voxel and its present neighbours in A3D_TAB_NBR27, all 27 offsets, both ends
 *   through A3D_TAB_ORIGROW: never across batch samples.  N, S_a, M_ab = the integer sums of cnt, sum, mom over it.
 *   N < 3: no normal.  Else recentre EXACTLY, in integers, about R_a = floor(S_a / N):
 *       s_a = S_a - N R_a;       m_ab = M_ab - R_a S_b - R_b S_a + N R_a R_b
 *   (= the sums of (X_a - R_a) and (X_a - R_a)(X_b - R_b): 0 <= s_a < N, and m_aa <= M_aa + N since the sum of squares about
 *   the mean is the least, so both fit int64 and wrapping 64-bit arithmetic yields them exactly whatever the intermediates do).
 *   Convert s_a, m_ab and N to double (round to nearest even).  From here on doubles:
 *       C_ab = m_ab - (s_a * s_b) / N                              (a, b = 0..2; C is symmetric, V starts as the identity)
 *   6 SWEEPS of cyclic Jacobi, each over the pairs (p, q) = (0, 1), (0, 2), (1, 2) in this order, r the third index.  A pair
 *   whose C_pq == 0 is skipped.  Else, with app = C_pp, aqq = C_qq, apq = C_pq:
 *       theta = (aqq - app) / (2 * apq)
 *       t = 1 / (|theta| + sqrt(theta * theta + 1));   if theta < 0: t = -t      (an infinite theta * theta gives t = 0)
 *       c = 1 / sqrt(t * t + 1);   s = t * c;   h = t * apq
 *       C_pp = app - h;   C_qq = aqq + h;   C_pq = C_qp = 0
 *       arp = C_rp, arq = C_rq:   C_rp = C_pr = c * arp - s * arq;   C_rq = C_qr = s * arp + c * arq
 *       for k = 0..2, vkp = V_kp, vkq = V_kq:   V_kp = c * vkp - s * vkq;   V_kq = s * vkp + c * vkq
 *   d = (C_00, C_11, C_22).  imin = 0; if d_1 < d_imin: imin = 1; if d_2 < d_imin: imin = 2 (ties: the lowest index); imax
 *   likewise with >; d_mid = d of the remaining index, or d_imin when imin == imax.  The normal is VALID iff
 *   d_mid * 2^20 > d_imax and d_imax < +inf (the product is exact): a neighbourhood narrower than 1/1024 of its length, in
 *   standard deviation, is a line and has no normal.  v = column imin of V.
 *   THE SIGN.  With a viewpoint:  mean_a = origin[a] + quantum * ((double)R_a + s_a / N);
 *       g = (v_0 * (vp_0 - mean_0) + v_1 * (vp_1 - mean_1)) + v_2 * (vp_2 - mean_2);   g < 0: v = -v (towards the viewpoint)
 *   Without: the component of largest |v_a| (the first of equals) is made positive: if it is < 0, v = -v.
 *   normal = (float)v per component;  variation = (float)(max(d_imin, 0) / ((d_0 + d_1) + d_2)), 0 when that sum is not > 0
 *   (the surface variation: 0 on a plane, 1/3 for an isotropic blob).  A voxel without a valid normal has normal (0, 0, 0)
 *   and variation 0.
 *   THE LIFT: normal_full[i] = normal_qv[inverse_map[i]], (0, 0, 0) for a row outside 0..n-1.
 *   OUTPUTS, all optional but the summary: normal_qv_dev fp32 [n][3], variation_qv_dev fp32 [n], count_qv_dev int32 [n] (the
 *   neighbourhood's N), moments_qv_dev int64 [n][10] (stage A's own words of the voxel: cnt, sum[3], mom[6]), normal_full_dev
 *   fp32 [n_full][3].  The summary (cleared by the call): counted vertices, voxels with and without a valid normal, the error
 *   word.  Integer sums, one atomic per workgroup and counter.
 *   The workspace: a3d_normals_workspace_bytes(n) bytes, 256-byte aligned, cleared by the call.  The library allocates
 *   nothing and does not synchronise; the stages are launches -- no grid barrier, no spin-wait.  Two calls give the same
 *   bytes in every output, and so does any permutation of the vertices (with their map entries).
 *   A3D_ERR_INVALID with nothing launched and nothing written: no arguments, no scene, n != the scene's level-0 size, n_full
 *   > 0 without xyz_dev, n_full < 0 or beyond the bound above, bits outside 0..20, a quantum that is not a positive power of
 *   two, an origin or (with has_viewpoint) a viewpoint that is not finite, no summary_dev, a workspace that is missing, too
 *   small or misaligned.
 *   LIMITS: all vertices of a voxel share one normal (shading is faceted at the voxel size); the sign is only as good as the
 *   viewpoint (a3d_orient_normals, below, carries a sign from voxel to voxel). */
#define A3D_NORMALS_RANGE     1
#define A3D_NORMALS_BAD_INDEX 2
typedef struct a3d_normals_summary {
  int64_t counted;                  /* vertices that counted */
  int64_t valid;                    /* voxels with a valid normal */
  int64_t invalid;                  /* voxels without one */
  int32_t err;                      /* A3D_NORMALS_RANGE | A3D_NORMALS_BAD_INDEX */
  int32_t reserved_;
} a3d_normals_summary;             /* 32 bytes */
typedef struct a3d_estimate_normals_args {
  const a3d_scene* scene;
  int64_t        n;
  const float*   xyz_dev;           /* [n_full][3] */
  const int64_t* inverse_map_dev;   /* [n_full] or NULL: identity */
  int64_t        n_full;
  float*         normal_qv_dev;     /* out [n][3] or NULL */
  float*         variation_qv_dev;  /* out [n] or NULL */
  int32_t*       count_qv_dev;      /* out [n] or NULL */
  int64_t*       moments_qv_dev;    /* out [n][10] or NULL */
  float*         normal_full_dev;   /* out [n_full][3] or NULL */
  a3d_normals_summary* summary_dev;
  void*          workspace_dev;
  size_t         workspace_bytes;
  double         origin[3];
  double         quantum;
  double         viewpoint[3];      /* looked at only with has_viewpoint */
  int32_t        bits;
  int32_t        has_viewpoint;
} a3d_estimate_normals_args;       /* 168 bytes */
size_t a3d_normals_workspace_bytes(int64_t n);
int    a3d_estimate_normals(const a3d_estimate_normals_args* args, void* stream);

/* Host only, no GPU: STAGE B of one neighbourhood from its integer sums (count = N, sum3 = S, mom6 = M; HOST arrays), by the
 * function the kernel calls: out5 = normal[3], variation, valid as 0 or 1.  origin: a HOST array of 3; viewpoint: a HOST
 * array of 3, or NULL for the sign without one.  A3D_ERR_INVALID for a NULL array, count < 0 or a quantum that is not a
 * positive power of two. */
int    a3d_normals_solve(int64_t count, const int64_t* sum3, const int64_t* mom6, const double* origin, double quantum,
                         const double* viewpoint, float* out5);

/* ONE SIGN FOR A WHOLE SURFACE: the normals of a3d_estimate_normals oriented consistently by PROPAGATION from seed voxels over
 * the adjacency of a3d_label_pieces (csrc/session_orient.hip).  The viewpoint sign is right for the walls of a room scanned
 * from inside and wrong for the far sides of everything that stands in it; this call carries a trusted sign from a seed along
 * the surface, flipping wherever two neighbouring normals disagree.  The rule is this library's: the reference's tool has no
 * counterpart.  Everything but the edge function is an integer, and that function is one fixed sequence of fp32 operations.
 *
 * a3d_orient_normals.  scene, n = its level-0 size (rows in the CALLER's order), n <= A3D_ORIENT_MAX_ROWS = 2^21 (a path has
 * fewer than n edges of cost <= 1024: every path cost fits 31 bits).  normal_qv_dev fp32 [n][3].
 *   ADMITTED ROWS: a row whose three components are finite and not all zero (-0 is zero).  Any other row takes no part and
 *   keeps its bytes.
 *   EDGE: two admitted neighbours under the connectivity (6, 18 or 26, the offsets a3d_label_pieces admits; A3D_TAB_NBR27,
 *   both ends through A3D_TAB_ORIGROW: never across batch samples).  For the normals a and b, in fp32, every operation
 *   rounded on its own (no fma contraction), as NSIM above:
 *       dot = (a0*b0 + a1*b1) + a2*b2
 *       w = 1 + (int)floorf(1023.0f * fmaxf(1.0f - fabsf(dot), 0.0f))          an integer in 1 .. 1024 (a NaN dot gives 1)
 *       flip = dot < 0
 *   Both are symmetric bit for bit.  a3d_orient_edge(a, b, &w, &flip) is the same function on the host (HOST arrays of 3;
 *   A3D_ERR_INVALID for a NULL pointer), so a test without a GPU holds the very function the kernel calls.
 *   SEEDS, mode A3D_ORIENT_GIVEN: seed_qv_dev uint8 [n]; an admitted row with a non-zero entry is a seed whose sign is trusted
 *   as it stands -- unless seed_flip_dev uint8 [n] (optional) holds a non-zero entry for it: then its normal is negated first.
 *   SEEDS, mode A3D_ORIENT_NEAREST: component_qv_dev int32 [n] (< 0: in no component, else 0 .. n-1; a value >= n sets
 *   A3D_ORIENT_BAD_COMPONENT and the row is in none), position_qv_dev fp32 [n][3], viewpoint (doubles, finite).  A CANDIDATE
 *   is an admitted row in a component whose position is finite.  In double, every operation rounded on its own:
 *       dx = (double)p_x - vp_x (dy, dz likewise);   d2 = (dx*dx + dy*dy) + dz*dz
 *   Per component the seed is the candidate with the lexicographically least (d2, row) -- found without any dependence on
 *   order: one pass of 64-bit atomicMin on the bit pattern of d2 (d2 >= +0 or +inf: the patterns order like the values), one
 *   pass of atomicMin on the row among the candidates that hold that d2.  The seed's flip is g < 0 with
 *       g = (n0*(vp0 - p0) + n1*(vp1 - p1)) + n2*(vp2 - p2)                      in double, n and p converted first
 *   PHASE 1, distance and owner: the value of an admitted voxel v is the LEXICOGRAPHIC MINIMUM of (d, s) over the seeds s with a
 *   path of edges to v, d = the sum of w along the path, s = the seed's caller row: dist[v] = d, owner[v] = s, -1 where there
 *   is none.  There is no limit on d.  How: a3d_grow_voxels' method -- ONE word dist << 32 | owner, 64-bit atomicMin, only the
 *   voxels lowered in the sweep before offer, a sweep that lowered anything raises a device flag and the next launch returns
 *   at once when the flag is clear.  The fixed point is unique (the argument at a3d_grow_voxels), whatever order the
 *   relaxations land in.  The call launches exactly `sweeps` (1 .. A3D_ORIENT_MAX_SWEEPS) sweep kernels; the summary's
 *   `converged` is 1 when the last of them lowered nothing: then every output is the rule's.  When it is 0 the outputs are
 *   a safe intermediate state and depend on timing: call again with resume = 1 and the SAME arguments and workspace, and the
 *   call continues from the workspace's state (the edge table, the words, the front, the seeds' flips) instead of clearing
 *   it; since the fixed point is unique, resuming gives the same bytes as one long call.  resume = 1 on a workspace no call
 *   has filled for these arguments is undefined in its outputs (but stays inside its buffers).
 *   The 27 (w, flip) words of every voxel are tabulated once (one kernel, 2 bytes a slot) and the sweeps read the table, not
 *   the normals.
 *   PHASE 2, parent: a pure function of phase 1.  A seed has none.  Any other reached voxel v takes the neighbour u at the
 *   LOWEST offset slot k (0 .. 26, offset (k % 3 - 1, (k / 3) % 3 - 1, k / 9 - 1), among the admitted offsets) with
 *   owner[u] == owner[v] and dist[u] + w(u, v) == dist[v]; edge_flip[v] = flip(u, v).  Such a u exists at the fixed point
 *   (before it, a voxel without one is treated as a seed without a flip).  The parity of the path is NOT carried in the
 *   relaxed word: XOR is not monotone, and a transient word of parity 0 could never be raised again.
 *   PHASE 3, parity: parity[v] = the XOR of edge_flip along the parent chain, XOR the seed's flip.  Pointer jumping on two
 *   buffers of (ancestor, parity), each round a launch that reads one and writes the other, ceil(log2(n)) rounds (a chain
 *   has fewer than n edges).
 *   OUTPUTS, all optional but the summary: normal_out_qv_dev fp32 [n][3] (the input with the sign bit of every component
 *   flipped where parity == 1; the input's bytes elsewhere, rows not reached or not admitted included; it must not be the
 *   input array), flipped_qv_dev uint8 [n] (the parity), dist_qv_dev and owner_qv_dev int32 [n], normal_full_dev fp32
 *   [n_full][3] = the output normal of row inverse_map[i] (NULL map: the identity), (0, 0, 0) for a row outside 0..n-1, which
 *   sets A3D_ORIENT_BAD_INDEX.  The summary (cleared by the call): admitted rows, seeds, reached and unreached (admitted)
 *   rows, flipped rows, conflicts, the largest dist, converged, the error word.  CONFLICTS: the edges, each counted once,
 *   whose two OUTPUT normals have dot < 0 (the dot above; negating a normal negates it exactly): they remain where the
 *   regions of two seeds meet, and on a loop that cannot be oriented.  Integer sums and maxima, one atomic per workgroup and
 *   counter.  Two calls give the same bytes in every output.
 *   The workspace: a3d_orient_workspace_bytes(n) bytes (0 for n < 0 or n > 2^21), 256-byte aligned.  The library allocates
 *   nothing, does not synchronise and reads nothing back; the phases are launches -- no grid barrier, no spin-wait.
 *   A3D_ERR_INVALID with nothing launched and nothing written: no arguments, no scene, n != the scene's level-0 size or
 *   n > 2^21, a connectivity other than 6 / 18 / 26, sweeps outside 1 .. 4096, a mode or a resume that is neither 0 nor 1, no
 *   normal_qv_dev with n > 0, mode GIVEN without seed_qv_dev, mode NEAREST without component_qv_dev or position_qv_dev or with
 *   a viewpoint that is not finite, no summary_dev, normal_out_qv_dev == normal_qv_dev, a workspace that is missing, too small
 *   or misaligned, n_full < 0 or >= 2^31.
 *   LIMITS: a shortest-path tree, not a minimum spanning tree; one normal per voxel, so a plate one voxel thick has one side;
 *   the cost scale 1 .. 1024 is this library's choice and is not tuned on real scans. */
#define A3D_ORIENT_MAX_ROWS   (1 << 21)
#define A3D_ORIENT_MAX_SWEEPS 4096
#define A3D_ORIENT_GIVEN      0
#define A3D_ORIENT_NEAREST    1
#define A3D_ORIENT_BAD_INDEX     1
#define A3D_ORIENT_BAD_COMPONENT 2
typedef struct a3d_orient_summary {
  int64_t admitted;
  int64_t seeds;
  int64_t reached;                  /* voxels with dist >= 0, the seeds included */
  int64_t unreached;                /* admitted voxels without a seed to reach them */
  int64_t flipped;
  int64_t conflicts;
  int32_t max_dist;
  int32_t converged;                /* 1: the last sweep lowered nothing */
  int32_t err;                      /* A3D_ORIENT_BAD_INDEX | A3D_ORIENT_BAD_COMPONENT */
  int32_t reserved_;
} a3d_orient_summary;              /* 64 bytes */
typedef struct a3d_orient_normals_args {
  const a3d_scene* scene;
  int64_t        n;
  const float*   normal_qv_dev;     /* [n][3] */
  const uint8_t* seed_qv_dev;       /* [n], mode GIVEN */
  const uint8_t* seed_flip_dev;     /* [n] or NULL, mode GIVEN */
  const int32_t* component_qv_dev;  /* [n], mode NEAREST */
  const float*   position_qv_dev;   /* [n][3], mode NEAREST */
  const int64_t* inverse_map_dev;   /* [n_full] or NULL: identity */
  int64_t        n_full;
  float*         normal_out_qv_dev; /* out [n][3] or NULL */
  uint8_t*       flipped_qv_dev;    /* out [n] or NULL */
  int32_t*       dist_qv_dev;       /* out [n] or NULL */
  int32_t*       owner_qv_dev;      /* out [n] or NULL */
  float*         normal_full_dev;   /* out [n_full][3] or NULL */
  a3d_orient_summary* summary_dev;
  void*          workspace_dev;
  size_t         workspace_bytes;
  double         viewpoint[3];      /* mode NEAREST */
  int32_t        mode;              /* A3D_ORIENT_GIVEN, A3D_ORIENT_NEAREST */
  int32_t        connectivity;
  int32_t        sweeps;
  int32_t        resume;
} a3d_orient_normals_args;         /* 176 bytes */
size_t a3d_orient_workspace_bytes(int64_t n);
int    a3d_orient_normals(const a3d_orient_normals_args* args, void* stream);
int    a3d_orient_edge(const float* a, const float* b, int32_t* w, int32_t* flip);

/* LABELS TO AND FROM ANOTHER POINT SET: an index over an arbitrary point set and the bulk, exact nearest-point query against
 * it (csrc/session_transfer.hip).  a3d_nearest_rows scans every row for at most 64 queries a call, which is right for a click;
 * this serves a million queries.  The reference has no counterpart.  The rule is a3d_nearest_rows' with a cutoff:
 *
 * THE RULE.  For query q take every source row p whose three coordinates are finite.  d2 = ((px-qx)^2 + (py-qy)^2) + (pz-qz)^2
 * in fp32 from the differences, every operation rounded on its own (no fma contraction).  r2 = fl32(max_distance *
 * max_distance), rounded once.  nearest_out[q] = the FIRST arg-min of d2 among the rows with d2 <= r2: ties go to the lowest
 * source row, whichever cells the candidates sit in.  When no row qualifies, or q has a coordinate that is not finite:
 * nearest_out[q] = -1 and d2_out[q] = +inf.  labels_out[q] = labels_src[nearest_out[q]], or fill without a match.
 *
 * a3d_point_index_create builds the index over xyz_dev fp32 [n][3] (0 <= n < 2^31) with cubic cells of cell_size (fp32, finite,
 * > 0): the cell of a coordinate is floor(fl32(x / cell_size)).  A row with a coordinate that is not finite is left out and
 * counted; a row with |floor(fl32(x / cell_size))| > 2^20 on some axis cannot be keyed: it is left out too and the build sets
 * A3D_TRANSFER_UNKEYABLE, which every query's summary repeats -- such an index answers as if those rows were absent, so
 * treat the bit as an error.  The index lives in the caller's workspace (a3d_point_index_workspace_bytes(n) bytes, 256-byte
 * aligned; 0 for n < 0 or n >= 2^31), as an a3d_scene does: keep the workspace until a3d_point_index_destroy, which frees the
 * host handle only.  xyz_dev is not needed after the build.  The build is a chain of launches on `stream` (one radix sort in
 * its launch-chain form among them) and does not synchronise.
 *
 * a3d_point_index_nearest answers m queries (queries_dev fp32 [m][3], 0 <= m < 2^31) with 0 < max_distance <= cell_size / 2,
 * both compared in fp32; anything else is A3D_ERR_INVALID.  Within that bound the 27 cells around a query's cell hold every
 * row with d2 <= r2; where r2 is not a normal fp32 number (max_distance below 2^-63 or from 2^64 on) that
 * argument fails and the call tests every indexed row instead: the same rule, without the index's speed.
 * labels_src_dev int32 [n] may be NULL; labels_out_dev int32 [m] is given exactly when it is.  d2_out_dev fp32 [m] may be NULL.
 * summary_dev (8-byte aligned, cleared by the call): matched queries; unmatched queries with finite coordinates; queries with a
 * coordinate that is not finite (matched + unmatched + nonfinite = m); source rows left out as not finite; the error word.
 * Integer sums, one atomic per workgroup and counter: two calls give the same bytes in every output.
 * A3D_ERR_INVALID with nothing launched: no index, m out of range, m > 0 without queries_dev or nearest_out_dev, no
 * summary_dev, labels_out_dev without labels_src_dev or the reverse, a max_distance outside (0, cell_size / 2] or NaN; for
 * the build: n out of range, n > 0 without xyz_dev, a cell_size that is not finite and > 0, no or a misaligned workspace, no
 * `out` (A3D_ERR_WORKSPACE for one that is too small).
 * LIMITS: the nearest VERTEX, not the nearest point of a mesh's surface; one nearest row, no k-nearest vote; max_distance
 * at most half a cell; one point set per index. */
#define A3D_TRANSFER_UNKEYABLE   1   /* a source coordinate beyond 2^20 cells was left out */
#define A3D_TRANSFER_SORT_FAILED 2   /* the build's sort gave up waiting (as A3D_ERR_HIP of a scene build): the index is not usable */
typedef struct a3d_point_index a3d_point_index;
typedef struct a3d_transfer_summary {
  int64_t matched;                  /* queries with a row within max_distance */
  int64_t unmatched;                /* finite queries without one */
  int64_t nonfinite;                /* queries with a coordinate that is not finite */
  int64_t source_left_out;          /* source rows left out of the index as not finite */
  int32_t err;                      /* A3D_TRANSFER_UNKEYABLE | A3D_TRANSFER_SORT_FAILED */
  int32_t reserved_;
} a3d_transfer_summary;            /* 40 bytes */
size_t a3d_point_index_workspace_bytes(int64_t n);
int    a3d_point_index_create(const float* xyz_dev, int64_t n, float cell_size, void* workspace_dev, size_t workspace_bytes,
                              void* stream, a3d_point_index** out);
void   a3d_point_index_destroy(a3d_point_index* index);
int    a3d_point_index_nearest(const a3d_point_index* index, const float* queries_dev, int64_t m, float max_distance,
                               const int32_t* labels_src_dev, int32_t fill, int32_t* nearest_out_dev, float* d2_out_dev,
                               int32_t* labels_out_dev, a3d_transfer_summary* summary_dev, void* stream);

/* MORE OBJECTS LIKE THIS ONE: query by example on per-voxel features (csrc/session_match.hip) -- one prototype per example
 * class, and per voxel the best prototype under a cosine threshold.  The features are the backbone's output, fp32 [n][128]
 * (A3D_MATCH_CHANNELS).  The reference has no counterpart.  The rule is built so that every DECISION is reproducible to the
 * bit by a plain restatement (tests/match_rule.py); only the displayed score carries a tolerance.
 *
 * THE RULE, PROTOTYPES (a3d_feature_prototypes).  classes_dev int32 [n]: -1 = the row is no example, 0 .. n_classes-1 = its
 * class (1 <= n_classes <= 256); any other value sets A3D_MATCH_BAD_CLASS and the row is no example.  Every channel of an
 * example row goes to fixed point, X = llrint(f / quantum) with quantum = 2^-20 (A3D_MATCH_QUANTUM_BITS; the quotient is
 * exact, the rounding is to nearest even), accepted while |X| <= 2^40 (A3D_MATCH_FIXED_BITS).  A row with ANY channel beyond
 * that or not finite is left out as a whole and counted in examples_left_out.  sums_dev int64 [n_classes][128] and count_dev
 * int32 [n_classes] are the INTEGER sums of X and of 1 over the class's rows that count: they depend on no order.  The call
 * refuses n >= 2^22 (A3D_MATCH_MAX_EXAMPLE_ROWS: count * 2^40 <= 2^62 fits int64).  sums, count and the summary are cleared by
 * the call.  The prototype of class c is computed by the CALLER, in double and rounded once to fp32:
 *     p_c[i] = (float)(((double)sums[c][i] / (double)count[c]) * quantum)
 * (int64 -> double to nearest even, one division, one exact scaling, one rounding); a class with count 0 has no prototype.
 * Prototypes are NOT normalised: their squared length enters the test below, which lets a threshold of exactly 1 be met
 * exactly (a voxel that is a power of two times its prototype has dot * dot == nn * pp to the bit).
 *
 * THE RULE, MATCH (a3d_feature_match).  protos_dev fp32 [k][128] and proto_class_dev int32 [k] with 1 <= k <= 256
 * (A3D_MATCH_MAX_PROTOTYPES), classes in 0..255; c2 = cos_min * cos_min for a double cos_min in [0, 1], rounded once.  All
 * arithmetic is double.  With ONE accumulator each, starting at 0, channels ascending i = 0..127:
 *     nn = sum f_i * f_i;      pp_c = sum p_ci * p_ci;      dot_c = sum f_i * p_ci
 * Each product of two fp32 values is exact in double, so a fused multiply-add and a multiply then an add give the same bits;
 * only the order of the additions matters, and it is fixed (no split across lanes, no matrix cores).
 * A voxel CAN BE SCORED when all its channels are finite, nn > 0 and candidate_dev (uint8 [n], optional) is not 0 there; a
 * prototype TAKES PART when 0 < pp_c < +inf (one with a channel that is not finite also sets A3D_MATCH_BAD_PROTOTYPE, one
 * with a class outside 0..255 sets A3D_MATCH_BAD_CLASS and is not counted in the summary).  For a voxel that can be scored
 * ONE SCAN runs over the prototypes that take part, c ascending, with d2_c = dot_c * dot_c:
 *   best:  the first becomes the best; a later c replaces the best b when it BEATS it: with s = the sign of dot (-1, 0, 1),
 *          s_c != s_b: s_c > s_b;  both > 0: d2_c * pp_b > d2_b * pp_c;  both < 0: d2_c * pp_b < d2_b * pp_c;  both 0: no.
 *   match: c PASSES when dot_c > 0 and d2_c >= (c2 * (nn * pp_c)); the first that passes becomes the match; a later passing
 *          c replaces the match m when d2_c * pp_m > d2_m * pp_c.
 * Every multiplication is rounded on its own, with that parenthesisation; ties keep the lower index.  The comparison of
 * rounded products is not transitive in the last bit, so the ORDER of the scan is part of the rule.
 * OUTPUTS: match_qv_dev int32 [n] = proto_class of the match, -1 without one; best_qv_dev int32 [n] = the best's index, -1
 * where the voxel cannot be scored or no prototype takes part; score_qv_dev fp32 [n] = (float)(dot_b / sqrt(nn * pp_b)) of the
 * best b (double division and square root, one rounding to fp32), 0 where best is -1.  With inverse_map_dev int64 [n_full]:
 * match_full_dev int32 [n_full] and score_full_dev fp32 [n_full] = the values of voxel inverse_map[j]; an index outside
 * 0..n-1 sets A3D_MATCH_BAD_INDEX and is not followed (the two entries are not written).  The summary (8-byte aligned, cleared
 * by the call): matched voxels per class, rows with a channel that is not finite (whatever candidate says), the error word.
 * Integer sums, one atomic per workgroup and counter: two calls give the same bytes in every output.
 *
 * The library allocates nothing and does not synchronise; the stages are launches -- no grid barrier, no spin-wait.
 * A3D_ERR_INVALID with nothing launched and nothing written: no arguments; n < 0 or too large (2^22 for the prototypes, 2^31
 * for the match, also n_full); rows without feats_dev (or one that is not 16-byte aligned), classes_dev or the per-voxel
 * outputs; no sums_dev, count_dev, summary_dev (or sums, summary not 8-byte aligned); n_classes outside 1..256; k outside
 * 1..256; no protos_dev or proto_class_dev; cos_min outside [0, 1] or NaN; match_full_dev, score_full_dev or n_full > 0
 * without inverse_map_dev, or inverse_map_dev with n_full > 0 and without both.
 * LIMITS: one prototype per class, the mean -- an object whose parts look different is described badly by it; the features
 * are whatever the backbone learnt: nothing here makes them discriminative. */
#define A3D_MATCH_CHANNELS         128
#define A3D_MATCH_QUANTUM_BITS     20        /* quantum = 2^-20 */
#define A3D_MATCH_FIXED_BITS       40        /* |X| <= 2^40 */
#define A3D_MATCH_MAX_EXAMPLE_ROWS (1 << 22) /* a3d_feature_prototypes: n below this */
#define A3D_MATCH_MAX_PROTOTYPES   256       /* k, n_classes, and the classes counted */
#define A3D_MATCH_CHUNK            16        /* prototypes the match kernel stages in LDS at a time (a kernel constant, for tests) */
#define A3D_MATCH_BAD_CLASS        1
#define A3D_MATCH_BAD_INDEX        2
#define A3D_MATCH_BAD_PROTOTYPE    4
typedef struct a3d_prototypes_summary {
  int64_t examples;                 /* rows that were summed */
  int64_t examples_left_out;        /* example rows left out: a channel beyond 2^40 quanta or not finite */
  int32_t err;                      /* A3D_MATCH_BAD_CLASS */
  int32_t reserved_;
} a3d_prototypes_summary;          /* 24 bytes */
typedef struct a3d_feature_prototypes_args {
  const float*   feats_dev;         /* [n][128] */
  const int32_t* classes_dev;       /* [n] */
  int64_t        n;
  int64_t*       sums_dev;          /* out [n_classes][128] */
  int32_t*       count_dev;         /* out [n_classes] */
  a3d_prototypes_summary* summary_dev;
  int32_t        n_classes;
  int32_t        reserved_;
} a3d_feature_prototypes_args;     /* 56 bytes */
typedef struct a3d_match_summary {
  int64_t matched[A3D_MATCH_MAX_PROTOTYPES];   /* voxels whose match has this class */
  int64_t rows_nonfinite;           /* rows with a channel that is not finite */
  int32_t err;                      /* A3D_MATCH_BAD_CLASS | A3D_MATCH_BAD_INDEX | A3D_MATCH_BAD_PROTOTYPE */
  int32_t reserved_;
} a3d_match_summary;               /* 2064 bytes */
typedef struct a3d_feature_match_args {
  const float*   feats_dev;         /* [n][128] */
  int64_t        n;
  const float*   protos_dev;        /* [k][128] */
  const int32_t* proto_class_dev;   /* [k] */
  const uint8_t* candidate_dev;     /* [n] or NULL: every voxel */
  const int64_t* inverse_map_dev;   /* [n_full] or NULL: no lift */
  int64_t        n_full;
  int32_t*       match_qv_dev;      /* out [n] */
  int32_t*       best_qv_dev;       /* out [n] */
  float*         score_qv_dev;      /* out [n] */
  int32_t*       match_full_dev;    /* out [n_full], with inverse_map_dev */
  float*         score_full_dev;    /* out [n_full], with inverse_map_dev */
  a3d_match_summary* summary_dev;
  double         cos_min;
  int32_t        k;
  int32_t        reserved_;
} a3d_feature_match_args;          /* 120 bytes */
int    a3d_feature_prototypes(const a3d_feature_prototypes_args* args, void* stream);
int    a3d_feature_match(const a3d_feature_match_args* args, void* stream);

/* THE PLANES OF A SCAN: the few global planes a room is made of (floor, ceiling, walls, table tops), their equations, and
 * which voxels lie on each (csrc/session_planes.hip).  The reference has no counterpart; THE RULE is this library's, restated in
 * tests/planes_rule.py.  Hough votes are INTEGER counts (no order, no rounding); a plane is fitted from INTEGER sums by the
 * solve of a3d_estimate_normals; every test a row passes or fails is exact.  Two calls give the same bytes in every output.
 *
 * a3d_find_planes.  Per row i of n: normal_dev fp32 [n][3] (zeros = no normal; the caller's word that it is a unit vector),
 * pos_dev fp32 [n][3], optionally candidate_dev uint8 [n] (0 = the row takes no part).  origin, quantum, bits: the fixed-point
 * frame of a3d_measure_objects (n 2^(2 bits) <= 2^62, n < 2^31).  table_dev int32 [3 G G][3], G = A3D_PLANES_GRID = 16: the
 * HOST's table of cell-centre directions (below); the kernels never normalise.  By value: bin_width w >= 1 and dist_tol >= 0,
 * int64 in units of 2^-20 quanta (the units of C . X); cos_min, a double in [0, 1]; min_voxels >= 1; max_planes in
 * 1..A3D_PLANES_MAX.
 *   ADMISSION, the first failing test names the reason the row is left out for (summary.left_out[reason]):
 *     A3D_PLANES_OUT_CANDIDATE  candidate[i] == 0
 *     A3D_PLANES_OUT_NONFINITE  a component of the normal or of the position is a NaN or an infinity
 *     A3D_PLANES_OUT_ZERO       the normal is (+-0, +-0, +-0)
 *     A3D_PLANES_OUT_FRAME      X_a = llrint(((double)p_a - origin[a]) / quantum) has |X_a| > 2^bits on some axis
 *     A3D_PLANES_OUT_BINS       the offset bin k (below) lies outside 0..D-1
 *   DIRECTION CELL.  a = the axis of the component of largest magnitude (of equals the lowest axis); if n_a < 0 the normal is
 *   negated (its canonical sign); b = (a + 1) mod 3, c = (a + 2) mod 3.  With t_j = (j - G/2) / (G/2), j = 1..G-1 (dyadic):
 *     iu = the number of j with (double)n_b >= t_j * (double)n_a;   iv likewise with n_c
 *   (each product is exact in double, so the comparison is exact; no division).  cell = (a G + iu) G + iv.
 *   THE TABLE, made on the host (view.direction_table): for cell (a, iu, iv) the unit vector along e_a + u e_b + v e_c with
 *   u = (2 iu + 1 - G) / G, v likewise, in float64; table[cell][axis] = llrint(component * 2^20).
 *   OFFSET BIN.  d = table[cell] . X, an exact int64;  k = floor(d / w) + D/2, D = A3D_PLANES_BINS = 1024 (floor division of
 *   integers).  bin = cell D + k.  VOTES: H[bin] (int32, 3 G G D entries) counts the admitted rows of the bin.
 *   ROUNDS, at most 2 max_planes.  The REMAINING rows are the admitted rows no earlier round removed.
 *   1. PEAK.  score(bin) = H[bin - 1] + H[bin] + H[bin + 1], the neighbours taken inside the bin's direction cell only (0
 *      beyond k = 0 and k = D-1).  The peak is the bin of the highest score, of equals the lowest bin.  If its score <
 *      max(3, min_voxels / 4) (integer division) the call ENDS.  Votes are smoothed over OFFSET only: the offsets of
 *      neighbouring direction cells are taken along different directions, and smoothing across them lets rows far away leak
 *      into the seeds.
 *   2. SEEDS: the remaining rows of the peak's cell with |k - k_peak| <= 1 (their number is the score).  cnt, sum[3], mom[6] =
 *      the integer sums of 1, X, (XX, XY, XZ, YY, YZ, ZZ) over them.  FIT (below).
 *   3. Twice: the INLIERS of the fit are found, their integer sums taken, and the plane is FITTED again from those.  Then the
 *      FINAL inlier pass with the last fit: its count is the plane's inlier count, its sums go into the record.
 *      FIT: stage B of a3d_estimate_normals on (cnt, sum, mom), no viewpoint: normal fp32 [3] with the canonical sign, or
 *      invalid (cnt < 3, or a line).  N_a = llrint((double)normal_a * 2^20).  off, ONE int64, in integers only: with R_a =
 *      floor(sum_a / cnt) and s_a = sum_a - cnt R_a (stage B's own recentring),
 *          off = (N_0 R_0 + N_1 R_1 + N_2 R_2) + floor((N_0 s_0 + N_1 s_1 + N_2 s_2) / cnt)
 *      -- N . (the mean of the rows), rounded down to a whole unit of 2^-20 quanta.  No double takes part.
 *      INLIER: a remaining row with  |((double)normal_0 v_0 + (double)normal_1 v_1) + (double)normal_2 v_2| >= cos_min  (v the
 *      row's normal; three exact products, one accumulator, axes ascending) and  |N . X - off| <= dist_tol  (exact int64).
 *   4. RECORD.  If the final inlier count >= min_voxels the plane is recorded with the next id: plane_qv = id on its inliers,
 *      their votes are subtracted from H and they leave the remaining rows.
 *   5. SPENT.  Otherwise -- or when any fit of the round was invalid -- the round is spent: the SEEDS leave H and the remaining
 *      rows, no plane is recorded, and the next round goes on (a column or a sphere does not stop the search).
 *   The call ends as well once max_planes planes are recorded.
 *   THE RECORD.  normal (the last fit), N, off, inliers, score (the peak's), bin (the peak's), round (0-based), cnt / sum /
 *   mom of the final inliers, and
 *     offset = (float)((((double)normal_0 origin_0 + (double)normal_1 origin_1) + (double)normal_2 origin_2)
 *                      + (double)off * (quantum * 2^-20))          -- normal . p = offset in scene coordinates (a3d_section's form)
 *     rms    = (float)(sqrt(E / (double)cnt) * (quantum * 2^-20)),  E = (double)hi * 2^64 + (double)lo of the EXACT 128-bit
 *              integer  sum over the final inliers of (N . X - off)^2 = N^T mom N - 2 off (N . sum) + cnt off^2 = hi 2^64 + lo
 *   every double operation rounded on its own, in the order written.
 *   OUTPUTS.  plane_qv_dev int32 [n]: the id, -1 for no plane (every entry is written).  With inverse_map_dev int64 [n_full]:
 *   plane_full_dev int32 [n_full], plane_full[j] = plane_qv[inverse_map[j]]; an index outside 0..n-1 sets A3D_PLANES_BAD_INDEX
 *   and is not followed (the entry is not written).  out_dev (8-byte aligned, cleared by the call): A3D_PLANES_MAX records in
 *   the order found, then the summary: planes, rounds (that passed the stop test) and spent rounds, admitted rows, the rows left
 *   out per reason, the error word.  One copy to the host reads both.
 *   The workspace: a3d_planes_workspace_bytes(n) bytes, 256-byte aligned.  The library allocates nothing and does not
 *   synchronise; stages are launches -- no grid barrier, no spin-wait; a flag on the device turns the launches of the rounds
 *   after the end into no-ops, so nothing is read back inside the call.
 *   A3D_ERR_INVALID with nothing launched and nothing written: no arguments, n < 0 or beyond the bound, bits outside 0..20, a
 *   quantum that is not a positive power of two, an origin that is not finite, bin_width < 1, dist_tol < 0, either beyond 2^44,
 *   cos_min outside [0, 1], min_voxels < 1, max_planes outside 1..16, a missing normal_dev, pos_dev or plane_qv_dev (n > 0),
 *   table_dev or out_dev, out_dev misaligned, n_full < 0 or >= 2^31, plane_full_dev / n_full without inverse_map_dev or
 *   inverse_map_dev without plane_full_dev (n_full > 0), a workspace that is missing, too small or misaligned.
 *   LIMITS: a direction cell is about 7 degrees wide and an offset bin one bin_width deep: a plane whose normal lies on a cell
 *   border splits its votes and is found later, not lost; a plane more than D/2 bins from the origin of the frame along its
 *   normal is left out; no curved primitives. */
#define A3D_PLANES_MAX            16
#define A3D_PLANES_GRID           16
#define A3D_PLANES_BINS           1024
#define A3D_PLANES_SCALE_BITS     20
#define A3D_PLANES_OUT_CANDIDATE  0
#define A3D_PLANES_OUT_NONFINITE  1
#define A3D_PLANES_OUT_ZERO       2
#define A3D_PLANES_OUT_FRAME      3
#define A3D_PLANES_OUT_BINS       4
#define A3D_PLANES_BAD_INDEX      1
typedef struct a3d_plane {
  float   normal[3];                /* the last fit, canonical sign */
  float   offset;                   /* normal . p = offset in scene coordinates */
  int32_t inliers;
  int32_t score;                    /* the peak's */
  int32_t round;
  int32_t bin;                      /* the peak's flat bin index */
  int64_t count;                    /* the final inliers: 1, X, (XX, XY, XZ, YY, YZ, ZZ) */
  int64_t sum[3];
  int64_t mom[6];
  int64_t off;                      /* N . X = off */
  int32_t N[3];
  float   rms;
} a3d_plane;                        /* 136 bytes */
typedef struct a3d_planes_summary {
  int32_t n_planes, rounds, spent, admitted;
  int32_t left_out[5];              /* A3D_PLANES_OUT_* */
  int32_t err;                      /* A3D_PLANES_BAD_INDEX */
  int32_t reserved_[2];
} a3d_planes_summary;               /* 48 bytes */
typedef struct a3d_planes_out {
  a3d_plane plane[A3D_PLANES_MAX];
  a3d_planes_summary summary;
} a3d_planes_out;                   /* 2224 bytes */
typedef struct a3d_find_planes_args {
  const float*   normal_dev;        /* [n][3] */
  const float*   pos_dev;           /* [n][3] */
  const uint8_t* candidate_dev;     /* [n] or NULL */
  int64_t        n;
  const int32_t* table_dev;         /* [3 G G][3] */
  const int64_t* inverse_map_dev;   /* [n_full] or NULL */
  int64_t        n_full;
  int32_t*       plane_qv_dev;      /* out [n] */
  int32_t*       plane_full_dev;    /* out [n_full] or NULL */
  a3d_planes_out* out_dev;
  void*          workspace_dev;
  size_t         workspace_bytes;
  double         origin[3];
  double         quantum;
  double         cos_min;
  int64_t        bin_width;
  int64_t        dist_tol;
  int32_t        bits;
  int32_t        min_voxels;
  int32_t        max_planes;
  int32_t        reserved_;
} a3d_find_planes_args;            /* 168 bytes */
size_t a3d_planes_workspace_bytes(int64_t n);
int    a3d_find_planes(const a3d_find_planes_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * The session's view: id, depth and colour images of the scan for a pinhole camera (csrc/session.hip).
 * THE RULE: the image is, pixel by pixel, what the picks above return for the ray through that pixel's centre -- on a
 * mesh the first face by a3d_pick_mesh's watertight test, on a point cloud the first vertex within the radius by
 * a3d_pick_ray's key.  What the image shows as frontmost is what a click through that pixel hits, bit for bit.
 *
 * a3d_camera: the ray of pixel (u, v) = (column, row) starts at o; its direction is computed in fp32, every operation
 * rounded on its own (no fma contraction), in exactly this order:
 *     x = (d00[0] + (float)u * du[0]) + (float)v * dv[0]      (likewise y, z)
 *     len = sqrtf((x*x + y*y) + z*z);   d = (x / len, y / len, z / len)
 * with correctly rounded divide and sqrt.  d00 = the unnormalised direction of pixel (0, 0)'s centre, du / dv = its change
 * per column / row.  1 <= width, height <= 4096; d00, du, dv finite and linearly independent.
 *
 * Primitives are binned to screen tiles of 16 x 16 pixels by a conservative bound, then every pixel runs
 * the exact test on its tile's list; primitives whose bound cannot be established (the camera inside or within reach of
 * their bounding box, a bound of more than 256 tiles) are tested by every pixel.  Pixel values do not depend on the order
 * of the lists.  The library allocates nothing: workspace_dev holds a3d_render_workspace_bytes(n_primitives, width,
 * height, pair_capacity) bytes (256-byte aligned), pair_capacity = the (tile, primitive) pairs it has room for.  A call
 * that needs more writes NOTHING to the images, sets bit 1 of header flags and reports pairs_needed; call again with a
 * workspace of that capacity.  Calls that share a workspace must be ordered.
 * ------------------------------------------------------------------------------------------ */
#define A3D_RENDER_MAX_SIZE 4096
#define A3D_RENDER_TILE 16
#define A3D_RENDER_BAD_INDEX 1       /* header flags bit 0: a face index outside 0..n-1 was skipped */
#define A3D_RENDER_OVERFLOW  2       /* header flags bit 1: pair_capacity too small, images untouched */
typedef struct a3d_camera {
  float   o[3];
  float   d00[3];
  float   du[3];
  float   dv[3];
  int32_t width, height;
} a3d_camera;
typedef struct a3d_render_header {
  int32_t flags;
  int32_t n_everywhere;        /* primitives that every pixel tested (no bound) */
  int64_t pairs_needed;        /* (tile, primitive) pairs of this call */
} a3d_render_header;
typedef struct a3d_render_out {
  int32_t* id_dev;             /* [h][w] face (mesh) or vertex (points); -1 = nothing */
  float*   t_dev;              /* [h][w] ray parameter of the hit; +inf = nothing */
  float*   u_dev;              /* [h][w] or NULL (mesh only): weight of the face's second vertex, as a3d_pick_mesh computes it */
  float*   v_dev;              /* [h][w] or NULL (mesh only): weight of its third vertex; both 0 where nothing was hit */
  a3d_render_header* header_dev;
} a3d_render_out;
size_t a3d_render_workspace_bytes(int64_t n_primitives, int width, int height, int64_t pair_capacity);

/* Host only, no GPU: what the bound derives from a camera, in double.  out[0..8] = the rows of the inverse of the matrix
 * with columns du, dv, d00 (a world vector p relative to o has screen position (row0.p / row2.p, row1.p / row2.p)),
 * out[9..11] = the rows' Euclidean norms, out[12] = an upper bound on the length of every pixel's unnormalised direction.
 * Returns A3D_ERR_INVALID for a camera the renders refuse. */
int    a3d_render_camera_bounds(const a3d_camera* camera, double* out13);

/* Mesh: per pixel the face a3d_pick_mesh returns for that pixel's ray (smallest t, ties -> the lower face index,
 * double-sided, edges inclusive; degenerate, NaN and out-of-range faces skipped, the last flagged), its t and -- when
 * u_dev / v_dev are given -- the barycentric weights.  m == 0 is valid: an all-background image. */
int    a3d_render_mesh(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m, const a3d_camera* camera,
                       const a3d_render_out* out, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Point cloud: per pixel the vertex a3d_pick_ray returns for that pixel's ray and the radius (t > 0, perpendicular
 * distance^2 <= r^2; smallest t, then smaller distance^2, then lower row) and its t.  n == 0 is valid.  u_dev / v_dev are
 * ignored. */
int    a3d_render_points(const float* xyz_dev, int64_t n, float radius, const a3d_camera* camera, const a3d_render_out* out,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* rgb_dev uint8 [h][w][3] from an id image and per-vertex colours colors_dev fp32 [n][3].  faces_dev NULL: ids are
 * vertices, the pixel takes the vertex's colour.  Else ids are faces and c = ((1 - u - v) c0 + u c1) + v c2 per channel in
 * fp32 without contraction, 1 - u - v = (1 - u) - v.  id -1: background (HOST array of 3).  Quantisation:
 * (uint8)(min(max(c, 0), 1) * 255 + 0.5f).  An id or a face's index outside its table gives the background. */
int    a3d_render_shade(const int32_t* id_dev, const float* u_dev, const float* v_dev, const int32_t* faces_dev, int64_t m,
                        const float* colors_dev, int64_t n, const float* background, uint8_t* rgb_dev, int width, int height,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * Looking INTO a scan: section planes and back-face culling, for the picks and the view together (csrc/session.hip).
 * The counterpart of what the GUI's user gets from the near plane of Open3D's camera when zooming through a wall; THE RULE
 * IS THIS LIBRARY'S, and the rule of the view stays true under it: the image is, pixel by pixel, what a click through that
 * pixel picks under the same section, bit for bit.  All arithmetic below is fp32, every operation rounded on its own (no
 * fma contraction), in the order written, divisions correctly rounded: a numpy float32 restatement gives the same bits.
 *
 * a3d_section: n_planes planes (nx, ny, nz, c), each keeping the side n . p >= c, and a culling mode.  Refused with
 * A3D_ERR_INVALID before anything else of a call is looked at (no GPU is needed to be refused): n_planes outside 0..8; cull
 * outside 0..2, or not 0 in a point-cloud call; a used plane with a value that is not finite or with nx*nx + ny*ny + nz*nz
 * outside [0.5, 2] (normals are meant to be unit vectors; the bound keeps den and the quotients below finite).
 *
 * MESH: a section cuts the RAY, not the faces.  Once per ray (o, d):
 *     t_lo = 0, t_hi = +inf, empty = false
 *     for k = 0 .. n_planes - 1:
 *         den = (nx*dx + ny*dy) + nz*dz;   so = (nx*ox + ny*oy) + nz*oz
 *         den > 0:  t_lo = fmaxf(t_lo, (c - so) / den)
 *         den < 0:  t_hi = fminf(t_hi, (c - so) / den)
 *         else   :  if !(so >= c) empty = true           (the ray runs inside a plane's direction: all of it or nothing)
 * where fmaxf(a, q) stands for q > a ? q : a and fminf(a, q) for q < a ? q : a: a NaN q leaves the bound alone, and of two
 * zeros the bound's own stays, so that the bits of t_lo and t_hi are defined down to the sign of a zero.
 * A crossing that a3d_pick_mesh's test accepts counts iff !empty && t >= t_lo && t <= t_hi, both ends inclusive; all else
 * is a3d_pick_mesh's: the smallest t, then the lower face index; u, v and the hit point of the face found.  The interval is
 * ONE pair per ray, so two faces that share an edge still classify every ray consistently: a section opens no crack.
 *
 * CULLING (meshes).  A face (a, b, c) is FRONT for a ray when its vertices appear counter-clockwise seen from the ray's
 * origin: g . d < 0 for g = (b - a) x (c - a), the vector a3d_vertex_normals sums.  The crossing test's shear keeps the
 * winding, so the facing is read off its det = (U + V) + W alone: det > 0 is FRONT, det < 0 is BACK (det == 0 is no hit
 * anyway).  A3D_CULL_BACK drops the back faces, A3D_CULL_FRONT the front faces.  Scanned surfaces face the scanner: seen
 * from outside a room, its near walls are back faces.
 *
 * POINT CLOUD: a vertex (x, y, z) shows iff (nx*x + ny*y) + nz*z >= c for every plane (a NaN fails); a3d_pick_ray's test
 * runs on the vertices that show.  This does not depend on the ray.
 *
 * The view's binning is not touched: the rule lives in the exact per-pixel test, and a list that was conservative stays so
 * when fewer primitives pass.  Workspaces are those of the calls without a section.
 * ------------------------------------------------------------------------------------------ */
#define A3D_SECTION_MAX_PLANES 8
#define A3D_CULL_NONE 0
#define A3D_CULL_BACK 1
#define A3D_CULL_FRONT 2
typedef struct a3d_section {
  int32_t n_planes;            /* 0 .. A3D_SECTION_MAX_PLANES */
  int32_t cull;                /* A3D_CULL_*; meshes only */
  float   planes[A3D_SECTION_MAX_PLANES][4];   /* (nx, ny, nz, c): the KEPT side is n . p >= c */
} a3d_section;                 /* 136 bytes */

/* The four calls above under a section; everything else is theirs.  section NULL = none.  With NULL, or with no plane and
 * A3D_CULL_NONE, a call runs the code of its counterpart without a section and writes the same bytes. */
int    a3d_pick_ray_section(const float* xyz_dev, int64_t n, const float* origin, const float* direction, float radius,
                            const a3d_section* section, a3d_pick_result* result_dev, void* workspace_dev,
                            size_t workspace_bytes, void* stream);
int    a3d_pick_mesh_section(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m, const float* origin,
                             const float* direction, const a3d_section* section, a3d_pick_mesh_result* result_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);
int    a3d_render_mesh_section(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m, const a3d_camera* camera,
                               const a3d_section* section, const a3d_render_out* out, void* workspace_dev,
                               size_t workspace_bytes, void* stream);
int    a3d_render_points_section(const float* xyz_dev, int64_t n, float radius, const a3d_camera* camera,
                                 const a3d_section* section, const a3d_render_out* out, void* workspace_dev,
                                 size_t workspace_bytes, void* stream);

/* Host only, no GPU: the interval of the ray (origin, direction; HOST arrays of 3) under the section's planes, by the
 * function the kernels call: out3 = t_lo, t_hi, empty as 0 or 1.  The direction is taken as it is.  section NULL: 0, +inf, 0.
 * A3D_ERR_INVALID for a section the calls refuse or a NULL array. */
int    a3d_section_ray(const a3d_section* section, const float* origin, const float* direction, float* out3);

/* ------------------------------------------------------------------------------------------
 * Lighting the view (csrc/session.hip): per-vertex normals, a lit colour pass for meshes, a depth-based one for point
 * clouds.  The counterpart of the GUI's compute_vertex_normals and its "defaultLit" material (gui.py:556-557, 135).
 * Open3D's lit material (a sun plus image-based light) is not reproduced: THE RULES BELOW ARE THIS LIBRARY'S, as the pick
 * rules are.  All arithmetic is fp32, every operation rounded on its own (no fma contraction), in exactly the order
 * written, divide and sqrtf correctly rounded: a numpy float32 restatement gives the same bits.
 *
 * VERTEX NORMALS.  Every vertex has the list of its incident corners (face, corner), ascending by face, then by corner, in
 * CSR form: offsets_dev int64 [n + 1], corners_dev int32 [3 m] holding 3 * face + corner (a vertex listed twice in a face
 * appears twice).  For a face f = (a, b, c): e1 = P[b] - P[a], e2 = P[c] - P[a],
 *     g = (e1y*e2z - e1z*e2y,  e1z*e2x - e1x*e2z,  e1x*e2y - e1y*e2x)          (area weighted, not normalised)
 * A face contributes only if its three indices lie in 0..n-1 and all three components of g are finite.  Per component
 *     s = (((0 + g_1) + g_2) + ...) in list order;    l2 = (sx*sx + sy*sy) + sz*sz
 *     N = s / sqrtf(l2) per component if l2 > 0 and finite, else N = (0, 0, 0)
 * (an isolated vertex, degenerate faces only, NaN).  One thread per vertex walks its own list: no atomics, two calls give
 * the same bytes.  List entries outside 0..3m-1 and ranges outside the list are skipped.  normals_out_dev fp32 [n][3].
 * No workspace.  3 m must fit int32.  The lists are the caller's to build (a stable sort of the 3 m vertex indices).
 * ------------------------------------------------------------------------------------------ */
int    a3d_vertex_normals(const float* xyz_dev, int64_t n, const int32_t* faces_dev, int64_t m, const int64_t* offsets_dev,
                          const int32_t* corners_dev, float* normals_out_dev, void* stream);

/* Lit colour image of a MESH render: the inputs of a3d_render_shade (width and height are the camera's), the vertex
 * normals normals_dev fp32 [n][3], the camera that rendered the ids and ambient in [0, 1].  Per pixel: the base colour c
 * exactly as a3d_render_shade computes it; a pixel with id -1, or an id or a face's index outside its table, gets the
 * background, unshaded.  Else, with the face's vertices 0, 1, 2 and w = (1 - u) - v,
 *     Nn = (w*N0 + u*N1) + v*N2 per component;     l2 = (Nx*Nx + Ny*Ny) + Nz*Nz
 *     d  = the pixel's unit ray direction by the a3d_camera rule above
 *     k0 = fminf(fabsf((Nx*dx + Ny*dy) + Nz*dz) / sqrtf(l2), 1) if l2 > 0 and finite, else k0 = 1
 *     k  = ambient + (1 - ambient) * k0;           each channel c * k, then a3d_render_shade's quantisation
 * -- a double-sided light at the camera.  ambient == 1 gives k == 1 exactly: the image of a3d_render_shade, byte for byte.
 * u_dev and v_dev are needed; faces_dev may be NULL only when m == 0 (every pixel the background). */
int    a3d_render_shade_lit(const int32_t* id_dev, const float* u_dev, const float* v_dev, const int32_t* faces_dev, int64_t m,
                            const float* colors_dev, int64_t n, const float* normals_dev, const a3d_camera* camera,
                            float ambient, const float* background, uint8_t* rgb_dev, void* stream);

/* Lit colour image of a POINT CLOUD render whose vertices have been given normals (a3d_estimate_normals' normal_full): the
 * inputs of a3d_render_shade for a cloud (ids are vertices; width and height are the camera's), normals_dev fp32 [n][3], the
 * camera that rendered the ids and ambient in [0, 1].  Per pixel with 0 <= id < n (else the background, unshaded): the base
 * colour c = the vertex's; N = normals[id] as stored;
 *     l2 = (Nx*Nx + Ny*Ny) + Nz*Nz;     d = the pixel's unit ray direction by the a3d_camera rule
 *     k0 = fminf(fabsf((Nx*dx + Ny*dy) + Nz*dz) / sqrtf(l2), 1) if l2 > 0 and finite, else k0 = 1
 *     k  = ambient + (1 - ambient) * k0;           each channel c * k, then a3d_render_shade's quantisation
 * -- a3d_render_shade_lit's rule with the pixel's vertex in place of the interpolated corner normals.  A vertex without a
 * valid normal (zero, NaN) keeps its colour.  ambient == 1 gives a3d_render_shade's image byte for byte. */
int    a3d_render_shade_lit_points(const int32_t* id_dev, const float* colors_dev, int64_t n, const float* normals_dev,
                                   const a3d_camera* camera, float ambient, const float* background, uint8_t* rgb_dev,
                                   void* stream);

/* CULLING A CLOUD without touching a render or pick kernel (csrc/session_normals.hip): xyz_out_dev fp32 [n][3] = a copy of
 * xyz_dev in which every culled vertex has all three coordinates NaN (bits 0x7fc00000).  eye: a HOST array of 3, finite;
 * mode A3D_CULL_BACK or A3D_CULL_FRONT.  Per vertex, in fp32, every operation rounded on its own:
 *     g = (Nx*(x - ex) + Ny*(y - ey)) + Nz*(z - ez)
 * The vertex is BACK when g > 0 (its normal points away from the eye) and FRONT when g < 0; A3D_CULL_BACK hides the BACK
 * vertices, A3D_CULL_FRONT the FRONT ones.  A zero or NaN normal, a NaN coordinate, or g == 0 is neither: the vertex is
 * copied as it is.  Optionally hidden_dev uint8 [n] (1 = hidden, every byte written) and count_dev int64 [1] (8-byte
 * aligned, cleared by the call: the hidden vertices, one atomic per workgroup).  xyz_out_dev may be xyz_dev itself.
 * WHY THIS IS ENOUGH: a vertex with NaN coordinates fails a3d_pick_ray's test, is binned nowhere by the view (its exact
 * test never passes) and is in view nowhere for a3d_select_vertices, so picks, renders and selections of the copy see
 * exactly the vertices that show, the ids stay vertex ids, and "the image is what a click through that pixel picks" keeps
 * holding as long as pick and view use the copy of the same eye.  (A selection of the copy reports A3D_SELECT_NOT_FINITE.)
 * A3D_ERR_INVALID with nothing launched: n < 0 or n >= 2^31, a mode that is neither, eye NULL or not finite, n > 0 with
 * xyz_dev, normals_dev or xyz_out_dev NULL, a misaligned count_dev.  No workspace. */
int    a3d_cull_points(const float* xyz_dev, const float* normals_dev, int64_t n, const float* eye, int mode,
                       float* xyz_out_dev, uint8_t* hidden_dev, int64_t* count_dev, void* stream);

/* Depth-shaded colour image, for POINT CLOUDS (which have no normals): the inputs of a3d_render_shade, the render's t image
 * t_dev fp32 [h][w] and strength >= 0 (finite).  For a pixel p whose base colour c is not the background:
 *     r(q) = fmaxf(t_p - t_q, 0) / t_p for a neighbour q inside the image whose id >= 0, else 0
 *     s = (((0 + r(left)) + r(right)) + r(up)) + r(down);     k = 1 / (1 + strength * s);     each channel c * k
 * -- a pixel darkens by how far it lies behind its neighbours.  strength == 0 gives a3d_render_shade's image byte for byte.
 * faces_dev NULL: ids are vertices; else a mesh's images (u_dev, v_dev needed), shaded the same way. */
int    a3d_render_shade_depth(const int32_t* id_dev, const float* t_dev, const float* u_dev, const float* v_dev,
                              const int32_t* faces_dev, int64_t m, const float* colors_dev, int64_t n, float strength,
                              const float* background, uint8_t* rgb_dev, int width, int height, void* stream);

/* ------------------------------------------------------------------------------------------
 * The annotation in the view (csrc/session.hip): which object a pixel belongs to, borders between objects, and the clicks
 * themselves.  The reference's user reads all three off Open3D's window by eye; a headless session answers them in data.
 * THE RULES ARE THIS LIBRARY'S.  Both calls are per-pixel passes without atomics or workspace: two calls give the same
 * bytes.  All arithmetic is fp32, every operation rounded on its own (no fma contraction), in the order written.
 *
 * THE LABEL IMAGE: label_out_dev int32 [h][w] from a render's id / u / v images and per-vertex labels labels_dev int32 [n].
 *   faces_dev NULL (a cloud): label = labels[id] if 0 <= id < n, else -1.
 *   A mesh: -1 unless 0 <= id < m and the face's three indices lie in 0..n-1 (a3d_render_shade's tests for the background).
 *   Else, with w = (1 - u) - v, the label of the face's HEAVIEST corner:
 *       corner 0 if w >= u && w >= v;   else corner 1 if u >= v;   else corner 2
 *   A tie goes to the lower corner (u == w: corner 0; u == v above w: corner 1).  A NaN in u or in v makes w NaN as well,
 *   so both tests fail: NaN weights end at corner 2.
 *   This partitions a face among its three vertices by straight borders that meet at the centroid.  It is NOT the vertex a
 *   click on the pixel snaps to: that is the scene's nearest vertex by Euclidean distance (a3d_nearest_rows), which on a
 *   sliver can be another corner or a vertex of another face.
 *   -1 means "shows nothing"; label values are passed through unchecked (0 = background by the session's convention).
 * ------------------------------------------------------------------------------------------ */
int    a3d_render_labels(const int32_t* id_dev, const float* u_dev, const float* v_dev, const int32_t* faces_dev, int64_t m,
                         const int32_t* labels_dev, int64_t n, int32_t* label_out_dev, int width, int height, void* stream);

/* Outlines and click markers composed over a colour image: rgb_out_dev uint8 [h][w][3] from rgb_in_dev (the same layout),
 * the label image label_dev, the render's t image t_dev (+inf = nothing) and the marker table markers_dev fp32
 * [n_markers][6] = (x, y, t, r, g, b): a position in pixels (the centre of pixel (u, v) is the position (u, v)), the ray
 * parameter of the marked point as the t image holds it, a colour.  0 <= n_markers <= A3D_MAX_CLICKS, radius >=
 * inner_radius >= 0 in pixels and depth_slack >= 0 in world units, all finite; else A3D_ERR_INVALID.  outline: a HOST
 * array of 3, or NULL for no outlines (label_dev may then be NULL); border: a HOST array of 3.
 * Per pixel p = (px, py), in this order:
 *   1. the bytes of rgb_in, unchanged;
 *   2. if outline is given and L_p >= 1 and some 4-neighbour INSIDE the image has a label != L_p (one that shows -1 or the
 *      background 0 counts as different): the outline colour.  So the background and "nothing" are never outlined, an
 *      object that ends at the image's edge gets no outline there, and between two objects both sides are drawn.
 *   3. for k = 0 .. n_markers-1 in table order:  dx = (float)px - x_k, dy = (float)py - y_k, d2 = dx*dx + dy*dy; the marker
 *      covers the pixel if d2 <= radius*radius and t_k - t_p <= depth_slack (a pixel that shows nothing has t_p = +inf:
 *      the test passes); the pixel then takes the marker's colour if d2 <= inner_radius*inner_radius, else border.  The
 *      LAST covering marker wins, as the last cube wins in a3d_session_paint.  A marker with a NaN in any of its six
 *      fields covers nothing.
 * Colours are quantised by a3d_render_shade's rule.  Markers arrive already projected: the kernel holds comparisons and
 * two products, no matrix inverse.  Every pixel walks the whole table (staged in LDS); there is no culling by tile.
 * rgb_out_dev == rgb_in_dev is allowed -- a pixel reads only its own colour and writes only its own, its neighbours are read
 * from the label image; buffers that overlap in part are refused. */
int    a3d_render_annotate(const uint8_t* rgb_in_dev, const int32_t* label_dev, const float* t_dev, const float* markers_dev,
                           int n_markers, float radius, float inner_radius, float depth_slack, const float* outline,
                           const float* border, uint8_t* rgb_out_dev, int width, int height, void* stream);

/* ------------------------------------------------------------------------------------------
 * Correcting a labelling by hand (csrc/session_region.hip): a region of the screen as a mask image, the vertices a camera
 * sees inside it, and a manual label layer laid over the model's labels.  The reference's tool has no counterpart (Open3D
 * gives it no lasso): THE RULES ARE THIS LIBRARY'S.  All arithmetic is fp32, every operation rounded on its own (no fma
 * contraction), in the order written, divide and sqrtf correctly rounded: a numpy float32 restatement gives the same bits.
 * Positions are in pixels as everywhere above: the centre of pixel (u, v) is the position (u, v).
 *
 * THE REGION MASK: mask_dev uint8 [h][w], in/out, from a shape given by k points (x, y) -- points: a HOST array fp32 [k][2],
 * they travel by value in the kernel arguments -- and a mode.  1 <= width, height <= 4096.  Per pixel p = ((float)u, (float)v):
 *   A3D_REGION_POLYGON, 3 <= k <= A3D_REGION_MAX_POINTS, even-odd: covered = the parity of the edges a = P[j],
 *     b = P[(j + 1) % k] with
 *         (a.y > p.y) != (b.y > p.y)   and   p.x < ((b.x - a.x) * (p.y - a.y)) / (b.y - a.y) + a.x
 *     (the quotient is looked at only where the first test holds: there b.y != a.y).  Vertices may lie outside the image;
 *     a polygon that crosses itself is valid, the parity is what it is.  An edge through a pixel's centre: the pixel is
 *     inside when the polygon lies to its right, outside when it lies to its left (`<`); a pixel's centre on a horizontal
 *     edge is inside when the polygon lies at larger y, outside when it lies at smaller y (`>`).  radius is not looked at.
 *   A3D_REGION_STROKE, 1 <= k <= A3D_REGION_MAX_POINTS, radius r > 0 finite: covered iff for some segment j = 0 .. k-2
 *     (k == 1: the one segment a = b = P[0], a disc), a = P[j], b = P[j + 1]:
 *         e = b - a;  w = p - a;  L = e.x*e.x + e.y*e.y
 *         h = 0 if !(L > 0), else q = (w.x*e.x + w.y*e.y) / L,  h = q < 0 ? 0 : (q > 1 ? 1 : q)
 *         dx = w.x - h*e.x;  dy = w.y - h*e.y;  dx*dx + dy*dy <= r*r
 *     (a repeated point is a disc as well; a NaN q, possible only from overflow, passes both comparisons and stays).
 *   mode: A3D_REGION_REPLACE mask = covered; A3D_REGION_ADD mask |= covered; A3D_REGION_SUBTRACT mask &= !covered.  A byte
 *   that is read counts as 1 when it is not 0; the bytes written are 0 or 1; every byte is written.
 * A3D_ERR_INVALID with nothing launched (no GPU is needed to be refused): a point that is not finite, k outside its
 * range, a shape or mode that is none of the above, a size outside 1..4096, a stroke's radius not finite or <= 0, points
 * or mask_dev NULL.  No workspace, no atomic: two calls give the same bytes.
 * ------------------------------------------------------------------------------------------ */
#define A3D_REGION_MAX_POINTS 256
#define A3D_REGION_POLYGON  0
#define A3D_REGION_STROKE   1
#define A3D_REGION_REPLACE  0
#define A3D_REGION_ADD      1
#define A3D_REGION_SUBTRACT 2
int    a3d_region_mask(int width, int height, int shape, const float* points, int n_points, float radius, int mode,
                       uint8_t* mask_dev, void* stream);

/* WHICH VERTICES THE CAMERA SEES INSIDE THE MASK: one streaming pass over the n rows of xyz_dev, selected_dev uint8 [n] = 0
 * or 1, every byte written.  rows = the inverse of the matrix with columns du, dv, d00 as a3d_render_camera_bounds computes
 * it in double (its out[0..8]), each value rounded to fp32 ONCE by the caller: the kernel holds no matrix inverse.  Per
 * vertex p = (px, py, pz), in this order (R0, R1, R2 = rows[0..2], rows[3..5], rows[6..8]; o = the camera's):
 *   1. w = p - o per component;  a = (R0x*wx + R0y*wy) + R0z*wz, likewise b (R1) and c (R2).  In front iff c > 0.
 *      x = a / c, y = b / c.
 *   2. xr = floorf(x + 0.5f), yr = floorf(y + 0.5f).  In the image iff xr >= 0 && xr < (float)width && yr >= 0 &&
 *      yr < (float)height (a NaN fails); only then u = (int)xr, v = (int)yr -- no float outside the image is converted.
 *      A position exactly on x = -0.5 rounds to pixel 0, one exactly on x = width - 0.5 to pixel width: outside.
 *   3. The vertex shows iff (nx*px + ny*py) + nz*pz >= c_k for every plane of the section: the point-cloud rule of
 *      a3d_section, applied to the vertices of clouds and meshes alike; cull is not looked at (it is checked for its range).
 *   4. in_view = 1, 2 and 3 all pass.
 *   5. mask[v][u] != 0.
 *   6. Only when t_dev is given (the VISIBLE mode): d = the unit ray of pixel (u, v) by the a3d_camera rule,
 *      tt = (wx*dx + wy*dy) + wz*dz -- the t of a3d_pick_ray, the same formula in the same order -- and the vertex passes
 *      iff tt - t[v][u] <= slack.  t = +inf (the pixel shows nothing) passes; a NaN fails.  With t_dev NULL (the THROUGH
 *      mode) everything under the mask is selected, whatever lies in front of it.
 *   7. selected[i] = 4, 5 and 6 all pass.
 * On the image of a3d_render_points of the same rows under the same camera and section, with slack 0 and a mask of ones, every
 * vertex the id image shows at the pixel it projects to is selected: its tt is bit for bit the t the image holds there.
 * summary_dev (cleared by the call): the number of selected vertices, of vertices in view, and flags: bit 0
 * (A3D_SELECT_NOT_FINITE) = some vertex has a coordinate that is not finite (it is in view nowhere).  Integer sums, reduced
 * per workgroup, one atomic per workgroup and counter: identical from run to run.
 * A3D_ERR_INVALID with nothing launched: a camera the renders refuse; a section the section calls refuse; slack negative
 * or not finite; a rows value that is not finite; n < 0 or n >= 2^31; mask_dev or summary_dev NULL; n > 0 with xyz_dev or
 * selected_dev NULL.  n == 0 is valid.  No workspace. */
#define A3D_SELECT_NOT_FINITE 1
typedef struct a3d_select_summary {
  int64_t selected;
  int64_t in_view;
  int32_t flags;
  int32_t reserved_;
} a3d_select_summary;              /* 24 bytes */
typedef struct a3d_select_args {
  const float*   xyz_dev;           /* [n][3] */
  int64_t        n;
  a3d_camera     camera;
  float          rows[9];           /* rows of [du dv d00]^-1, fp32 */
  float          slack;             /* >= 0, world units; used only with t_dev */
  const uint8_t* mask_dev;          /* [h][w] */
  const float*   t_dev;             /* [h][w] a render's t image, or NULL: select through everything */
  const a3d_section* section;       /* HOST, or NULL: none */
  uint8_t*       selected_dev;      /* out [n] */
  a3d_select_summary* summary_dev;
} a3d_select_args;
int    a3d_select_vertices(const a3d_select_args* args, void* stream);

/* THE MANUAL LAYER over the model's labels: two full-resolution arrays, manual_on_dev uint8 [n] (not 0 = this vertex is
 * overridden) and manual_obj_dev int32 [n] (the object it is given, 0..255) -- two arrays and no -1 sentinel, so that the
 * REMAP half of a3d_session_edit renumbers manual_obj_dev as it renumbers any labels.  Per vertex i, in this order:
 *   1. if op != A3D_OVERLAY_NONE and selected_dev is given and selected[i] != 0:
 *        A3D_OVERLAY_PAINT: on = 1, manual_obj[i] = obj;      A3D_OVERLAY_ERASE: on = 0 (manual_obj[i] stays)
 *      The two arrays are written only where this alters them.
 *   2. L = on ? manual_obj[i] : labels_in[i]
 *   3. labels_out[i] = L
 *   4. colors_out[i] = the palette entry of L > 0 with the wrap of a3d_session_paint (L >= n_palette: entry
 *      1 + (L - 1) % (n_palette - 1)), the vertex's own colour colors_full[i] for L == 0.  No click cubes.
 * An L outside 0..255 sets bit 0 of the summary's err and leaves labels_out[i] and colors_out[i] unwritten.
 * summary_dev (cleared by the call), int64 sums: changed = vertices whose layer entry step 1 altered (on flipped, or
 * manual_obj replaced by another value while on); overridden = on after the call; differing = on && manual_obj[i] !=
 * labels_in[i] after the call, compared as plain int32.  Integer sums, one atomic per workgroup and counter.
 * labels_out_dev and colors_out_dev may be NULL TOGETHER: a pure layer update, steps 3 and 4 skipped (colors_full_dev and
 * palette_dev are then not looked at).  A3D_ERR_INVALID with nothing launched: n < 0 or n >= 2^31; an op that is none of
 * the three; obj outside 0..255; summary_dev NULL; n > 0 with labels_in_dev, manual_on_dev or manual_obj_dev NULL; one
 * output without the other; with outputs: colors_full_dev or palette_dev NULL, n_palette outside 2..256. */
#define A3D_OVERLAY_NONE  0
#define A3D_OVERLAY_PAINT 1
#define A3D_OVERLAY_ERASE 2
typedef struct a3d_overlay_summary {
  int64_t changed;
  int64_t overridden;
  int64_t differing;
  int32_t err;                      /* bit 0 = a label outside 0..255 where it was used */
  int32_t reserved_;
} a3d_overlay_summary;             /* 32 bytes */
typedef struct a3d_session_overlay_args {
  const int32_t* labels_in_dev;     /* [n] the model's labels, lifted to the vertices */
  int64_t        n;
  uint8_t*       manual_on_dev;     /* in/out [n] */
  int32_t*       manual_obj_dev;    /* in/out [n] */
  const uint8_t* selected_dev;      /* [n] or NULL */
  const float*   colors_full_dev;   /* [n][3] */
  const float*   palette_dev;       /* [n_palette][3] */
  int32_t*       labels_out_dev;    /* out [n], or NULL together with colors_out_dev */
  float*         colors_out_dev;    /* out [n][3] */
  a3d_overlay_summary* summary_dev;
  int32_t        op;                /* A3D_OVERLAY_* */
  int32_t        obj;               /* 0..255; used by A3D_OVERLAY_PAINT */
  int32_t        n_palette;
  int32_t        reserved_;
} a3d_session_overlay_args;
int    a3d_session_overlay(const a3d_session_overlay_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mask losses (first piece of SURVEY.md section 8 row f-2).
 * Replaces: SetCriterion.loss_bce / loss_dice (models/criterion.py:14-110) for ONE sample and ONE
 * prediction level: losses_dev[0] = mean_i w_i * CE(logits_i, target_i), losses_dev[1] = mean_i w_i *
 * dice_i (per-point soft IoU of softmax(logits_i) against the one-hot target, eps = 1e-6; NaN in both if
 * a target is outside 0..n_classes-1).  grad_logits_dev (optional, [n][n_classes]) receives
 * d(coef_bce * losses[0] + coef_dice * losses[1]) / d logits.  weights_dev NULL = all ones;
 * workspace: 64 bytes.
 * ------------------------------------------------------------------------------------------ */
int    a3d_mask_losses(const float* logits_dev, const int32_t* target_dev, const float* weights_dev,
                       int64_t n, int n_classes, float coef_bce, float coef_dice,
                       float* losses_dev, float* grad_logits_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * On-device voxelisation.
 * Replaces: ME.utils.sparse_quantize(coordinates, quantization_size, return_index=True,
 * return_inverse=True) (datasets/InterMultiObj3DSegDataset.py:67-75): q = int32(floor(xyz / size)) in
 * the input's own dtype (is_f64: 0 = float32 [n][3], 1 = float64), voxels in first-occurrence order,
 * unique_map[v] = first point of voxel v, inverse_map[i] = voxel of point i.  Output arrays must hold
 * n_points entries; *n_voxels (HOST) receives the voxel count (one stream synchronisation).
 * ------------------------------------------------------------------------------------------ */
size_t a3d_quantize_workspace_bytes(int64_t n_points);
int    a3d_sparse_quantize(const void* xyz_dev, int is_f64, int64_t n_points, double quantization_size,
                           int32_t* coords_out_dev, int64_t* unique_map_dev, int64_t* inverse_map_dev,
                           int64_t* n_voxels, void* workspace_dev, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AGILE3D_HIP_H */
