/*
 * i2v_hip.h -- C ABI of libi2v_hip.so: hand-written HIP (gfx950 / MI355X) kernels for the
 * I2V-Adapter denoising path.
 *
 * The reference (xUhEngwAng/I2V-Adapter-Unofficial) has no FFI: the path sits behind a Python module
 * API and its arithmetic is executed by torch/aten kernels reached through `diffusers`.
 * Each entry point below replaces the aten kernel family named in its comment, at the reference call
 * site cited (file:line relative to /root/reference; i2v = src/modules/i2v_adapter.py,
 * unet = src/models/unet_motion_cross_frame_attn.py, pipe = src/pipelines/pipeline_i2v_adapter.py).
 *
 * Conventions
 *   - plain C: raw device pointers + explicit sizes/strides; no torch types.
 *   - activations are fp16, TOKEN-MAJOR CHANNELS-LAST: x[image][pixel][channel]; strides are in ELEMENTS.
 *   - every function is asynchronous on the caller's `stream` (a hipStream_t), never allocates, never
 *     synchronises, never touches the null stream => safe inside hipGraph capture.
 *   - return value: 0 ok, <0 error (I2V_ERR_*); i2v_last_error() returns a thread-local message.
 *   - the caller owns every buffer (including workspaces, whose sizes the *_workspace_bytes helpers give).
 */
#ifndef I2V_HIP_H
#define I2V_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define I2V_ABI_VERSION 35

#define I2V_OK 0
#define I2V_ERR_INVALID_ARG (-1)
#define I2V_ERR_UNSUPPORTED (-2)
#define I2V_ERR_LAUNCH (-3)

typedef void* i2v_stream_t; /* hipStream_t */

int i2v_abi_version(void);
const char* i2v_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * GEMM / implicit-GEMM convolution with fused epilogue (MFMA, fp16 in, fp32 accumulate, fp16 out)
 *
 *   C[m, n] = epi( sum_k A[m, k] * W[n, k]  + bias[n] + rowvec[m / rows_per_vec, n] + residual[m', n] )
 *             * out_scale
 *
 * replaces aten addmm / conv2d(+bias) at: attention projections to_q/to_k/to_v/to_out (diffusers
 * `Attention`, constructed i2v:32-37,409-418), GEGLU feed-forward (i2v:554), 1x1 proj_in/proj_out
 * (i2v:219-226,299-305), ResnetBlock2D conv1/conv2/conv_shortcut/time_emb_proj (unet:203-214,384-395,
 * 563-574,594-605), Downsample2D/Upsample2D convs (unet:250-259,431-432), conv_in/conv_out
 * (unet:757-759,879-881), motion-module proj_in/proj_out/q/k/v/out/ff (unet:232-244), time embedding MLP
 * (unet:766-770), ImageProjection (unet:1284-1287).
 * ------------------------------------------------------------------------------------------------ */
enum {
  I2V_EPI_NONE = 0,
  I2V_EPI_GELU = 1,  /* erf GELU on the result                                                     */
  I2V_EPI_GEGLU = 2  /* W rows interleaved (value_i, gate_i): C[m, n/2] = v * gelu_erf(g); N even   */
};

enum {
  I2V_STORE_ROWMAJOR = 0, /* C[m * ldc + n]                                                         */
  I2V_STORE_ROWPERM = 1,  /* rows arrive in (b, pixel, frame) order and are stored (and the residual
                             is read) in (b, frame, pixel) order: m = (b*hw + p)*frames + f ->
                             m' = (b*frames + f)*hw + p            (motion-module exit)   */
  I2V_STORE_VT = 2,       /* transposed, batched: element (m, n) -> C[((n / vt_len) * M + m) * vt_ld
                             + n % vt_len]; used with A = weight [C, K], W = tokens [T, K] to emit
                             V^T[batch][channel][key] for the attention kernels                     */
  I2V_STORE_VT_T = 3      /* the same V^T[batch][channel][key] output from the NATURAL operand order
                             (A = tokens [T, K], W = weight [C, K]): element (m, n) -> C[((m / vt_len) * N + n)
                             * vt_ld + m % vt_len]; lets large V projections run on the 256-row tile kernel  */
};

enum {
  I2V_A_PLAIN = 0,  /* A is [M, K] row-major (optionally two sources concatenated along K)          */
  I2V_A_CONV3X3 = 1 /* A is gathered on the fly from an NHWC image: K = 9 * cin, k = tap * cin + ci */
};

typedef struct i2v_gemm_params {
  const void* a;        /* fp16 */
  int64_t lda;
  const void* a2;       /* optional second K-range source (skip-connection concat, unet:478); NULL if unused */
  int64_t lda2;
  int32_t k_split;      /* columns [0, k_split) come from a, [k_split, K) from a2; multiple of 8     */
  int32_t a_mode;       /* I2V_A_*                                                                  */
  const void* w;        /* fp16 [N, K] row-major (torch Linear / repacked conv weight)               */
  int64_t ldw;
  const void* bias;     /* fp16 [N] or NULL                                                          */
  const void* residual; /* fp16 [M, N] (ld = ldr) or NULL                                            */
  int64_t ldr;
  const void* rowvec;   /* fp16 [M / rows_per_vec, N] (ld = ld_rowvec) or NULL: time-embedding add   */
  int64_t ld_rowvec;
  int32_t rows_per_vec;
  int32_t rowvec_period; /* > 0 (a power of two): the vector of row m is rowvec[m % rowvec_period] (positional-embedding
                            table of the motion modules: tokens are in (b, pixel, frame) order, period = frames);
                            with I2V_STORE_VT_T the table is passed TRANSPOSED, [N, ld_rowvec >= period]          */
  /* LayerNorm folded into the GEMM (i2v:444-445, 510, 539 and the motion modules' norm1/2/3).  With W' = W o gamma
     (the w passed here), ln_wsum fp32 [N] = sum_k W'[n][k] (summed from the fp16-ROUNDED W') and bias = W beta + b:
        C[m][n] = rstd_m (sum_k A[m][k] W'[n][k] - mean_m ln_wsum[n]) + bias[n]   = (LayerNorm(A) W^T + b)[m][n]
     where mean_m / rstd_m = 1 / sqrt(var_m + ln_eps) are the statistics of row m of A over its K columns, computed
     INSIDE the kernel from the A tiles its K loop streams anyway: the normalised activations are never written to /
     read back from HBM and there is no statistics pass.  NULL = plain GEMM.  Only the 8-wave LDS-DMA kernel
     implements it (single-source A, no residual): i2v_gemm_ln_supported() tells whether a problem qualifies. */
  const void* ln_wsum;
  float ln_eps;
  void* c;              /* fp16                                                                      */
  int64_t ldc;
  int32_t M, N, K;
  int32_t epilogue;     /* I2V_EPI_*                                                                 */
  int32_t store_mode;   /* I2V_STORE_*                                                               */
  int32_t frames, hw;   /* I2V_STORE_ROWPERM                                                         */
  int32_t vt_len, vt_ld;/* I2V_STORE_VT / I2V_STORE_VT_T                                             */
  float out_scale;
  /* I2V_A_CONV3X3 geometry: input image [n_img, in_h, in_w, cin] fp16 (pixel stride = lda elements),
     3x3 kernel, padding 1, `stride` 1 or 2; `upsample` = 1 applies nearest-2x to the input first
     (Upsample2D).
     `upsample` = 2: the same convolution of the nearest-2x up-sampled input (out = exactly 2 in) with the up-sampling FOLDED INTO
     THE WEIGHTS: the 3x3 taps of output pixel (2 i + py, 2 j + px) touch only 2 x 2 source pixels, so each output parity
     ("phase" ph = 2 py + px) is a 2x2 convolution of the source image, K = 4 * cin.  w holds four matrices [N, 4 * cin], matrix ph
     at w + ph * w_batch_stride, rows_per_w = M / 4; column k = t * cin + ci (conv_kblock = 64: ((ci / 64) * 4 + t) * 64 + ci % 64)
     of tap t = 2 ty + tx multiplies source pixel (i + py - 1 + ty, j + px - 1 + tx) (outside the image: zero) and holds the sum of
     the 3x3 taps (ky, kx) that land on it: rows py = 0: ty = 0 <- ky 0, ty = 1 <- ky 1 + 2; py = 1: ty = 0 <- ky 0 + 1,
     ty = 1 <- ky 2; columns the same with px / kx.  Bias only (no residual, rowvec, gn_partial, residual_lo / c_lo); the 8-wave
     kernel only: i2v_gemm_upconv_fold_supported() tells whether a problem qualifies.
     `asym_pad` = 1 (stride 2 only): no padding at the top / left and one zero row / column at the
     bottom / right = diffusers Downsample2D(padding=0) of the VAE encoder (F.pad(x, (0, 1, 0, 1)) + conv stride 2).
     M = n_img * out_h * out_w. */
  int32_t n_img, in_h, in_w, cin, out_h, out_w, stride, upsample, asym_pad;
  /* order of the 9 * cin contraction index of I2V_A_CONV3X3 (and of w's columns): 0 = tap-major, k = tap * cin + ci;
     64 = channel-block-major, k = ((ci / 64) * 9 + tap) * 64 + ci % 64 (cin % 64 == 0): the 9 taps of one 64-channel
     block are consecutive K tiles, so the 8 re-reads of an input pixel follow each other closely (measured: conv class
     12.40 -> 12.24 ms per step). */
  int32_t conv_kblock;
  /* Per-batch weights (GroupNorm folded into the proj_in GEMM of a transformer / motion-module entry, i2v:218-226, A9:
     the norm's per-image scale multiplies the weights, its shift becomes a per-image bias -- i2v_groupnorm_fold_f16):
     rows [i * rows_per_w, (i + 1) * rows_per_w) of A use the weight matrix w + i * w_batch_stride (elements).
     rows_per_w = 0: one weight matrix.  8-wave kernel only (N % 320 == 0, M and rows_per_w multiples of the row tile). */
  int64_t w_batch_stride;
  int32_t rows_per_w;
  /* A rows gathered through the (batch, frame, pixel) -> (batch, pixel, frame) permutation (the motion modules' entry,
     SURVEY A9): output row m = (b * a_perm_hw + p) * a_perm_frames + f reads A row (b * a_perm_frames + f) * a_perm_hw + p.
     a_perm_frames = 0: none; otherwise a power of two <= 64.  Same kernel restriction. */
  int32_t a_perm_frames, a_perm_hw;
  /* optional fp32 scratch for split-K (small M, long K: the 8 x 8 level's convolutions): when it holds at least
     i2v_gemm_workspace_bytes(p) bytes the K loop is split over several workgroups whose fp32 partial tiles are
     summed by a second kernel that applies the epilogue; NULL / too small => no split. */
  void* workspace;
  int64_t workspace_bytes;
  /* 1: c is FP32 [M, N] (ld = ldc elements) instead of fp16.  Row-major store, no GEGLU; narrow outputs only (the
     generic 4-wave kernel): the UNet's 4-channel conv_out (unet:879-881, 1443) hands the noise prediction to
     i2v_ddim_cfg_step without an fp16 rounding that the CFG combine (pipe:686-688) would amplify by up to
     2 * guidance_scale - 1. */
  int32_t c_is_f32;
  /* (ABI 8) optional: GroupNorm statistics of the result for the norm that consumes it (ResnetBlock2D conv1 -> norm2, unet:203-214;
     diffusers ResnetBlock2D), written by the epilogue so that i2v_groupnorm_f16 needs no statistics pass over the tensor:
     fp32 [n_img][out_h * out_w / R][gn_groups][2] = per (image, block of R consecutive rows, group) the mean and the sum of squared
     deviations over the block's rows x the group's channels, R = i2v_gemm_gn_partial_rows(p) (> 0 where implemented: un-split
     I2V_A_CONV3X3 problems of the 8-wave kernel, no residual, images of whole row blocks).  Hand the buffer and R to
     i2v_gn_params.gpartial_in / gpartial_rows.  NULL: none. */
  void* gn_partial;
  int32_t gn_groups;
  /* (ABI 9) the PRECISE residual stream: the stream between modules (outputs of conv_in, every ResnetBlock2D, spatial transformer,
     motion module, down sampler; pipe:666-697 runs it in fp32 on the reference's CPU path) as an fp16 PAIR hi + lo, hi = fp16(x),
     lo = fp16(x - hi): hi is the tensor every MFMA / LDS-DMA operand reads as before, lo carries the 11 bits the rounding dropped, so
     the identity path of a residual add no longer re-rounds the stream at every module (0.78 of the 0.89e-3 rms).
       residual_lo  fp16 [M, N] (ld = ldr), needs `residual`: the value added is (float)residual + (float)residual_lo
       c_lo         fp16 [M, N] (ld = ldc, row order of c): receives fp16(v - (float)fp16(v)) of the fp32 result v that c rounds
     Row-major / row-permuted fp16 stores without GEGLU / GELU, no LayerNorm fold, no GroupNorm partials.  NULL: none. */
  const void* residual_lo;
  void* c_lo;
} i2v_gemm_params;

int i2v_gemm_f16(const i2v_gemm_params* p, i2v_stream_t stream);
/* 1 if i2v_gemm_f16 accepts this problem with ln_wsum set (pointers are not dereferenced), else 0. */
int i2v_gemm_ln_supported(const i2v_gemm_params* p);
/* 1 if i2v_gemm_f16 accepts this problem with rows_per_w / a_perm_frames set (pointers are not dereferenced), else 0. */
int i2v_gemm_batch_supported(const i2v_gemm_params* p);
/* 1 if i2v_gemm_f16 accepts this I2V_A_CONV3X3 problem with upsample = 2 (pointers are not dereferenced), else 0. */
int i2v_gemm_upconv_fold_supported(const i2v_gemm_params* p);
/* bytes of `workspace` with which i2v_gemm_f16 would split K for this problem (0: it would not split). */
int64_t i2v_gemm_workspace_bytes(const i2v_gemm_params* p);
/* rows per block of the GroupNorm partials i2v_gemm_f16 would write for this problem with gn_partial set (gn_groups must be set;
   pointers are not dereferenced); 0: not implemented for it. */
int32_t i2v_gemm_gn_partial_rows(const i2v_gemm_params* p);

/* (ABI 19) Which kernel a problem takes.  i2v_gemm_f16 dispatches to one of several dozen kernel instantiations; the route names
   the one a problem gets, decided by the same function the launch follows (there is no second copy of the rules). */
enum {
  I2V_ROUTE_GENERIC = 0,   /* the 4-wave register-staged kernel (csrc/gemm.hip): `generic_tile`, `vec4`              */
  I2V_ROUTE_CONV_THIN = 1, /* the halo-tile kernel of narrow 3x3 convolutions (csrc/conv_thin.hip)                    */
  I2V_ROUTE_BIG_TILE = 2,  /* the 8-wave LDS-DMA kernel (csrc/gemm_big.hip), one output tile per workgroup / walk     */
  I2V_ROUTE_BIG_DEEP = 3,  /* ... its deep-pipeline form (three / four LDS stages)                                     */
  I2V_ROUTE_BIG_SPLITK = 4 /* ... with K split over workgroups and the reduce pass                                     */
};
enum { I2V_EXTRA_NONE = 0, I2V_EXTRA_LNF = 1, I2V_EXTRA_HILO = 2, I2V_EXTRA_GNS = 4, I2V_EXTRA_UPF = 8 };

/* (a struct tag only: the query below carries the same name) */
struct i2v_gemm_route {
  int32_t family;       /* I2V_ROUTE_*                                                                                */
  int32_t a_mode;       /* I2V_A_* (echoed: the kernels are instantiated per A source)                                */
  int32_t rows, cols;   /* tile: 8-wave kernel 256 / 128 x 320 / 256 / 128; generic 128 / 64 x 128 / 64; thin 0, 0    */
  int32_t stages;       /* LDS stages of the 8-wave kernel (2; deep: 3 / 4), else 0                                   */
  int32_t splits, kps;  /* split-K: K ranges and 64-deep K tiles per range, else 0                                    */
  int32_t extra;        /* I2V_EXTRA_*: what the 8-wave kernel adds to the plain epilogue (LayerNorm fold, hi + lo
                           stores, GroupNorm partials, folded up-sampling); 0 for the other families                 */
  int32_t persistent;   /* 1: the persistent tile walk (I2V_GEMM_PERSIST)                                             */
  int32_t generic_tile; /* generic kernel: 0 = 128x128, 1 = 128x64, 2 = 64x128, 3 = 64x64; else -1                    */
  int32_t vec4;         /* generic kernel: 1 = 8-byte vector epilogue, 0 = element by element; else -1                */
  int32_t epilogue;     /* I2V_EPI_* (echoed)                                                                         */
  int32_t store_mode;   /* I2V_STORE_* (echoed)                                                                       */
};

/* The route i2v_gemm_f16 would take for p (its workspace and pointers as attached; pointers are only tested for null and
   alignment): pure host arithmetic, no device call.  The problem's arguments are NOT validated here; < 0 on null arguments. */
int i2v_gemm_route(const i2v_gemm_params* p, struct i2v_gemm_route* route);
/* The route of the calling thread's most recent i2v_gemm_f16 that reached a launch (< 0: none yet). */
int i2v_gemm_last_route(struct i2v_gemm_route* route);
/* 1 if the kernel instantiation that `route` names (family, a_mode, rows, cols, stages, extra, persistent, generic_tile,
   epilogue, store_mode; splits / kps / vec4 are run-time arguments and are not read) is in the launch table, else 0.  Read from
   the launch table itself. */
int i2v_gemm_kernel_exists(const struct i2v_gemm_route* route);

/* ------------------------------------------------------------------------------------------------
 * Flash-style attention forward (MFMA QK^T / PV, wavefront-shuffle online softmax).
 *   O[bq, l, h, :] (+)= softmax_j( scale * Q[bq, l, h, :] . K[bq / kv_group, j, h, :] ) V[bq / kv_group, j, h, :]
 * replaces F.scaled_dot_product_attention at:
 *   K1 cross-frame adapter attention i2v:483-492  (kv_group = num_frames: every frame reads frame-0 K/V)
 *   K2 spatial self-attention        i2v:468-473  (kv_group = 1)
 *   K3 text cross-attention + IP-Adapter decoupled branch i2v:527-532, unet:1263-1279
 *      (second call with accumulate = 1, acc_scale = ip scale)
 * V is passed TRANSPOSED: vt[b][h*d + i][key] (see I2V_STORE_VT), row stride vt_row_stride >= lk rounded
 * up to 8; entries past lk may hold garbage (they are masked in-kernel).  head_dim % 8 == 0, <= 160.
 * One (batch, head) slice of K ((lk + 128) * k_row_stride elements) and of V^T (head_dim * vt_row_stride) must
 * span less than 1 GiB (the kernel addresses them with 32-bit buffer offsets); larger inputs are rejected with
 * I2V_ERR_INVALID_ARG.  Numerics: scale * log2(e) is folded into the fp16 Q fragments (one extra fp16
 * rounding of Q), softmax in base 2 with fp32 accumulation, P rounded to fp16 for the PV product.
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2v_attn_params {
  const void* q;  int64_t q_row_stride, q_batch_stride;
  const void* k;  int64_t k_row_stride, k_batch_stride;
  const void* vt; int64_t vt_row_stride, vt_batch_stride;
  void* o;        int64_t o_row_stride, o_batch_stride;
  int32_t batch_q, kv_group, heads, head_dim, lq, lk;
  float scale;
  int32_t accumulate;
  float acc_scale;
  float* lse;     /* optional (ABI 6): fp32 [batch_q][heads][lq], the log2-sum-exp of the scaled logits of every query row,
                     written by the forward pass itself (what i2v_attention_lse_f32 recomputes; the training step keeps it
                     for i2v_attention_bwd_f16).  NULL: not written.  Not combined with accumulate.  It is the statistic of
                     the kernel's own logits (Q is scaled and rounded to fp16 before Q K^T): within 1e-3 of max|lse| of
                     i2v_attention_lse_f32's, which is the one that makes the backward's recomputed rows of P sum to 1.    */
} i2v_attn_params;

int i2v_attention_f16(const i2v_attn_params* p, i2v_stream_t stream);

/* (ABI 35) Which kernel an attention-forward problem takes.  i2v_attention_f16 dispatches to 112 kernel instantiations: 8 head-dim
   classes <dqk, dpv> (<32,16> <32,32> <64,48> <64,64> <96,80> <96,96> <128,128> <160,160>: head_dim takes the first whose dpv
   holds it), each with or without a spare V^T row (spare: head_dim < dpv, the PV MFMA computes the row sum), with qt = 1 | 2
   16-row query tiles per wave (2 from lq >= 128 on, except the <128,128> class; I2V_ATTN_QT overrides), as a one-trip kernel or as
   one that walks qbw query blocks per workgroup (walk: a single key tile and at least 2048 workgroups; I2V_ATTN_WALK=0 turns it
   off), on kvt = 64-key tiles; dqk = 64 also on 96-key tiles (64 < lk <= 96) and dqk <= 64 on 128-key tiles (I2V_ATTN_KVT=128
   only).  The route is decided by the same function the launch follows, and `remap` by the function the kernel itself calls. */
struct i2v_attn_route {
  int32_t dqk, dpv;   /* the head-dim class: head_dim padded to the QK^T contraction (32) and to the PV tile (16)             */
  int32_t spare;      /* 1: head_dim < dpv                                                                                    */
  int32_t qt;         /* 16-row query tiles per wave, 1 | 2: a workgroup owns 64 qt query rows per block                      */
  int32_t kvt;        /* keys per tile: 64 | 96 | 128                                                                         */
  int32_t walk;       /* 1: the kernel that walks qbw (> 1) consecutive query blocks per workgroup                            */
  int32_t qbw;        /* query blocks per workgroup, 1..8 (a run-time argument)                                               */
  int32_t grid_x, grid_y, grid_z; /* the launch: ceil(ceil(lq / (64 qt)) / qbw) x heads x batch_q workgroups                  */
  int32_t remap;      /* how a workgroup finds its (query block, head, batch): 0 natural order, 1 the short-key re-deal
                         (lk <= 128, grid_x grid_z % 8 == 0), 2 the pair re-deal (grid_y grid_z % 8 == 0)                     */
};

/* The route i2v_attention_f16 would take for these sizes: pure host arithmetic, no device call.  The sizes are validated as the
   launch validates them (< 0: the launch would refuse them, or a null argument). */
int i2v_attention_route(int32_t batch_q, int32_t kv_group, int32_t heads, int32_t head_dim, int32_t lq, int32_t lk,
                        struct i2v_attn_route* route);
/* The route of the calling thread's most recent i2v_attention_f16 that reached a launch (< 0: none yet). */
int i2v_attention_last_route(struct i2v_attn_route* route);
/* 1 if the kernel instantiation that `route` names (dqk, dpv, spare, qt, kvt, walk; qbw, the grid and remap are run-time values
   and are not read) is in the launch table, else 0.  Read from the launch table itself. */
int i2v_attn_kernel_exists(const struct i2v_attn_route* route);

/* ------------------------------------------------------------------------------------------------
 * Temporal (motion-module) self-attention: sequence = frames (<= 32) of one pixel; tokens are in
 * (b, pixel, frame) order so each pixel's q/k rows are `frames` consecutive rows; vt is
 * vt[pixel][h*d + i][frame] with row stride vt_ld (>= frames rounded up to 8).
 * Replaces SDPA inside diffusers TransformerTemporalModel (unet:323-326,520-523,688-691).
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2v_tattn_params {
  const void* q; int64_t q_row_stride;
  const void* k; int64_t k_row_stride;
  const void* vt; int32_t vt_ld;
  void* o; int64_t o_row_stride;
  int32_t n_pixels, frames, heads, head_dim;
  float scale;
} i2v_tattn_params;

int i2v_temporal_attention_f16(const i2v_tattn_params* p, i2v_stream_t stream);

/* (ABI 20) Which kernel a temporal-attention problem takes.  i2v_temporal_attention_f16 dispatches to 48 kernel instantiations:
   8 head-dim classes <dqk, dpv> (<32,16> <32,32> <64,48> <64,64> <96,80> <96,96> <128,128> <160,160>: head_dim takes the first
   whose dpv holds it), each in an LDS-staged form (frames <= 16, one pixel's operands within 64 KiB of LDS and within 256 * 4
   16-byte chunks per operand, o 16-byte aligned with a row stride that is a multiple of 8; I2V_TATTN_LDS=0 turns the form off)
   with pf = 1..4 chunks per thread, and in a register form with nqt = 1 (frames <= 16) or 2 query tiles.  The route is decided
   by the same function the launch follows (there is no second copy of the rules). */
enum { I2V_TATTN_LDS_FORM = 0, I2V_TATTN_REG_FORM = 1 };

/* (a struct tag only, as i2v_gemm_route) */
struct i2v_tattn_route {
  int32_t form;     /* I2V_TATTN_*_FORM                                                                      */
  int32_t dqk, dpv; /* the head-dim class: head_dim padded to the QK^T contraction (32) and to the PV tile (16) */
  int32_t pf;       /* LDS form: 16-byte chunks per thread and operand, 1..4; register form 0                */
  int32_t nqt;      /* register form: 16-query tiles per wave, 1 | 2; LDS form 0                             */
  int32_t blocks;   /* workgroups of the launch                                                              */
};

/* The route i2v_temporal_attention_f16 would take for p: pure host arithmetic, no device call.  p is validated as the launch
   validates it (< 0: the launch would refuse it, or a null argument); pointers are only tested for null and alignment. */
int i2v_temporal_attention_route(const i2v_tattn_params* p, struct i2v_tattn_route* route);
/* The route of the calling thread's most recent i2v_temporal_attention_f16 that reached a launch (< 0: none yet). */
int i2v_temporal_attention_last_route(struct i2v_tattn_route* route);
/* 1 if the kernel instantiation that `route` names (form, dqk, dpv, pf, nqt; blocks is a run-time argument and is not read) is
   in the launch table, else 0.  Read from the launch table itself. */
int i2v_tattn_kernel_exists(const struct i2v_tattn_route* route);

/* ------------------------------------------------------------------------------------------------
 * The whole attention sub-block of a motion module's temporal transformer block in one launch:
 *     n = LayerNorm(x) * gamma + beta + pe[row % frames];  q, k, v = n Wq^T, n Wk^T, n Wv^T (no bias);
 *     out[rows of pixel][head h] = softmax(q_h k_h^T * scale) v_h over the `frames` rows of each pixel
 * for rows in (batch, pixel, frame) order -- `norm1 -> attn1` / `norm2 -> attn2` of the BasicTransformerBlock inside
 * diffusers TransformerTemporalModel up to (not including) to_out (unet:232-244, 413-425, 607-619), which
 * the caller applies with i2v_gemm_f16 (+ residual).  LayerNorm output, q, k, v and P are rounded to fp16 where the
 * un-fused kernels store them; statistics, logits, softmax and accumulation in fp32.
 * gamma: fp32 [channels]; shift: fp32 [frames][channels] = beta[c] + pe[frame][c] (the LayerNorm shift and the sinusoidal
 * table of SURVEY A10 pre-added: both are constants of the module).
 * w_qkv: per head its rows of Wq, Wk, Wv, each zero-padded to P = pad16(head_dim) rows, stored in MFMA-fragment order:
 * fp16 [heads][3][channels / 32][P / 16][64][8] with element [h][part][s][t][l][j] = W_part[h * head_dim + 16 t + (l & 15)]
 * [32 s + 8 (l >> 4) + j]  (i2v_motion_attn_pack_rows(heads, head_dim) * channels elements in all).
 * Implemented for the SD-1.5 64^2 level: i2v_motion_attn_supported(...) != 0 (channels 320, 8 heads of 40, 16 frames,
 * rows a multiple of 128); any other shape returns I2V_ERR_INVALID_ARG and callers use the un-fused kernels.
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2v_motion_attn_params {
  const void* x; int64_t ldx;           /* fp16 [rows, channels] */
  const void* gamma;                    /* fp32 [channels] */
  const void* shift; int64_t ld_shift;  /* fp32 [frames, channels] */
  const void* w_qkv;
  void* out; int64_t ldo;               /* fp16 [rows, channels] */
  int64_t rows;
  int32_t channels, heads, head_dim, frames;
  float eps, scale;
  /* (ABI 8) optional, both or neither: the sub-block's out-projection and residual in the same launch --
   * out = x + o to_out[0].weight^T + to_out[0].bias (what the caller otherwise does with i2v_gemm_f16 + residual).
   * w_o: to_out[0].weight [channels, channels] in the fragment order of i2v_cross_attn_fused_f16's w_q (rows grouped per head-sized
   * slice); b_o: fp32 [channels].  out may be x. */
  const void* w_o; const void* b_o;
} i2v_motion_attn_params;

int32_t i2v_motion_attn_supported(int64_t rows, int32_t channels, int32_t heads, int32_t head_dim, int32_t frames);
int32_t i2v_motion_attn_pack_rows(int32_t heads, int32_t head_dim);
int i2v_motion_attn_f16(const i2v_motion_attn_params* p, i2v_stream_t stream);

/* (ABI 28) The same sub-block at the SD-1.5 32^2 level -- channels 640, 8 heads of 80, 16 frames, rows a multiple of 64 -- on
 * 64-row tiles, always WITH the out-projection and residual (w_o and b_o are required).  Same parameter struct, same weight
 * layouts (head_dim 80 is five whole 16-row tiles: no padding rows); i2v_motion_attn_supported / i2v_motion_attn_f16 answer
 * for the 64^2 level as before. */
int32_t i2v_motion_attn_wide_supported(int64_t rows, int32_t channels, int32_t heads, int32_t head_dim, int32_t frames);
int i2v_motion_attn_wide_f16(const i2v_motion_attn_params* p, i2v_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * `norm2 -> attn2` of the spatial transformer block (i2v:510-533) up to (not including) to_out, for a context that fits
 * the registers (the 77 CLIP tokens), in one launch: n = LayerNorm(x) * gamma + beta; q = n Wq^T;
 *     out[row][head h] = softmax(q_h K_h^T * scale) V_h   with K = ctx_k rows, V^T = ctx_vt rows of the row's context
 * (rows [i * rows_per_ctx, (i + 1) * rows_per_ctx) attend to context i: the frames of one sample share its prompt).
 * Replaces native_layer_norm + to_q + SDPA(q, to_k(ctx), to_v(ctx)); the context projections are the caller's (they do
 * not depend on the step).  gamma, beta: fp32 [channels]; w_q: to_q's rows per head, zero-padded to pad16(head_dim), in the
 * fragment order of i2v_motion_attn_f16's w_qkv with one part ([heads][channels / 32][P / 16][64][8],
 * i2v_cross_attn_fused_pack_rows(heads, head_dim) * channels elements).
 * ctx_frag: the context's projected keys and values as the MFMA operand fragments the kernel keeps in registers, packed once
 * per prompt: fp16 [n_ctx][heads][30][64][4] (i2v_cross_attn_fused_ctx_elems(n_ctx, heads, head_dim) elements) with
 *   [c][h][3 kt + t][16 g + r][j]      = K[c][key = 16 kt + r][h * head_dim + 16 t + 4 g + j]       (kt < 5, t < 3)
 *   [c][h][15 + 5 t + kt][16 g + r][j] = V[c][key = 16 kt + 4 g + j][h * head_dim + 16 t + r]
 * and zero wherever key >= ctx_len or the channel offset >= head_dim.
 * Implemented where i2v_cross_attn_fused_supported(...) != 0: channels 320, 8 heads of 40, ctx_len <= 80, rows and
 * rows_per_ctx multiples of 128 (the SD-1.5 64^2 level).
 * ip_frag (optional, NULL = none): the IP-Adapter's image tokens of the same contexts (unet:1263-1279) packed the
 * same way from to_k_ip / to_v_ip (ip_len <= 16 tokens, i.e. key tile 0 of the layout): out += ip_scale * softmax(q K_ip^T * scale) V_ip.
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2v_cross_attn_fused_params {
  const void* x; int64_t ldx;            /* fp16 [rows, channels] */
  const void* gamma; const void* beta;   /* fp32 [channels] */
  const void* w_q;
  const void* ctx_frag;
  void* out; int64_t ldo;                /* fp16 [rows, channels] */
  int64_t rows, rows_per_ctx;
  int32_t channels, heads, head_dim, ctx_len;
  float eps, scale;
  const void* ip_frag; int32_t ip_len; float ip_scale;
  /* (ABI 8) optional, both or neither: out = x + o to_out[0].weight^T + to_out[0].bias in the same launch (as i2v_motion_attn_params) */
  const void* w_o; const void* b_o;
} i2v_cross_attn_fused_params;

int32_t i2v_cross_attn_fused_supported(int64_t rows, int32_t channels, int32_t heads, int32_t head_dim, int32_t ctx_len,
                                       int64_t rows_per_ctx);
int32_t i2v_cross_attn_fused_pack_rows(int32_t heads, int32_t head_dim);
int64_t i2v_cross_attn_fused_ctx_elems(int32_t n_ctx, int32_t heads, int32_t head_dim);
int i2v_cross_attn_fused_f16(const i2v_cross_attn_fused_params* p, i2v_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * (ABI 8) LayerNorm 1 and the projections in front of the spatial block's self- / cross-frame attention in one launch
 * (i2v:444-445 `norm1`, 468-473 `attn1` to_q / to_k / to_v, 483-492 the adapter's to_q):
 *     n = LayerNorm(x) gamma + beta;   qk[r, :] = n[r] W_qk^T  (n_qk = 2 C: [q | k], 3 C: [q | k | q_adapter], or C: [k] alone);
 *     vt[r / rows_per_image][c][r % rows_per_image] = (n[r] W_v^T)[c]     (the V^T operand of i2v_attention_f16)
 * replaces native_layer_norm + three / four aten addmm (+ the transpose SDPA does internally).  LayerNorm output rounded to fp16
 * where the un-fused kernels store it; statistics and accumulation in fp32.  gamma, beta: fp32 [channels].
 * w: the rows of [W_qk ; W_v] ((n_qk + C) x C, diffusers Linear layout) per 16-row tile in MFMA-fragment order
 *    [(n_qk + C) / 16][C / 32][64][8]: element [T][s][l][j] = W[16 T + (l & 15)][32 s + 8 (l >> 4) + j].
 * Implemented for the SD-1.5 64^2 level (i2v_ln_qkv_supported: channels 320, rows and rows_per_image multiples of 128; 0 also when
 * the current device refuses the kernel's 160 KB of LDS).
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2v_ln_qkv_params {
  const void* x; int64_t ldx;            /* fp16 [rows, channels] */
  const void* gamma; const void* beta;   /* fp32 [channels] */
  const void* w;
  void* qk; int64_t ld_qk;               /* fp16 [rows, n_qk] */
  void* vt; int64_t vt_batch_stride, vt_row_stride;   /* fp16 [rows / rows_per_image][channels][>= rows_per_image] */
  int64_t rows, rows_per_image;
  int32_t channels, n_qk;
  float eps;
  /* > 0: image i's rows_per_image rows start at x + i * x_image_stride elements instead of following image i - 1 -- the frame-0
     rows of every clip read in place for the adapter's K0 | V0^T (n_qk = C: [k] only; i2v:484-492, no gathered copy) */
  int64_t x_image_stride;
} i2v_ln_qkv_params;

int32_t i2v_ln_qkv_supported(int64_t rows, int32_t channels, int32_t n_qk, int64_t rows_per_image);
int i2v_ln_qkv_f16(const i2v_ln_qkv_params* p, i2v_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The GEGLU feed-forward of a transformer block in one launch (i2v:539-561 `norm3 -> ff -> + residual`; the temporal block's
 * FeedForward):  out = x + W2 (value o gelu(gate)) + b2  with  [value | gate] = (LayerNorm(x) gamma + beta) W1^T + b1.
 * The inner activation (rows x inner) never leaves the CU.  LayerNorm output and the inner activation are rounded to fp16 where
 * the un-fused kernels store them; statistics, GELU (common.h gelu_erf) and accumulation in fp32.  out may alias x.
 * gamma, beta: fp32 [channels]; b2: fp32 [channels].  Packed operands (fp16 unless noted), with the inner dimension in chunks of 128:
 *   w1 [inner / 128][8][2][channels / 32][64][8]: element [ch][w][u][s][l][j] =
 *      W1[(m & 1) * inner + 128 ch + 16 w + 8 u + (m >> 1)][32 s + 8 (l >> 4) + j], m = l & 15  (diffusers GEGLU.proj: rows
 *      [0, inner) are the values, [inner, 2 inner) the gates: a 16-row tile holds 8 (value, gate) pairs);
 *   b1 fp32 [inner / 128][8][2][16]: the same rows' biases;
 *   w2 [8][inner / 128][4][3][64][8]: element [w][ch][ks][t][l][j] = W2[n = 40 w + 16 t + (l & 15)][128 ch + 32 ks + 8 (l >> 4) + j],
 *      zero where 16 t + (l & 15) >= 40.
 * Implemented for the SD-1.5 64^2 level (i2v_ff_fused_supported: channels 320, inner 1280, rows a multiple of 128; 0 also when
 * the current device refuses the kernel's 160 KB of LDS -- callers then take the un-fused GEMM pair).
 *
 * Optional tail (ABI 8; w3 != NULL): the Linear that follows the block in the same launch --
 *     out[perm(r)] = res2[perm(r)] + y[r] W3^T + b3,   y = x + FF(LayerNorm(x)) rounded to fp16 as the un-fused kernel stores it
 * i.e. the spatial transformer's proj_out with its residual (i2v:298-314; perm = identity) or the motion module's proj_out
 * (perm_frames = F > 0, a power of two: rows arrive in (batch, pixel, frame) order, and out / res2 are addressed in
 * (batch, frame, pixel) order with perm_hw pixels per image -- I2V_STORE_ROWPERM of i2v_gemm_f16).  w3: W3 [channels, channels]
 * per 40-row slice in fragment order, the layout of i2v_cross_attn_fused_params.w_q ([8][channels / 32][3][64][8]); b3 fp32
 * [channels]; res2 fp16 rows of ld_res2 elements.  With the tail, out must not alias x when perm_frames > 0.
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2v_ff_fused_params {
  const void* x; int64_t ldx;            /* fp16 [rows, channels] */
  const void* gamma; const void* beta;   /* fp32 [channels] */
  const void* w1; const void* b1;
  const void* w2; const void* b2;
  void* out; int64_t ldo;                /* fp16 [rows, channels] */
  int64_t rows;
  int32_t channels, inner;
  float eps;
  /* tail (all zero: none) */
  const void* w3; const void* b3;
  const void* res2; int64_t ld_res2;
  int32_t perm_frames, perm_hw;
  /* (ABI 9) the precise residual stream through the tail (see i2v_gemm_params.residual_lo / c_lo): res2_lo [rows of ld_res2] is
     added with res2, out_lo [rows of ldo] receives the low half of the result.  Tail only; both or neither. */
  const void* res2_lo;
  void* out_lo;
} i2v_ff_fused_params;

int32_t i2v_ff_fused_supported(int64_t rows, int32_t channels, int32_t inner);
/* ... with the tail: rows in (batch, pixel, frame) order of `perm_frames` frames and `perm_hw` pixels per image (0, 0: no permutation) */
int32_t i2v_ff_fused_tail_supported(int64_t rows, int32_t channels, int32_t inner, int32_t perm_frames, int32_t perm_hw);
int i2v_ff_fused_f16(const i2v_ff_fused_params* p, i2v_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GroupNorm (+ optional SiLU) on token-major fp16: statistics in fp32.
 *   stat group = (frames_per_stat consecutive images) x (all pixels) x (C / groups channels)
 *   frames_per_stat = 1: ResnetBlock2D norm1/norm2, Transformer2D norm, conv_norm_out
 *                        (unet:203-214, i2v:218, unet:870-873)
 *   frames_per_stat = F: TransformerTemporalModel.norm, statistics over (C/G, F, H, W)
 * x may be two sources concatenated along channels (c1 from x, c2 from x2: skip concat, unet:478).
 * out_perm = 1 writes rows in (b, pixel, frame) order (motion-module entry).
 * workspace: i2v_groupnorm_workspace_bytes(...) bytes of scratch, fp32.
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2v_gn_params {
  const void* x;  int32_t c1;
  const void* x2; int32_t c2;
  const void* gamma; const void* beta; /* fp16 [c1 + c2] */
  void* y;                              /* fp16 [n_img, hw, c1 + c2] */
  int32_t n_img, hw, groups, frames_per_stat;
  float eps;
  int32_t silu;
  int32_t out_perm; int32_t frames; /* out_perm: images are (b, f); output row = (b*hw + p)*frames + f */
  void* workspace;
  /* (ABI 8) optional: the statistics as per-group partials written by the producing convolution (i2v_gemm_params.gn_partial) --
     fp32 [n_img][hw / gpartial_rows][groups][2]; the statistics pass over x is skipped.  frames_per_stat 1, no out_perm, no x2. */
  const void* gpartial_in; int32_t gpartial_rows;
} i2v_gn_params;

int64_t i2v_groupnorm_workspace_bytes(int32_t n_img, int32_t hw, int32_t channels);
int i2v_groupnorm_f16(const i2v_gn_params* p, i2v_stream_t stream);
/* GroupNorm (no activation) folded into the Linear / 1x1 conv that consumes it (the entry of every spatial transformer
 * and motion module: norm -> proj_in, i2v:218-226): the statistics of p->x are computed as above, then instead of
 * writing the normalised tensor, per statistics group s (= image, or clip when frames_per_stat > 1)
 *     w_out[s][n][c]  = fp16(w[n][c] * a[s][c])              a = gamma * rstd
 *     bias_out[s][n]  = fp16(bias[n] + sum_c w[n][c] b[s][c])  b = beta - mean * a
 * so that proj_in(GroupNorm(x)) = x w_out[s]^T + bias_out[s] (i2v_gemm_params.w_batch_stride / rows_per_w, bias through
 * rowvec / rows_per_vec): the normalised activations are never written to / read back from HBM.  p->y, silu, out_perm
 * are ignored.  w [n_out, ldw >= C] fp16, w_out [n_img / frames_per_stat, n_out, C], bias_out [.., n_out] fp16. */
int i2v_groupnorm_fold_f16(const i2v_gn_params* p, const void* w, int64_t ldw, const void* bias, int32_t n_out,
                           void* w_out, void* bias_out, i2v_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm over the channel axis (fp32 statistics), optional additive positional embedding
 * y[r, :] = LN(x[r, :]) * gamma + beta (+ pe[r % pe_period, :])
 * replaces native_layer_norm at i2v:445,514,539 and, with pe, LN + SinusoidalPositionalEmbedding of the
 * motion-module block.
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2v_ln_params {
  const void* x; int64_t ldx;
  const void* gamma; const void* beta; /* fp16 [C] */
  const void* pe; int64_t ld_pe; int32_t pe_period; /* fp16 [pe_period, C] or NULL */
  void* y; int64_t ldy;
  int32_t rows, C;
  float eps;
  /* x_rows_per_batch > 0: the input is a batch of row blocks, output row r reads x + (r / x_rows_per_batch) *
   * x_batch_stride + (r % x_rows_per_batch) * ldx (elements).  The cross-frame attention normalises only the frame-0
   * rows of each clip (i2v:484: `norm_hidden_states[0:batch:num_frames]`): rows_per_batch = tokens per frame, batch
   * stride = one clip, read in place instead of through a gathered copy.  0: one dense matrix (the output is always dense). */
  int32_t x_rows_per_batch; int64_t x_batch_stride;
} i2v_ln_params;

int i2v_layernorm_f16(const i2v_ln_params* p, i2v_stream_t stream);

/* y[r, :cols] = softmax(scale * x[r, :cols]) row-wise, fp16 in / out, fp32 statistics (in place allowed).  The VAE
 * mid-block attention (diffusers Attention with ONE head of dim 512, AutoencoderKL decode / encode, pipe:305,627)
 * exceeds the flash kernel's head_dim limit: its QK^T and PV products run as i2v_gemm_f16 calls around this kernel. */
int i2v_softmax_rows_f16(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t cols, float scale,
                         i2v_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Layout edges, embeddings and the sampler step
 * ------------------------------------------------------------------------------------------------ */
/* NCHW (fp32 if src_is_f32 else fp16) [n, c, h*w] -> token-major fp16 [n, h*w, c_pad], channels >= c zeroed
 * (sample.reshape + conv_in input, unet:1358). */
int i2v_nchw_to_tokens(const void* src, int32_t src_is_f32, void* dst, int32_t n, int32_t c, int32_t hw,
                       int32_t c_pad, i2v_stream_t stream);
/* token-major (fp32 if src_is_f32 else fp16) [n, hw, ld] (first c channels) -> NCHW (fp32 if dst_is_f32 else fp16)
 * (unet:1446). */
int i2v_tokens_to_nchw(const void* src, int32_t src_is_f32, int64_t ld, void* dst, int32_t dst_is_f32, int32_t n,
                       int32_t c, int32_t hw, i2v_stream_t stream);
/* Timesteps(dim, flip_sin_to_cos=True, shift 0): out[b, :] = [cos(t*w) | sin(t*w)] fp16 (unet:763,1336).
 * t is fp32 [n]; if t_index != NULL, t is a table of t_rows entries and the single value
 * t[clamp(*t_index, 0, t_rows - 1)] is used for every row (graph replay). */
int i2v_timestep_embedding(const float* t, const int32_t* t_index, int32_t t_rows, void* out, int32_t n,
                           int32_t dim, i2v_stream_t stream);
/* out[0, :] = table[clamp(*row_index, 0, rows - 1), :] (fp16, cols % 8 == 0): the pipeline computes
 * time_emb_proj(silu(time_embedding(time_proj(t)))) of every resnet (unet:1336-1343) for ALL timesteps of the
 * schedule once per sample; a replayed step picks its row by the device-side step counter (pipe:666 `for i, t in ...`). */
int i2v_select_row_f16(const void* table, int64_t ld, int32_t rows, const int32_t* row_index, void* out, int32_t cols,
                       i2v_stream_t stream);
/* y = silu(x), fp16, n elements (nonlinearity(temb), ResnetBlock2D). */
int i2v_silu_f16(const void* x, void* y, int64_t n, i2v_stream_t stream);
/* y[r, :] = x[r / repeat, :]  (repeat_interleave of temb / context rows, unet:1344,1355). */
int i2v_repeat_rows_f16(const void* x, void* y, int64_t rows_in, int64_t cols, int32_t repeat,
                        i2v_stream_t stream);
/* dst[b, r, :cols] = src[b, r, :cols] for b < batches, r < rows: fp16 strided 3-D copy (strides in elements).
 * Used to gather the frame-0 tokens of every clip (i2v:484) and to split text / image context tokens. */
int i2v_copy3d_f16(const void* src, int64_t src_batch_stride, int64_t ld_src, void* dst, int64_t dst_batch_stride,
                   int64_t ld_dst, int64_t batches, int64_t rows, int64_t cols, i2v_stream_t stream);

/* (ABI 9) `ctx_frag` of i2v_cross_attn_fused_f16 from the projected context as the other kernels take it: k fp16 [n_ctx * ctx_len, ldk]
 * (head h in columns h * head_dim ..), vt fp16 V^T[n_ctx][heads * head_dim][>= ctx_len] (row / batch strides in elements) ->
 * out fp16 [n_ctx][heads][2 * 5 * ceil(head_dim / 16)][64][4] (i2v_pack_ctx_fragments_elems() elements), zero beyond ctx_len (<= 80)
 * and head_dim.  Serves i2v:527-532 / unet:1263-1279 (to_k / to_v of the prompt and of the IP-Adapter's image tokens); until ABI 9
 * the host mirror assembled it with torch index ops, which kept a whole-model forward from being library launches only. */
int64_t i2v_pack_ctx_fragments_elems(int32_t n_ctx, int32_t heads, int32_t head_dim);
int i2v_pack_ctx_fragments_f16(const void* k, int64_t ldk, const void* vt, int64_t vt_row_stride, int64_t vt_batch_stride, void* out,
                               int32_t n_ctx, int32_t heads, int32_t head_dim, int32_t ctx_len, i2v_stream_t stream);

/* One DDIM step around the UNet call, pipe:666-691, split in the two halves that bracket it.
 *   prep : latents[:, 0] = cond (pipe:669); model_in = tokens(cat([latents] * cfg_copies)) fp16, channels
 *          padded to c_pad (pipe:672-673; scale_model_input is the identity for DDIM).
 *   step : eps = u + g (c - u) (pipe:686-688); x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t);
 *          x_prev = sqrt(a_prev) x0 + sqrt(1-a_prev) eps (pipe:691); then *step_index advances by one
 *          and wraps to 0 after n_steps (the table row read is clamped to [0, n_steps - 1]).
 * latents fp32 [b, f, c, hw]; cond fp32 [b, c, hw]; noise_pred tokens [cfg_copies*b*f, hw, ld_np], fp32 if np_is_f32
 * (the conv_out GEMM with c_is_f32) else fp16;
 * coef fp32 [n_steps][4] = {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)}; step_index device int32. */
int i2v_ddim_prep(float* latents, const float* cond, void* model_in, int32_t b, int32_t f, int32_t c,
                  int32_t hw, int32_t c_pad, int32_t cfg_copies, i2v_stream_t stream);
int i2v_ddim_cfg_step(float* latents, const void* noise_pred, int32_t np_is_f32, int64_t ld_np, const float* coef, int32_t n_steps,
                      int32_t* step_index, float guidance_scale, int32_t b, int32_t f, int32_t c, int32_t hw,
                      int32_t cfg_copies, i2v_stream_t stream);

/* (ABI 10) The DPM-Solver++ (2M, midpoint, data prediction) form of the step half, for DPMSolverMultistepScheduler: the same
 * CFG combine and the same layouts as i2v_ddim_cfg_step (i2v_ddim_prep is reused unchanged: scale_model_input is the identity), then
 *   x0 = (x - s_s0 eps) / a_s0;  x_t = (s_t / s_s0) x + c_cur x0 + c_prev x0_prev;  x0_prev := x0
 * and *step_index advances / wraps as in the DDIM step.
 * coef fp32 [n_steps][6] = {a_s0, s_s0, s_t / s_s0, c_cur, c_prev, order}, with a = 1 / sqrt(sigma^2 + 1), s = sigma a,
 * lambda = log a - log s, h = lambda_t - lambda_s0 and, for order 2, r0 = (lambda_s0 - lambda_s1) / h:
 *   order 1: c_cur = a_t (1 - e^-h), c_prev = 0;
 *   order 2: c_cur = a_t (1 - e^-h) (1 + 1 / (2 r0)), c_prev = -a_t (1 - e^-h) / (2 r0).
 * x0_prev fp32 [b, f, c, hw]: the previous step's data prediction.  A row with order 1 does not read it (its contents before the
 * first step of a sample do not matter); every row writes it. */
int i2v_dpm_cfg_step(float* latents, float* x0_prev, const void* noise_pred, int32_t np_is_f32, int64_t ld_np, const float* coef,
                     int32_t n_steps, int32_t* step_index, float guidance_scale, int32_t b, int32_t f, int32_t c, int32_t hw,
                     int32_t cfg_copies, i2v_stream_t stream);

/* (ABI 14) The latent-consistency (LCM) form of the step half, for LCMScheduler (diffusers 0.24 LCMScheduler.step, epsilon prediction):
 * the same CFG combine and the same layouts as i2v_dpm_cfg_step, then
 *   x0 = (x - sb_t eps) / sa_t;  den = c_out x0 + c_skip x;  x' = sa_p den + sb_p z,  z = noise[min(step, n_noise - 1)]
 * and *step_index advances / wraps as in the DDIM step.
 * coef fp32 [n_steps][6] = {sa_t, sb_t, c_skip, c_out, sa_p, sb_p}: sa = sqrt(a), sb = sqrt(1 - a) at this step's timestep (t) and at the
 * next one (p); c_skip = 0.25 / (s^2 + 0.25), c_out = s / sqrt(s^2 + 0.25) with s = t * timestep_scaling.  The last row of a schedule
 * has sa_p = 1, sb_p = 0 (the step returns `den`).
 * noise fp32 [n_noise][b, f, c, hw]: the Gaussian draw each step but the last re-noises with, one row per step, read on the device by
 * the step counter (a replayed hipGraph has no per-step host draw).  A row with sb_p == 0 does not read it; noise may be NULL only
 * when n_steps == 1.  16-byte accesses when hw % 4 == 0 and latents and noise are 16-byte aligned, scalar ones otherwise. */
int i2v_lcm_cfg_step(float* latents, const float* noise, int32_t n_noise, const void* noise_pred, int32_t np_is_f32, int64_t ld_np,
                     const float* coef, int32_t n_steps, int32_t* step_index, float guidance_scale, int32_t b, int32_t f, int32_t c,
                     int32_t hw, int32_t cfg_copies, i2v_stream_t stream);

/* (ABI 29) The sigma-space form of both halves of the step, for EulerDiscreteScheduler and EulerAncestralDiscreteScheduler (diffusers
 * 0.24, epsilon prediction).  One coefficient table serves both launches:
 *   coef fp32 [n_steps][4] = {sigma, 1 / sqrt(sigma^2 + 1), sigma_to, sigma_up}
 * with sigma_to = sigma_next, sigma_up = 0 for Euler and sigma_to = sigma_down = sqrt(sigma_next^2 - sigma_up^2),
 * sigma_up = sqrt(sigma_next^2 (sigma^2 - sigma_next^2) / sigma^2) for the ancestral sampler (its last row: both 0).
 *   prep : i2v_ddim_prep with scale_model_input: latents[:, 0] = cond, UNSCALED (pipe:669); model_in = fp16(v * coef[step][1]), frame 0
 *          included (the reference scales after the overwrite, pipe:669-673).  step = clamp(*step_index, 0, n_steps - 1); the counter
 *          is read, not advanced.  ld_coef >= 2: the row stride of `coef` in floats (4 for the table above).
 *   step : the same CFG combine and the same layouts as i2v_lcm_cfg_step, then in fp32
 *            x' = x + eps (sigma_to - sigma) + sigma_up z,  z = noise[min(step, n_noise - 1)]
 *          and *step_index advances / wraps as in the DDIM step.  noise fp32 [n_noise][b, f, c, hw], one row per step, n_noise >=
 *          n_steps; a row with sigma_up == 0 does not read it.  noise may be NULL when no row has sigma_up != 0 (Euler): the table is
 *          device memory, so that is the caller's to guarantee -- with NULL every row runs as if sigma_up were 0.  16-byte accesses when
 *          hw % 4 == 0 and latents and noise are 16-byte aligned, scalar ones otherwise. */
int i2v_sigma_prep(float* latents, const float* cond, void* model_in, const float* coef, int32_t ld_coef, int32_t n_steps,
                   const int32_t* step_index, int32_t b, int32_t f, int32_t c, int32_t hw, int32_t c_pad, int32_t cfg_copies,
                   i2v_stream_t stream);
int i2v_euler_cfg_step(float* latents, const float* noise, int32_t n_noise, const void* noise_pred, int32_t np_is_f32, int64_t ld_np,
                       const float* coef, int32_t n_steps, int32_t* step_index, float guidance_scale, int32_t b, int32_t f, int32_t c,
                       int32_t hw, int32_t cfg_copies, i2v_stream_t stream);

/* (ABI 11) FreeU (pipe:155-181 enable_freeu; unet:453-478, 1213-1227: diffusers 0.24 apply_freeu / fourier_filter with threshold 1) on the
 * two operands of an up block's skip concatenation, before `cat([hidden, skip], 1)` (unet:478); one launch, new tensors out (neither
 * input is modified, and no output may alias its input).  hidden [n, h, w, c1], skip [n, h, w, c2] fp16 token-major, dense.
 *   hidden_out[..., :c1 / 2] = hidden[..., :c1 / 2] * b (fp32 product, rounded once); the other channels are copied bit for bit.
 *   skip_out = Re(ifftn(ifftshift(mask * fftshift(fftn(skip))))) over (h, w), mask = s on [h/2-1 : h/2+1, w/2-1 : w/2+1] and 1 elsewhere.
 *     The box holds the four frequencies (k, l) in {0, -1}^2, so
 *       skip_out = skip + (s - 1) / (h w) * Re( sum_{(k, l)} X[k, l] e^{+2 pi i (k y / h + l x / w)} ),  X = DFT of the plane:
 *     seven fp32 sums per (image, channel) plane and one rounding of the corrected value.
 * hidden_lo / hidden_out_lo: NULL together, or the low halves of the precise residual stream's fp16 pair (i2v_gemm_params.c_lo):
 * the product is then taken of hi + lo and written as a pair, and the copied channels keep both halves.
 * I2V_ERR_INVALID_ARG ("not implemented for this problem") for h < 2 or w < 2 -- the reference's box slice wraps there and the
 * four-frequency form does not hold --, h or w > 256, c1 or c2 not a multiple of 8. */
int i2v_freeu_f16(const void* hidden, const void* hidden_lo, void* hidden_out, void* hidden_out_lo, const void* skip, void* skip_out,
                  int32_t n, int32_t h, int32_t w, int32_t c1, int32_t c2, float b, float s, i2v_stream_t stream);

/* (ABI 12) Blend-and-stitch of the tiled VAE (pipe:139-153 enable_vae_tiling / disable_vae_tiling -> diffusers 0.24
 * AutoencoderKL.tiled_decode / tiled_encode: tiles of tile_latent_min_size / tile_sample_min_size every `overlap`, each through the
 * decoder / encoder on its own, then blend_v with the tile above, blend_h with the tile to the left, crop to `limit`, concatenate).
 * One launch per tile writes exactly out[:, :, oy : oy + min(th, limit), ox : ox + min(tw, limit)] of the fp32 NCHW image
 * [n, c, out_h, out_w] and nothing else; it fuses tokens_to_nchw, both blends, the crop and both concatenations.
 *   tile [n, th, tw, ld], up [n, up_h, tw, ld] (the tile above), left [n, th, left_w, ld], upleft [n, up_h, left_w, ld] (the diagonal
 *   one): the RAW outputs of the decoder (fp32, src_is_f32: conv_out with c_is_f32, its real leading dimension) or of quant_conv
 *   (fp16), token-major, first c channels.  NULL = no such neighbour; upleft only together with both up and left.
 * With ev = min(up_h, th, blend_extent), eh = min(left_w, tw, blend_extent), uy = up_h - ev + y, lx = left_w - eh + x and
 * lerp(a, b, w) = a (1 - w) + b w in fp32:
 *   FU  = x < eh ? lerp(upleft[uy, lx], up[uy, x], x / eh) : up[uy, x]        v   = y < ev ? lerp(FU, tile[y, x], y / ev) : tile[y, x]
 *   FL  = y < ev ? lerp(upleft[uy, lx], left[y, lx], y / ev) : left[y, lx]    out = x < eh ? lerp(FL, v, x / eh) : v
 * which equals diffusers' in-place raster-order blends whenever a tile that has a successor is >= 2 blend_extent long (overlap factor
 * <= 1/3: the rows / columns a tile hands on lie outside its own blend zone); no source is modified and the launches of a grid are
 * independent.  Outside the blend zones the source passes through bit for bit.  Sources are read with 16-byte loads along ld when
 * ld is a multiple of 8 (fp16) / 4 (fp32) and the pointers are 16-byte aligned, 12-byte loads for fp32 with ld = c = 3.
 * I2V_ERR_INVALID_ARG: c > ld, limit <= 0, blend_extent <= 0, a crop rectangle that leaves the destination, upleft without up and left. */
int i2v_vae_tile_blend(const void* tile, const void* up, const void* left, const void* upleft, int32_t src_is_f32, int32_t n, int32_t th,
                       int32_t tw, int64_t ld, int32_t c, int32_t up_h, int32_t left_w, int32_t blend_extent, int32_t limit, void* out,
                       int32_t out_h, int32_t out_w, int32_t oy, int32_t ox, i2v_stream_t stream);

/* (ABI 13) LoRA merge (pipe:57 LoraLoaderMixin, unet:108 UNet2DConditionLoadersMixin: load_lora_weights / fuse_lora / the
 * cross_attention_kwargs "scale"): the low-rank updates of up to I2V_LORA_MAX_ADAPTERS adapters folded into ONE weight matrix, one launch,
 *   dst[o, i] = round( base[o, i] + sum_j scale_j * sum_r up_j[o, r] * down_j[r, i] ),   j < n_adapters, r < rank_j.
 * base, dst [out, in] row-major and dense, both fp16 or both fp32 (is_f32); a conv weight [Cout, Cin, kh, kw] is the same problem with
 * in = Cin kh kw (kohya and diffusers store conv LoRAs as down [r, Cin, kh, kw], up [Cout, r, 1, 1]).  dst must not overlap base or a
 * factor; base is not modified.  Every adapter: down fp16 [rank, in], up fp16 [out, rank], dense, 1 <= rank <= I2V_LORA_MAX_RANK.
 * The adapter list is read on the host and travels BY VALUE in the kernel arguments: no device-side table, no allocation, no
 * synchronisation, like every other entry point.
 *   The products run on the MFMA (fp16 in, fp32 accumulate; a rank that is no multiple of the MFMA's k is zero-padded in LDS, not in
 *   memory); scale_j multiplies adapter j's fp32 product (never an fp16 factor); the result is rounded ONCE from the fp32 sum of base and
 *   all adapters, so it does not depend on the order of the adapters beyond fp32 summation.  An element whose low-rank sum is exactly
 *   zero -- n_adapters = 0, all scales 0 -- takes base's bits: -0, subnormals, infinities and NaN payloads come through unchanged.
 * 16-byte loads / stores of base / dst when in is a multiple of 8 (fp16) / 4 (fp32) and both pointers are 16-byte aligned, an
 * element-wise form otherwise (conv_in: 320 x 36); the factors likewise per adapter (rank % 8, in % 8, alignment).
 * I2V_ERR_INVALID_ARG: null pointers, out or in < 1, n_adapters > I2V_LORA_MAX_ADAPTERS, a rank outside 1 .. I2V_LORA_MAX_RANK, dst
 * overlapping base or a factor. */
#define I2V_LORA_MAX_ADAPTERS 8
#define I2V_LORA_MAX_RANK 256
typedef struct i2v_lora_adapter {
  const void* down; /* fp16 [rank, in]  */
  const void* up;   /* fp16 [out, rank] */
  int32_t rank;
  float scale;
} i2v_lora_adapter;
int i2v_lora_merge(void* dst, const void* base, int32_t is_f32, int32_t out, int32_t in, const i2v_lora_adapter* adapters,
                   int32_t n_adapters, i2v_stream_t stream);

/* (ABI 15) FreeInit (https://arxiv.org/abs/2312.07537; diffusers 0.24 FreeInitMixin, `enable_free_init`): the re-initialisation between two
 * sampling rounds of one clip.  All tensors fp32, dense, in the pipeline's latent layout [b, f, c, h, w]; per (b, c) volume over (f, h, w):
 *   z_t = sqrt_alpha * latents + sqrt_one_minus_alpha * init_noise                          (scheduler.add_noise, fused into the load)
 *   out = Re ifftn( ifftshift( fftshift(fftn(z_t)) * lpf + fftshift(fftn(z_rand)) * (1 - lpf) ) )
 *       = z_rand + Re ifftn( ifftshift(lpf) * fftn(z_t - z_rand) )                          (what is computed: one transform pair)
 * latents: the previous round's clean result; init_noise: the noise the first round started from; z_rand: a fresh draw; lpf fp32
 * [f, h, w]: the low-pass table in diffusers' CENTRED layout -- index (t, y, x) multiplies frequency (t - f/2, y - h/2, x - w/2), i.e. the
 * fftshift-ed spectrum.  The table is read as given (built on the host: an "ideal" filter's `<=` must not be re-evaluated in fp32).  At
 * odd sizes the centred table is not symmetric about the zero frequency, so the inverse is a full complex one and its real part is taken
 * last; nothing assumes a Hermitian spectrum.  An all-zero table returns z_rand bit for bit.
 * Every axis is a direct DFT in fp32 FMAs (any length, no radix plan, no FFT library) with per-workgroup twiddle tables indexed by the
 * integer (k n) mod N; five launches: rows forward (z_t - z_rand formed on load), columns forward, frames forward x lpf x frames
 * inverse, columns inverse, rows inverse (+ z_rand).  The complex volume lives in `workspace` (caller-owned, 8-byte aligned, at least
 * i2v_freeinit_workspace_bytes(b, f, c, h, w) = 8 b f c h w bytes, every byte of it written before it is read).
 * I2V_ERR_INVALID_ARG: null pointers, f outside 1..32, h or w outside 1..128, b or c < 1, more than 2^30 values, a workspace that is too
 * small or overlaps an operand, `out` overlapping an input (i2v_freeinit_workspace_bytes returns the same code for bad sizes). */
int64_t i2v_freeinit_workspace_bytes(int32_t b, int32_t f, int32_t c, int32_t h, int32_t w);
int i2v_freeinit_mix(const float* latents, const float* init_noise, const float* z_rand, const float* lpf, float* out, void* workspace,
                     int64_t workspace_bytes, int32_t b, int32_t f, int32_t c, int32_t h, int32_t w, float sqrt_alpha,
                     float sqrt_one_minus_alpha, i2v_stream_t stream);

/* (ABI 16) FreeNoise (https://arxiv.org/abs/2310.15169; diffusers AnimateDiffFreeNoiseMixin.enable_free_noise / FreeNoiseTransformerBlock):
 * clips longer than the motion modules' positional table.  The temporal attention of a motion module runs on sliding windows of `length`
 * frames -- positions restart in every window -- and a frame's result is the weighted mean of the windows that cover it.  A window is a
 * `length`-frame clip of the (b, pixel, frame) row layout, so the existing attention entry points run it unchanged on n_pixels * windows
 * "pixels"; these two entry points move the rows into windows and back.  fp16 rows of c values (c a multiple of 8), unit stride along c,
 * row strides ld_* in elements (multiples of 8, >= c), 16-byte aligned pointers, dst never overlapping src.
 *   i2v_freenoise_gather_f16   src [n_pixels, frames, c] -> dst [n_pixels, windows, length, c]:
 *       dst[p, w, j, :] = src[p, starts[w] + j, :], bit for bit.  starts: DEVICE int32 [windows] (the trailing window is one more entry;
 *       a captured step holds no host value).
 *   i2v_freenoise_blend_f16    src [n_pixels, windows, length, c] -> dst [n_pixels, frames, c]:
 *       dst[p, f, :] = sum_k coef[f, k] * src[p, idx[f, k], :],  idx in [0, windows * length) = w * length + j.
 *       idx DEVICE int32 [frames, pairs], coef DEVICE fp32 [frames, pairs], pairs in 1..33 (ceil(length / stride) + 1); the normalised
 *       coefficients are the host's (fp64, rounded to fp32).  Pair 0 is always read; a later pair with coefficient 0 is padding and is
 *       not read (give it index 0).  fp32 accumulation -- pair 0 as a product, the others as fmas --, one rounding to fp16: a frame whose
 *       only coefficient is 1.0 leaves as the bits of its source row.
 * Both are gathers with one owner per output row (no atomics, no LDS, deterministic) that stream 16 bytes per lane; table entries are
 * clamped to the operand on the device, so a corrupt table cannot cause an access outside it.
 * I2V_ERR_INVALID_ARG: null pointers, n_pixels / windows < 1, length outside 1..frames, windows > frames, c not a multiple of 8, a bad row
 * stride or alignment, 2^31 rows or more, overlapping operands, pairs outside 1..33. */
int i2v_freenoise_gather_f16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, const int32_t* starts, int64_t n_pixels,
                             int32_t frames, int32_t windows, int32_t length, int32_t c, i2v_stream_t stream);
int i2v_freenoise_blend_f16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, const int32_t* idx, const float* coef,
                            int64_t n_pixels, int32_t frames, int32_t windows, int32_t length, int32_t pairs, int32_t c,
                            i2v_stream_t stream);

/* (ABI 17) The CLIP text tower (transformers CLIPTextModel as the pipeline's encode_prompt calls it, pipe:412-453; SD-1.5: 12 pre-LN layers,
 * width 768, 12 heads of 64, 77 tokens).  Its projections and LayerNorms are i2v_gemm_f16 / i2v_layernorm_f16; these are the three kernels the
 * UNet has no use for.  Not per-step work: a prompt is encoded once per sample.
 *   i2v_clip_embed_f16      out[b * len + l, :] = fp16(float(tok[ids[b, l], :]) + float(pos[l, :])).  tok fp16 [vocab, hidden], pos fp16
 *       [max_positions, hidden], out fp16 [batch * len, hidden], all dense.  ids: DEVICE int32 [batch, len]; ids_host: the HOST copy of the same
 *       table, which is what is validated -- an id outside [0, vocab) is rejected before anything is launched (the kernel also clamps what it
 *       reads on the device, so a device table that differs from its host copy gives wrong numbers, never an access outside tok).
 *       I2V_ERR_INVALID_ARG: null pointers, an id out of range, len > max_positions, hidden % 8 != 0, misaligned or overlapping operands.
 *   i2v_clip_attention_f16  causal multi-head self-attention of one short sequence per batch entry:
 *           out[b * len + i, h * 64 + :] = softmax_j<=i( scale * q[b, i, h, :] . k[b, j, h, :] ) v[b, j, h, :]
 *       q, k and v are read in place from the packed result of one QKV GEMM: qkv fp16 [batch * len, ld_qkv], head h of q / k / v of a row in
 *       columns q_off / k_off / v_off + h * 64 (offsets multiples of 8); out fp16 [batch * len, ld_out].  No transposed V, no mask tensor: key j
 *       is visible to query i iff j <= i (and j < len), by index compare, so no row is ever fully masked.  The kernel is
 *       i2v_clip_vision_attention_f16's with the causal mask (csrc/short_attention.hip): grid (batch * heads, ceil(len / 64)), the head's whole K
 *       and V^T staged in LDS, padded to the MFMA tile there only (nothing at or beyond row batch * len is read or written).
 *       Numerics: Q K^T and P V on MFMA with fp32 accumulation, softmax in fp32 in base 2 with the logits scaled by scale * log2(e) in fp32, P
 *       rounded to fp16 for P V, the row sum taken over the unrounded P.
 *       I2V_ERR_UNSUPPORTED: head_dim != 64, len > 128.  I2V_ERR_INVALID_ARG: null / misaligned / overlapping operands, bad strides or offsets.
 *   i2v_quick_gelu_f16      y = fp16(x * sigmoid(1.702 x)) evaluated in fp32 (CLIP's "quick_gelu").  Any n >= 1; y may be x (in place), and may not
 *       overlap it otherwise; 16-byte aligned operands take 16 bytes per lane, the tail and unaligned operands one value per lane. */
int i2v_clip_embed_f16(const void* tok, const void* pos, const int32_t* ids, const int32_t* ids_host, void* out, int32_t batch, int32_t len,
                       int32_t vocab, int32_t max_positions, int32_t hidden, i2v_stream_t stream);
int i2v_clip_attention_f16(const void* qkv, int64_t ld_qkv, int32_t q_off, int32_t k_off, int32_t v_off, void* out, int64_t ld_out,
                           int32_t batch, int32_t len, int32_t heads, int32_t head_dim, float scale, i2v_stream_t stream);
int i2v_quick_gelu_f16(const void* x, void* y, int64_t n, i2v_stream_t stream);

/* (ABI 18) The CLIP vision tower (transformers CLIPVisionModelWithProjection as the pipeline's encode_image calls it, pipe:323-345; IP-Adapter's
 * image encoder, OpenCLIP ViT-H/14: 32 pre-LN layers, width 1280, 16 heads of 80, 256 patches of 14 px + the class token = 257 tokens).  Its
 * projections and LayerNorms are i2v_gemm_f16 / i2v_layernorm_f16, its quick-GELU (ViT-L/14) i2v_quick_gelu_f16; these are the three kernels
 * nothing else has a use for.  Not per-step work: an image is encoded once per sample.
 *   i2v_clip_patchify_f16   the im2col of the patch embedding (a bias-free convolution of kernel = stride = patch): pixel_values fp16
 *       [batch, channels, size, size] dense -> out fp16 [batch * (size / patch)^2, ld_out].  Row b * P + py * (size / patch) + px holds patch
 *       (py, px) in column order (c, dy, dx) -- the order of patch_embedding.weight.flatten(1) -- and columns channels * patch^2 .. ld_out - 1
 *       are written as ZERO, so the embedding is i2v_gemm_f16 against the weight zero-padded to the same row length (ViT-H/14: 588 -> 592, the
 *       GEMM's K % 8 == 0).  ld_out a multiple of 8, >= channels * patch^2.
 *       I2V_ERR_INVALID_ARG: size % patch != 0, null / misaligned / overlapping operands, a bad ld_out; nothing is launched.
 *   i2v_clip_vision_embed_f16   out[b, 0, :] = fp16(float(cls) + float(pos[0])), out[b, 1 + t, :] = fp16(float(patch[b * patches + t]) +
 *       float(pos[1 + t])): cls fp16 [hidden], patch fp16 [batch * patches, ld_patch] (the GEMM's result), pos fp16 [patches + 1, hidden] dense,
 *       out fp16 [batch * (patches + 1), hidden] dense.  hidden % 8 == 0 (one 16-byte chunk per lane).
 *   i2v_clip_vision_attention_f16   NON-causal multi-head self-attention of one sequence per batch entry:
 *           out[b * len + i, h * d + :] = softmax_j<len( scale * q[b, i, h, :] . k[b, j, h, :] ) v[b, j, h, :]
 *       The argument list is i2v_clip_attention_f16's: q, k, v read in place from the packed result of one QKV GEMM (qkv fp16 [batch * len,
 *       ld_qkv], head h of q / k / v in columns q_off / k_off / v_off + h * head_dim, offsets multiples of 8), out fp16 [batch * len, ld_out].
 *       Grid (batch * heads, ceil(len / 64)): a workgroup of 4 waves owns 64 queries and stages the head's whole K (head_dim padded with zeros to
 *       the MFMA K-step, 80 -> 96) and V^T (keys padded with zeros to a multiple of 32) in LDS, 78 KB (d 80: 105 KB).  Key j is visible iff j < len, by index
 *       compare (P of a pad key is exactly 0; key 0 is always visible, so no row is fully masked); rows at or beyond batch * len are never
 *       read, only queries < len are stored.  Numerics as i2v_clip_attention_f16 (the same kernel without the causal mask): MFMA 16x16x32
 *       with fp32 accumulation, softmax in fp32 in base 2 with the logits scaled by scale * log2(e) in fp32, P rounded to fp16 for P V, the
 *       row sum taken over the unrounded P.
 *       I2V_ERR_UNSUPPORTED (nothing launched): head_dim not 64 or 80, len > 288 (L_max: 18 key tiles; ViT-H/14 at 224 px is 257).
 *       I2V_ERR_INVALID_ARG: null / misaligned / overlapping operands, bad strides or offsets. */
int i2v_clip_patchify_f16(const void* pixel_values, void* out, int64_t ld_out, int32_t batch, int32_t channels, int32_t size, int32_t patch,
                          i2v_stream_t stream);
int i2v_clip_vision_embed_f16(const void* cls, const void* patch, int64_t ld_patch, const void* pos, void* out, int32_t batch, int32_t patches,
                              int32_t hidden, i2v_stream_t stream);
int i2v_clip_vision_attention_f16(const void* qkv, int64_t ld_qkv, int32_t q_off, int32_t k_off, int32_t v_off, void* out, int64_t ld_out,
                                  int32_t batch, int32_t len, int32_t heads, int32_t head_dim, float scale, i2v_stream_t stream);

/* (ABI 21) The attention of IP-Adapter Plus's Resampler (diffusers' Resampler / IPAdapterPlusImageProjection, the reference's unet:1234-1239: 16
 * learned queries attend to the 257 penultimate hidden states of the image encoder AND to themselves).  Not per-step work: an image prompt is
 * projected once per sample.
 *   i2v_perceiver_attention_f16   multi-head attention of a short block of queries over the CONCATENATION of two row sources:
 *           out[b * n_q + i, h * 64 + :] = softmax_j( scale * q[b, i, h, :] . k[b, j, h, :] ) v[b, j, h, :],   j < len_a + len_b
 *           k / v[b, j] = row b * len_a + j of source A for j < len_a, row b * len_b + (j - len_a) of source B otherwise
 *       q fp16 [batch * n_q, ld_q], head h in columns q_off + h * 64.  A source is the packed K | V result of a GEMM: fp16 [batch * len, ld],
 *       head h of k / v in columns k_off / v_off + h * 64 (all offsets and strides multiples of 8).  kv_b may be NULL when len_b == 0.  q, A and B
 *       are read-only and MAY ALIAS (in the Resampler B is the latents' packed q | k | v buffer, the memory q is read from); out fp16
 *       [batch * n_q, ld_out] may overlap none of them, and only its rows < batch * n_q, columns < heads * 64 are written.
 *       The kernel is i2v_clip_vision_attention_f16's at head_dim 64 (csrc/short_attention.hip: one kernel for the three entry points), with a
 *       query block of its own and the key rows taken from two sources.
 *       Grid (batch * heads): a workgroup of 4 waves owns all queries of one (batch, head) and stages the head's whole K and V^T (keys padded
 *       with zeros to a multiple of 32) in 78 KB of LDS, A's rows then B's; after that nothing depends on where the A / B boundary was, so the
 *       same keys split differently give bit-equal results.  Key j is visible iff j < len_a + len_b, by index compare; no row beyond a source's
 *       batch * len is read.  Numerics as i2v_clip_vision_attention_f16: MFMA 16x16x32 with fp32 accumulation, softmax in fp32 in base 2 with the
 *       logits scaled by scale * log2(e) in fp32, P rounded to fp16 for P V, the row sum taken over the unrounded P, one rounding at the store.
 *       I2V_ERR_UNSUPPORTED (nothing launched): head_dim != 64, n_q > 64, len_a + len_b > 288.
 *       I2V_ERR_INVALID_ARG (nothing launched): len_a < 1, len_b < 0, null / misaligned operands, out overlapping an input, bad strides or offsets. */
int i2v_perceiver_attention_f16(const void* q, int64_t ld_q, int32_t q_off, const void* kv_a, int64_t ld_a, int32_t ka_off, int32_t va_off,
                                int32_t len_a, const void* kv_b, int64_t ld_b, int32_t kb_off, int32_t vb_off, int32_t len_b, void* out,
                                int64_t ld_out, int32_t batch, int32_t n_q, int32_t heads, int32_t head_dim, float scale, i2v_stream_t stream);

/* (ABI 22) ControlNet residuals (unet:1299-1300: down_block_additional_residuals / mid_block_additional_residual; the adds of unet:329-330,
 * 1379-1389 and 1402-1403): up to I2V_ADD_RES_MAX (skip, residual) pairs of different sizes in one launch,
 *           dst_i = skip_i + s * res_i,     s = scale_table[min(max(step_idx[0], 0), scale_rows - 1)]
 *       scale_table fp32 [scale_rows] and step_idx (one int32) are DEVICE memory, read by the kernel: one captured launch serves a schedule
 *       whose control is on for some steps and off for others.  step_idx NULL: row 0.  scale_table NULL: s = 1.
 *       All tensors fp16, dense, numel values each; dst may be skip (in place) or other memory, and may not overlap anything else.
 *       Arithmetic in fp32 with one rounding to fp16.  Where s * res is exactly zero the skip's bits are kept (s = 0: bit-equal, -0 included).
 *       The precise residual stream (i2v_gemm_params.residual_lo / c_lo): skip_lo / dst_lo both given -- the sum is
 *       (skip + skip_lo) + s * res in fp32, dst = rn16(sum), dst_lo = rn16(sum - dst), so the pair stays a pair.
 *       Grid: at most 2048 workgroups of 256 lanes stride over 16 KB tiles (16 bytes per lane and access); a workgroup finds the tensor of a
 *       tile through prefix sums carried in the launch's own parameter block -- no descriptor table in device memory, no allocation.
 *       I2V_ERR_INVALID_ARG (nothing launched): n outside 1..I2V_ADD_RES_MAX, numel not a positive multiple of 8, a null dst / skip / res,
 *       skip_lo and dst_lo not both given or both null, a pointer that is not 16-byte aligned, scale_table with scale_rows < 1. */
#define I2V_ADD_RES_MAX 16
typedef struct i2v_add_residuals_entry {
  void* dst;
  void* dst_lo;
  const void* skip;
  const void* skip_lo;
  const void* res;
  int64_t numel;
} i2v_add_residuals_entry;
typedef struct i2v_add_residuals_params {
  i2v_add_residuals_entry t[I2V_ADD_RES_MAX];
  int32_t n;
  int32_t scale_rows;
  const float* scale_table;
  const int32_t* step_idx;
} i2v_add_residuals_params;
int i2v_add_residuals_f16(const i2v_add_residuals_params* p, i2v_stream_t stream);

/* (ABI 33) The residuals of several ControlNets (diffusers' MultiControlNetModel) into the UNet's skip tensors in ONE launch: for up to
 * I2V_ADD_RES_MAX tensors and n_nets in 1..I2V_ADD_RES_NETS_MAX nets,
 *           dst_i = skip_i + sum_k s_k * res_k_i,     s_k = scale_table[k * scale_rows + min(max(step_idx[0], 0), scale_rows - 1)]
 *       scale_table fp32 [n_nets, scale_rows] (one row of scale_rows values per net) and step_idx (one int32) are DEVICE memory, read
 *       by the kernel.  step_idx NULL: row 0.  scale_table NULL: every s_k = 1.  res[k] for k >= n_nets is not read.
 *       The skip is read once and written once whatever n_nets is: (n_nets + 2) streams, not the 3 n_nets of one
 *       i2v_add_residuals_f16 launch per net, and one rounding to fp16, not n_nets.
 *       Arithmetic in fp32, every operation rounded on its own (no fused multiply-add): p_k = s_k * res_k, acc = p_0 + p_1 + ... in
 *       net order, dst = rn16(skip + acc); with the precise residual stream (skip_lo / dst_lo both given)
 *       sum = (skip + skip_lo) + acc, dst = rn16(sum), dst_lo = rn16(sum - dst).  Where every p_k is exactly zero the skip's bits (and
 *       its low half's) are kept, -0 included.  Hence, bit for bit: n_nets = 1 is i2v_add_residuals_f16 on the same operands, and a
 *       net whose products are all exactly zero (s_k = 0) changes no bit of what the remaining nets give.
 *       All tensors fp16, dense, numel values each; dst may be skip (in place) and may not overlap anything else, no res in particular.
 *       Grid and tile walk as i2v_add_residuals_f16: at most 2048 workgroups of 256 lanes over 16 KB tiles, the tensor of a tile found
 *       through prefix sums in the launch's own parameter block; one kernel per n_nets.
 *       I2V_ERR_INVALID_ARG (nothing launched): n outside 1..I2V_ADD_RES_MAX, n_nets outside 1..I2V_ADD_RES_NETS_MAX, a null dst / skip /
 *       res[k < n_nets], numel not a positive multiple of 8, a pointer that is not 16-byte aligned, skip_lo and dst_lo not both given or
 *       both null, dst_lo == dst, dst or dst_lo equal to a res, scale_table with scale_rows < 1, scale_table / step_idx not 4-byte
 *       aligned. */
#define I2V_ADD_RES_NETS_MAX 4
typedef struct i2v_add_multi_residuals_entry {
  void* dst;
  void* dst_lo;
  const void* skip;
  const void* skip_lo;
  const void* res[I2V_ADD_RES_NETS_MAX];
  int64_t numel;
} i2v_add_multi_residuals_entry;
typedef struct i2v_add_multi_residuals_params {
  i2v_add_multi_residuals_entry t[I2V_ADD_RES_MAX];
  int32_t n;
  int32_t n_nets;
  int32_t scale_rows;
  const float* scale_table;
  const int32_t* step_idx;
} i2v_add_multi_residuals_params;
int i2v_add_multi_residuals_f16(const i2v_add_multi_residuals_params* p, i2v_stream_t stream);

/* (ABI 23) The layer of AutoencoderTiny (TAESD, diffusers' AutoencoderTiny): a 3x3 / pad 1 / stride 1 convolution with Cin = Cout = 64 on
 * token-major fp16 images [n_img, height, width, 64] and its epilogue in one launch,
 *           out = act_out( act_mid(conv(x) + bias) + residual ),      act = ReLU where relu_mid / relu_out is non-zero, else identity
 *       fp32 arithmetic, one rounding to fp16.  bias (fp16 [64]) and residual are optional.  x, out and residual each have their own pixel
 *       stride (ldx / ldo / ldr, in elements): >= 64, a multiple of 8, bases 16-byte aligned; only the 64 channels of a pixel are touched.
 *       Any height, width >= 1: edge tiles are zero-filled inside the image's own halo and never read the neighbouring image.
 *       w: the weight [64, 64, 3, 3] in the kernel's MFMA-fragment order, 36864 fp16 (`kernels.pack_conv_c64`; Cin < 64 zero-padded):
 *           w[(((tap * 2 + s) * 4 + b) * 64 + 16 g + l) * 8 + j] = W[cout = 32 (b >> 1) + 8 (l >> 2) + 4 (b & 1) + (l & 3)][cin = 32 s + 8 g + j][tap]
 *       out may BE residual (same base and stride); out overlapping x is refused (other workgroups read x as halo).
 *       A halo-tile kernel with the whole weight resident in LDS (120 KB), persistent over 8 x 16-pixel tiles: one workgroup per CU walks
 *       tiles b, b + grid, ...  max_workgroups > 0 caps the grid (a dispatch override: tests drive the multi-tile walk at tiny shapes);
 *       0: one workgroup per CU.  The result does not depend on the grid.
 *       I2V_ERR_INVALID_ARG (nothing launched): null / misaligned operands, cin or cout != 64, a bad stride, out overlapping x, w or (other
 *       than being it) the residual.  I2V_ERR_UNSUPPORTED: the device refuses the kernel its LDS. */
typedef struct i2v_conv_c64_params {
  const void* x;
  int64_t ldx;
  const void* w;
  const void* bias;
  const void* residual;
  int64_t ldr;
  void* out;
  int64_t ldo;
  int32_t n_img, height, width;
  int32_t cin, cout;
  int32_t relu_mid, relu_out;
  int32_t max_workgroups;
} i2v_conv_c64_params;
int i2v_conv3x3_c64_f16(const i2v_conv_c64_params* p, i2v_stream_t stream);
/* (ABI 31) The same layer with a per-channel PReLU in the middle -- the layer of the Real-ESRGAN compact upscaler (SRVGGNetCompact,
 * upscaler.py):
 *           act_mid(v) = v >= 0 ? v : slope[c] * v        in fp32, before the residual add and the single rounding
 *       slope: fp32 [64], non-null, 16-byte aligned.  ReLU and leaky ReLU are this epilogue with slope 0 and 0.1 (slope 1: the plain layer).
 *       The second instantiation of the kernel above: a lane holds the 16 slopes of its channels in registers beside their bias.  relu_mid
 *       must be 0; relu_out, residual, strides, max_workgroups and every argument check are those of i2v_conv3x3_c64_f16.
 *       I2V_ERR_INVALID_ARG in addition: a null or misaligned slope, relu_mid != 0, out overlapping slope. */
int i2v_conv3x3_c64_prelu_f16(const i2v_conv_c64_params* p, const void* slope, i2v_stream_t stream);
/* (ABI 23) AutoencoderTiny's entry mover: src NCHW [n, c, hw] fp32 (src_is_f32) or fp16, c <= 64, through
 *           I2V_TAESD_PREP_IDENTITY  v                 I2V_TAESD_PREP_UNIT  (v + 1) / 2  (the encoder's input)
 *           I2V_TAESD_PREP_CLAMP     3 tanh(v / 3)     (the decoder's latent clamp)
 *           I2V_TAESD_PREP_UNIT_CLAMP  min(max((v + 1) / 2, 0), 1)     (ABI 31: the upscaler's input, [-1, 1] frames to RGB in [0, 1])
 *       in fp32, to token-major fp16 dst [n, hw, 64] with pixel stride ld_dst (>= 64, a multiple of 8, 16-byte aligned base); channels
 *       c .. 63 are written as zeros.  I2V_ERR_INVALID_ARG: null / misaligned / overlapping operands, c outside 1..64, an unknown mode.
 *       (The value 3 stays an unknown mode: ABI 23 .. 30 refuse it and callers may rely on that.) */
#define I2V_TAESD_PREP_IDENTITY 0
#define I2V_TAESD_PREP_UNIT 1
#define I2V_TAESD_PREP_CLAMP 2
#define I2V_TAESD_PREP_UNIT_CLAMP 4
int i2v_taesd_prep_f16(const void* src, int32_t src_is_f32, void* dst, int64_t ld_dst, int32_t n, int32_t c, int32_t hw, int32_t mode,
                       i2v_stream_t stream);
/* (ABI 31) The upscaler's exit (SRVGGNetCompact.forward: PixelShuffle(s)(body(x)) + nearest-upsampled x, then the caller's clamp), one launch:
 *       y: token-major fp16 [n, h, w] pixels of stride ld (>= 64, a multiple of 8, 16-byte aligned base), the exit convolution's result;
 *          channel k = (col * s + dy) * s + dx (PyTorch's PixelShuffle order), k < 3 s^2 -- no other channel is read.
 *       src: the network's NCHW source [n, 3, h, w], fp32 (src_is_f32) or fp16, BEFORE the entry map; entry_mode is that map,
 *          I2V_TAESD_PREP_IDENTITY or I2V_TAESD_PREP_UNIT_CLAMP.       out: NCHW fp32 [n, 3, s h, s w], 16-byte aligned.
 *       In fp32, in this order:   base = entry(src[n, col, y, x]);   v = float(y[n, y, x, k]) + base;   clamp != 0: v = min(max(v, 0), 1);
 *          signed_out != 0: v = 2 v - 1;   out[n, col, s y + dy, s x + dx] = v.        |out - exact| <= 2^-22 (|y| + |base| + 1).
 *       s = 1 .. 4.  One lane owns the s contiguous outputs of one (col, dy) of one input pixel (a 16-byte store at s = 4) and a wave 64
 *       consecutive pixels of a row; a capped grid strides.  Nothing outside out's n * 3 * s h * s w values is written.  No workspace.
 *       I2V_ERR_INVALID_ARG (nothing launched): null / misaligned operands, out overlapping y or src, s outside 1..4, a bad ld, an entry
 *       map other than the two. */
int i2v_pixel_shuffle_add_f32(const void* y, int64_t ld, const void* src, int32_t src_is_f32, float* out, int32_t n, int32_t h, int32_t w,
                              int32_t s, int32_t entry_mode, int32_t clamp, int32_t signed_out, i2v_stream_t stream);

/* (ABI 34) The layer of an RRDBNet dense block (Real-ESRGAN x4plus; upscaler.RRDBNet): a 3x3 / pad 1 / stride 1 convolution of the FIRST cin
 * channels of a token-major fp16 image x [n_img, height, width] (pixel stride ldx >= cin) to cout channels, with a leaky ReLU and two scaled
 * residual stages, one launch:
 *           v = conv(x[..., 0:cin]) + bias;   v = v >= 0 ? v : slope v;   out = fp16( s2 * (s1 * v + r1) + r2 )
 *       fp32 arithmetic in this order, one rounding.  cin: 64, 96, 128, 160 or 192; cout: 32 or 64; slope 1: no activation.  bias (fp16
 *       [cout]), r1 and r2 (token-major fp16, cout channels, strides ldr1 / ldr2) are optional: an absent residual adds 0.  Strides are in
 *       elements, multiples of 8; bases 16-byte aligned.  No channel >= cin of x is read, only the cout channels of out's pixels are written.
 *       A dense block lives in one buffer of 192 channels (no concatenation): out may be OTHER CHANNELS OF x's PIXELS -- the same stride and
 *       a channel offset c0 = ((out - x) mod ldx) with c0 >= cin and c0 + cout <= ldx; any other overlap of out with x is refused (other
 *       workgroups read x as halo).  out may BE r1 or r2 (same base and stride); any other overlap with them, w or bias is refused.
 *       w: [cout, cin, 3, 3] in the kernel's MFMA-fragment order, 9 cin cout fp16 (`kernels.pack_conv_dense`), 32 output channels after 32:
 *           w[((((half * (cin / 32) + chunk) * 9 + tap) * 2 + b) * 64 + 16 g + l) * 8 + j]
 *               = W[cout = 32 half + 8 (l >> 2) + 4 b + (l & 3)][cin = 32 chunk + 8 g + j][tap]
 *       A halo-tile kernel, persistent over 16 x 16-pixel tiles, with the weight of 32 output channels resident in LDS (576 cin bytes) and
 *       the halo staged in double-buffered 32-channel chunks (2 x 21504 bytes): 78 .. 150 KB, one workgroup per CU.  cout 64: even and
 *       odd workgroups own one half each (a single workgroup walks the tiles twice).  max_workgroups > 0 caps the grid, 0: one per CU;
 *       the result does not depend on the grid.
 *       I2V_ERR_INVALID_ARG (nothing launched): null / misaligned operands, cin or cout outside the lists, a bad stride, a refused overlap,
 *       a NaN scalar.  I2V_ERR_UNSUPPORTED: the device refuses the kernel its LDS. */
typedef struct i2v_conv_dense_params {
  const void* x;
  int64_t ldx;
  const void* w;
  const void* bias;
  const void* r1;
  int64_t ldr1;
  const void* r2;
  int64_t ldr2;
  void* out;
  int64_t ldo;
  int32_t n_img, height, width;
  int32_t cin, cout;
  float slope, s1, s2;
  int32_t max_workgroups;
} i2v_conv_dense_params;
int i2v_conv3x3_dense_f16(const i2v_conv_dense_params* p, i2v_stream_t stream);
/* (ABI 34) i2v_conv3x3_c64_prelu_f16 on the nearest-2x upsampling of x, which is never written: p->height and p->width are the OUTPUT's (both
 *       even), x holds n_img images of half that size, and halo pixel (y, x) of the output grid reads source pixel (y >> 1, x >> 1) -- zero
 *       outside the grid.  The third instantiation of the 64-channel kernel; only its fetch differs.  residual and out are at the output size.
 *       Every argument check is that entry's, with x's extent taken at the source size; in addition an odd height or width is refused. */
int i2v_conv3x3_c64_up2_prelu_f16(const i2v_conv_c64_params* p, const void* slope, i2v_stream_t stream);
/* (ABI 34) RRDBNet's exit: y token-major fp16 [n, h, w] pixels of stride ld (>= 3, any), channels 0..2 read -> out NCHW fp32 [n, 3, h, w]:
 *           v = float(y[n, y, x, col]);   clamp != 0: v = min(max(v, 0), 1);   signed_out != 0: v = 2 v - 1        (exact but for 2 v - 1: 2^-24)
 *       I2V_ERR_INVALID_ARG: null / misaligned operands, out overlapping y, ld < 3. */
int i2v_rgb_exit_f32(const void* y, int64_t ld, float* out, int32_t n, int32_t h, int32_t w, int32_t clamp, int32_t signed_out,
                     i2v_stream_t stream);

/* (ABI 24) T2I-Adapter (diffusers 0.24 `T2IAdapter`, adapter_type "full_adapter"; t2i_adapter.py).  The adapter reads the control frames
 * only -- never the latents or the timestep -- so its network runs once per sample and a denoising step adds four stored feature maps to the
 * UNet's down path (down_intrablock_additional_residuals; the hook of unet:329-330).  Three movers of the once-per-sample network and the
 * per-step add.  All four: 16 bytes per lane and access, a capped grid that strides, no workspace, nothing allocated.
 *
 * PixelUnshuffle(8): src NCHW [n, c, h, w] fp32 (src_is_f32) or fp16, c = 1 or 3, h and w multiples of 8 -> tokens fp16
 *       dst [n, h / 8, w / 8, 64 c] with PyTorch's channel order c * 64 + dy * 8 + dx; one rounding (fp32 -> fp16), none for fp16.
 *       I2V_ERR_INVALID_ARG: null / misaligned (16 bytes) / overlapping operands, c not 1 or 3, h or w no positive multiple of 8. */
int i2v_pixel_unshuffle8_f16(const void* src, int32_t src_is_f32, void* dst, int32_t n, int32_t c, int32_t h, int32_t w, i2v_stream_t stream);
/* AvgPool2d(2, stride 2, ceil_mode=True) on tokens: src fp16 [n, h, w, c] -> dst fp16 [n, ceil(h / 2), ceil(w / 2), c], c % 8 == 0.  A window
 *       at the edge of an odd size holds 2 taps or 1 and divides by that count: fp32 sum of the in-bounds taps times 1, 1/2 or 1/4, one
 *       rounding.  I2V_ERR_INVALID_ARG: null / misaligned / overlapping operands, a size < 1, c no positive multiple of 8. */
int i2v_avgpool2x_f16(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c, i2v_stream_t stream);
/* dst = max(src, 0), fp16, numel % 8 == 0; dst may be src (in place) and may not overlap it otherwise. */
int i2v_relu_f16(const void* src, void* dst, int64_t numel, i2v_stream_t stream);
/* The per-step add:   dst[i] = x[i] + s * feat[i mod feat_numel],     s = scale_table[min(max(step_idx[0], 0), scale_rows - 1)]
 *       x, dst fp16 [numel], feat fp16 [feat_numel], numel % feat_numel == 0, feat_numel % 8 == 0: one copy of the features serves every
 *       repetition of the batch (both classifier-free-guidance halves).  scale_table fp32 [scale_rows] and step_idx (one int32) are DEVICE
 *       memory, read by the kernel (a captured launch follows a scale schedule by the step counter); step_idx NULL: row 0; scale_table
 *       NULL: s = 1.  dst may be x (in place); dst may not overlap feat.
 *       Per element the arithmetic is i2v_add_residuals_f16's, and the results are bit-equal to it on feat repeated numel / feat_numel
 *       times: fp32, one rounding to fp16; where s * feat is exactly zero x's bits are kept (-0 included); with x_lo / dst_lo (both or
 *       neither: the precise residual stream) the sum is (x + x_lo) + s * feat, dst = rn16(sum), dst_lo = rn16(sum - dst).
 *       Grid: at most 2048 workgroups of 256 lanes stride over 16 KB tiles, four independent accesses per lane in flight; the wrap point of
 *       feat is chunk-aligned, so no 16-byte access straddles it.
 *       I2V_ERR_INVALID_ARG (nothing launched): a null x / feat / dst, x_lo and dst_lo not both given or both null, numel no multiple of
 *       feat_numel, feat_numel no positive multiple of 8, a pointer not 16-byte aligned, dst overlapping feat, scale_table with scale_rows < 1. */
int i2v_add_broadcast_residual_f16(const void* x, const void* x_lo, const void* feat, void* dst, void* dst_lo, int64_t numel, int64_t feat_numel,
                                   const float* scale_table, int32_t scale_rows, const int32_t* step_idx, i2v_stream_t stream);

/* (ABI 25) Prompt travel (diffusers AnimateDiffFreeNoiseMixin: `prompt` as a dict {frame: text}; pipeline `encode_prompt_travel`): one text
 * context per frame, interpolated between the keyframes' embeddings.
 *       out[r] = (1 - w[r]) * src[lo[r]] + w[r] * src[hi[r]],      r = 0 .. n_out - 1
 *       src fp16 [n_src, e] with row stride ld_src, out fp16 [n_out, e] with row stride ld_out (strides in values, >= e, multiples of 8);
 *       e % 8 == 0: rows are read and written 16 bytes at a time.  lo, hi (int32 [n_out]) and w (fp32 [n_out]) are DEVICE memory.
 *       Arithmetic: fp32, fma(w, src[hi], (1 - w) * src[lo]), one rounding to fp16.  A row with w == 0 is a copy of src[lo] and does not
 *       read src[hi]; a row with w == 1 is a copy of src[hi] and does not read src[lo] -- bit-exact, and whatever the other row holds
 *       (NaN included) does not reach the output.  With w = 0 everywhere the launch is a row gather.
 *       PRECONDITION (not checked: the tables live on the device): 0 <= lo[r], hi[r] < n_src and w[r] finite.  The Python wrapper
 *       builds the tables on the host and checks them before the upload.
 *       Grid: at most 2048 workgroups of 256 lanes stride over the 16-byte chunks of all rows; no workspace, nothing allocated.
 *       I2V_ERR_INVALID_ARG (nothing launched): a null pointer, src / out not 16-byte or a table not 4-byte aligned, n_src or n_out < 1,
 *       e no positive multiple of 8, a stride below e or no multiple of 8, out overlapping src, n_out * e / 8 >= 2^31 - 2^19. */
int i2v_interp_rows_f16(const void* src, int64_t ld_src, int32_t n_src, const int32_t* lo, const int32_t* hi, const float* w, void* out,
                        int64_t ld_out, int32_t n_out, int32_t e, i2v_stream_t stream);

/* (ABI 26) Video-to-video with a mask (diffusers' inpainting update for a 4-channel UNet; pipeline `video=` / `mask_image=`): the one launch
 * inside a denoising step, after the scheduler-step kernel.  In place on the latents:
 *       latents[n, c, p] = m * latents[n, c, p] + (1 - m) * (coef[r][0] * source[n, c, p] + coef[r][1] * noise[n, c, p])
 *       m = mask[n, p]: one mask plane serves all channels; 1 regenerates (the latent stays), 0 keeps the source, any float is taken.
 *       latents, source, noise fp32 [images, channels, hw] and mask fp32 [images, hw], all contiguous; images = batch * frames.
 *       coef fp32 [coef_rows, 2] and step_idx (int32 [1]) are DEVICE memory; r = clamp(step_idx[0], 0, coef_rows - 1).  The kernel READS
 *       the counter and does not advance it.
 *       Table convention: the scheduler-step kernels (i2v_ddim_cfg_step, i2v_dpm_cfg_step, i2v_lcm_cfg_step) have already advanced the
 *       counter when this kernel reads it, and they wrap it to 0 after the last row.  So row 0 = (1, 0): the clean source, after the
 *       last step; row r >= 1 = (sqrt(abar), sqrt(1 - abar)) of timesteps[r], the noise level the next step expects.  A one-step
 *       schedule falls on row 0.
 *       Arithmetic, all fp32: t = coef[r][1] == 0 ? coef[r][0] * source : fma(coef[r][1], noise, coef[r][0] * source), where the
 *       product with coef[r][0] == 1 is the source itself;
 *       m == 1: the latent's bits are kept (nothing is computed: -0 survives, source and noise do not reach the output);
 *       m == 0: the result is t, so with the row (1, 0) it is the source's bits; otherwise fma(1 - m, t, m * latent).
 *       Grid: at most 2048 workgroups of 256 lanes stride over 16 KB tiles of 16-byte chunks, four chunks of every operand in flight
 *       per lane; with hw % 4 != 0 (latent planes such as 5 x 7) every value finds its own mask value and the last numel % 4 values
 *       take a scalar path.  No workspace, nothing allocated.
 *       I2V_ERR_INVALID_ARG (nothing launched): a null pointer, images / channels / hw / coef_rows < 1, latents / source / noise / mask
 *       not 16-byte or coef / step_idx not 4-byte aligned, latents overlapping source, noise or mask,
 *       images * channels * hw >= 2^31 - 2^19. */
int i2v_masked_renoise_f32(float* latents, const float* source, const float* noise, const float* mask, const float* coef, int32_t coef_rows,
                           const int32_t* step_idx, int64_t images, int32_t channels, int32_t hw, i2v_stream_t stream);

/* (ABI 30) Hires fix (pipeline `enable_hires_fix` / `upscale_latents`): the latent upscale between the two passes with the second pass's
 * re-noise fused in.  Once per sample, outside the captured step.
 *       out[p, Y, X] = a * sum_ky sum_kx wy[Y][ky] * wx[X][kx] * src[p, iy[Y][ky], ix[X][kx]]  +  b * noise[p, Y, X]
 *       src fp32 [planes, h, w]; out and noise fp32 [planes, H, W]; planes = batch * frames * channels; all contiguous.
 *       noise may be NULL: then b is ignored and nothing is read for it.
 *       Upscaling only, H >= h and W >= w: every mode then needs at most four taps per axis.  iy int32 [H, 4] / wy fp32 [H, 4] are the
 *       source rows and weights of every output row, ix int32 [W, 4] / wx fp32 [W, 4] those of every output column, DEVICE memory, built
 *       on the host in fp64 and rounded once (hires_fix.resize_tables).  An unused tap has weight 0 and a valid index.  The kernel does
 *       no coordinate arithmetic; it clamps every index into the source plane before use, so a damaged table never reads out of bounds.
 *       Arithmetic, all fp32, nothing contracted: term(ky, kx) = (wy * wx) * src; the 16 terms are added in the order ky outer, kx inner,
 *       from the first term on (15 additions) to r; out = a * r without noise, (a * r) + (b * noise) with it -- the operations of
 *       i2v_axpby_f32, so one fused launch gives the bits of a resize followed by i2v_axpby_f32(out, noise, a, b).
 *       |out - exact| <= 2^-19 (|a| sum |wy| |wx| |src| + |b| |noise|) against fp64 from the same fp32 tables.  A weight of exactly 1
 *       beside zeros (nearest modes; every mode at H == h, W == w) with a == 1 returns the source value (finite sources; -0 becomes +0).
 *       Grid: at most 4096 workgroups of 256 lanes stride over tiles of 512 16-byte chunks of the flat output, one chunk per lane and
 *       step: one 16-byte store and one 16-byte noise load per chunk, the taps through the caches.  With W % 4 != 0 a chunk may straddle
 *       rows and every value finds its own row and column; the last numel % 4 values take a scalar path.  No workspace.
 *       I2V_ERR_INVALID_ARG (nothing launched): a null src / out / table, planes / h / w < 1, H < h or W < w (a downscale), out / noise /
 *       a table not 16-byte or src not 4-byte aligned, planes * H * W >= 2^31 - 2^19, out overlapping src, noise or a table. */
int i2v_resize_renoise_f32(const float* src, float* out, const float* noise, const int32_t* iy, const float* wy, const int32_t* ix,
                           const float* wx, float a, float b, int64_t planes, int32_t h, int32_t w, int32_t H, int32_t W,
                           i2v_stream_t stream);

/* (ABI 27) Prompt weighting (the `(text:1.3)` / `[text]` emphasis syntax of SD-1.5 front ends; pipeline `enable_prompt_weighting` /
 * `encode_weighted_prompt`): every token's embedding times its weight, then the prompt rescaled to its unweighted mean.  Once per sample.
 *       S0[p] = sum src[p, t, c],  S1[p] = sum weights[p, t] * src[p, t, c]      over all tokens * dim values of prompt p, fp32
 *       r[p]  = restore_mean ? S0[p] / S1[p] : exactly 1.0f
 *       out[p, t, c] = fp16_rn((float(src[p, t, c]) * weights[p, t]) * r[p])      two fp32 multiplies in that order, one rounding
 *       src fp16 [n_prompts, tokens, dim] and out the same, token rows ld_src / ld_out values apart (>= dim, multiples of 8; prompt p
 *       starts at row p * tokens); weights fp32 [n_prompts, tokens] contiguous; ratio_out fp32 [n_prompts] or NULL receives r[p].
 *       All DEVICE memory.  dim % 8 == 0: rows are read and written 16 bytes at a time.
 *       A ratio that is not finite (the weights cancel the prompt's mean, or the mean is 0 / 0) is written to ratio_out as it is and
 *       the outputs take r = 1: out = fp16_rn(src * w).  The caller reads ratio_out and decides (the pipeline raises ValueError).
 *       Order of the sums, fixed: per lane over the 16-byte chunks q = lane, lane + 1024, ... (chunk q = token q / (dim / 8), its 8
 *       values in order), then the wave's xor butterfly (1, 2, ... 32), then the 16 waves' partials in wave order.  Repeats are
 *       bit-equal; with all weights 1 S1 is S0's sequence of operations, so r == 1.0f and out equals src bit for bit.
 *       In place: out == src with ld_out == ld_src is allowed (a prompt belongs to one workgroup, whose barrier between the sums and
 *       the apply orders every load of pass 1 before any store of pass 2); any other overlap is refused.
 *       Grid: one workgroup of 1024 lanes per prompt, both passes in it; the apply re-reads src (L2).  No atomics, no workspace.
 *       I2V_ERR_INVALID_ARG (nothing launched): a null src / weights / out, n_prompts or tokens < 1, dim no positive multiple of 8, a
 *       stride below dim or no multiple of 8, src / out not 16-byte or weights / ratio_out not 4-byte aligned, tokens * stride >= 2^31
 *       (the kernel indexes a prompt with 32 bits), out overlapping src other than in place, out overlapping weights or ratio_out. */
int i2v_weight_embeds_f16(const void* src, const float* weights, void* out, float* ratio_out, int32_t n_prompts, int32_t tokens,
                          int32_t dim, int64_t ld_src, int64_t ld_out, int32_t restore_mean, i2v_stream_t stream);

/* First-frame-similarity prior and the initial add_noise of the sampling loop, pipe:647-656:
 *   prior   = mask * GaussianBlur3x3(cond) + (1 - mask) * cond, mask = (mask_uniform < strength), per frame (pipe:648-654)
 *   latents = sqrt_alpha * prior + sqrt_one_minus_alpha * noise                          (scheduler.add_noise, pipe:656)
 * cond fp32 [b, c, h, w]; mask_uniform, noise, latents fp32 [b, f, c, h, w].  The blur is torchvision's
 * GaussianBlur(kernel_size=3) for one sigma (pipe:112): separable taps (k_edge, k_center, k_edge), reflect padding. */
int i2v_first_frame_prior_f32(const float* cond, const float* mask_uniform, const float* noise, float* latents,
                              int32_t b, int32_t f, int32_t c, int32_t h, int32_t w, float k_center, float k_edge,
                              float strength, float sqrt_alpha, float sqrt_one_minus_alpha, i2v_stream_t stream);

/* DiagonalGaussianDistribution.sample() of the VAE encoder (vae.encode(image).latent_dist.sample(), pipe:627):
 * moments fp32 [n, 2 c, hw] = (mean | logvar) along the channel axis; out = mean + exp(0.5 clamp(logvar, -30, 20)) eps,
 * eps / out fp32 [n, c, hw]. */
int i2v_gaussian_sample_f32(const float* moments, const float* eps, float* out, int32_t n, int32_t c, int32_t hw,
                            i2v_stream_t stream);


/* ------------------------------------------------------------------------------------------------
 * Backward kernels of the adapter training step.  The reference trains only
 * i2v_adapter.to_q / to_out (unet:979-1026) through the whole frozen UNet with torch autograd
 * (src/train_image_to_video.py:839-884: forward with enable_cross_frame_attn, MSE without the first frame :848-856,
 * backward, clip, step); these entry points replace the aten backward kernels that autograd dispatches for one
 * I2VAdapterTransformerBlock (i2v:420-565): SDPA backward, native_layer_norm_backward, the GEGLU chunk / gelu backward,
 * bias-gradient sums, mse_loss backward.  Linear dgrad / wgrad are i2v_gemm_f16 over transposed weights / activations.
 * Gradients are fp16 (scaled by the caller's loss scale) except the fp32 statistics and the fp32 bias gradient.
 * ------------------------------------------------------------------------------------------------ */
/* lse[bq][h][l] = log2 sum_j exp2(scale * log2(e) * Q[bq, l, h, :] . K[bq / kv_group, j, h, :]), fp32
 * [batch_q, heads, lq]: the softmax statistic of the forward attention described by p (p->vt, p->o, accumulate are
 * ignored).  The backward recomputes P from it instead of storing the lq x lk scores. */
int i2v_attention_lse_f32(const i2v_attn_params* p, float* lse, i2v_stream_t stream);

/* Flash-attention backward (aten _scaled_dot_product_*_attention_backward behind i2v:468-473, 483-492, 527-532):
 *   P = exp2(scale log2e Q K^T - lse),  dP = dO V^T,  dS = P o (dP - delta),  delta[bq][h][l] = sum_i dO o O
 *   dQ = scale dS K          (one sweep over the keys per 16-query wave)
 *   dK = scale dS^T Q,  dV = P^T dO  summed over the kv_group batch entries that share K / V (the F frames of a clip for
 *                        the cross-frame adapter attention: dK0 / dV0), one sweep over the queries per 16-key wave.
 * q, k, v, dout, dq, dk, dv are token-major [batch][token][heads * head_dim] views (row / batch strides in elements);
 * qt, kt, doutt are channel-major copies [batch][heads * head_dim][token] (i2v_transpose_f16; rows zero-filled up to the
 * next multiple of 8 tokens).  dk = NULL skips the dK / dV sweep (frozen context K / V of the text cross-attention); qt,
 * doutt, dv are then unused.  Any lq, lk (short sequences -- the <= 32 frames of one pixel in the motion modules, batch =
 * pixels -- run with most of a 32-row block masked).  No atomics: gradients are run-to-run identical. */
typedef struct i2v_attn_bwd_params {
  const void* q;     int64_t q_row_stride, q_batch_stride;
  const void* qt;    int64_t qt_row_stride, qt_batch_stride;
  const void* k;     int64_t k_row_stride, k_batch_stride;
  const void* kt;    int64_t kt_row_stride, kt_batch_stride;
  const void* v;     int64_t v_row_stride, v_batch_stride;
  const void* dout;  int64_t do_row_stride, do_batch_stride;
  const void* doutt; int64_t dot_row_stride, dot_batch_stride;
  const float* lse;   /* [batch_q, heads, lq] from i2v_attention_lse_f32 */
  const float* delta; /* [batch_q, heads, lq] from i2v_rowdot_heads_f32(dO, O) */
  void* dq;          int64_t dq_row_stride, dq_batch_stride;
  void* dk;          int64_t dk_row_stride, dk_batch_stride;
  void* dv;          int64_t dv_row_stride, dv_batch_stride;
  int32_t batch_q, kv_group, heads, head_dim, lq, lk;
  float scale;
  int32_t kv_partitions; /* (ABI 6) > 1: the kv_group query batches that share one K / V (the frames of a clip in the cross-frame
                            attention) are dealt to kv_partitions workgroups per key block instead of one -- that form has
                            batch_q / kv_group times fewer workgroups than the self-attention and cannot fill the chip alone;
                            kv_group % kv_partitions == 0.  The partial dK / dV go to dkv_partial and a second kernel sums them
                            into dk / dv (fixed order: run-to-run identical).  0 / 1: off.                                       */
  float* dkv_partial;    /* scratch, fp32 [2][kv_partitions][batch_q / kv_group * lk][heads * head_dim]                       */
} i2v_attn_bwd_params;
int i2v_attention_bwd_f16(const i2v_attn_bwd_params* p, i2v_stream_t stream);

/* (ABI 32) Which kernels an attention-backward problem takes.  i2v_attention_bwd_f16 and i2v_attention_lse_f32 dispatch to 47 kernel
   instantiations: 7 head-dim classes <ks, dt> (<1,2> <2,3> <2,4> <3,5> <3,6> <4,8> <5,10> for head_dim <= 32, 48, 64, 80, 96, 128,
   160), the dQ sweep in the forms DQ1 (one 16-query tile per wave) | DQ2 (two tiles, lq >= 512) | DQ2_LDS (... with the key-side
   operands staged in LDS, lk >= 64), the dK / dV sweep in DKV1 | DKV2 (lk >= 512) | DKV2_LDS32 (lq >= 64) | DKV2_LDS64 (lq >= 128,
   64 staged queries per barrier), the two-tile forms in the classes with dt <= 6 only; the log-sum-exp in LSE (ks 1..5) | LSE_LDS
   (lq >= 512, lk >= 64, ks <= 3).  I2V_ATTN_BWD_LDS=0 turns the LDS-staged forms off, I2V_ATTN_BWD_QB=32 the 64-query stage (both
   read once per process).  The route is decided by the same function the launches follow (there is no second copy of the rules). */
enum { I2V_ATTN_BWD_DQ1 = 0, I2V_ATTN_BWD_DQ2 = 1, I2V_ATTN_BWD_DQ2_LDS = 2 };
enum { I2V_ATTN_BWD_DKV1 = 0, I2V_ATTN_BWD_DKV2 = 1, I2V_ATTN_BWD_DKV2_LDS32 = 2, I2V_ATTN_BWD_DKV2_LDS64 = 3 };
enum { I2V_ATTN_LSE = 0, I2V_ATTN_LSE_LDS = 1 };
enum { I2V_ATTN_BWD_KIND_DQ = 0, I2V_ATTN_BWD_KIND_DKV = 1, I2V_ATTN_BWD_KIND_LSE = 2 };   /* the kernel families of the launch table */

/* (a struct tag only, as i2v_gemm_route) */
struct i2v_attn_bwd_route {
  int32_t ks, dt;         /* the head-dim class: 32-channel contraction steps, 16-channel output tiles                        */
  int32_t dq_form;        /* I2V_ATTN_BWD_DQ*                                                                                 */
  int32_t dkv_form;       /* I2V_ATTN_BWD_DKV*, -1 without the dK / dV sweep                                                  */
  int32_t lse_form;       /* I2V_ATTN_LSE*: the form i2v_attention_lse_f32 takes for the same sizes                           */
  int32_t kv_partitions;  /* the i2v_attn_bwd_params.kv_partitions the library recommends for the sizes (1 = off): a power of
                             two <= 8 dividing kv_group that brings the dK / dV sweep to about one thousand workgroups        */
  int32_t dq_blocks, dkv_blocks; /* grid x of the two sweeps (dkv_blocks 0 without the dK / dV sweep)                         */
};

/* The route i2v_attention_bwd_f16 (need_dkv = 0: called with dk = NULL) and i2v_attention_lse_f32 take for these sizes: pure host
   arithmetic, no pointers, no device call.  The sizes are validated as the launches validate them (< 0: refused). */
int i2v_attention_bwd_route(int32_t batch_q, int32_t kv_group, int32_t heads, int32_t head_dim, int32_t lq, int32_t lk,
                            int32_t need_dkv, struct i2v_attn_bwd_route* route);
/* The route of the calling thread's most recent i2v_attention_bwd_f16 that reached a launch (< 0: none yet).  kv_partitions is the
   count that launch ran with (what the caller passed; 1 when off or without the dK / dV sweep); lse_form is that of the thread's
   most recent i2v_attention_lse_f32, -1 before one. */
int i2v_attention_bwd_last_route(struct i2v_attn_bwd_route* route);
/* 1 if the instantiation that `route` names for the kernel family `kind` (I2V_ATTN_BWD_KIND_*: DQ reads ks, dt, dq_form; DKV ks, dt,
   dkv_form; LSE ks, lse_form) is in the launch table, else 0.  Read from the launch table itself. */
int i2v_attn_bwd_kernel_exists(int32_t kind, const struct i2v_attn_bwd_route* route);

/* dst[b][c][r] = src[b][r][c] for r < rows, c < cols (fp16; strides in elements); dst columns [rows, rows rounded up to 8)
 * are zero-filled (ld_dst must cover them).  Channel-major copies of token-major activations: the K^T / Q^T / dO^T
 * operands of i2v_attention_bwd_f16 and the operands of a weight gradient dW = dY^T X as i2v_gemm_f16(a = dY^T, w = X^T). */
int i2v_transpose_f16(const void* src, int64_t src_batch_stride, int64_t ld_src, void* dst, int64_t dst_batch_stride,
                      int64_t ld_dst, int32_t batches, int32_t rows, int32_t cols, i2v_stream_t stream);
/* out[(b * heads + h) * rows_per_batch + l] = sum_i a[b * rows_per_batch + l][h * head_dim + i] * b[..][..], fp32:
 * delta = rowsum(dO o O) per head. */
int i2v_rowdot_heads_f32(const void* a, int64_t lda, const void* b, int64_t ldb, float* out, int64_t rows,
                         int32_t rows_per_batch, int32_t heads, int32_t head_dim, i2v_stream_t stream);
/* LayerNorm backward, input gradient only (the norms are frozen; native_layer_norm_backward behind i2v:445, 514, 539):
 * dx[r] = rstd (gy - mean(gy) - xh mean(gy o xh)) + add[r], gy = dn o gamma, xh = (x - mean) rstd; add (the gradient
 * arriving over the residual path) may be NULL. */
int i2v_layernorm_bwd_f16(const void* x, int64_t ldx, const void* dn, int64_t lddn, const void* gamma, const void* add,
                          int64_t ldadd, void* dx, int64_t lddx, int32_t rows, int32_t C, float eps, i2v_stream_t stream);
/* GEGLU backward (i2v:554): h [rows, 2 inner] is the pre-activation in the interleaved (value_i, gate_i) column order of
 * I2V_EPI_GEGLU, dy [rows, inner] -> dh[.., 2i] = dy gelu(gate), dh[.., 2i + 1] = dy value gelu'(gate). */
int i2v_geglu_bwd_f16(const void* h, int64_t ldh, const void* dy, int64_t lddy, void* dh, int64_t lddh, int64_t rows,
                      int32_t inner, i2v_stream_t stream);
/* GEGLU forward from a stored pre-activation (ABI 6): y[r][i] = h[r][2 i] gelu_erf(h[r][2 i + 1]), h [rows][>= 2 inner] with
 * (value, gate) interleaved as the I2V_EPI_GEGLU GEMM packs its weights, y [rows][>= inner]; inner % 8 == 0.  The training
 * forward keeps h for i2v_geglu_bwd_f16 and derives y from it (diffusers GEGLU.forward, i2v:554). */
int i2v_geglu_f16(const void* h, int64_t ldh, void* y, int64_t ldy, int64_t rows, int32_t inner, i2v_stream_t stream);
/* out[c] += sum_r x[r][c], fp32 (the bias gradient of a Linear; the caller zeroes out before the first call). */
int i2v_colsum_f32(const void* x, int64_t ldx, float* out, int64_t rows, int32_t cols, i2v_stream_t stream);
/* out[c] += sum_r a[r][c] b[r][c], fp32: the gain gradient of a LayerNorm / GroupNorm, d gamma = sum dy o xhat -- the
 * motion modules' norms train under `--update_motion_modules` (train_image_to_video.py:452, 669; unet:984-999). */
int i2v_colsum_prod_f32(const void* a, int64_t lda, const void* b, int64_t ldb, float* out, int64_t rows, int32_t cols,
                        i2v_stream_t stream);
/* Both sums with a result that does not depend on block scheduling (the two above add their 256-row block sums with fp32
 * atomics): out[c] += sum_r a[r][c] (b == NULL) or sum_r a[r][c] b[r][c]; the block sums go to `workspace`
 * (i2v_colsum_workspace_bytes(rows, cols) bytes) and are added in block order.  What the training step uses: every
 * data-parallel rank and every rerun gets the same bias / gain gradients bit for bit. */
int64_t i2v_colsum_workspace_bytes(int64_t rows, int32_t cols);
int i2v_colsum_det_f32(const void* a, int64_t lda, const void* b, int64_t ldb, float* out, int64_t rows, int32_t cols,
                       void* workspace, i2v_stream_t stream);
/* Seed gradient of the training loss (train_image_to_video.py:848-856: MSE summed over every frame but the first of each
 * clip, divided by the number of unmasked elements): grad[img][l][c] = coef (y - target) for img % frames != 0, else 0;
 * coef = 2 * loss_scale / count is the caller's.  y, target, grad fp16 [n_img, tokens, channels]. */
int i2v_masked_mse_grad_f16(const void* y, const void* target, void* grad, int64_t n_img, int32_t tokens, int32_t channels,
                            int32_t frames, float coef, i2v_stream_t stream);
/* The same seed from an fp32 prediction and an fp32 target -- F.mse_loss(model_pred.float(), target.float()),
 * train_image_to_video.py:848 -- with grad in fp16 and rowsq[img * tokens + l] = sum_c (y - target)^2 (0 on masked rows): the
 * loss is sum(rowsq) / count, summed by the caller in a fixed order. */
int i2v_masked_mse_grad_f32(const float* y, const float* target, void* grad, float* rowsq, int64_t n_img, int32_t tokens,
                            int32_t channels, int32_t frames, float coef, i2v_stream_t stream);
/* GroupNorm (+SiLU) backward, input gradient only (native_group_norm_backward + silu_backward behind ResnetBlock2D norm1 /
 * norm2, Transformer2D norm, the motion modules' clip-wide norm and conv_norm_out; the norms are frozen): p describes the
 * FORWARD call (x [, x2], gamma, beta, n_img, hw, groups, frames_per_stat, eps, silu; y and out_perm unused), dy is the
 * gradient of its output [n_img, hw, c1 + c2]; dx [n_img, hw, c1] (and dx2 [.., c2] for a channel-concatenated input).
 * The forward statistics are recomputed (the inference forward keeps none).  workspace: fp32,
 * i2v_groupnorm_bwd_workspace_bytes(...) bytes. */
int64_t i2v_groupnorm_bwd_workspace_bytes(int32_t n_img, int32_t hw, int32_t channels);
int i2v_groupnorm_bwd_f16(const i2v_gn_params* p, const void* dy, void* dx, void* dx2, i2v_stream_t stream);
/* out = a + b over n fp16 elements (n % 8 == 0): gradients meeting at a skip connection (unet:478) or a residual branch. */
int i2v_add_f16(const void* a, const void* b, void* out, int64_t n, i2v_stream_t stream);
/* row permutation (batch, frame, pixel) <-> (batch, pixel, frame) of [batches * frames * hw, channels] fp16 (the motion
 * modules run in pixel-major row order; to_pixel_major = 1: dst row (b hw + p) F + f = src row (b F + f) hw + p). */
int i2v_permute_rows_f16(const void* src, void* dst, int64_t batches, int32_t frames, int32_t hw, int32_t channels,
                         int32_t to_pixel_major, i2v_stream_t stream);
/* dst [n, 2h, 2w, C]: dst[2y][2x] = src[y][x], zero elsewhere: the input gradient of Downsample2D's stride-2 convolution
 * (unet:250-259) is the stride-1 convolution of this tensor with the flipped, transposed weights. */
int i2v_zero_insert2x_f16(const void* src, void* dst, int64_t n_img, int32_t h, int32_t w, int32_t channels, i2v_stream_t stream);
/* dst [n, h, w, C] = sums of the 2 x 2 blocks of src [n, 2h, 2w, C]: input gradient of Upsample2D's nearest-2x (unet:431-432). */
int i2v_sum_pool2x_f16(const void* src, void* dst, int64_t n_img, int32_t h, int32_t w, int32_t channels, i2v_stream_t stream);
/* Optimiser step of the adapter parameters (train_image_to_video.py:876-882: clip_grad_norm_, AdamW.step) over ONE flat fp32
 * bucket (the same bucket the RCCL all-reduce sums): i2v_sumsq_f32 adds sum x^2 into *out (zeroed by the caller);
 * i2v_adamw_f32 is torch.optim.AdamW's update (decoupled weight decay, bias correction with `step` >= 1) on
 * g = grad * grad_coef * min(1, max_norm / (sqrt(*norm_sq) * grad_coef + 1e-6)): grad_coef folds 1 / loss_scale and the
 * data-parallel mean, the clip coefficient is read from device memory (no host round trip); norm_sq = NULL or
 * max_norm <= 0: no clipping. */
int i2v_sumsq_f32(const float* x, int64_t n, float* out, i2v_stream_t stream);
int i2v_adamw_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int32_t step, float grad_coef, const float* norm_sq,
                  float max_norm, i2v_stream_t stream);

/* The same step as ONE call that is safe under fp16 loss scaling and identical on every data-parallel rank
 * (train_image_to_video.py:306-308 `--mixed_precision fp16`: accelerate's GradScaler skips a step whose gradients hold
 * inf / NaN; :876-882 clip + step): sum grad^2 as per-workgroup partials (`partials`, fp32 [n_partials <= 1024]) summed
 * in a fixed order into *norm_sq -- no atomics, so every rank derives the same clip coefficient from the same all-reduced
 * bucket --; a non-finite norm sets *found_inf = 1 and the update is a no-op (parameters, both moments and the
 * bias-correction step unchanged), otherwise *found_inf = 0, *applied_steps += 1 and AdamW runs with bias correction
 * 1 - beta^(*applied_steps).  The caller reads *found_inf when it wants to back its loss scale off; nothing here syncs. */
int i2v_adamw_guarded_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                          float beta1, float beta2, float eps, float weight_decay, float grad_coef, float max_norm,
                          float* partials, int32_t n_partials, float* norm_sq, int32_t* applied_steps, int32_t* found_inf,
                          i2v_stream_t stream);

/* y = a y + b x over n fp32 values: gradient accumulation over micro-batches (`accelerator.accumulate`,
 * train_image_to_video.py:486, 785: a = 1, b = 1 / gradient_accumulation_steps) and the exponential moving average of the
 * trained weights (`--use_ema`, :673-677, 888-889: a = decay, b = 1 - decay). */
int i2v_axpby_f32(float* y, const float* x, float a, float b, int64_t n, i2v_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Model handle (ABI 8; whole-model forward since ABI 9): the layer of SURVEY 8(b) over the entry points above for a host that is
 * NOT this package's Python mirror -- it serves `self.unet = unet`, `self.unet(latent_model_input, t, ...)` and the hipGraph per
 * DDIM step (pipe:96, 676-683; unet:1289-1451).
 *
 * The handle owns (a) the model's configuration, (b) a registry of the caller's weight buffers by key, (c) the step's problem
 * (i2v_unet_plan), (d) a LAUNCH PLAN of one forward for that problem and (e) optionally one captured step.
 *
 * The launch plan (i2v_unet_set_plan) is the forward of unet:1289-1451 as data: the exact sequence of this header's entry points
 * one `UNetMotionCrossFrameAttnModel.forward` issues for the planned problem -- entry-point id + its parameter struct (or flat
 * arguments) per launch -- with every device pointer replaced by a relocation:
 *     weight  (key index, byte offset)   resolved through the registry (i2v_unet_set_weight), so `set_weight` decides what the
 *                                        forward reads.  Keys are the KERNEL-LAYOUT packs of the host mirror
 *                                        (`<module path>#<pack name>`: conv weights in contraction order, GEGLU rows interleaved,
 *                                        LayerNorm-folded projections, MFMA-fragment-ordered operands of the fused kernels ...),
 *                                        exported once, offline, with the plan (handle.py `record_forward_plan`,
 *                                        `export_weights`); no packing arithmetic happens at run time
 *     arena   (byte offset)              an activation / workspace inside ONE caller-owned arena of i2v_unet_activation_bytes()
 *                                        bytes (i2v_unet_set_workspace): the recorded allocation pattern of the forward
 *     io      (slot, byte offset)        one of the forward's arguments (I2V_IO_*)
 * i2v_unet_forward resolves them and issues the launches in C on the caller's stream: no Python, no torch, no allocation, no
 * synchronisation -- capturable between i2v_unet_capture_step and i2v_unet_end_capture together with the host's own DDIM update
 * (i2v_ddim_prep / i2v_ddim_cfg_step).  The plan is made by recording the host mirror once per (problem, switches) in the build
 * environment -- the sequencing logic of blocks.py / kernels.py is not duplicated in C++.
 * One handle per (device, stream); not thread-safe; no call synchronises the device except i2v_unet_destroy's release of the graph.
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2v_unet i2v_unet;
typedef struct i2v_unet_config {
  int32_t in_channels, out_channels;                 /* 4, 4 (unet:701-702) */
  int32_t block_out_channels[4];                     /* 320, 640, 1280, 1280 (unet:708) */
  int32_t layers_per_block, num_attention_heads;     /* 2, 8 */
  int32_t cross_attention_dim, norm_num_groups;      /* 768, 32 */
  int32_t motion_max_seq_length, motion_num_attention_heads;   /* 32, 8 (unet:725-726) */
  int32_t use_motion_mid_block, ip_num_tokens;       /* 1; 0 = no IP-Adapter, else 4 (unet:1284-1287) */
} i2v_unet_config;
typedef struct i2v_unet_plan_t {
  int32_t batch, frames, height, width;              /* latent sizes: batch counts the CFG copies */
  int32_t ctx_len, has_ip;
} i2v_unet_plan_t;
#define I2V_DTYPE_F16 0
#define I2V_DTYPE_F32 1
/* the forward's arguments as relocation slots of a launch plan */
enum { I2V_IO_SAMPLE = 0, I2V_IO_TIMESTEPS = 1, I2V_IO_CONTEXT = 2, I2V_IO_IMAGE_EMBEDS = 3, I2V_IO_OUT = 4, I2V_IO_SLOTS = 5 };

int i2v_unet_create(const i2v_unet_config* cfg, i2v_unet** out);
int i2v_unet_destroy(i2v_unet* h);
/* registers (or replaces) the caller's buffer for a key; ndim <= 4.  The library never copies or frees it. */
int i2v_unet_set_weight(i2v_unet* h, const char* key, const void* ptr, int32_t dtype, int32_t ndim, const int64_t* shape);
/* the registered buffer of a key (0 and *ptr = NULL when absent); shape may be NULL */
int i2v_unet_get_weight(const i2v_unet* h, const char* key, const void** ptr, int32_t* dtype, int32_t* ndim, int64_t* shape);
int64_t i2v_unet_num_weights(const i2v_unet* h);
/* validates and records the step's problem: frames <= motion_max_seq_length (unet:725), positive sizes (latent sizes that are
 * not multiples of 8 take the forward_upsample_size path, unet:1304-1311: a matter of the recorded plan), ctx_len >= 1; a new
 * problem drops the launch plan and the captured step */
int i2v_unet_plan(i2v_unet* h, const i2v_unet_plan_t* plan);
/* (ABI 9) installs a launch plan (the blob handle.py `record_forward_plan` writes; copied).  Checked: magic / version, the ABI
 * version it was recorded against, sizeof of every parameter struct it carries, entry-point ids, relocation targets inside their
 * payloads, and that it was recorded for exactly the planned problem (i2v_unet_plan first).  Drops the captured step. */
int i2v_unet_set_plan(i2v_unet* h, const void* blob, int64_t bytes);
/* bytes of the ONE arena the installed plan's activations and workspaces live in (0 without a plan) */
int64_t i2v_unet_activation_bytes(const i2v_unet* h);
/* launches of the installed plan / distinct weight keys it names (0 without a plan); the i-th key (NULL out of range) */
int32_t i2v_unet_plan_launches(const i2v_unet* h);
int32_t i2v_unet_plan_num_keys(const i2v_unet* h);
const char* i2v_unet_plan_key(const i2v_unet* h, int32_t i);
/* the caller's arena: >= i2v_unet_activation_bytes() bytes, 256-byte aligned, alive as long as forwards / a captured step use it */
int i2v_unet_set_workspace(i2v_unet* h, void* arena, int64_t bytes);
/* (ABI 9) unet:1289-1451 for the planned problem: sample fp16 [batch, frames, in_channels, height, width], timesteps fp32 [batch],
 * context fp16 [batch, ctx_len, cross_attention_dim], image_embeds fp16 [batch, clip_dim] or NULL (needed iff the plan was
 * recorded with the IP-Adapter), out [batch, frames, out_channels, height, width] in the sample's dtype.  Asynchronous on `stream`.
 * I2V_ERR_INVALID_ARG: no plan / arena, a weight key of the plan that is not registered (named in i2v_last_error), a NULL
 * argument the plan reads; errors of the launches themselves are returned as they come. */
int i2v_unet_forward(i2v_unet* h, const void* sample, const void* timesteps, const void* context, const void* image_embeds,
                     void* out, i2v_stream_t stream);
/* (ABI 9) the general form: runs the installed plan with `io[slot]` as its arguments (n_io <= I2V_IO_SLOTS; the rest NULL).
 * i2v_unet_forward is i2v_unet_run with {sample, timesteps, context, image_embeds, out}.  Plans of OTHER launch sequences of the host
 * mirror use it with their own slot meaning (handle.py `record_plan`): the per-sample preparation (context K / V^T of the 16
 * cross-attention layers + the time-embedding table of the schedule; `record_prepare_plan`) and one whole DDIM step -- i2v_ddim_prep,
 * the UNet on the CFG batch as the pipeline routes it, i2v_ddim_cfg_step, pipe:666-697 -- (`record_step_plan`), whose per-sample
 * buffers are registered by name like weights (`sample#...`).  tests/c_host/denoise_host.c runs the reference's whole denoising
 * loop (pipe:663-700) that way. */
int i2v_unet_run(i2v_unet* h, const void* const* io, int32_t n_io, i2v_stream_t stream);
/* begin / end the capture of one step on `stream` (hipStreamBeginCapture, relaxed mode): everything launched on the stream in
 * between -- i2v_unet_forward and the host's DDIM kernels -- becomes the handle's step; i2v_unet_abort_capture ends a capture
 * whose launches failed and discards it */
int i2v_unet_capture_step(i2v_unet* h, i2v_stream_t stream);
int i2v_unet_end_capture(i2v_unet* h);
int i2v_unet_abort_capture(i2v_unet* h);
/* launch the captured step once (asynchronous on `stream`); I2V_ERR_INVALID_ARG when nothing has been captured */
int i2v_unet_replay_step(i2v_unet* h, i2v_stream_t stream);
int32_t i2v_unet_has_step(const i2v_unet* h);

#ifdef __cplusplus
}
#endif
#endif /* I2V_HIP_H */
