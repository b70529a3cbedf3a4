// The CLIP vision tower's three own kernels (transformers CLIPVisionModelWithProjection as the pipeline's encode_image calls it, pipe:323-345;
// IP-Adapter's image encoder is OpenCLIP ViT-H/14: 32 pre-LN layers, width 1280, 16 heads of 80, 16 x 16 patches of 14 px + a class token
// = 257 tokens).  Everything else of the tower -- the patch embedding itself, the q|k|v / out / fc1 / fc2 projections, the LayerNorms,
// the visual projection -- runs on the GEMM and LayerNorm entry points the UNet uses.
//
//   patchify     pixel_values [B, C, S, S] -> rows [B * (S/p)^2, ld]: row b P + py (S/p) + px is patch (py, px) in column order (c, dy, dx)
//                (the order of patch_embedding.weight.flatten(1)), columns C p p .. ld - 1 written as zero: the im2col of the strided
//                convolution, so that the patch embedding is one GEMM against the weight zero-padded to the same ld
//   embed        out[b, 0, :] = fp16(float(cls) + float(pos[0])), out[b, 1 + t, :] = fp16(float(patch[b P + t]) + float(pos[1 + t])):
//                one 16-byte chunk of one row per lane
//   attention    NON-causal multi-head self-attention of one sequence per batch entry, len <= CV_MAX_L = 288 (18 key tiles; ViT-H/14 at
//                224 px has 257 tokens), head_dim 64 or 80, q / k / v read in place from the packed [B * L, 3 * hidden] result of one
//                QKV GEMM
//
// None of this is per-step work: an image is encoded once per sample.  The kernels are written to be obviously inside their operands,
// not to be fast.
//
// The attention kernel.  Grid (batch * heads, query blocks): a workgroup of 4 waves owns 64 queries of one (batch, head), a wave one
// tile of 16 of them -- ViT-H at batch 1 is 16 x 5 = 80 workgroups instead of 16.  Every workgroup stages the head's WHOLE K and V in
// LDS (a head's K and V are 2 x 257 x 80 halves = 82 KB, read from L2 by the 5 workgroups that share them): K row-major with the head
// dimension padded to the MFMA K-step with ZEROS (d 80 -> 96: 2.5 steps become 3; rows of 96 + 8 halves, so the 16 rows of a fragment
// read start in different banks), V TRANSPOSED (Vt[d][key], keys padded to a multiple of 32 with zeros).  Rows at and beyond len are
// never read from memory: their LDS image is zero.  Q does not go through LDS: a lane reads the 16-byte chunks of its own query row
// that its A / B fragment holds (zero for a pad query and for the pad of d).
//
//   S^T = K Q^T      A = K rows (lane: key l & 15, d 32 ks + 8 (l >> 4) + j), B = Q rows (lane: query l & 15, same d): DP / 32 MFMAs per
//                    16 x 16 tile.  D: lane holds S^T[key 4 (l >> 4) + r][query l & 15]: 4 consecutive keys of one query.
//   softmax          over a query's keys = over the lane's registers and the lanes l ^ 16, l ^ 32, l ^ 48: fp32, base 2, logits scaled
//                    by scale * log2(e) IN FP32 (Q is not rescaled).  Key j is visible iff j < len, by index compare; an invisible
//                    logit is -inf, its P exactly 0.  Key 0 is visible to every query: no row is fully masked, the row sum is > 0.
//   O^T = V^T P^T    as in clip_text.hip: the summation index k = 8 (l >> 4) + j stands for key 32 tp + 4 (l >> 4) + j (j < 4),
//                    32 tp + 16 + 4 (l >> 4) + j - 4 (j >= 4), which makes the B operand the 8 fp16-rounded P values the lane already
//                    holds from key tiles 2 tp and 2 tp + 1 and the A operand two 8-byte reads of a Vt row.  An odd tile count (257
//                    tokens = 17 tiles) is completed by a tile of zeros: P = 0 against Vt's zero padding, finite by construction.
//                    D: lane holds O^T[d 4 (l >> 4) + r][query l & 15]: one 8-byte store per 16 channels.
//
// Only queries < len are stored.  A pad query's column is computed (on finite numbers) and dropped.
#include "common.h"

namespace {

constexpr int CV_THREADS = 256;
constexpr int CV_MAX_BLOCKS = 256 * 8;
constexpr int CV_MAX_L = 288;                       // 18 key tiles = 9 pairs
constexpr int CV_KT = CV_MAX_L / 16;
constexpr int CV_LDV = CV_MAX_L + 8;                // halves per Vt row in LDS
constexpr int CV_QPW = 16 * (CV_THREADS / 64);      // queries per workgroup

template <int D>
struct cv_lds {
  static constexpr int DP = (D + 31) & ~31;         // head_dim padded to the MFMA K-step: 64, 96
  static constexpr int LDK = DP + 8;                // halves per K row in LDS
  static constexpr int K_HALVES = CV_MAX_L * LDK;
  static constexpr int V_HALVES = D * CV_LDV;
  static constexpr size_t BYTES = (size_t)(K_HALVES + V_HALVES) * sizeof(f16);
};

__global__ __launch_bounds__(CV_THREADS) void clip_patchify_kernel(const f16* __restrict__ px, f16* __restrict__ out, int64_t ld, int ch_row,
                                                                   int chans, int size, int patch, int grid, int64_t total) {
  const int kk = chans * patch * patch, pp = patch * patch;
  for (int64_t i = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CV_THREADS) {
    const int64_t row = i / ch_row;
    const int ch = (int)(i - row * ch_row);
    const int b = (int)(row / (grid * grid)), t = (int)(row - (int64_t)b * grid * grid);
    const int py = t / grid, pxi = t - py * grid;
    const f16* img = px + (int64_t)b * chans * size * size + (int64_t)(py * patch) * size + pxi * patch;
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = 8 * ch + e;
      f16 v = (f16)0.f;
      if (col < kk) {
        const int c = col / pp, r = col - c * pp, dy = r / patch, dx = r - dy * patch;
        v = img[((int64_t)c * size + dy) * size + dx];
      }
      o[e] = v;
    }
    *reinterpret_cast<f16x8*>(out + row * ld + 8 * ch) = o;
  }
}

__global__ __launch_bounds__(CV_THREADS) void clip_vision_embed_kernel(const f16* __restrict__ cls, const f16* __restrict__ patch, int64_t ldp,
                                                                       const f16* __restrict__ pos, f16* __restrict__ out, int patches,
                                                                       int chunks, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CV_THREADS) {
    const int64_t row = i / chunks;
    const int ch = (int)(i - row * chunks);
    const int b = (int)(row / (patches + 1)), l = (int)(row - (int64_t)b * (patches + 1));
    const f16x8 x = l == 0 ? ld_global_16B(cls + 8 * ch) : ld_global_16B(patch + ((int64_t)b * patches + l - 1) * ldp + 8 * ch);
    const f16x8 p = ld_global_16B(pos + ((int64_t)l * chunks + ch) * 8);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)((float)x[e] + (float)p[e]);
    *reinterpret_cast<f16x8*>(out + i * 8) = o;
  }
}

template <int D>
__global__ __launch_bounds__(CV_THREADS) void clip_vision_attention_kernel(const f16* __restrict__ qkv, int64_t ld, int q_off, int k_off,
                                                                           int v_off, f16* __restrict__ out, int64_t ldo, int len, int heads,
                                                                           float c) {
  using L = cv_lds<D>;
  constexpr int DP = L::DP, LDK = L::LDK, KS = DP / 32, DT = D / 16, DCH = D / 8;
  static_assert(D % 16 == 0 && CV_MAX_L % 32 == 0, "whole output tiles per head, whole key-tile pairs");
  // K [CV_MAX_L][LDK] | Vt [D][CV_LDV]: 116736 bytes at d = 80, 115200 at d = 64 -- one workgroup per CU
  static_assert(L::BYTES <= 160 * 1024, "K and Vt of one head must fit gfx950's 160 KB of LDS");
  extern __shared__ __attribute__((aligned(16))) f16 cv_smem[];
  f16* Ks = cv_smem;
  f16* Vt = cv_smem + L::K_HALVES;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int lp = (len + 15) & ~15, lk = (len + 31) & ~31;            // key rows padded to the tile / the tile pair: <= CV_MAX_L
  const f16* base = qkv + (int64_t)b * len * ld + h * D;

  for (int i = tid; i < lp * (DP / 8); i += CV_THREADS) {
    const int row = i / (DP / 8), ch = i - row * (DP / 8);
    f16x8 k = zero8();
    if (row < len && ch < DCH) k = ld_global_16B(base + (int64_t)row * ld + k_off + 8 * ch);
    *reinterpret_cast<f16x8*>(&Ks[row * LDK + 8 * ch]) = k;
  }
  for (int i = tid; i < lk * DCH; i += CV_THREADS) {
    const int row = i / DCH, ch = i - row * DCH;
    f16x8 v = zero8();
    if (row < len) v = ld_global_16B(base + (int64_t)row * ld + v_off + 8 * ch);
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(8 * ch + e) * CV_LDV + row] = v[e];
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
  const int qt = blockIdx.y * (CV_THREADS / 64) + wave, nkt = lp >> 4;
  if (qt >= nkt) return;                                               // wave-uniform, after the only barrier
  const float ninf = -__builtin_inff();
  const int query = qt * 16 + c16;
  f16x8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = zero8();
    if (query < len && 32 * ks + 8 * g < D) qf[ks] = ld_global_16B(base + (int64_t)query * ld + q_off + 32 * ks + 8 * g);
  }
  f32x4 s[CV_KT];
  float m = ninf;
#pragma unroll
  for (int kt = 0; kt < CV_KT; ++kt) {
    s[kt] = f32x4{ninf, ninf, ninf, ninf};
    if (kt < nkt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        acc = mfma16x16x32(*reinterpret_cast<const f16x8*>(&Ks[(kt * 16 + c16) * LDK + 32 * ks + 8 * g]), qf[ks], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = (kt * 16 + 4 * g + r < len) ? acc[r] * c : ninf;
        s[kt][r] = v;
        m = fmaxf(m, v);
      }
    }
  }
  m = lane_xor32_max(lane_xor16_max(m));                               // finite: key 0 is visible to every query
  float lsum = 0.f;
  f16x8 pf[CV_KT / 2];
#pragma unroll
  for (int tp = 0; tp < CV_KT / 2; ++tp) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float sv = s[2 * tp + (j >> 2)][j & 3];
      const float p = sv == ninf ? 0.f : __builtin_amdgcn_exp2f(sv - m);
      lsum += p;
      pf[tp][j] = (f16)p;
    }
  }
  lsum = lane_xor32_sum(lane_xor16_sum(lsum));                         // > 0 without a guard: key 0 contributes exp2(s0 - m) > 0 or is the max
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tp = 0; tp < CV_KT / 2; ++tp) {
    if (2 * tp < nkt) {                                                // keys < 32 tp + 32 <= lk: inside Vt's zero-padded rows
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const f16* vrow = &Vt[(dt * 16 + c16) * CV_LDV + 32 * tp + 4 * g];
        const f16x4 lo = *reinterpret_cast<const f16x4*>(vrow), hi = *reinterpret_cast<const f16x4*>(vrow + 16);
        const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[dt] = mfma16x16x32(vf, pf[tp], o[dt]);
      }
    }
  }
  if (query < len) {
    const float inv = 1.0f / lsum;
    f16* orow = out + ((int64_t)b * len + query) * ldo + h * D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      f16x4 w;
#pragma unroll
      for (int r = 0; r < 4; ++r) w[r] = (f16)(o[dt][r] * inv);
      *reinterpret_cast<f16x4*>(orow + dt * 16) = w;
    }
  }
}

inline bool cv_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool cv_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}
inline unsigned cv_grid(int64_t items) {
  const int64_t g = i2v_cdiv(items, CV_THREADS);
  return (unsigned)(g < 1 ? 1 : (g < CV_MAX_BLOCKS ? g : CV_MAX_BLOCKS));
}

template <int D>
int cv_launch_attention(const void* qkv, int64_t ld_qkv, int q_off, int k_off, int v_off, void* out, int64_t ld_out, int batch, int len,
                        int heads, float scale, hipStream_t s) {
  if (i2v_big_lds_kernel_cus(reinterpret_cast<const void*>(clip_vision_attention_kernel<D>), cv_lds<D>::BYTES) <= 0)
    I2V_FAIL(I2V_ERR_LAUNCH, "i2v_clip_vision_attention_f16: the device refuses %zu bytes of LDS per workgroup", cv_lds<D>::BYTES);
  const int qblocks = (int)i2v_cdiv(len, CV_QPW);
  hipLaunchKernelGGL(clip_vision_attention_kernel<D>, dim3((unsigned)(batch * heads), (unsigned)qblocks), dim3(CV_THREADS), cv_lds<D>::BYTES, s,
                     reinterpret_cast<const f16*>(qkv), ld_qkv, q_off, k_off, v_off, reinterpret_cast<f16*>(out), ld_out, len, heads,
                     scale * 1.44269504088896340736f);
  return i2v_check_launch("i2v_clip_vision_attention_f16");
}

}  // namespace

extern "C" int i2v_clip_patchify_f16(const void* pixel_values, void* out, int64_t ld_out, int32_t batch, int32_t channels, int32_t size,
                                     int32_t patch, i2v_stream_t stream) {
  I2V_CHECK_ARG(pixel_values && out, "i2v_clip_patchify_f16: null pointer");
  I2V_CHECK_ARG(batch > 0 && channels > 0 && size > 0 && patch > 0, "i2v_clip_patchify_f16: batch %d channels %d size %d patch %d must be positive",
                batch, channels, size, patch);
  I2V_CHECK_ARG(size <= 4096 && patch <= 256 && channels <= 64, "i2v_clip_patchify_f16: size %d patch %d channels %d too large", size, patch, channels);
  I2V_CHECK_ARG(size % patch == 0, "i2v_clip_patchify_f16: image size %d is not a multiple of the patch size %d", size, patch);
  const int grid = size / patch;
  const int64_t kk = (int64_t)channels * patch * patch, rows = (int64_t)batch * grid * grid;
  I2V_CHECK_ARG(ld_out % 8 == 0 && ld_out >= kk && ld_out < ((int64_t)1 << 24),
                "i2v_clip_patchify_f16: out row stride %lld must be a multiple of 8, at least channels * patch * patch = %lld", (long long)ld_out,
                (long long)kk);
  I2V_CHECK_ARG(rows < ((int64_t)1 << 31) && (int64_t)batch * channels * size * size < ((int64_t)1 << 40), "i2v_clip_patchify_f16: problem too large");
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(pixel_values) & 1) == 0 && cv_al16(out),
                "i2v_clip_patchify_f16: pixel_values must be 2-byte, out 16-byte aligned");
  I2V_CHECK_ARG(!cv_overlap(out, rows * ld_out * 2, pixel_values, (int64_t)batch * channels * size * size * 2),
                "i2v_clip_patchify_f16: out is a new tensor (it must not overlap pixel_values)");
  const int ch_row = (int)(ld_out / 8);
  const int64_t total = rows * ch_row;
  hipLaunchKernelGGL(clip_patchify_kernel, dim3(cv_grid(total)), dim3(CV_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(pixel_values), reinterpret_cast<f16*>(out), ld_out, ch_row, channels, size, patch, grid, total);
  return i2v_check_launch("i2v_clip_patchify_f16");
}

extern "C" int i2v_clip_vision_embed_f16(const void* cls, const void* patch, int64_t ld_patch, const void* pos, void* out, int32_t batch,
                                         int32_t patches, int32_t hidden, i2v_stream_t stream) {
  I2V_CHECK_ARG(cls && patch && pos && out, "i2v_clip_vision_embed_f16: null pointer");
  I2V_CHECK_ARG(batch > 0 && patches > 0, "i2v_clip_vision_embed_f16: batch %d patches %d must be positive", batch, patches);
  I2V_CHECK_ARG(hidden > 0 && hidden % 8 == 0, "i2v_clip_vision_embed_f16: hidden %d must be a positive multiple of 8", hidden);
  I2V_CHECK_ARG(ld_patch % 8 == 0 && ld_patch >= hidden && ld_patch < ((int64_t)1 << 24),
                "i2v_clip_vision_embed_f16: patch row stride %lld must be a multiple of 8, at least hidden", (long long)ld_patch);
  I2V_CHECK_ARG((int64_t)batch * (patches + 1) < ((int64_t)1 << 31), "i2v_clip_vision_embed_f16: problem too large (%lld rows)",
                (long long)batch * (patches + 1));
  I2V_CHECK_ARG(cv_al16(cls) && cv_al16(patch) && cv_al16(pos) && cv_al16(out), "i2v_clip_vision_embed_f16: pointers must be 16-byte aligned");
  const int64_t rows = (int64_t)batch * (patches + 1), out_bytes = rows * hidden * 2;
  I2V_CHECK_ARG(!cv_overlap(out, out_bytes, cls, (int64_t)hidden * 2) && !cv_overlap(out, out_bytes, pos, (int64_t)(patches + 1) * hidden * 2) &&
                    !cv_overlap(out, out_bytes, patch, (((int64_t)batch * patches - 1) * ld_patch + hidden) * 2),
                "i2v_clip_vision_embed_f16: out is a new tensor (it must not overlap the class token, the patches or the position table)");
  const int chunks = hidden / 8;
  const int64_t total = rows * chunks;
  hipLaunchKernelGGL(clip_vision_embed_kernel, dim3(cv_grid(total)), dim3(CV_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(cls), reinterpret_cast<const f16*>(patch), ld_patch, reinterpret_cast<const f16*>(pos),
                     reinterpret_cast<f16*>(out), patches, chunks, total);
  return i2v_check_launch("i2v_clip_vision_embed_f16");
}

extern "C" int i2v_clip_vision_attention_f16(const void* qkv, int64_t ld_qkv, int32_t q_off, int32_t k_off, int32_t v_off, void* out,
                                             int64_t ld_out, int32_t batch, int32_t len, int32_t heads, int32_t head_dim, float scale,
                                             i2v_stream_t stream) {
  I2V_CHECK_ARG(qkv && out, "i2v_clip_vision_attention_f16: null pointer");
  I2V_CHECK_ARG(batch > 0 && heads > 0 && len > 0 && head_dim > 0, "i2v_clip_vision_attention_f16: batch %d heads %d len %d head_dim %d must be positive",
                batch, heads, len, head_dim);
  if (head_dim != 64 && head_dim != 80)
    I2V_FAIL(I2V_ERR_UNSUPPORTED, "i2v_clip_vision_attention_f16: head_dim %d is not supported (64 and 80)", head_dim);
  if (len > CV_MAX_L) I2V_FAIL(I2V_ERR_UNSUPPORTED, "i2v_clip_vision_attention_f16: %d tokens are not supported (at most %d)", len, CV_MAX_L);
  const int64_t hidden = (int64_t)heads * head_dim;
  I2V_CHECK_ARG(hidden < (1 << 20) && (int64_t)batch * heads < ((int64_t)1 << 31) && (int64_t)batch * len < ((int64_t)1 << 31),
                "i2v_clip_vision_attention_f16: problem too large (batch %d, heads %d)", batch, heads);
  I2V_CHECK_ARG(q_off >= 0 && k_off >= 0 && v_off >= 0 && q_off % 8 == 0 && k_off % 8 == 0 && v_off % 8 == 0,
                "i2v_clip_vision_attention_f16: column offsets %d / %d / %d must be non-negative multiples of 8", q_off, k_off, v_off);
  I2V_CHECK_ARG(ld_qkv % 8 == 0 && ld_qkv < ((int64_t)1 << 24) && q_off + hidden <= ld_qkv && k_off + hidden <= ld_qkv && v_off + hidden <= ld_qkv,
                "i2v_clip_vision_attention_f16: row stride %lld must be a multiple of 8 that holds every offset + heads * head_dim", (long long)ld_qkv);
  I2V_CHECK_ARG(ld_out % 8 == 0 && ld_out >= hidden && ld_out < ((int64_t)1 << 24), "i2v_clip_vision_attention_f16: out row stride %lld must be a "
                "multiple of 8, at least heads * head_dim", (long long)ld_out);
  I2V_CHECK_ARG(cv_al16(qkv) && cv_al16(out), "i2v_clip_vision_attention_f16: pointers must be 16-byte aligned");
  I2V_CHECK_ARG(scale > 0.f && scale < 3.0e38f, "i2v_clip_vision_attention_f16: scale must be positive and finite");
  const int64_t rows = (int64_t)batch * len;
  I2V_CHECK_ARG(!cv_overlap(qkv, rows * ld_qkv * 2, out, ((rows - 1) * ld_out + hidden) * 2),
                "i2v_clip_vision_attention_f16: out is a new tensor (it must not overlap qkv)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (head_dim == 64) return cv_launch_attention<64>(qkv, ld_qkv, q_off, k_off, v_off, out, ld_out, batch, len, heads, scale, s);
  return cv_launch_attention<80>(qkv, ld_qkv, q_off, k_off, v_off, out, ld_out, batch, len, heads, scale, s);
}
