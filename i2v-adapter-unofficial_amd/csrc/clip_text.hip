// The CLIP text tower's three own kernels (transformers CLIPTextModel as the pipeline calls it, pipe:412-453): everything else of the
// tower -- the QKV / out / fc1 / fc2 projections, the LayerNorms -- runs on the GEMM and LayerNorm entry points the UNet uses.
//
//   embed        out[b*L + l, :] = fp16(float(tok[ids[b, l], :]) + float(pos[l, :]))      one 16-byte chunk of one row per lane
//   attention    causal multi-head self-attention of a short sequence (L <= 128, head_dim 64), q / k / v read in place from the packed
//                [B*L, 3*hidden] result of one QKV GEMM
//   quick-GELU   y = fp16(x * sigmoid(1.702 x)) in fp32, any n, in place or not
//
// None of this is per-step work: a prompt is encoded once per sample, 2 x 77 tokens.  The kernels are written to be obviously inside
// their operands, not to be fast -- the whole tower is launch-latency bound.
//
// The attention kernel.  One workgroup of 4 waves per (batch, head).  The head's Q and K slices go to LDS row-major (rows padded to the
// MFMA tile, L = 77 -> 80; 72 halves per row, so the 16 rows of a fragment read start in different banks), V goes to LDS TRANSPOSED
// (Vt[d][key], key padded to a multiple of 32).  Rows at and beyond L are never read from memory: their LDS image is zero.  A wave owns
// 16 query rows at a time (query tile qt = wave, wave + 4) and the key tiles 0 .. qt (tiles right of the diagonal are not computed):
//
//   S^T = K Q^T      A = K rows (lane: key l & 15, d 8 (l >> 4) + j), B = Q rows (lane: query l & 15, same d): two MFMAs per 16 x 16 tile.
//                    D: lane holds S^T[key 4 (l >> 4) + r][query l & 15] -- a lane's 4 values of a tile are 4 CONSECUTIVE KEYS of ONE QUERY.
//   softmax          over a query's keys = over the lane's registers and the 4 lanes l ^ 16, l ^ 32, l ^ 48 (two permlane swaps): fp32, base 2,
//                    logits scaled by scale * log2(e) IN FP32 (Q is not rescaled).  Key j is visible to query i iff j <= i && j < L, by index
//                    compare; an invisible logit is -inf, its P exactly 0.  Key 0 is visible to every query: no row is fully masked.
//   O^T = V^T P^T    the MFMA's summation index k is only a label both operands must agree on: k = 8 (l >> 4) + j  <->  key 32 tp + 4 (l >> 4) + j
//                    (j < 4), 32 tp + 16 + 4 (l >> 4) + j - 4 (j >= 4) makes the B operand exactly the 8 fp16-rounded P values the lane already
//                    holds from key tiles 2 tp and 2 tp + 1 -- P never goes through LDS -- and the A operand two 8-byte reads of a Vt row.  An odd
//                    tile count is completed by a tile of zeros (P = 0 against Vt's zero padding, which is finite by construction).
//                    D: lane holds O^T[d 4 (l >> 4) + r][query l & 15] -- the same query as its softmax denominator, 4 consecutive d: one 8-byte store.
//
// Only queries < L are stored.  A pad query's column is computed (on finite numbers) and dropped.
#include "common.h"

namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_MAX_BLOCKS = 256 * 8;

__global__ __launch_bounds__(CT_THREADS) void clip_embed_kernel(const f16* __restrict__ tok, const f16* __restrict__ pos,
                                                                const int32_t* __restrict__ ids, f16* __restrict__ out, int len, int vocab,
                                                                int chunks, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CT_THREADS) {
    const int row = (int)(i / chunks), ch = (int)(i - (int64_t)row * chunks);
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);      // the host has checked its copy; a device table that differs cannot leave tok
    const int l = row % len;
    const f16x8 t = ld_global_16B(tok + ((int64_t)id * chunks + ch) * 8);
    const f16x8 p = ld_global_16B(pos + ((int64_t)l * chunks + ch) * 8);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)((float)t[e] + (float)p[e]);
    *reinterpret_cast<f16x8*>(out + i * 8) = o;
  }
}

__device__ __forceinline__ float quick_gelu_f(float x) { return x / (1.0f + __expf(-1.702f * x)); }

// nvec 16-byte chunks on the vector path (0 when a pointer is not 16-byte aligned), the rest one value per lane
__global__ __launch_bounds__(CT_THREADS) void quick_gelu_kernel(const f16* x, f16* y, int64_t nvec, int64_t n) {
  const int64_t t0 = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x, step = (int64_t)gridDim.x * CT_THREADS;
  for (int64_t i = t0; i < nvec; i += step) {
    const f16x8 v = ld_global_16B(x + i * 8);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)quick_gelu_f((float)v[e]);
    *reinterpret_cast<f16x8*>(y + i * 8) = o;
  }
  for (int64_t i = nvec * 8 + t0; i < n; i += step) y[i] = (f16)quick_gelu_f((float)x[i]);
}

constexpr int CA_D = 64;          // head_dim
constexpr int CA_MAX_L = 128;
constexpr int CA_LDQ = CA_D + 8;  // halves per Q / K row in LDS
constexpr int CA_LDV = CA_MAX_L + 8;  // halves per Vt row in LDS

__global__ __launch_bounds__(CT_THREADS) void clip_attention_kernel(const f16* __restrict__ qkv, int64_t ld, int q_off, int k_off, int v_off,
                                                                    f16* __restrict__ out, int64_t ldo, int len, int heads, float c) {
  __shared__ __attribute__((aligned(16))) f16 Qs[CA_MAX_L * CA_LDQ];
  __shared__ __attribute__((aligned(16))) f16 Ks[CA_MAX_L * CA_LDQ];
  __shared__ __attribute__((aligned(16))) f16 Vt[CA_D * CA_LDV];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int lp = (len + 15) & ~15, lk = (len + 31) & ~31;            // query / key rows padded to the tile: <= 128
  const f16* base = qkv + (int64_t)b * len * ld + h * CA_D;

  for (int i = tid; i < lp * 8; i += CT_THREADS) {
    const int row = i >> 3, ch = i & 7;
    f16x8 q = zero8(), k = zero8();
    if (row < len) {
      q = ld_global_16B(base + (int64_t)row * ld + q_off + 8 * ch);
      k = ld_global_16B(base + (int64_t)row * ld + k_off + 8 * ch);
    }
    *reinterpret_cast<f16x8*>(&Qs[row * CA_LDQ + 8 * ch]) = q;
    *reinterpret_cast<f16x8*>(&Ks[row * CA_LDQ + 8 * ch]) = k;
  }
  for (int i = tid; i < lk * 8; i += CT_THREADS) {
    const int row = i >> 3, ch = i & 7;
    f16x8 v = zero8();
    if (row < len) v = ld_global_16B(base + (int64_t)row * ld + v_off + 8 * ch);
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(8 * ch + e) * CA_LDV + row] = v[e];
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
  const float ninf = -__builtin_inff();
  for (int qt = wave; qt < (lp >> 4); qt += CT_THREADS / 64) {            // wave-uniform: every lane of a wave is active below
    const int query = qt * 16 + c16;
    const f16x8 q0 = *reinterpret_cast<const f16x8*>(&Qs[query * CA_LDQ + 8 * g]);
    const f16x8 q1 = *reinterpret_cast<const f16x8*>(&Qs[query * CA_LDQ + 32 + 8 * g]);
    f32x4 s[8];
    float m = ninf;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      s[kt] = f32x4{ninf, ninf, ninf, ninf};
      if (kt <= qt) {
        const f16x8 k0 = *reinterpret_cast<const f16x8*>(&Ks[(kt * 16 + c16) * CA_LDQ + 8 * g]);
        const f16x8 k1 = *reinterpret_cast<const f16x8*>(&Ks[(kt * 16 + c16) * CA_LDQ + 32 + 8 * g]);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = mfma16x16x32(k0, q0, acc);
        acc = mfma16x16x32(k1, q1, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kt * 16 + 4 * g + r;
          const float v = (key <= query && key < len) ? acc[r] * c : ninf;
          s[kt][r] = v;
          m = fmaxf(m, v);
        }
      }
    }
    m = lane_xor32_max(lane_xor16_max(m));                               // finite: key 0 is visible to every query
    float lsum = 0.f;
    f16x8 pf[4];
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float sv = s[2 * tp + (j >> 2)][j & 3];
        const float p = sv == ninf ? 0.f : __builtin_amdgcn_exp2f(sv - m);
        lsum += p;
        pf[tp][j] = (f16)p;
      }
    }
    lsum = lane_xor32_sum(lane_xor16_sum(lsum));
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
      if (2 * tp <= qt) {                                                // keys < 32 tp + 32 <= lk: inside Vt's zero-padded rows
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const f16* vrow = &Vt[(dt * 16 + c16) * CA_LDV + 32 * tp + 4 * g];
          const f16x4 lo = *reinterpret_cast<const f16x4*>(vrow), hi = *reinterpret_cast<const f16x4*>(vrow + 16);
          const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[dt] = mfma16x16x32(vf, pf[tp], o[dt]);
        }
      }
    }
    if (query < len) {
      const float inv = 1.0f / lsum;
      f16* orow = out + ((int64_t)b * len + query) * ldo + h * CA_D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        f16x4 w;
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = (f16)(o[dt][r] * inv);
        *reinterpret_cast<f16x4*>(orow + dt * 16) = w;
      }
    }
  }
}

inline bool ct_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool ct_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}
inline unsigned ct_grid(int64_t items) {
  const int64_t g = i2v_cdiv(items, CT_THREADS);
  return (unsigned)(g < 1 ? 1 : (g < CT_MAX_BLOCKS ? g : CT_MAX_BLOCKS));
}

}  // namespace

extern "C" int i2v_clip_embed_f16(const void* tok, const void* pos, const int32_t* ids, const int32_t* ids_host, void* out, int32_t batch,
                                  int32_t len, int32_t vocab, int32_t max_positions, int32_t hidden, i2v_stream_t stream) {
  I2V_CHECK_ARG(tok && pos && ids && ids_host && out, "i2v_clip_embed_f16: null pointer");
  I2V_CHECK_ARG(batch > 0 && len > 0 && vocab > 0 && max_positions > 0, "i2v_clip_embed_f16: batch %d len %d vocab %d max_positions %d must be positive",
                batch, len, vocab, max_positions);
  I2V_CHECK_ARG(len <= max_positions, "i2v_clip_embed_f16: %d tokens for a position table of %d rows", len, max_positions);
  I2V_CHECK_ARG(hidden > 0 && hidden % 8 == 0, "i2v_clip_embed_f16: hidden %d must be a positive multiple of 8", hidden);
  I2V_CHECK_ARG((int64_t)batch * len < ((int64_t)1 << 31), "i2v_clip_embed_f16: problem too large (%lld rows)", (long long)batch * len);
  I2V_CHECK_ARG(ct_al16(tok) && ct_al16(pos) && ct_al16(out), "i2v_clip_embed_f16: pointers must be 16-byte aligned");
  const int64_t rows = (int64_t)batch * len;
  for (int64_t i = 0; i < rows; ++i)
    I2V_CHECK_ARG(ids_host[i] >= 0 && ids_host[i] < vocab, "i2v_clip_embed_f16: token id %d at (%lld, %lld) is outside the vocabulary of %d",
                  ids_host[i], (long long)(i / len), (long long)(i % len), vocab);
  const int64_t out_bytes = rows * hidden * 2;
  I2V_CHECK_ARG(!ct_overlap(out, out_bytes, tok, (int64_t)vocab * hidden * 2) && !ct_overlap(out, out_bytes, pos, (int64_t)max_positions * hidden * 2) &&
                    !ct_overlap(out, out_bytes, ids, rows * 4),
                "i2v_clip_embed_f16: out is a new tensor (it must not overlap the tables or the ids)");
  const int chunks = hidden / 8;
  const int64_t total = rows * chunks;
  hipLaunchKernelGGL(clip_embed_kernel, dim3(ct_grid(total)), dim3(CT_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(tok), reinterpret_cast<const f16*>(pos), ids, reinterpret_cast<f16*>(out), len, vocab, chunks,
                     total);
  return i2v_check_launch("i2v_clip_embed_f16");
}

extern "C" int i2v_clip_attention_f16(const void* qkv, int64_t ld_qkv, int32_t q_off, int32_t k_off, int32_t v_off, void* out, int64_t ld_out,
                                      int32_t batch, int32_t len, int32_t heads, int32_t head_dim, float scale, i2v_stream_t stream) {
  I2V_CHECK_ARG(qkv && out, "i2v_clip_attention_f16: null pointer");
  I2V_CHECK_ARG(batch > 0 && heads > 0 && len > 0 && head_dim > 0, "i2v_clip_attention_f16: batch %d heads %d len %d head_dim %d must be positive",
                batch, heads, len, head_dim);
  if (head_dim != CA_D) I2V_FAIL(I2V_ERR_UNSUPPORTED, "i2v_clip_attention_f16: head_dim %d is not supported (only %d)", head_dim, CA_D);
  if (len > CA_MAX_L) I2V_FAIL(I2V_ERR_UNSUPPORTED, "i2v_clip_attention_f16: %d positions are not supported (at most %d)", len, CA_MAX_L);
  const int64_t hidden = (int64_t)heads * CA_D;
  I2V_CHECK_ARG(hidden < (1 << 20) && (int64_t)batch * heads < ((int64_t)1 << 31) && (int64_t)batch * len < ((int64_t)1 << 31),
                "i2v_clip_attention_f16: problem too large (batch %d, heads %d)", batch, heads);
  I2V_CHECK_ARG(q_off >= 0 && k_off >= 0 && v_off >= 0 && q_off % 8 == 0 && k_off % 8 == 0 && v_off % 8 == 0,
                "i2v_clip_attention_f16: column offsets %d / %d / %d must be non-negative multiples of 8", q_off, k_off, v_off);
  I2V_CHECK_ARG(ld_qkv % 8 == 0 && ld_qkv < ((int64_t)1 << 24) && q_off + hidden <= ld_qkv && k_off + hidden <= ld_qkv && v_off + hidden <= ld_qkv,
                "i2v_clip_attention_f16: row stride %lld must be a multiple of 8 that holds every offset + heads * head_dim", (long long)ld_qkv);
  I2V_CHECK_ARG(ld_out % 8 == 0 && ld_out >= hidden && ld_out < ((int64_t)1 << 24), "i2v_clip_attention_f16: out row stride %lld must be a multiple of 8, "
                "at least heads * head_dim", (long long)ld_out);
  I2V_CHECK_ARG(ct_al16(qkv) && ct_al16(out), "i2v_clip_attention_f16: pointers must be 16-byte aligned");
  I2V_CHECK_ARG(scale > 0.f && scale < 3.0e38f,"i2v_clip_attention_f16: scale must be positive and finite");
  const int64_t rows = (int64_t)batch * len;
  I2V_CHECK_ARG(!ct_overlap(qkv, rows * ld_qkv * 2, out, ((rows - 1) * ld_out + hidden) * 2),
                "i2v_clip_attention_f16: out is a new tensor (it must not overlap qkv)");
  hipLaunchKernelGGL(clip_attention_kernel, dim3((unsigned)(batch * heads)), dim3(CT_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(qkv), ld_qkv, q_off, k_off, v_off, reinterpret_cast<f16*>(out), ld_out, len, heads,
                     scale * 1.44269504088896340736f);
  return i2v_check_launch("i2v_clip_attention_f16");
}

extern "C" int i2v_quick_gelu_f16(const void* x, void* y, int64_t n, i2v_stream_t stream) {
  I2V_CHECK_ARG(x && y, "i2v_quick_gelu_f16: null pointer");
  I2V_CHECK_ARG(n > 0 && n < ((int64_t)1 << 40), "i2v_quick_gelu_f16: n %lld must be in [1, 2^40)", (long long)n);
  I2V_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 1) == 0, "i2v_quick_gelu_f16: pointers must be 2-byte aligned");
  I2V_CHECK_ARG(x == y || !ct_overlap(x, n * 2, y, n * 2), "i2v_quick_gelu_f16: y is x (in place) or does not overlap it");
  const int64_t nvec = (ct_al16(x) && ct_al16(y)) ? n / 8 : 0;
  const int64_t items = nvec > n - nvec * 8 ? nvec : n - nvec * 8;
  hipLaunchKernelGGL(quick_gelu_kernel, dim3(ct_grid(items)), dim3(CT_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(x), reinterpret_cast<f16*>(y), nvec, n);
  return i2v_check_launch("i2v_quick_gelu_f16");
}
