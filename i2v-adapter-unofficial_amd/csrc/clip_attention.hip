// The attention kernel of both CLIP towers: multi-head self-attention of one short sequence per batch entry, q / k / v read in place
// from the packed [B * L, 3 * hidden] result of one QKV GEMM.  One template, three instantiations, two entry points:
//
//   i2v_clip_attention_f16          <64, causal>                  the text tower (clip_text.py): head_dim 64, len <= 128
//   i2v_clip_vision_attention_f16   <64, not causal>, <80, ...>   the vision tower (clip_vision.py): head_dim 64 or 80, len <= CA_MAX_L = 288
//                                                                 (18 key tiles; ViT-H/14 at 224 px has 257 tokens)
//
// None of this is per-step work: a prompt and an image are encoded once per sample.  The kernel is written to be obviously inside its
// operands, not to be fast.
//
// Grid (batch * heads, query blocks): a workgroup of 4 waves owns 64 queries of one (batch, head), a wave one tile of 16 of them --
// ViT-H at batch 1 is 16 x 5 = 80 workgroups instead of 16.  Every workgroup stages the head's WHOLE K and V in LDS (a head's K and V
// are 2 x 257 x 80 halves = 82 KB, read from L2 by the 5 workgroups that share them): K row-major with the head dimension padded to the
// MFMA K-step with ZEROS (d 80 -> 96: 2.5 steps become 3; rows of DP + 8 halves, so the 16 rows of a fragment read start in different
// banks), V TRANSPOSED (Vt[d][key], keys padded to a multiple of 32 with zeros).  Rows at and beyond len are never read from memory:
// their LDS image is zero.  Q does not go through LDS: a lane reads the 16-byte chunks of its own query row that its A / B fragment
// holds (zero for a pad query and for the pad of d).
//
//   S^T = K Q^T      A = K rows (lane: key l & 15, d 32 ks + 8 (l >> 4) + j), B = Q rows (lane: query l & 15, same d): DP / 32 MFMAs per
//                    16 x 16 tile.  D: lane holds S^T[key 4 (l >> 4) + r][query l & 15] -- a lane's 4 values of a tile are 4 CONSECUTIVE
//                    KEYS of ONE QUERY.
//   softmax          over a query's keys = over the lane's registers and the lanes l ^ 16, l ^ 32, l ^ 48 (two permlane swaps): fp32,
//                    base 2, logits scaled by scale * log2(e) IN FP32 (Q is not rescaled).  Key j is visible to query i iff j < len
//                    (CAUSAL: && j <= i), by index compare; an invisible logit is -inf, its P exactly 0.  Key 0 is visible to every
//                    query -- also under the causal mask, 0 <= i -- so no row is fully masked: the row max is finite, the row sum > 0.
//                    CAUSAL skips the key tiles right of the query tile's diagonal: they would be all -inf, and as they are they add an
//                    exact + 0.f to the row sum.
//   O^T = V^T P^T    the MFMA's summation index k is only a label both operands must agree on: k = 8 (l >> 4) + j  <->  key
//                    32 tp + 4 (l >> 4) + j (j < 4), 32 tp + 16 + 4 (l >> 4) + j - 4 (j >= 4) makes the B operand exactly the 8
//                    fp16-rounded P values the lane already holds from key tiles 2 tp and 2 tp + 1 -- P never goes through LDS -- and
//                    the A operand two 8-byte reads of a Vt row.  Key tiles are taken in PAIRS: an odd tile count (257 tokens = 17
//                    tiles; CAUSAL: an even query tile) is completed by a partner tile whose P is 0 against Vt rows that are real V or
//                    the zero padding -- finite by construction, which is why the staging is never trimmed to the keys a query block
//                    can see.
//                    D: lane holds O^T[d 4 (l >> 4) + r][query l & 15] -- the same query as its softmax denominator, 4 consecutive d:
//                    one 8-byte store per 16 channels.
//
// Only queries < len are stored.  A pad query's column is computed (on finite numbers) and dropped.
#include "common.h"

namespace {

constexpr int CA_THREADS = 256;
constexpr int CA_MAX_L = 288;                       // 18 key tiles = 9 pairs
constexpr int CA_TEXT_MAX_L = 128;                  // the text entry's envelope
constexpr int CA_KT = CA_MAX_L / 16;
constexpr int CA_LDV = CA_MAX_L + 8;                // halves per Vt row in LDS
constexpr int CA_QPW = 16 * (CA_THREADS / 64);      // queries per workgroup

template <int D>
struct ca_lds {
  static constexpr int DP = (D + 31) & ~31;         // head_dim padded to the MFMA K-step: 64, 96
  static constexpr int LDK = DP + 8;                // halves per K row in LDS
  static constexpr int K_HALVES = CA_MAX_L * LDK;
  static constexpr int V_HALVES = D * CA_LDV;
  static constexpr size_t BYTES = (size_t)(K_HALVES + V_HALVES) * sizeof(f16);
};

template <int D, bool CAUSAL>
__global__ __launch_bounds__(CA_THREADS) void clip_attention_kernel(const f16* __restrict__ qkv, int64_t ld, int q_off, int k_off, int v_off,
                                                                    f16* __restrict__ out, int64_t ldo, int len, int heads, float c) {
  using L = ca_lds<D>;
  constexpr int DP = L::DP, LDK = L::LDK, KS = DP / 32, DT = D / 16, DCH = D / 8;
  static_assert(D % 16 == 0 && CA_MAX_L % 32 == 0, "whole output tiles per head, whole key-tile pairs");
  // K [CA_MAX_L][LDK] | Vt [D][CA_LDV]: 116736 bytes at d = 80, 115200 at d = 64 -- one workgroup per CU
  static_assert(L::BYTES <= 160 * 1024, "K and Vt of one head must fit gfx950's 160 KB of LDS");
  extern __shared__ __attribute__((aligned(16))) f16 ca_smem[];
  f16* Ks = ca_smem;
  f16* Vt = ca_smem + L::K_HALVES;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int lp = (len + 15) & ~15, lk = (len + 31) & ~31;            // key rows padded to the tile / the tile pair: <= CA_MAX_L
  const f16* base = qkv + (int64_t)b * len * ld + h * D;

  for (int i = tid; i < lp * (DP / 8); i += CA_THREADS) {
    const int row = i / (DP / 8), ch = i - row * (DP / 8);
    f16x8 k = zero8();
    if (row < len && ch < DCH) k = ld_global_16B(base + (int64_t)row * ld + k_off + 8 * ch);
    *reinterpret_cast<f16x8*>(&Ks[row * LDK + 8 * ch]) = k;
  }
  for (int i = tid; i < lk * DCH; i += CA_THREADS) {
    const int row = i / DCH, ch = i - row * DCH;
    f16x8 v = zero8();
    if (row < len) v = ld_global_16B(base + (int64_t)row * ld + v_off + 8 * ch);
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(8 * ch + e) * CA_LDV + row] = v[e];
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
  const int qt = blockIdx.y * (CA_THREADS / 64) + wave, nkt = lp >> 4;
  if (qt >= nkt) return;                                               // wave-uniform, after the only barrier
  const float ninf = -__builtin_inff();
  const int query = qt * 16 + c16;
  f16x8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = zero8();
    if (query < len && 32 * ks + 8 * g < D) qf[ks] = ld_global_16B(base + (int64_t)query * ld + q_off + 32 * ks + 8 * g);
  }
  f32x4 s[CA_KT];
  float m = ninf;
#pragma unroll
  for (int kt = 0; kt < CA_KT; ++kt) {
    s[kt] = f32x4{ninf, ninf, ninf, ninf};
    if (kt < nkt && (!CAUSAL || kt <= qt)) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        acc = mfma16x16x32(*reinterpret_cast<const f16x8*>(&Ks[(kt * 16 + c16) * LDK + 32 * ks + 8 * g]), qf[ks], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * 16 + 4 * g + r;
        const float v = (key < len && (!CAUSAL || key <= query)) ? acc[r] * c : ninf;
        s[kt][r] = v;
        m = fmaxf(m, v);
      }
    }
  }
  m = lane_xor32_max(lane_xor16_max(m));                               // finite: key 0 is visible to every query
  float lsum = 0.f;
  f16x8 pf[CA_KT / 2];
#pragma unroll
  for (int tp = 0; tp < CA_KT / 2; ++tp) {
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
  for (int tp = 0; tp < CA_KT / 2; ++tp) {
    if (2 * tp < nkt && (!CAUSAL || 2 * tp <= qt)) {                   // keys < 32 tp + 32 <= lk: inside Vt's zero-padded rows
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const f16* vrow = &Vt[(dt * 16 + c16) * CA_LDV + 32 * tp + 4 * g];
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

template <int D, bool CAUSAL>
int ca_launch(const char* name, const f16* qkv, int64_t ld_qkv, int q_off, int k_off, int v_off, f16* out, int64_t ld_out, int batch, int len,
              int heads, float scale, hipStream_t s) {
  if (i2v_big_lds_kernel_cus(reinterpret_cast<const void*>(clip_attention_kernel<D, CAUSAL>), ca_lds<D>::BYTES) <= 0)
    I2V_FAIL(I2V_ERR_LAUNCH, "%s: the device refuses %zu bytes of LDS per workgroup", name, ca_lds<D>::BYTES);
  hipLaunchKernelGGL((clip_attention_kernel<D, CAUSAL>), dim3((unsigned)(batch * heads), (unsigned)i2v_cdiv(len, CA_QPW)), dim3(CA_THREADS),
                     ca_lds<D>::BYTES, s, qkv, ld_qkv, q_off, k_off, v_off, out, ld_out, len, heads, scale * 1.44269504088896340736f);
  return i2v_check_launch(name);
}

// the argument checks of both entry points, once.  An envelope is (causal, max_len, head_dim 64 and -- d80 -- 80); outside it the
// status is I2V_ERR_UNSUPPORTED, any other bad argument is I2V_ERR_INVALID_ARG, and nothing is launched either way.
int clip_attention_check_and_launch(const char* name, bool causal, int max_len, bool d80, const void* qkv, int64_t ld_qkv, int32_t q_off,
                                    int32_t k_off, int32_t v_off, void* out, int64_t ld_out, int32_t batch, int32_t len, int32_t heads,
                                    int32_t head_dim, float scale, i2v_stream_t stream) {
  I2V_CHECK_ARG(qkv && out, "%s: null pointer", name);
  I2V_CHECK_ARG(batch > 0 && heads > 0 && len > 0 && head_dim > 0, "%s: batch %d heads %d len %d head_dim %d must be positive", name, batch, heads,
                len, head_dim);
  if (head_dim != 64 && !(d80 && head_dim == 80))
    I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: head_dim %d is not supported (%s)", name, head_dim, d80 ? "64 and 80" : "only 64");
  if (len > max_len)
    I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: %d %s are not supported (at most %d)", name, len, causal ? "positions" : "tokens", max_len);
  const int64_t hidden = (int64_t)heads * head_dim;
  I2V_CHECK_ARG(hidden < (1 << 20) && (int64_t)batch * heads < ((int64_t)1 << 31) && (int64_t)batch * len < ((int64_t)1 << 31),
                "%s: problem too large (batch %d, heads %d)", name, batch, heads);
  I2V_CHECK_ARG(q_off >= 0 && k_off >= 0 && v_off >= 0 && q_off % 8 == 0 && k_off % 8 == 0 && v_off % 8 == 0,
                "%s: column offsets %d / %d / %d must be non-negative multiples of 8", name, q_off, k_off, v_off);
  I2V_CHECK_ARG(ld_qkv % 8 == 0 && ld_qkv < ((int64_t)1 << 24) && q_off + hidden <= ld_qkv && k_off + hidden <= ld_qkv && v_off + hidden <= ld_qkv,
                "%s: row stride %lld must be a multiple of 8 that holds every offset + heads * head_dim", name, (long long)ld_qkv);
  I2V_CHECK_ARG(ld_out % 8 == 0 && ld_out >= hidden && ld_out < ((int64_t)1 << 24),
                "%s: out row stride %lld must be a multiple of 8, at least heads * head_dim", name, (long long)ld_out);
  I2V_CHECK_ARG(i2v_al16(qkv) && i2v_al16(out), "%s: pointers must be 16-byte aligned", name);
  I2V_CHECK_ARG(scale > 0.f && scale < 3.0e38f, "%s: scale must be positive and finite", name);
  const int64_t rows = (int64_t)batch * len;
  I2V_CHECK_ARG(!i2v_overlap(qkv, rows * ld_qkv * 2, out, ((rows - 1) * ld_out + hidden) * 2), "%s: out is a new tensor (it must not overlap qkv)",
                name);
  const f16* in = reinterpret_cast<const f16*>(qkv);
  f16* o = reinterpret_cast<f16*>(out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (causal) return ca_launch<64, true>(name, in, ld_qkv, q_off, k_off, v_off, o, ld_out, batch, len, heads, scale, s);
  if (head_dim == 64) return ca_launch<64, false>(name, in, ld_qkv, q_off, k_off, v_off, o, ld_out, batch, len, heads, scale, s);
  return ca_launch<80, false>(name, in, ld_qkv, q_off, k_off, v_off, o, ld_out, batch, len, heads, scale, s);
}

}  // namespace

extern "C" int i2v_clip_attention_f16(const void* qkv, int64_t ld_qkv, int32_t q_off, int32_t k_off, int32_t v_off, void* out, int64_t ld_out,
                                      int32_t batch, int32_t len, int32_t heads, int32_t head_dim, float scale, i2v_stream_t stream) {
  return clip_attention_check_and_launch("i2v_clip_attention_f16", true, CA_TEXT_MAX_L, false, qkv, ld_qkv, q_off, k_off, v_off, out, ld_out, batch,
                                         len, heads, head_dim, scale, stream);
}

extern "C" int i2v_clip_vision_attention_f16(const void* qkv, int64_t ld_qkv, int32_t q_off, int32_t k_off, int32_t v_off, void* out,
                                             int64_t ld_out, int32_t batch, int32_t len, int32_t heads, int32_t head_dim, float scale,
                                             i2v_stream_t stream) {
  return clip_attention_check_and_launch("i2v_clip_vision_attention_f16", false, CA_MAX_L, true, qkv, ld_qkv, q_off, k_off, v_off, out, ld_out,
                                         batch, len, heads, head_dim, scale, stream);
}
