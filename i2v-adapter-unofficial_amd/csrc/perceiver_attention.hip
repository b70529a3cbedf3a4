// The attention of IP-Adapter Plus's Resampler (blocks.py: Resampler): a short block of learned queries attends to a key
// sequence that is the CONCATENATION of two row sources,
//
//   keys of batch entry b = rows [b * len_a, (b + 1) * len_a) of source A, then rows [b * len_b, (b + 1) * len_b) of source B
//
// each source the packed K | V result of a GEMM with its own row stride and column offsets -- in the Resampler A is [Wk;Wv] over
// ln0(x) (257 image tokens) and B the latents' own packed q | k | v buffer (16 rows), the same memory q is read from.  Nobody
// materialises torch.cat([ln0(x), ln1(latents)], dim=-2).  One entry point: i2v_perceiver_attention_f16, head_dim 64, n_q <= 64,
// len_a + len_b <= PA_MAX_L = 288.
//
// Once-per-sample work of batch * heads small problems: written, like csrc/clip_attention.hip -- whose scheme this is -- to be obviously
// inside its operands, not to be fast.
//
// Grid (batch * heads): a workgroup of 4 waves owns ALL (<= 64) queries of one (batch, head), a wave one tile of 16 of them; a wave whose
// tile starts at or beyond n_q leaves after the only barrier.  The workgroup stages the head's whole K and V in LDS: K row-major (rows of
// 64 + 8 halves, so the 16 rows of a fragment read start in different banks), V TRANSPOSED (Vt[d][key], keys padded to a multiple of 32
// with zeros).  LDS row r < len_a comes from A's row r, row len_a <= r < len_a + len_b from B's row r - len_a; rows at and beyond
// len = len_a + len_b are never read from memory: their LDS image is zero.  After the staging nothing knows where the A / B boundary
// was, so a query's arithmetic depends on the concatenated key sequence only: the same keys split differently give bit-equal outputs.
// Q does not go through LDS: a lane reads the 16-byte chunks of its own query row that its B fragment holds (zero for a pad query).
//
//   S^T = K Q^T      A = K rows (lane: key l & 15, d 32 ks + 8 (l >> 4) + j), B = Q rows (lane: query l & 15, same d): 2 MFMAs per 16 x 16
//                    tile.  D: lane holds S^T[key 4 (l >> 4) + r][query l & 15] -- 4 CONSECUTIVE KEYS of ONE QUERY.
//   softmax          over a query's keys = over the lane's registers and the lanes l ^ 16, l ^ 32, l ^ 48: fp32, base 2, logits scaled by
//                    scale * log2(e) IN FP32 (Q is not rescaled).  Key j is visible iff j < len, by index compare; an invisible logit
//                    is -inf, its P exactly 0.  len_a >= 1, so key 0 is visible to every query: the row max is finite, the row sum > 0.
//   O^T = V^T P^T    k = 8 (l >> 4) + j  <->  key 32 tp + 4 (l >> 4) + j (j < 4), 32 tp + 16 + 4 (l >> 4) + j - 4 (j >= 4): the B operand
//                    is exactly the 8 fp16-rounded P values the lane already holds from key tiles 2 tp and 2 tp + 1, the A operand two
//                    8-byte reads of a Vt row.  Key tiles are taken in PAIRS: an odd tile count is completed by a partner tile whose P
//                    is 0 against Vt's zero padding.
//                    D: lane holds O^T[d 4 (l >> 4) + r][query l & 15]: one 8-byte store per 16 channels.
//
// Only queries < n_q are stored, columns [h * 64, h * 64 + 64) of their out row.
#include "common.h"

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_D = 64;                            // head_dim
constexpr int PA_MAX_L = 288;                       // 18 key tiles = 9 pairs
constexpr int PA_MAX_Q = 16 * (PA_THREADS / 64);    // queries per workgroup = the most the entry takes
constexpr int PA_KT = PA_MAX_L / 16;
constexpr int PA_LDK = PA_D + 8;                    // halves per K row in LDS
constexpr int PA_LDV = PA_MAX_L + 8;                // halves per Vt row in LDS
constexpr int PA_K_HALVES = PA_MAX_L * PA_LDK;
constexpr int PA_V_HALVES = PA_D * PA_LDV;
constexpr size_t PA_LDS_BYTES = (size_t)(PA_K_HALVES + PA_V_HALVES) * sizeof(f16);      // 79360

struct pa_src {         // one key / value source: rows [b * len, (b + 1) * len) of a packed fp16 matrix
  const f16* p;
  int64_t ld;
  int k_off, v_off, len;
};

__global__ __launch_bounds__(PA_THREADS) void perceiver_attention_kernel(const f16* q, int64_t ldq, int q_off, pa_src a, pa_src bs, f16* out,
                                                                         int64_t ldo, int n_q, int heads, float c) {
  constexpr int KS = PA_D / 32, DT = PA_D / 16, DCH = PA_D / 8;
  static_assert(PA_MAX_L % 32 == 0 && PA_LDS_BYTES <= 160 * 1024, "whole key-tile pairs; K and Vt of one head fit gfx950's 160 KB of LDS");
  extern __shared__ __attribute__((aligned(16))) f16 pa_smem[];
  f16* Ks = pa_smem;
  f16* Vt = pa_smem + PA_K_HALVES;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int len = a.len + bs.len;
  const int lp = (len + 15) & ~15, lk = (len + 31) & ~31;            // key rows padded to the tile / the tile pair: <= PA_MAX_L
  const f16* abase = a.p + (int64_t)b * a.len * a.ld + h * PA_D;
  const f16* bbase = bs.p + (int64_t)b * bs.len * bs.ld + h * PA_D;     // never dereferenced when bs.len == 0

  // rows [0, lk) x DCH chunks: K's rows [lp, lk) are not read by the QK loop (kt < nkt), Vt's are (as zeros)
  for (int i = tid; i < lk * DCH; i += PA_THREADS) {
    const int row = i / DCH, ch = i - row * DCH;
    f16x8 k = zero8(), v = zero8();
    if (row < a.len) {
      const f16* r = abase + (int64_t)row * a.ld + 8 * ch;
      k = ld_global_16B(r + a.k_off);
      v = ld_global_16B(r + a.v_off);
    } else if (row < len) {
      const f16* r = bbase + (int64_t)(row - a.len) * bs.ld + 8 * ch;
      k = ld_global_16B(r + bs.k_off);
      v = ld_global_16B(r + bs.v_off);
    }
    if (row < lp) *reinterpret_cast<f16x8*>(&Ks[row * PA_LDK + 8 * ch]) = k;
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(8 * ch + e) * PA_LDV + row] = v[e];
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
  const int nkt = lp >> 4;
  if (wave * 16 >= n_q) return;                                        // wave-uniform, after the only barrier
  const float ninf = -__builtin_inff();
  const int query = wave * 16 + c16;
  f16x8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = zero8();
    if (query < n_q) qf[ks] = ld_global_16B(q + ((int64_t)b * n_q + query) * ldq + q_off + h * PA_D + 32 * ks + 8 * g);
  }
  f32x4 s[PA_KT];
  float m = ninf;
#pragma unroll
  for (int kt = 0; kt < PA_KT; ++kt) {
    s[kt] = f32x4{ninf, ninf, ninf, ninf};
    if (kt < nkt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        acc = mfma16x16x32(*reinterpret_cast<const f16x8*>(&Ks[(kt * 16 + c16) * PA_LDK + 32 * ks + 8 * g]), qf[ks], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * 16 + 4 * g + r;
        const float v = key < len ? acc[r] * c : ninf;
        s[kt][r] = v;
        m = fmaxf(m, v);
      }
    }
  }
  m = lane_xor32_max(lane_xor16_max(m));                               // finite: key 0 is visible to every query
  float lsum = 0.f;
  f16x8 pf[PA_KT / 2];
#pragma unroll
  for (int tp = 0; tp < PA_KT / 2; ++tp) {
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
  for (int tp = 0; tp < PA_KT / 2; ++tp) {
    if (2 * tp < nkt) {                                                // keys < 32 tp + 32 <= lk: inside Vt's staged, zero-padded rows
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const f16* vrow = &Vt[(dt * 16 + c16) * PA_LDV + 32 * tp + 4 * g];
        const f16x4 lo = *reinterpret_cast<const f16x4*>(vrow), hi = *reinterpret_cast<const f16x4*>(vrow + 16);
        const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[dt] = mfma16x16x32(vf, pf[tp], o[dt]);
      }
    }
  }
  if (query < n_q) {
    const float inv = 1.0f / lsum;
    f16* orow = out + ((int64_t)b * n_q + query) * ldo + h * PA_D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      f16x4 w;
#pragma unroll
      for (int r = 0; r < 4; ++r) w[r] = (f16)(o[dt][r] * inv);
      *reinterpret_cast<f16x4*>(orow + dt * 16) = w;
    }
  }
}

}  // namespace

extern "C" int i2v_perceiver_attention_f16(const void* q, int64_t ld_q, int32_t q_off, const void* kv_a, int64_t ld_a, int32_t ka_off,
                                           int32_t va_off, int32_t len_a, const void* kv_b, int64_t ld_b, int32_t kb_off, int32_t vb_off,
                                           int32_t len_b, void* out, int64_t ld_out, int32_t batch, int32_t n_q, int32_t heads,
                                           int32_t head_dim, float scale, i2v_stream_t stream) {
  const char* name = "i2v_perceiver_attention_f16";
  I2V_CHECK_ARG(q && kv_a && out && (kv_b || len_b == 0), "%s: null pointer", name);
  I2V_CHECK_ARG(batch > 0 && heads > 0 && n_q > 0 && head_dim > 0 && len_a > 0 && len_b >= 0,
                "%s: batch %d heads %d n_q %d head_dim %d len_a %d must be positive, len_b %d non-negative", name, batch, heads, n_q, head_dim,
                len_a, len_b);
  if (head_dim != PA_D) I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: head_dim %d is not supported (only %d)", name, head_dim, PA_D);
  if (n_q > PA_MAX_Q) I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: %d queries are not supported (at most %d)", name, n_q, PA_MAX_Q);
  if ((int64_t)len_a + len_b > PA_MAX_L)
    I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: %d + %d keys are not supported (at most %d)", name, len_a, len_b, PA_MAX_L);
  const int64_t hidden = (int64_t)heads * head_dim;
  I2V_CHECK_ARG(hidden < (1 << 20) && (int64_t)batch * heads < ((int64_t)1 << 31) && (int64_t)batch * PA_MAX_L < ((int64_t)1 << 31),
                "%s: problem too large (batch %d, heads %d)", name, batch, heads);
  I2V_CHECK_ARG(q_off >= 0 && ka_off >= 0 && va_off >= 0 && q_off % 8 == 0 && ka_off % 8 == 0 && va_off % 8 == 0,
                "%s: column offsets %d / %d / %d must be non-negative multiples of 8", name, q_off, ka_off, va_off);
  I2V_CHECK_ARG(ld_q % 8 == 0 && ld_q < ((int64_t)1 << 24) && q_off + hidden <= ld_q,
                "%s: q row stride %lld must be a multiple of 8 that holds q_off + heads * head_dim", name, (long long)ld_q);
  I2V_CHECK_ARG(ld_a % 8 == 0 && ld_a < ((int64_t)1 << 24) && ka_off + hidden <= ld_a && va_off + hidden <= ld_a,
                "%s: source A's row stride %lld must be a multiple of 8 that holds every offset + heads * head_dim", name, (long long)ld_a);
  if (len_b > 0) {
    I2V_CHECK_ARG(kb_off >= 0 && vb_off >= 0 && kb_off % 8 == 0 && vb_off % 8 == 0,
                  "%s: column offsets %d / %d of source B must be non-negative multiples of 8", name, kb_off, vb_off);
    I2V_CHECK_ARG(ld_b % 8 == 0 && ld_b < ((int64_t)1 << 24) && kb_off + hidden <= ld_b && vb_off + hidden <= ld_b,
                  "%s: source B's row stride %lld must be a multiple of 8 that holds every offset + heads * head_dim", name, (long long)ld_b);
    I2V_CHECK_ARG(i2v_al16(kv_b), "%s: pointers must be 16-byte aligned", name);
  }
  I2V_CHECK_ARG(ld_out % 8 == 0 && ld_out >= hidden && ld_out < ((int64_t)1 << 24),
                "%s: out row stride %lld must be a multiple of 8, at least heads * head_dim", name, (long long)ld_out);
  I2V_CHECK_ARG(i2v_al16(q) && i2v_al16(kv_a) && i2v_al16(out), "%s: pointers must be 16-byte aligned", name);
  I2V_CHECK_ARG(scale > 0.f && scale < 3.0e38f, "%s: scale must be positive and finite", name);
  // q, A and B are read-only and may alias one another (B is the latents' own q | k | v buffer); out may overlap none of them
  const int64_t qrows = (int64_t)batch * n_q, out_bytes = ((qrows - 1) * ld_out + hidden) * 2;
  I2V_CHECK_ARG(!i2v_overlap(q, qrows * ld_q * 2, out, out_bytes) && !i2v_overlap(kv_a, (int64_t)batch * len_a * ld_a * 2, out, out_bytes) &&
                    !(len_b > 0 && i2v_overlap(kv_b, (int64_t)batch * len_b * ld_b * 2, out, out_bytes)),
                "%s: out is a new tensor (it must not overlap q or a key / value source)", name);
  if (i2v_big_lds_kernel_cus(reinterpret_cast<const void*>(perceiver_attention_kernel), PA_LDS_BYTES) <= 0)
    I2V_FAIL(I2V_ERR_LAUNCH, "%s: the device refuses %zu bytes of LDS per workgroup", name, PA_LDS_BYTES);
  const pa_src a = {reinterpret_cast<const f16*>(kv_a), ld_a, ka_off, va_off, len_a};
  const pa_src bsrc = {reinterpret_cast<const f16*>(len_b > 0 ? kv_b : kv_a), len_b > 0 ? ld_b : 0, len_b > 0 ? kb_off : 0,
                       len_b > 0 ? vb_off : 0, len_b};
  hipLaunchKernelGGL(perceiver_attention_kernel, dim3((unsigned)(batch * heads)), dim3(PA_THREADS), PA_LDS_BYTES,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(q), ld_q, q_off, a, bsrc,
                     reinterpret_cast<f16*>(out), ld_out, n_q, heads, scale * 1.44269504088896340736f);
  return i2v_check_launch(name);
}
