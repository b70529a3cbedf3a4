// The attention of one SHORT key sequence per batch entry, for the work that runs once per sample: both CLIP towers and IP-Adapter
// Plus's Resampler.  One template, three instantiations, three entry points:
//
//   i2v_clip_attention_f16          <64, causal>                  the text tower (clip_text.py): head_dim 64, len <= 128
//   i2v_clip_vision_attention_f16   <64, not causal>, <80, ...>   the vision tower (clip_vision.py): head_dim 64 or 80, len <= SA_MAX_L = 288
//                                                                 (18 key tiles; ViT-H/14 at 224 px has 257 tokens)
//   i2v_perceiver_attention_f16     <64, not causal>              the Resampler (blocks.py): head_dim 64, n_q <= 64, len_a + len_b <= 288
//
// n_q queries per batch entry attend to a key sequence that is the CONCATENATION of two row sources,
//
//   keys of batch entry b = rows [b * len_a, (b + 1) * len_a) of source A, then rows [b * len_b, (b + 1) * len_b) of source B
//
// each source a packed fp16 matrix with its own row stride and K / V column offsets.  The towers read q, k and v in place from the
// packed [B * L, 3 * hidden] result of one QKV GEMM: source A is that buffer, len_b = 0, q is the same buffer and n_q = len.  The
// Resampler's A is [Wk;Wv] over ln0(x) (257 image tokens) and its B the latents' own packed q | k | v buffer (16 rows), the memory q
// is read from: nobody materialises torch.cat([ln0(x), ln1(latents)], dim=-2).  The kernel is written to be obviously inside its
// operands, not to be fast.
//
// Grid (batch * heads, query blocks): a workgroup of 4 waves owns 64 queries of one (batch, head), a wave one tile of 16 of them; a
// wave whose tile starts at or beyond n_q leaves after the only barrier.  Every workgroup stages the head's WHOLE K and V in LDS: K
// row-major with the head dimension padded to the MFMA K-step with ZEROS (d 80 -> 96: 2.5 steps become 3; rows of DP + 8 halves, so
// the 16 rows of a fragment read start in different banks), V TRANSPOSED (Vt[d][key], keys padded to a multiple of 32 with zeros).
// LDS row r < len_a comes from A's row r, row len_a <= r < len = len_a + len_b from B's row r - len_a; rows at and beyond len are
// never read from memory: their LDS image is zero.  After the staging nothing knows where the A / B boundary was, so a query's
// arithmetic depends on the concatenated key sequence only: the same keys split differently give bit-equal outputs.  Q does not go
// through LDS: a lane reads the 16-byte chunks of its own query row that its B fragment holds (zero for a pad query and for the
// pad of d).
//
//   S^T = K Q^T      A = K rows (lane: key l & 15, d 32 ks + 8 (l >> 4) + j), B = Q rows (lane: query l & 15, same d): DP / 32 MFMAs per
//                    16 x 16 tile.  D: lane holds S^T[key 4 (l >> 4) + r][query l & 15] -- a lane's 4 values of a tile are 4 CONSECUTIVE
//                    KEYS of ONE QUERY.
//   softmax          over a query's keys = over the lane's registers and the lanes l ^ 16, l ^ 32, l ^ 48 (two permlane swaps): fp32,
//                    base 2, logits scaled by scale * log2(e) IN FP32 (Q is not rescaled).  Key j is visible to query i iff j < len
//                    (CAUSAL: && j <= i), by index compare; an invisible logit is -inf, its P exactly 0.  len_a >= 1 and 0 <= i, so
//                    key 0 is visible to every query: no row is fully masked, the row max is finite, the row sum > 0.  CAUSAL skips
//                    the key tiles right of the query tile's diagonal: they would be all -inf, and as they are they add an exact
//                    + 0.f to the row sum.
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
// Only queries < n_q are stored, columns [h * D, h * D + D) of their out row.  A pad query's column is computed (on finite numbers)
// and dropped.
#include "common.h"

namespace {

constexpr int SA_THREADS = 256;
constexpr int SA_MAX_L = 288;                       // 18 key tiles = 9 pairs
constexpr int SA_TEXT_MAX_L = 128;                  // the text entry's envelope
constexpr int SA_KT = SA_MAX_L / 16;
constexpr int SA_LDV = SA_MAX_L + 8;                // halves per Vt row in LDS
constexpr int SA_QPW = 16 * (SA_THREADS / 64);      // queries per workgroup = the most the Resampler's entry takes

template <int D>
struct sa_lds {                                     // K [SA_MAX_L][LDK] | Vt [D][SA_LDV]
  static constexpr int DP = (D + 31) & ~31;         // head_dim padded to the MFMA K-step: 64, 96
  static constexpr int LDK = DP + 8;                // halves per K row in LDS
  static constexpr int K_HALVES = SA_MAX_L * LDK;
  static constexpr int V_HALVES = D * SA_LDV;
  static constexpr size_t BYTES = (size_t)(K_HALVES + V_HALVES) * sizeof(f16);
};
// of gfx950's 160 KB of LDS per CU: two workgroups per CU at d = 64, one at d = 80
static_assert(sa_lds<64>::BYTES == 79360 && sa_lds<80>::BYTES == 107264, "K and Vt of one head, as DESIGN 4.11 states them");

struct sa_src {         // one key / value source: rows [b * len, (b + 1) * len) of a packed fp16 matrix
  const f16* p;
  int64_t ld;
  int k_off, v_off, len;
};

// q, a.p and bs.p are read-only and may be one buffer: no __restrict__
template <int D, bool CAUSAL>
__global__ __launch_bounds__(SA_THREADS) void short_attention_kernel(const f16* q, int64_t ldq, int q_off, int n_q, sa_src a, sa_src bs, f16* out,
                                                                     int64_t ldo, int heads, float c) {
  using L = sa_lds<D>;
  constexpr int DP = L::DP, LDK = L::LDK, KS = DP / 32, DT = D / 16, DCH = D / 8;
  static_assert(D % 16 == 0 && SA_MAX_L % 32 == 0, "whole output tiles per head, whole key-tile pairs");
  extern __shared__ __attribute__((aligned(16))) f16 sa_smem[];
  f16* Ks = sa_smem;
  f16* Vt = sa_smem + L::K_HALVES;
  const int tid = threadIdx.x;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int len = a.len + bs.len;
  const int lp = (len + 15) & ~15, lk = (len + 31) & ~31;            // key rows padded to the tile / the tile pair: <= SA_MAX_L
  // LDS rows [row0, row0 + s.len) of K (the pad of d zero) and of Vt from one source, which is never dereferenced when s.len == 0.
  // A source at a time, not a row's source picked by `row < a.len`: the compiler turns that select into a per-row load of the
  // chosen source's fields from the argument block, a second memory latency in front of every row's
  auto stage = [&](const sa_src& s, int row0) {
    const f16* base = s.p + (int64_t)b * s.len * s.ld + h * D;
    for (int i = tid; i < s.len * (DP / 8); i += SA_THREADS) {
      const int row = i / (DP / 8), ch = i - row * (DP / 8);
      *reinterpret_cast<f16x8*>(&Ks[(row0 + row) * LDK + 8 * ch]) = ch < DCH ? ld_global_16B(base + (int64_t)row * s.ld + s.k_off + 8 * ch) : zero8();
    }
    for (int i = tid; i < s.len * DCH; i += SA_THREADS) {
      const int row = i / DCH, ch = i - row * DCH;
      const f16x8 v = ld_global_16B(base + (int64_t)row * s.ld + s.v_off + 8 * ch);
#pragma unroll
      for (int e = 0; e < 8; ++e) Vt[(8 * ch + e) * SA_LDV + row0 + row] = v[e];
    }
  };
  stage(a, 0);
  stage(bs, a.len);
  // the zero rows, which no memory stands behind: K's [len, lp), Vt's [len, lk)
  for (int i = tid; i < (lp - len) * (DP / 8); i += SA_THREADS)
    *reinterpret_cast<f16x8*>(&Ks[(len + i / (DP / 8)) * LDK + 8 * (i % (DP / 8))]) = zero8();
  for (int i = tid; i < (lk - len) * D; i += SA_THREADS) Vt[(i % D) * SA_LDV + len + i / D] = (f16)0.f;
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
  const int qt = blockIdx.y * (SA_THREADS / 64) + wave, nkt = lp >> 4;
  if (qt * 16 >= n_q) return;                                          // wave-uniform, after the only barrier
  const float ninf = -__builtin_inff();
  const int query = qt * 16 + c16;
  f16x8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = zero8();
    if (query < n_q && 32 * ks + 8 * g < D) qf[ks] = ld_global_16B(q + ((int64_t)b * n_q + query) * ldq + q_off + h * D + 32 * ks + 8 * g);
  }
  f32x4 s[SA_KT];
  float m = ninf;
#pragma unroll
  for (int kt = 0; kt < SA_KT; ++kt) {
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
  f16x8 pf[SA_KT / 2];
#pragma unroll
  for (int tp = 0; tp < SA_KT / 2; ++tp) {
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
  for (int tp = 0; tp < SA_KT / 2; ++tp) {
    if (2 * tp < nkt && (!CAUSAL || 2 * tp <= qt)) {                   // keys < 32 tp + 32 <= lk: inside Vt's staged, zero-padded rows
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const f16* vrow = &Vt[(dt * 16 + c16) * SA_LDV + 32 * tp + 4 * g];
        const f16x4 lo = *reinterpret_cast<const f16x4*>(vrow), hi = *reinterpret_cast<const f16x4*>(vrow + 16);
        const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[dt] = mfma16x16x32(vf, pf[tp], o[dt]);
      }
    }
  }
  if (query < n_q) {
    const float inv = 1.0f / lsum;
    f16* orow = out + ((int64_t)b * n_q + query) * ldo + h * D + 4 * g;
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
int sa_launch(const char* name, const f16* q, int64_t ld_q, int q_off, int n_q, const sa_src& a, const sa_src& b, f16* out, int64_t ld_out,
              int batch, int heads, float scale, hipStream_t s) {
  if (i2v_big_lds_kernel_cus(reinterpret_cast<const void*>(short_attention_kernel<D, CAUSAL>), sa_lds<D>::BYTES) <= 0)
    I2V_FAIL(I2V_ERR_LAUNCH, "%s: the device refuses %zu bytes of LDS per workgroup", name, sa_lds<D>::BYTES);
  hipLaunchKernelGGL((short_attention_kernel<D, CAUSAL>), dim3((unsigned)(batch * heads), (unsigned)i2v_cdiv(n_q, SA_QPW)), dim3(SA_THREADS),
                     sa_lds<D>::BYTES, s, q, ld_q, q_off, n_q, a, b, out, ld_out, heads, scale * 1.44269504088896340736f);
  return i2v_check_launch(name);
}

// one read-only operand: `rows` rows of stride ld, of which the heads * head_dim columns at off0 and at off1 are read.  It may alias
// another operand; it may not overlap out.
int sa_check_operand(const char* name, const char* what, const void* p, int64_t ld, int32_t off0, int32_t off1, int64_t rows, int64_t hidden,
                     const void* out, int64_t out_bytes) {
  I2V_CHECK_ARG(off0 >= 0 && off1 >= 0 && off0 % 8 == 0 && off1 % 8 == 0, "%s: %s: column offsets %d / %d must be non-negative multiples of 8",
                name, what, off0, off1);
  I2V_CHECK_ARG(ld % 8 == 0 && ld < ((int64_t)1 << 24) && off0 + hidden <= ld && off1 + hidden <= ld,
                "%s: %s: row stride %lld must be a multiple of 8 that holds every offset + heads * head_dim", name, what, (long long)ld);
  I2V_CHECK_ARG(i2v_al16(p), "%s: %s: pointers must be 16-byte aligned", name, what);
  I2V_CHECK_ARG(!i2v_overlap(p, rows * ld * 2, out, out_bytes), "%s: out is a new tensor (it must not overlap %s)", name, what);
  return I2V_OK;
}

// The argument checks of all three entry points, once, and the launch.  An entry has checked its own envelope before (outside it the
// status is I2V_ERR_UNSUPPORTED): head_dim is 64 or 80, 1 <= n_q, 1 <= a.len, 0 <= b.len, a.len + b.len <= SA_MAX_L, pointers not null
// (b.p may be when b.len == 0).  Any other bad argument is I2V_ERR_INVALID_ARG, and nothing is launched either way.
int sa_check_and_launch(const char* name, bool causal, const char* q_name, const void* q, int64_t ld_q, int32_t q_off, int32_t n_q, sa_src a,
                        sa_src b, void* out, int64_t ld_out, int32_t batch, int32_t heads, int32_t head_dim, float scale, i2v_stream_t stream) {
  const int64_t hidden = (int64_t)heads * head_dim;
  I2V_CHECK_ARG(hidden < (1 << 20) && (int64_t)batch * heads < ((int64_t)1 << 31) && (int64_t)batch * SA_MAX_L < ((int64_t)1 << 31),
                "%s: problem too large (batch %d, heads %d)", name, batch, heads);
  I2V_CHECK_ARG(ld_out % 8 == 0 && ld_out >= hidden && ld_out < ((int64_t)1 << 24),
                "%s: out row stride %lld must be a multiple of 8, at least heads * head_dim", name, (long long)ld_out);
  I2V_CHECK_ARG(i2v_al16(out), "%s: out: pointers must be 16-byte aligned", name);
  I2V_CHECK_ARG(scale > 0.f && scale < 3.0e38f, "%s: scale must be positive and finite", name);
  const int64_t out_bytes = (((int64_t)batch * n_q - 1) * ld_out + hidden) * 2;
  if (int st = sa_check_operand(name, q_name, q, ld_q, q_off, q_off, (int64_t)batch * n_q, hidden, out, out_bytes)) return st;
  if (int st = sa_check_operand(name, "source A", a.p, a.ld, a.k_off, a.v_off, (int64_t)batch * a.len, hidden, out, out_bytes)) return st;
  if (b.len == 0) b = sa_src{a.p, 0, 0, 0, 0};
  else if (int st = sa_check_operand(name, "source B", b.p, b.ld, b.k_off, b.v_off, (int64_t)batch * b.len, hidden, out, out_bytes)) return st;
  const f16* qp = reinterpret_cast<const f16*>(q);
  f16* o = reinterpret_cast<f16*>(out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (causal) return sa_launch<64, true>(name, qp, ld_q, q_off, n_q, a, b, o, ld_out, batch, heads, scale, s);
  if (head_dim == 64) return sa_launch<64, false>(name, qp, ld_q, q_off, n_q, a, b, o, ld_out, batch, heads, scale, s);
  return sa_launch<80, false>(name, qp, ld_q, q_off, n_q, a, b, o, ld_out, batch, heads, scale, s);
}

// a CLIP tower's entry: the envelope is (causal, max_len, head_dim 64 and -- d80 -- 80); q, k and v are columns of ONE packed buffer
int clip_attention_entry(const char* name, bool causal, int max_len, bool d80, const void* qkv, int64_t ld_qkv, int32_t q_off, int32_t k_off,
                         int32_t v_off, void* out, int64_t ld_out, int32_t batch, int32_t len, int32_t heads, int32_t head_dim, float scale,
                         i2v_stream_t stream) {
  I2V_CHECK_ARG(qkv && out, "%s: null pointer", name);
  I2V_CHECK_ARG(batch > 0 && heads > 0 && len > 0 && head_dim > 0, "%s: batch %d heads %d len %d head_dim %d must be positive", name, batch, heads,
                len, head_dim);
  if (head_dim != 64 && !(d80 && head_dim == 80))
    I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: head_dim %d is not supported (%s)", name, head_dim, d80 ? "64 and 80" : "only 64");
  if (len > max_len)
    I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: %d %s are not supported (at most %d)", name, len, causal ? "positions" : "tokens", max_len);
  return sa_check_and_launch(name, causal, "qkv", qkv, ld_qkv, q_off, len, sa_src{reinterpret_cast<const f16*>(qkv), ld_qkv, k_off, v_off, len},
                             sa_src{nullptr, 0, 0, 0, 0}, out, ld_out, batch, heads, head_dim, scale, stream);
}

}  // namespace

extern "C" int i2v_clip_attention_f16(const void* qkv, int64_t ld_qkv, int32_t q_off, int32_t k_off, int32_t v_off, void* out, int64_t ld_out,
                                      int32_t batch, int32_t len, int32_t heads, int32_t head_dim, float scale, i2v_stream_t stream) {
  return clip_attention_entry("i2v_clip_attention_f16", true, SA_TEXT_MAX_L, false, qkv, ld_qkv, q_off, k_off, v_off, out, ld_out, batch, len,
                              heads, head_dim, scale, stream);
}

extern "C" int i2v_clip_vision_attention_f16(const void* qkv, int64_t ld_qkv, int32_t q_off, int32_t k_off, int32_t v_off, void* out,
                                             int64_t ld_out, int32_t batch, int32_t len, int32_t heads, int32_t head_dim, float scale,
                                             i2v_stream_t stream) {
  return clip_attention_entry("i2v_clip_vision_attention_f16", false, SA_MAX_L, true, qkv, ld_qkv, q_off, k_off, v_off, out, ld_out, batch, len,
                              heads, head_dim, scale, stream);
}

extern "C" int i2v_perceiver_attention_f16(const void* q, int64_t ld_q, int32_t q_off, const void* kv_a, int64_t ld_a, int32_t ka_off,
                                           int32_t va_off, int32_t len_a, const void* kv_b, int64_t ld_b, int32_t kb_off, int32_t vb_off,
                                           int32_t len_b, void* out, int64_t ld_out, int32_t batch, int32_t n_q, int32_t heads,
                                           int32_t head_dim, float scale, i2v_stream_t stream) {
  const char* name = "i2v_perceiver_attention_f16";
  I2V_CHECK_ARG(q && kv_a && out && (kv_b || len_b == 0), "%s: null pointer", name);
  I2V_CHECK_ARG(batch > 0 && heads > 0 && n_q > 0 && head_dim > 0 && len_a > 0 && len_b >= 0,
                "%s: batch %d heads %d n_q %d head_dim %d len_a %d must be positive, len_b %d non-negative", name, batch, heads, n_q, head_dim,
                len_a, len_b);
  if (head_dim != 64) I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: head_dim %d is not supported (only 64)", name, head_dim);
  if (n_q > SA_QPW) I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: %d queries are not supported (at most %d)", name, n_q, SA_QPW);
  if ((int64_t)len_a + len_b > SA_MAX_L)
    I2V_FAIL(I2V_ERR_UNSUPPORTED, "%s: %d + %d keys are not supported (at most %d)", name, len_a, len_b, SA_MAX_L);
  return sa_check_and_launch(name, false, "q", q, ld_q, q_off, n_q, sa_src{reinterpret_cast<const f16*>(kv_a), ld_a, ka_off, va_off, len_a},
                             sa_src{reinterpret_cast<const f16*>(kv_b), ld_b, kb_off, vb_off, len_b}, out, ld_out, batch, heads, head_dim, scale,
                             stream);
}
