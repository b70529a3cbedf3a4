// LoRA merge: dst[o, i] = round(base[o, i] + sum_j scale_j * sum_r up_j[o, r] * down_j[r, i]) for one weight matrix [out, in] (a conv
// weight [Cout, Cin, kh, kw] is the same problem with in = Cin kh kw), j < n <= I2V_LORA_MAX_ADAPTERS adapters of fp16 factors, one
// launch.  base / dst fp16 or fp32; the low-rank products run on the MFMA with fp32 accumulation, scale_j multiplies adapter j's fp32
// product (never an fp16 factor), and the result is rounded ONCE from the fp32 sum of base and all adapters -- which is why this is
// not n passes of i2v_gemm_f16 with a residual (n roundings, an order-dependent result, a transposed copy of `down`, K padding in
// memory and no fp32 weights).
//
// A workgroup (4 waves) owns a 64 (out) x 128 (in) tile of the weight; wave w its rows 16 w .. 16 w + 15.  The product is taken
// TRANSPOSED, D'[in, out] = down^T[in, r] * up^T[r, out] with mfma 16x16x32: the accumulator's register index then runs along `in`
// (the unit-stride axis of base / dst), and with the row permutation  MFMA row i of (group t, half m)  <->  column 32 t + 8 (i >> 2) +
// 4 m + (i & 3)  a lane ends up holding 8 CONSECUTIVE columns of one weight row: one 16-byte load of base and one 16-byte store of dst
// per lane and group (fp16; two of each for fp32).  The factor tiles of one 32-deep k chunk are staged once per workgroup in LDS --
// up [64 rows][32 k] as it lies in memory, down [32 k][128 cols] transposed to [col][k] (written as (k, k + 1) pairs) so that both
// MFMA operands are 16-byte LDS reads -- zero-filled past `rank`, `out` and `in`: ranks that are no multiple of 32 are padded here, not in memory.
//
// An element whose low-rank sum is exactly zero (no adapters, all scales 0) takes base's BITS: -0, subnormals, infinities and NaN
// payloads come through unchanged.
#include "common.h"

namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_ROWS = 64;        // out rows per workgroup (16 per wave)
constexpr int LM_COLS = 128;       // in columns per workgroup (4 groups of 32 per wave)
constexpr int LM_K = 32;           // rank chunk = the MFMA's k
constexpr int LM_LD = 40;          // LDS row stride in halves (80 B: 16-byte aligned rows, 20-bank stride)

struct LoraAdapters {
  i2v_lora_adapter a[I2V_LORA_MAX_ADAPTERS];
};

__device__ __forceinline__ bool is_zero_bits(float x) { return (__builtin_bit_cast(uint32_t, x) << 1) == 0u; }

template <bool F32, bool VEC>
__global__ __launch_bounds__(LM_THREADS) void lora_merge_kernel(void* __restrict__ dst_, const void* __restrict__ base_, int out, int in,
                                                                LoraAdapters ad, int n) {
  __shared__ __attribute__((aligned(16))) f16 s_up[LM_ROWS][LM_LD];
  __shared__ __attribute__((aligned(16))) f16 s_dn[LM_COLS][LM_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int row0 = (int)blockIdx.y * LM_ROWS, col0 = (int)blockIdx.x * LM_COLS;

  f32x4 tot[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) tot[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int j = 0; j < n; ++j) {
    const f16* __restrict__ up = reinterpret_cast<const f16*>(ad.a[j].up);
    const f16* __restrict__ down = reinterpret_cast<const f16*>(ad.a[j].down);
    const int rank = ad.a[j].rank;
    const float scale = ad.a[j].scale;
    const bool up_vec = (rank & 7) == 0 && (reinterpret_cast<uintptr_t>(up) & 15) == 0;
    const bool dn_vec = (in & 7) == 0 && (reinterpret_cast<uintptr_t>(down) & 15) == 0;
    f32x4 p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < rank; k0 += LM_K) {
      {  // up[row0 + r][k0 + g .. + 7] -> s_up[r][g ..]: one 8-element piece per thread
        const int r = tid >> 2, g = (tid & 3) * 8;
        const int grow = row0 + r, k = k0 + g;
        f16x8 v = zero8();
        if (grow < out && k < rank) {
          const f16* src = up + (int64_t)grow * rank + k;
          if (up_vec) {      // (rank % 8 == 0: a piece is inside or outside as a whole)
            v = *reinterpret_cast<const f16x8*>(src);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (k + e < rank) v[e] = src[e];
          }
        }
        *reinterpret_cast<f16x8*>(&s_up[r][g]) = v;
      }
      {  // down[k0 + 2 kp + {0, 1}][col0 + c .. + 7] -> s_dn[c ..][2 kp .. + 1] (transposed): one piece of two k rows per thread,
         // written as 8 four-byte pairs -- a wave's lanes run along k (16 pairs = 16 banks), its 4 column groups share them (4-way)
        const int kp = tid & 15, c = (tid >> 4) * 8;
        const int k = k0 + 2 * kp, gc = col0 + c;
        f16x8 v0 = zero8(), v1 = zero8();
        if (gc < in) {
          const f16* src = down + (int64_t)k * in + gc;
          if (dn_vec) {      // (in % 8 == 0: a piece is inside or outside as a whole)
            if (k < rank) v0 = *reinterpret_cast<const f16x8*>(src);
            if (k + 1 < rank) v1 = *reinterpret_cast<const f16x8*>(src + in);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              if (gc + e < in) {
                if (k < rank) v0[e] = src[e];
                if (k + 1 < rank) v1[e] = src[(int64_t)in + e];
              }
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) *reinterpret_cast<f16x2*>(&s_dn[c + e][2 * kp]) = f16x2{v0[e], v1[e]};
      }
      __syncthreads();
      // B' = up^T: lane holds up[row 16 wave + fr][k = 8 fq + e];  A' = down^T with the row permutation above
      const f16x8 bu = *reinterpret_cast<const f16x8*>(&s_up[wave * 16 + fr][8 * fq]);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const int c = 32 * t + 8 * (fr >> 2) + 4 * m + (fr & 3);
          const f16x8 adn = *reinterpret_cast<const f16x8*>(&s_dn[c][8 * fq]);
          p[2 * t + m] = mfma16x16x32(adn, bu, p[2 * t + m]);
        }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) tot[i][r] = fmaf(scale, p[i][r], tot[i][r]);
  }

  // lane: weight row row0 + 16 wave + fr, columns col0 + 32 t + 8 fq + (4 m + r) = element 4 m + r of its 8-column piece of group t
  const int row = row0 + wave * 16 + fr;
  if (row >= out) return;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = col0 + 32 * t + 8 * fq;
    if (c >= in) continue;
    const int64_t off = (int64_t)row * in + c;
    if constexpr (!F32) {
      const f16* b = reinterpret_cast<const f16*>(base_) + off;
      f16* d = reinterpret_cast<f16*>(dst_) + off;
      if constexpr (VEC) {      // (in % 8 == 0: the piece is inside as a whole)
        f16x8 v = *reinterpret_cast<const f16x8*>(b);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float s = tot[2 * t + (e >> 2)][e & 3];
          if (!is_zero_bits(s)) v[e] = (f16)((float)v[e] + s);
        }
        *reinterpret_cast<f16x8*>(d) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (c + e < in) {
            const float s = tot[2 * t + (e >> 2)][e & 3];
            const f16 x = b[e];
            d[e] = is_zero_bits(s) ? x : (f16)((float)x + s);
          }
        }
      }
    } else {
      const float* b = reinterpret_cast<const float*>(base_) + off;
      float* d = reinterpret_cast<float*>(dst_) + off;
      if constexpr (VEC) {      // (in % 4 == 0: each half of the piece is inside or outside as a whole)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          if (c + 4 * m < in) {
            f32x4 v = *reinterpret_cast<const f32x4*>(b + 4 * m);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float s = tot[2 * t + m][r];
              if (!is_zero_bits(s)) v[r] = v[r] + s;
            }
            *reinterpret_cast<f32x4*>(d + 4 * m) = v;
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          if (c + e < in) {
            const float s = tot[2 * t + (e >> 2)][e & 3];
            const float x = b[e];
            d[e] = is_zero_bits(s) ? x : x + s;
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" int i2v_lora_merge(void* dst, const void* base, int32_t is_f32, int32_t out, int32_t in, const i2v_lora_adapter* adapters,
                              int32_t n_adapters, i2v_stream_t stream) {
  I2V_CHECK_ARG(dst && base, "i2v_lora_merge: null pointer");
  I2V_CHECK_ARG(out >= 1 && in >= 1, "i2v_lora_merge: out %d in %d", out, in);
  I2V_CHECK_ARG(n_adapters >= 0 && n_adapters <= I2V_LORA_MAX_ADAPTERS, "i2v_lora_merge: %d adapters (at most %d in one launch)",
                n_adapters, I2V_LORA_MAX_ADAPTERS);
  I2V_CHECK_ARG(n_adapters == 0 || adapters, "i2v_lora_merge: null adapter list");
  I2V_CHECK_ARG((int64_t)out * in < (int64_t)1 << 40, "i2v_lora_merge: problem too large");
  I2V_CHECK_ARG(i2v_cdiv(out, LM_ROWS) <= 65535, "i2v_lora_merge: out %d exceeds the grid", out);
  const int64_t wbytes = (int64_t)out * in * (is_f32 ? 4 : 2);
  I2V_CHECK_ARG(!i2v_overlap(dst, wbytes, base, wbytes), "i2v_lora_merge: dst and base must not alias (base is not modified)");
  LoraAdapters ad = {};
  for (int j = 0; j < n_adapters; ++j) {
    const i2v_lora_adapter& a = adapters[j];
    I2V_CHECK_ARG(a.down && a.up, "i2v_lora_merge: adapter %d: null pointer", j);
    I2V_CHECK_ARG(a.rank >= 1 && a.rank <= I2V_LORA_MAX_RANK, "i2v_lora_merge: adapter %d: rank %d (1 .. %d)", j, a.rank,
                  I2V_LORA_MAX_RANK);
    I2V_CHECK_ARG(!i2v_overlap(dst, wbytes, a.down, (int64_t)a.rank * in * 2) && !i2v_overlap(dst, wbytes, a.up, (int64_t)out * a.rank * 2),
                  "i2v_lora_merge: adapter %d: dst must not alias a factor", j);
    ad.a[j] = a;
  }
  const bool vec = in % (is_f32 ? 4 : 8) == 0 && i2v_al16(dst) && i2v_al16(base);
  const dim3 grid((unsigned)i2v_cdiv(in, LM_COLS), (unsigned)i2v_cdiv(out, LM_ROWS));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define LM_LAUNCH(F32, VEC) \
  hipLaunchKernelGGL((lora_merge_kernel<F32, VEC>), grid, dim3(LM_THREADS), 0, st, dst, base, (int)out, (int)in, ad, (int)n_adapters)
  if (is_f32) {
    if (vec) LM_LAUNCH(true, true); else LM_LAUNCH(true, false);
  } else {
    if (vec) LM_LAUNCH(false, true); else LM_LAUNCH(false, false);
  }
#undef LM_LAUNCH
  return i2v_check_launch("i2v_lora_merge");
}
