// Prompt weighting (the `(text:1.3)` / `[text]` emphasis syntax; pipeline `encode_weighted_prompt`): every token's embedding times its
// weight, then the whole prompt rescaled so that its mean is the unweighted one.
//   i2v_weight_embeds_f16   out[p, t, :] = fp16((float(src[p, t, :]) * w[p, t]) * r[p]),   r[p] = sum(src[p]) / sum(w[p] * src[p])
// Once per sample, not per step.  One workgroup per prompt does both passes: pass 1 the two fp32 sums over the prompt's tokens * dim
// values, a barrier, pass 2 the apply, which reads src again (355 KB at 231 x 768: from L2).  16-byte loads and stores, no atomics, no
// workspace.  The sums have ONE order -- per lane over a fixed stride, then the wave's butterfly, then the waves' partials from LDS in
// wave order, the same in every lane -- so repeats are bit-equal and the result does not depend on where the workgroup ran; with all
// weights 1 the two sums are the same sequence of operations, r == 1.0f and out is src bit for bit.
#include "common.h"

namespace {

constexpr int PW_THREADS = 1024;
constexpr int PW_WAVES = PW_THREADS / I2V_WAVE;

__device__ __forceinline__ float wave_sum_all(float x) {      // butterfly: every lane ends with the same bits
#pragma unroll
  for (int m = 1; m < I2V_WAVE; m <<= 1) x += __shfl_xor(x, m, I2V_WAVE);
  return x;
}

__global__ __launch_bounds__(PW_THREADS) void weight_embeds_kernel(const f16* src_,const float* __restrict__ weights, f16* out_,
                                                                    float* __restrict__ ratio_out, uint32_t tokens, uint32_t d8,
                                                                    uint32_t ld_src, uint32_t ld_out, int restore_mean) {
#pragma clang fp contract(off)      // S1 sums the ROUNDED products w * x: with w == 1 it is S0's sequence of operations
  __shared__ float part[2][PW_WAVES];
  const uint32_t p = blockIdx.x;
  // no __restrict__ on src / out: they may be the same buffer (in place); the barrier orders pass 1's loads before pass 2's stores
  const f16* src = src_ + (int64_t)p * tokens * ld_src;
  f16* out = out_ + (int64_t)p * tokens * ld_out;
  const float* w = weights + (int64_t)p * tokens;
  const uint32_t chunks = tokens * d8;                          // tokens * ld < 2^31 (host check), d8 * 8 <= ld
  float r = 1.0f;
  if (restore_mean) {
    float s0 = 0.0f, s1 = 0.0f;
    for (uint32_t q = threadIdx.x; q < chunks; q += PW_THREADS) {
      const uint32_t t = q / d8, c = q - t * d8;
      const f16x8 v = ld_global_16B(src + t * ld_src + c * 8);
      const float wt = w[t];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = (float)v[j];
        s0 += x;
        s1 += wt * x;
      }
    }
    s0 = wave_sum_all(s0);
    s1 = wave_sum_all(s1);
    if ((threadIdx.x & (I2V_WAVE - 1)) == 0) {
      part[0][threadIdx.x / I2V_WAVE] = s0;
      part[1][threadIdx.x / I2V_WAVE] = s1;
    }
    __syncthreads();      // also: every load of pass 1 has returned before any store of pass 2 (out may be src)
    s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (int i = 0; i < PW_WAVES; ++i) {
      s0 += part[0][i];
      s1 += part[1][i];
    }
    r = s0 / s1;
  }
  if (threadIdx.x == 0 && ratio_out) ratio_out[p] = r;
  // not finite (the weights cancel the mean, or the mean is 0 / 0): the outputs take 1, the caller reads the ratio.  Tested on the
  // bits: the library is built with -fno-honor-nans
  if ((__builtin_bit_cast(uint32_t, r) & 0x7f800000u) == 0x7f800000u) r = 1.0f;
  for (uint32_t q = threadIdx.x; q < chunks; q += PW_THREADS) {
    const uint32_t t = q / d8, c = q - t * d8;
    const f16x8 v = ld_global_16B(src + t * ld_src + c * 8);
    const float wt = w[t];
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)(((float)v[j] * wt) * r);      // two fp32 multiplies, one rounding to nearest even
    *reinterpret_cast<f16x8*>(out + t * ld_out + c * 8) = o;
  }
}

}  // namespace

extern "C" int i2v_weight_embeds_f16(const void* src, const float* weights, void* out, float* ratio_out, int32_t n_prompts, int32_t tokens,
                                     int32_t dim, int64_t ld_src, int64_t ld_out, int32_t restore_mean, i2v_stream_t stream) {
  I2V_CHECK_ARG(src && weights && out, "i2v_weight_embeds_f16: null pointer");
  I2V_CHECK_ARG(n_prompts > 0 && tokens > 0, "i2v_weight_embeds_f16: n_prompts %d, tokens %d must be positive", n_prompts, tokens);
  I2V_CHECK_ARG(dim > 0 && dim % 8 == 0, "i2v_weight_embeds_f16: dim %d must be a positive multiple of 8", dim);
  I2V_CHECK_ARG(ld_src >= dim && ld_out >= dim && ld_src % 8 == 0 && ld_out % 8 == 0,
                "i2v_weight_embeds_f16: row strides %lld / %lld must be multiples of 8 and at least dim = %d", (long long)ld_src,
                (long long)ld_out, dim);
  I2V_CHECK_ARG(i2v_al16(src) && i2v_al16(out), "i2v_weight_embeds_f16: src and out must be 16-byte aligned");
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(weights) & 3) == 0 && (reinterpret_cast<uintptr_t>(ratio_out) & 3) == 0,
                "i2v_weight_embeds_f16: weights and ratio_out must be 4-byte aligned");
  I2V_CHECK_ARG((int64_t)tokens * ld_src < ((int64_t)1 << 31) && (int64_t)tokens * ld_out < ((int64_t)1 << 31),
                "i2v_weight_embeds_f16: problem too large (tokens * row stride must be below 2^31)");
  const int64_t rows = (int64_t)n_prompts * tokens;
  const int64_t nb_src = ((rows - 1) * ld_src + dim) * 2, nb_out = ((rows - 1) * ld_out + dim) * 2;
  I2V_CHECK_ARG((src == out && ld_src == ld_out) || !i2v_overlap(out, nb_out, src, nb_src),
                "i2v_weight_embeds_f16: out overlaps src (in place is out == src with equal row strides)");
  I2V_CHECK_ARG(!i2v_overlap(weights, rows * 4, out, nb_out) && (!ratio_out || !i2v_overlap(ratio_out, (int64_t)n_prompts * 4, out, nb_out)),
                "i2v_weight_embeds_f16: out overlaps weights or ratio_out");
  hipLaunchKernelGGL(weight_embeds_kernel, dim3((unsigned)n_prompts), dim3(PW_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(src), weights, reinterpret_cast<f16*>(out), ratio_out, (uint32_t)tokens,
                     (uint32_t)(dim / 8), (uint32_t)ld_src, (uint32_t)ld_out, (int)restore_mean);
  return i2v_check_launch("i2v_weight_embeds_f16");
}
