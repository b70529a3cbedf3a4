// Prompt travel (diffusers AnimateDiffFreeNoiseMixin, `prompt` as a dict {frame: text}): one text context per frame, interpolated
// between the keyframes' embeddings.
//   i2v_interp_rows_f16   out[r] = (1 - w[r]) * src[lo[r]] + w[r] * src[hi[r]]      rows of E fp16 values, tables on the device
// One launch makes the per-frame contexts of a whole batch from the K encoded keyframe prompts; with w = 0 everywhere the same
// launch is a row gather (the IP-Adapter's image tokens, one set per sample -> one set per frame).
//
// Memory-bound: one 16-byte chunk (8 fp16) per lane and access, a capped grid that strides over the chunks of all rows.  A row
// with w == 0 reads only src[lo] and one with w == 1 only src[hi]: both are copies, bit for bit, and the row that is not
// referenced is never loaded (a NaN there cannot reach the output).
#include "common.h"

namespace {

constexpr int IR_THREADS = 256;
constexpr int IR_MAX_BLOCKS = 2048;

__global__ __launch_bounds__(IR_THREADS) void interp_rows_kernel(const f16* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ lo,
                                                                  const int32_t* __restrict__ hi, const float* __restrict__ wt,
                                                                  f16* __restrict__ out, int64_t ld_out, uint32_t chunks, uint32_t e8) {
  const uint32_t stride = gridDim.x * IR_THREADS;
  for (uint32_t q = blockIdx.x * IR_THREADS + threadIdx.x; q < chunks; q += stride) {      // chunks < 2^31 - stride (host check)
    const uint32_t r = q / e8, c = q - r * e8;
    const float w = wt[r];
    f16x8 o;
    if (w == 0.0f) {
      o = ld_global_16B(src + (int64_t)lo[r] * ld_src + c * 8);
    } else if (w == 1.0f) {
      o = ld_global_16B(src + (int64_t)hi[r] * ld_src + c * 8);
    } else {
      const f16x8 a = ld_global_16B(src + (int64_t)lo[r] * ld_src + c * 8);
      const f16x8 b = ld_global_16B(src + (int64_t)hi[r] * ld_src + c * 8);
      const float u = 1.0f - w;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (f16)fmaf(w, (float)b[j], u * (float)a[j]);      // fp32, one rounding to fp16
    }
    *reinterpret_cast<f16x8*>(out + (int64_t)r * ld_out + c * 8) = o;
  }
}

}  // namespace

extern "C" int i2v_interp_rows_f16(const void* src, int64_t ld_src, int32_t n_src, const int32_t* lo, const int32_t* hi, const float* w,
                                   void* out, int64_t ld_out, int32_t n_out, int32_t e, i2v_stream_t stream) {
  I2V_CHECK_ARG(src && lo && hi && w && out, "i2v_interp_rows_f16: null pointer");
  I2V_CHECK_ARG(n_src > 0 && n_out > 0, "i2v_interp_rows_f16: n_src %d, n_out %d must be positive", n_src, n_out);
  I2V_CHECK_ARG(e > 0 && e % 8 == 0, "i2v_interp_rows_f16: e %d must be a positive multiple of 8", e);
  I2V_CHECK_ARG(ld_src >= e && ld_out >= e && ld_src % 8 == 0 && ld_out % 8 == 0,
                "i2v_interp_rows_f16: row strides %lld / %lld must be multiples of 8 and at least e = %d", (long long)ld_src,
                (long long)ld_out, e);
  I2V_CHECK_ARG(i2v_al16(src) && i2v_al16(out), "i2v_interp_rows_f16: src and out must be 16-byte aligned");
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(lo) & 3) == 0 && (reinterpret_cast<uintptr_t>(hi) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(w) & 3) == 0,
                "i2v_interp_rows_f16: lo / hi / w must be 4-byte aligned");
  const int64_t chunks = (int64_t)n_out * (e / 8);
  I2V_CHECK_ARG(chunks < ((int64_t)1 << 31) - (int64_t)IR_MAX_BLOCKS * IR_THREADS && ld_src < ((int64_t)1 << 40) &&
                    ld_out < ((int64_t)1 << 40),
                "i2v_interp_rows_f16: problem too large");
  I2V_CHECK_ARG(!i2v_overlap(out, ((int64_t)(n_out - 1) * ld_out + e) * 2, src, ((int64_t)(n_src - 1) * ld_src + e) * 2),
                "i2v_interp_rows_f16: out overlaps src");
  hipLaunchKernelGGL(interp_rows_kernel, dim3(i2v_ew_grid(chunks, IR_THREADS, IR_MAX_BLOCKS)), dim3(IR_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(src), ld_src, lo, hi, w,
                     reinterpret_cast<f16*>(out), ld_out, (uint32_t)chunks, (uint32_t)(e / 8));
  return i2v_check_launch("i2v_interp_rows_f16");
}
