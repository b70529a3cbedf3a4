// FreeNoise (diffusers AnimateDiffFreeNoiseMixin / FreeNoiseTransformerBlock): the motion modules' temporal attention runs on sliding
// windows of `length` frames, and every frame's result is the weighted mean of the windows that cover it.  The attention kernels
// already do everything inside a window -- a window is a `length`-frame clip of the (b, pixel, frame) row layout -- so the two kernels
// here only move rows:
//
//   gather   [(b, pixel), frame, C]     -> [(b, pixel), window, j, C]      row (p, w, j) = source row (p, starts[w] + j), bit for bit
//   blend    [(b, pixel), window, j, C] -> [(b, pixel), frame, C]          row (p, f)    = sum_k coef[f][k] * source row (p, idx[f][k])
//
// The window starts and the (source row, coefficient) pairs are small DEVICE tables (the trailing window is one more table row, a
// captured step holds no host value).  Both are gathers with one owner per output row: no atomics, no LDS, deterministic.  The blend
// accumulates in fp32 -- the first pair as a product, the others as fmas, pairs with coefficient 0 (the padding) neither read nor
// added -- and rounds once, so a frame with the single coefficient 1.0 leaves as the bits of its source row (-0.0 and NaN included).
//
// Pure HBM traffic.  The work item is one 16-byte chunk (8 channels) of one output row; consecutive lanes take consecutive chunks, so
// a wave moves 1 KiB of contiguous destination (rows are 640 - 2560 bytes: a wave covers 0.4 - 1.6 rows, every row piece a contiguous
// run on both sides).  One 64-bit division splits the item into (row, chunk); rows are below 2^31, so the rest is 32-bit arithmetic.
// The grid is capped at 8 workgroups of 256 per CU and strides over the rest.  Table indices are clamped to the buffer on the device:
// a corrupt table gives wrong numbers, never an access outside the operands.
#include "common.h"

namespace {

constexpr int FN_THREADS = 256;
constexpr int FN_MAX_BLOCKS = 256 * 8;
constexpr int FN_MAX_PAIRS = 33;      // ceil(length / stride) + 1 at length 32, stride 1

__global__ __launch_bounds__(FN_THREADS) void freenoise_gather_kernel(const f16* __restrict__ src, int64_t ld_src, f16* __restrict__ dst,
                                                                      int64_t ld_dst, const int32_t* __restrict__ starts, int frames,
                                                                      int windows, int length, int chunks, int64_t total) {
  const int per_pixel = windows * length;
  for (int64_t i = (int64_t)blockIdx.x * FN_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * FN_THREADS) {
    const int64_t row64 = i / chunks;                     // the one 64-bit division: rows are below 2^31, the rest is 32-bit
    const unsigned row = (unsigned)row64, ch = (unsigned)(i - row64 * chunks);
    const unsigned pix = row / (unsigned)per_pixel, rem = row - pix * (unsigned)per_pixel;
    const unsigned w = rem / (unsigned)length, j = rem - w * (unsigned)length;
    int s = starts[w];
    s = s < 0 ? 0 : (s > frames - length ? frames - length : s);
    *reinterpret_cast<f16x8*>(dst + row64 * ld_dst + 8 * ch) =
        ld_global_16B(src + ((int64_t)pix * frames + s + (int)j) * ld_src + 8 * ch);
  }
}

__global__ __launch_bounds__(FN_THREADS) void freenoise_blend_kernel(const f16* __restrict__ src, int64_t ld_src, f16* __restrict__ dst,
                                                                     int64_t ld_dst, const int32_t* __restrict__ idx,
                                                                     const float* __restrict__ coef, int frames, int per_pixel, int pairs,
                                                                     int chunks, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * FN_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * FN_THREADS) {
    const int64_t row = i / chunks;                       // the one 64-bit division: rows are below 2^31, the rest is 32-bit
    const unsigned ch = (unsigned)(i - row * chunks);
    const unsigned pix = (unsigned)row / (unsigned)frames;
    const int f = (int)((unsigned)row - pix * (unsigned)frames);
    const f16* base = src + (int64_t)pix * per_pixel * ld_src + 8 * ch;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int k = 0; k < pairs; ++k) {
      const float a = coef[f * pairs + k];
      if (k > 0 && a == 0.f) continue;                       // padding: not read
      int r = idx[f * pairs + k];
      r = r < 0 ? 0 : (r >= per_pixel ? per_pixel - 1 : r);
      const f16x8 v = ld_global_16B(base + (int64_t)r * ld_src);
      if (k == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = a * (float)v[e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(a, (float)v[e], acc[e]);
      }
    }
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)acc[e];
    *reinterpret_cast<f16x8*>(dst + row * ld_dst + 8 * ch) = o;
  }
}

// the checks the two entry points share; `what` names the entry point
int fn_check(const char* what, const void* src, int64_t ld_src, const void* dst, int64_t ld_dst, int64_t n_pixels, int32_t frames,
             int32_t windows, int32_t length, int32_t c, int64_t src_rows, int64_t dst_rows) {
  I2V_CHECK_ARG(src && dst, "%s: null pointer", what);
  I2V_CHECK_ARG(n_pixels > 0 && windows > 0, "%s: n_pixels %lld windows %d must be positive", what, (long long)n_pixels, windows);
  I2V_CHECK_ARG(length >= 1 && length <= frames, "%s: length %d must be in [1, frames %d]", what, length, frames);
  I2V_CHECK_ARG(windows <= frames, "%s: %d windows for %d frames", what, windows, frames);
  I2V_CHECK_ARG(c > 0 && c % 8 == 0, "%s: c %d must be a positive multiple of 8", what, c);
  I2V_CHECK_ARG(ld_src >= c && ld_dst >= c && ld_src % 8 == 0 && ld_dst % 8 == 0 && ld_src < (1 << 20) && ld_dst < (1 << 20),
                "%s: row strides %lld / %lld must be multiples of 8, at least c %d", what, (long long)ld_src, (long long)ld_dst, c);
  I2V_CHECK_ARG(i2v_al16(src) && i2v_al16(dst), "%s: pointers must be 16-byte aligned", what);
  I2V_CHECK_ARG(src_rows < ((int64_t)1 << 31) && dst_rows < ((int64_t)1 << 31), "%s: problem too large (%lld / %lld rows)", what,
                (long long)src_rows, (long long)dst_rows);
  I2V_CHECK_ARG(!i2v_overlap(src, ((src_rows - 1) * ld_src + c) * 2, dst, ((dst_rows - 1) * ld_dst + c) * 2),
                "%s: dst is a new tensor (it must not overlap src)", what);
  return I2V_OK;
}

}  // namespace

extern "C" int i2v_freenoise_gather_f16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, const int32_t* starts, int64_t n_pixels,
                                        int32_t frames, int32_t windows, int32_t length, int32_t c, i2v_stream_t stream) {
  const int64_t src_rows = n_pixels * frames, dst_rows = n_pixels * windows * length;
  const int rc = fn_check("i2v_freenoise_gather_f16", src, ld_src, dst, ld_dst, n_pixels, frames, windows, length, c, src_rows, dst_rows);
  if (rc != I2V_OK) return rc;
  I2V_CHECK_ARG(starts != nullptr, "i2v_freenoise_gather_f16: null window table");
  const int chunks = c / 8;
  const int64_t total = dst_rows * chunks;
  hipLaunchKernelGGL(freenoise_gather_kernel, dim3(i2v_ew_grid(total, FN_THREADS, FN_MAX_BLOCKS)), dim3(FN_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(src), ld_src, reinterpret_cast<f16*>(dst), ld_dst, starts, frames, windows, length, chunks,
                     total);
  return i2v_check_launch("i2v_freenoise_gather_f16");
}

extern "C" int i2v_freenoise_blend_f16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, const int32_t* idx, const float* coef,
                                       int64_t n_pixels, int32_t frames, int32_t windows, int32_t length, int32_t pairs, int32_t c,
                                       i2v_stream_t stream) {
  const int64_t src_rows = n_pixels * windows * length, dst_rows = n_pixels * frames;
  const int rc = fn_check("i2v_freenoise_blend_f16", src, ld_src, dst, ld_dst, n_pixels, frames, windows, length, c, src_rows, dst_rows);
  if (rc != I2V_OK) return rc;
  I2V_CHECK_ARG(idx != nullptr && coef != nullptr, "i2v_freenoise_blend_f16: null pair table");
  I2V_CHECK_ARG(pairs >= 1 && pairs <= FN_MAX_PAIRS, "i2v_freenoise_blend_f16: pairs %d must be in [1, %d]", pairs, FN_MAX_PAIRS);
  const int chunks = c / 8;
  const int64_t total = dst_rows * chunks;
  hipLaunchKernelGGL(freenoise_blend_kernel, dim3(i2v_ew_grid(total, FN_THREADS, FN_MAX_BLOCKS)), dim3(FN_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(src), ld_src, reinterpret_cast<f16*>(dst), ld_dst, idx, coef, frames, windows * length, pairs,
                     chunks, total);
  return i2v_check_launch("i2v_freenoise_blend_f16");
}
