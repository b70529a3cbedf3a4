// The exit of the Real-ESRGAN compact upscaler (SRVGGNetCompact, upscaler.py): PixelShuffle(s) of the exit convolution's result plus the
// nearest-upsampled source, the clamp and the range map, token-major fp16 -> NCHW fp32 in one launch (i2v_pixel_shuffle_add_f32).
//
//   out[n, col, s y + dy, s x + dx] = range( clamp( float(y[n, y, x, (col s + dy) s + dx]) + entry(src[n, col, y, x]) ) )
//
// Memory-bound: 4 s^2 bytes written per 2 s^2 read.  One lane owns the s contiguous outputs (dx = 0 .. s - 1) of one (colour, dy) of
// one input pixel -- 16 bytes at s = 4 -- and a wave owns 64 consecutive input pixels of a row for ONE (colour, dy): its store is
// 64 s contiguous floats of an output row.  The 3 s (colour, dy) pairs of the same 64 pixels are consecutive waves of the flat index,
//   item = (((n H + y) XC + xc) 3 s + (col s + dy)) 64 + lane,      x = 64 xc + lane,      XC = ceil(W / 64),
// so the pixels of y of which a wave reads 2 s bytes each (of the 6 s^2 that the exit uses) are read by the waves next to it while
// they are in the caches, and the source row likewise.  Lanes with x >= W idle (a row's last chunk).
#include "common.h"

namespace {

struct PsArgs {
  const f16* y;
  const void* src;
  float* out;
  int64_t ld;
  uint32_t groups;      // n H XC 3 s: 64-lane groups
  int32_t H, W, XC;
  int32_t unit_in, clamp, signed_out;
};

template <int S, bool F32>
__global__ __launch_bounds__(256) void pixel_shuffle_add_kernel(const PsArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t gstride = gridDim.x * 4;
  for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < a.groups; g += gstride) {      // groups < 2^31 - 2^20: no wrap
    const uint32_t pair = g % (3 * S), r0 = g / (3 * S);
    const uint32_t xc = r0 % (uint32_t)a.XC, r1 = r0 / (uint32_t)a.XC;
    const uint32_t yy = r1 % (uint32_t)a.H, n = r1 / (uint32_t)a.H;
    const uint32_t col = pair / S, dy = pair - col * S;
    const uint32_t x = xc * 64 + lane;
    if (x >= (uint32_t)a.W) continue;
    const int64_t pix = ((int64_t)n * a.H + yy) * a.W + x;
    const int64_t si = (((int64_t)n * 3 + col) * a.H + yy) * a.W + x;
    float base = F32 ? reinterpret_cast<const float*>(a.src)[si] : (float)reinterpret_cast<const f16*>(a.src)[si];
    if (a.unit_in) base = fminf(fmaxf((base + 1.0f) * 0.5f, 0.0f), 1.0f);
    const f16* yp = a.y + pix * a.ld + pair * S;
    float v[S];
    if constexpr (S == 4) {
      const f16x4 t = *reinterpret_cast<const f16x4*>(yp);        // 8-byte aligned: ld % 8 == 0, pair * 4 elements
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (float)t[j];
    } else if constexpr (S == 2) {
      const f16x2 t = *reinterpret_cast<const f16x2*>(yp);
      v[0] = (float)t[0], v[1] = (float)t[1];
    } else {
#pragma unroll
      for (int j = 0; j < S; ++j) v[j] = (float)yp[j];
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
      float t = v[j] + base;
      if (a.clamp) t = fminf(fmaxf(t, 0.0f), 1.0f);
      if (a.signed_out) t = 2.0f * t - 1.0f;
      v[j] = t;
    }
    // (n, col, s yy + dy, s x): the flat output index is S times the lane's index in the row-major [n, 3, s H, W] grid
    float* op = a.out + (((((int64_t)n * 3 + col) * a.H + yy) * S + dy) * a.W + x) * S;
    if constexpr (S == 4) {
      *reinterpret_cast<f32x4*>(op) = f32x4{v[0], v[1], v[2], v[3]};
    } else if constexpr (S == 2) {
      *reinterpret_cast<f32x2*>(op) = f32x2{v[0], v[1]};
    } else {
#pragma unroll
      for (int j = 0; j < S; ++j) op[j] = v[j];
    }
  }
}

template <int S>
void ps_launch(const PsArgs& a, const bool f32, const unsigned grid, hipStream_t st) {
  if (f32)
    hipLaunchKernelGGL((pixel_shuffle_add_kernel<S, true>), dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((pixel_shuffle_add_kernel<S, false>), dim3(grid), dim3(256), 0, st, a);
}

}  // namespace

extern "C" int i2v_pixel_shuffle_add_f32(const void* y, int64_t ld, const void* src, int32_t src_is_f32, float* out, int32_t n, int32_t h,
                                         int32_t w, int32_t s, int32_t entry_mode, int32_t clamp, int32_t signed_out, i2v_stream_t stream) {
  I2V_CHECK_ARG(s >= 1 && s <= 4, "i2v_pixel_shuffle_add_f32: s %d must be 1..4", s);
  I2V_CHECK_ARG(y && src && out, "i2v_pixel_shuffle_add_f32: null pointer");
  I2V_CHECK_ARG(n >= 1 && h >= 1 && w >= 1, "i2v_pixel_shuffle_add_f32: n %d, h %d, w %d must be positive", n, h, w);
  I2V_CHECK_ARG(ld >= 64 && ld % 8 == 0 && ld < (1 << 20), "i2v_pixel_shuffle_add_f32: pixel stride ld %lld must be >= 64 and a multiple of 8",
                (long long)ld);
  I2V_CHECK_ARG(entry_mode == I2V_TAESD_PREP_IDENTITY || entry_mode == I2V_TAESD_PREP_UNIT_CLAMP,
                "i2v_pixel_shuffle_add_f32: entry_mode %d must be I2V_TAESD_PREP_IDENTITY or I2V_TAESD_PREP_UNIT_CLAMP", entry_mode);
  I2V_CHECK_ARG(i2v_al16(y) && i2v_al16(out) && (reinterpret_cast<uintptr_t>(src) & (src_is_f32 ? 3 : 1)) == 0,
                "i2v_pixel_shuffle_add_f32: y and out must be 16-byte aligned, src aligned to its element");
  const int64_t pixels = (int64_t)n * h * w, numel = pixels * 3 * s * s;
  const int64_t xc = i2v_cdiv(w, 64), groups = (int64_t)n * h * xc * 3 * s;
  const int64_t lim = ((int64_t)1 << 31) - (1 << 20);
  I2V_CHECK_ARG(pixels < lim && groups < lim && numel < ((int64_t)1 << 40), "i2v_pixel_shuffle_add_f32: problem too large");
  const int64_t yb = ((pixels - 1) * ld + 3 * s * s) * 2, sb = pixels * 3 * (src_is_f32 ? 4 : 2);
  I2V_CHECK_ARG(!i2v_overlap(out, numel * 4, y, yb) && !i2v_overlap(out, numel * 4, src, sb), "i2v_pixel_shuffle_add_f32: out overlaps y or src");
  PsArgs a;
  a.y = reinterpret_cast<const f16*>(y);
  a.src = src;
  a.out = out;
  a.ld = ld;
  a.groups = (uint32_t)groups;
  a.H = h;
  a.W = w;
  a.XC = (int32_t)xc;
  a.unit_in = entry_mode == I2V_TAESD_PREP_UNIT_CLAMP;
  a.clamp = clamp != 0;
  a.signed_out = signed_out != 0;
  const unsigned grid = i2v_ew_grid(groups * 64, 256, 8192);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool f32 = src_is_f32 != 0;
  if (s == 1)
    ps_launch<1>(a, f32, grid, st);
  else if (s == 2)
    ps_launch<2>(a, f32, grid, st);
  else if (s == 3)
    ps_launch<3>(a, f32, grid, st);
  else
    ps_launch<4>(a, f32, grid, st);
  return i2v_check_launch("i2v_pixel_shuffle_add_f32");
}

// The exit of RRDBNet (upscaler.RRDBNet): there is no shuffle and no base, only the layout change, the caller's clamp and the range map,
//   out[n, col, y, x] = range( clamp( float(y[n, y, x, col]) ) ),      token-major fp16 (pixel stride >= 3, any) -> NCHW fp32.
// One lane per pixel: three 2-byte loads of one pixel, three stores that are contiguous across the wave (one per colour plane).
namespace {

__global__ __launch_bounds__(256) void rgb_exit_kernel(const f16* __restrict__ y, const int64_t ld, float* __restrict__ out, const int64_t pixels,
                                                       const int64_t hw, const int clamp, const int signed_out) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += stride) {
    const int64_t img = i / hw, px = i - img * hw;
#pragma unroll
    for (int col = 0; col < 3; ++col) {
      float v = (float)y[i * ld + col];
      if (clamp) v = fminf(fmaxf(v, 0.0f), 1.0f);
      if (signed_out) v = 2.0f * v - 1.0f;
      out[(img * 3 + col) * hw + px] = v;
    }
  }
}

}  // namespace

extern "C" int i2v_rgb_exit_f32(const void* y, int64_t ld, float* out, int32_t n, int32_t h, int32_t w, int32_t clamp, int32_t signed_out,
                                i2v_stream_t stream) {
  I2V_CHECK_ARG(y && out, "i2v_rgb_exit_f32: null pointer");
  I2V_CHECK_ARG(n >= 1 && h >= 1 && w >= 1, "i2v_rgb_exit_f32: n %d, h %d, w %d must be positive", n, h, w);
  I2V_CHECK_ARG(ld >= 3 && ld < (1 << 20), "i2v_rgb_exit_f32: pixel stride ld %lld must be >= 3", (long long)ld);
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(y) & 1) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                "i2v_rgb_exit_f32: y and out must be aligned to their elements");
  const int64_t hw = (int64_t)h * w, pixels = hw * n;
  I2V_CHECK_ARG(pixels < ((int64_t)1 << 36), "i2v_rgb_exit_f32: problem too large");
  I2V_CHECK_ARG(!i2v_overlap(out, pixels * 12, y, ((pixels - 1) * ld + 3) * 2), "i2v_rgb_exit_f32: out overlaps y");
  const unsigned grid = i2v_ew_grid(pixels, 256, 8192);
  hipLaunchKernelGGL(rgb_exit_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(y), ld, out,
                     pixels, hw, clamp != 0, signed_out != 0);
  return i2v_check_launch("i2v_rgb_exit_f32");
}
