// T2I-Adapter (diffusers 0.24 T2IAdapter, adapter_type "full_adapter"): the three movers of the once-per-sample network
//   i2v_pixel_unshuffle8_f16   PixelUnshuffle(8) of the control frames, NCHW fp32 / fp16 -> tokens fp16
//   i2v_avgpool2x_f16          AvgPool2d(2, stride 2, ceil_mode=True) on tokens
//   i2v_relu_f16               the resnets' activation
// and the one kernel that runs inside a denoising step,
//   i2v_add_broadcast_residual_f16   out[i] = x[i] + s * feat[i mod feat_numel],   s = scale_table[min(step_idx[0], rows - 1)]
// The adapter's features depend on the control frames only, so a step adds four stored tensors to the UNet's down path and launches
// nothing else.  The modulo lets ONE copy of the features serve both classifier-free-guidance halves of the batch.
//
// All four are memory-bound: one 16-byte chunk (8 fp16) per lane and access, a capped grid that strides.  The add has the shape of
// i2v_add_residuals_f16 (controlnet.hip) -- AB_UNROLL independent accesses per lane in flight, 16 KB tiles -- and its arithmetic
// (ar_chunk, residual_chunk.h), so both give the same bits for the same operands.
#include "common.h"
#include "residual_chunk.h"

namespace {

constexpr int EW_THREADS = 256;
constexpr int EW_MAX_BLOCKS = 4096;

// ---------------------------------------------------------------------------------------------------------- pixel unshuffle
// chunk q of the output = (image n, pixel (y, x), channel c, row dy of the 8 x 8 patch): its 8 values are the 8 consecutive source
// pixels src[n][c][8 y + dy][8 x .. 8 x + 7] -- PyTorch's channel order c * 64 + dy * 8 + dx.  Stores are consecutive over the lanes.
template <typename T>
__global__ __launch_bounds__(EW_THREADS) void pixel_unshuffle8_kernel(const T* __restrict__ src, f16* __restrict__ dst, int64_t chunks, int c,
                                                                       int oh, int ow) {
  const int64_t stride = (int64_t)gridDim.x * EW_THREADS;
  const int w = ow * 8;
  for (int64_t q = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; q < chunks; q += stride) {
    const int dy = (int)(q & 7);
    const int64_t t = q >> 3;
    const int ch = (int)(t % c);
    const int64_t pix = t / c;
    const int x = (int)(pix % ow);
    const int64_t row = pix / ow;
    const int y = (int)(row % oh);
    const int64_t n = row / oh;
    const T* s = src + (((n * c + ch) * oh * 8 + (8 * y + dy)) * (int64_t)w + 8 * x);
    f16x8 o;
    if constexpr (std::is_same<T, float>::value) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(s), b = *reinterpret_cast<const f32x4*>(s + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = (f16)a[j];
        o[4 + j] = (f16)b[j];
      }
    } else {
      o = *reinterpret_cast<const f16x8*>(s);
    }
    *reinterpret_cast<f16x8*>(dst + q * 8) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------- average pool
// out[n, oy, ox, :] = mean of the in-bounds taps of the 2 x 2 window (ceil_mode: the last row / column of an odd size holds 2 or 1):
// fp32 sum times 1, 1/2 or 1/4 (exact factors), one rounding
__global__ __launch_bounds__(EW_THREADS) void avgpool2x_kernel(const f16* __restrict__ src, f16* __restrict__ dst, int64_t chunks, int h, int w,
                                                                int c8) {
  const int64_t stride = (int64_t)gridDim.x * EW_THREADS;
  const int oh = (h + 1) >> 1, ow = (w + 1) >> 1;
  for (int64_t q = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; q < chunks; q += stride) {
    const int cc = (int)(q % c8);
    const int64_t pix = q / c8;
    const int ox = (int)(pix % ow);
    const int64_t row = pix / ow;
    const int oy = (int)(row % oh);
    const int64_t n = row / oh;
    const int ny = 2 * oy + 1 < h ? 2 : 1, nx = 2 * ox + 1 < w ? 2 : 1;
    const f16* base = src + (((n * h + 2 * oy) * w + 2 * ox) * (int64_t)c8 + cc) * 8;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int dy = 0; dy < ny; ++dy)
      for (int dx = 0; dx < nx; ++dx) {
        const f16x8 v = ld_global_16B(base + ((int64_t)dy * w + dx) * c8 * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
      }
    const float inv = ny * nx == 4 ? 0.25f : (ny * nx == 2 ? 0.5f : 1.0f);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)(acc[j] * inv);
    *reinterpret_cast<f16x8*>(dst + q * 8) = o;
  }
}

// ---------------------------------------------------------------------------------------------------------- ReLU
__global__ __launch_bounds__(EW_THREADS) void relu_kernel(const f16* src, f16* dst, int64_t chunks) {
  const int64_t stride = (int64_t)gridDim.x * EW_THREADS;
  for (int64_t q = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; q < chunks; q += stride) {
    f16x8 v = ld_global_16B(src + q * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = v[j] < (f16)0 ? (f16)0 : v[j];
    *reinterpret_cast<f16x8*>(dst + q * 8) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------- the per-step add
constexpr int AB_THREADS = 256;
constexpr int AB_UNROLL = 4;
constexpr int AB_TILE = AB_THREADS * AB_UNROLL;      // 16-byte chunks per tile: 16 KB of each operand
constexpr int AB_MAX_BLOCKS = 2048;

struct AbArgs {
  f16* dst;
  f16* dst_lo;
  const f16* x;
  const f16* x_lo;
  const f16* feat;
  int64_t chunks;                                      // 16-byte chunks of x
  uint32_t fchunks;                                    // ... of feat (chunks % fchunks == 0): the wrap point is chunk-aligned
  uint32_t tiles;
  int32_t scale_rows;
  const float* scale_table;
  const int32_t* step_idx;
};

// the feature chunk of x's chunk `base + off`, from base_mod = base mod fchunks (uniform over the workgroup) and off < AB_TILE
__device__ __forceinline__ uint32_t ab_wrap(uint32_t base_mod, uint32_t off, uint32_t fchunks) {
  const uint32_t m = base_mod + off;                   // < 2^31 + AB_TILE: the host refuses fchunks >= 2^31
  if (fchunks >= (uint32_t)AB_TILE) return m >= fchunks ? m - fchunks : m;      // at most one wrap inside a tile
  return m % fchunks;
}

template <bool HAS_LO>
__device__ __forceinline__ void ab_tile(const AbArgs& a, int64_t base, uint32_t base_mod, float s) {
  f16x8 hi[AB_UNROLL], lo[AB_UNROLL], r[AB_UNROLL];
#pragma unroll
  for (int u = 0; u < AB_UNROLL; ++u) {
    const uint32_t off = threadIdx.x + u * AB_THREADS;
    const int64_t c = base + off;
    if (c < a.chunks) {
      hi[u] = ld_global_16B(a.x + c * 8);
      r[u] = ld_global_16B(a.feat + (int64_t)ab_wrap(base_mod, off, a.fchunks) * 8);
      if (HAS_LO) lo[u] = ld_global_16B(a.x_lo + c * 8);
    }
  }
#pragma unroll
  for (int u = 0; u < AB_UNROLL; ++u) {
    const int64_t c = base + threadIdx.x + u * AB_THREADS;
    if (c < a.chunks) {
      f16x8 o, ol;
      ar_chunk<HAS_LO>(hi[u], lo[u], r[u], s, o, ol);
      *reinterpret_cast<f16x8*>(a.dst + c * 8) = o;
      if (HAS_LO) *reinterpret_cast<f16x8*>(a.dst_lo + c * 8) = ol;
    }
  }
}

__global__ __launch_bounds__(AB_THREADS) void add_broadcast_residual_kernel(const AbArgs a) {
  float s = 1.0f;
  if (a.scale_table) {
    int row = a.step_idx ? a.step_idx[0] : 0;
    row = row < 0 ? 0 : (row > a.scale_rows - 1 ? a.scale_rows - 1 : row);
    s = a.scale_table[row];
  }
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t base = (int64_t)tile * AB_TILE;
    const uint32_t base_mod = (uint32_t)((uint64_t)base % a.fchunks);
    if (a.x_lo)
      ab_tile<true>(a, base, base_mod, s);
    else
      ab_tile<false>(a, base, base_mod, s);
  }
}

}  // namespace

extern "C" int i2v_pixel_unshuffle8_f16(const void* src, int32_t src_is_f32, void* dst, int32_t n, int32_t c, int32_t h, int32_t w,
                                        i2v_stream_t stream) {
  I2V_CHECK_ARG(src && dst, "i2v_pixel_unshuffle8_f16: null pointer");
  I2V_CHECK_ARG(n >= 1 && (c == 1 || c == 3), "i2v_pixel_unshuffle8_f16: n %d, c %d (1 or 3)", n, c);
  I2V_CHECK_ARG(h >= 8 && w >= 8 && h % 8 == 0 && w % 8 == 0, "i2v_pixel_unshuffle8_f16: h %d, w %d must be positive multiples of 8", h, w);
  I2V_CHECK_ARG(i2v_al16(src) && i2v_al16(dst), "i2v_pixel_unshuffle8_f16: src and dst must be 16-byte aligned");
  const int64_t elems = (int64_t)n * c * h * w;
  I2V_CHECK_ARG(elems < ((int64_t)1 << 40), "i2v_pixel_unshuffle8_f16: problem too large");
  I2V_CHECK_ARG(!i2v_overlap(dst, elems * 2, src, elems * (src_is_f32 ? 4 : 2)), "i2v_pixel_unshuffle8_f16: dst overlaps src");
  const int64_t chunks = elems / 8;
  const unsigned grid = i2v_ew_grid(chunks, EW_THREADS, EW_MAX_BLOCKS);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (src_is_f32)
    hipLaunchKernelGGL(pixel_unshuffle8_kernel<float>, dim3(grid), dim3(EW_THREADS), 0, st, reinterpret_cast<const float*>(src),
                       reinterpret_cast<f16*>(dst), chunks, c, h / 8, w / 8);
  else
    hipLaunchKernelGGL(pixel_unshuffle8_kernel<f16>, dim3(grid), dim3(EW_THREADS), 0, st, reinterpret_cast<const f16*>(src),
                       reinterpret_cast<f16*>(dst), chunks, c, h / 8, w / 8);
  return i2v_check_launch("i2v_pixel_unshuffle8_f16");
}

extern "C" int i2v_avgpool2x_f16(const void* src, void* dst, int32_t n, int32_t h, int32_t w, int32_t c, i2v_stream_t stream) {
  I2V_CHECK_ARG(src && dst, "i2v_avgpool2x_f16: null pointer");
  I2V_CHECK_ARG(n >= 1 && h >= 1 && w >= 1, "i2v_avgpool2x_f16: n %d, h %d, w %d", n, h, w);
  I2V_CHECK_ARG(c >= 8 && c % 8 == 0, "i2v_avgpool2x_f16: c %d must be a positive multiple of 8", c);
  I2V_CHECK_ARG(i2v_al16(src) && i2v_al16(dst), "i2v_avgpool2x_f16: src and dst must be 16-byte aligned");
  const int64_t in_elems = (int64_t)n * h * w * c;
  const int64_t out_elems = (int64_t)n * ((h + 1) / 2) * ((w + 1) / 2) * c;
  I2V_CHECK_ARG(in_elems < ((int64_t)1 << 40), "i2v_avgpool2x_f16: problem too large");
  I2V_CHECK_ARG(!i2v_overlap(dst, out_elems * 2, src, in_elems * 2), "i2v_avgpool2x_f16: dst overlaps src");
  const int64_t chunks = out_elems / 8;
  hipLaunchKernelGGL(avgpool2x_kernel, dim3(i2v_ew_grid(chunks, EW_THREADS, EW_MAX_BLOCKS)), dim3(EW_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(src), reinterpret_cast<f16*>(dst), chunks, h, w, c / 8);
  return i2v_check_launch("i2v_avgpool2x_f16");
}

extern "C" int i2v_relu_f16(const void* src, void* dst, int64_t numel, i2v_stream_t stream) {
  I2V_CHECK_ARG(src && dst, "i2v_relu_f16: null pointer");
  I2V_CHECK_ARG(numel > 0 && numel % 8 == 0, "i2v_relu_f16: %lld values, not a positive multiple of 8", (long long)numel);
  I2V_CHECK_ARG(i2v_al16(src) && i2v_al16(dst), "i2v_relu_f16: src and dst must be 16-byte aligned");
  I2V_CHECK_ARG(src == dst || !i2v_overlap(dst, numel * 2, src, numel * 2), "i2v_relu_f16: dst overlaps src without being it");
  const int64_t chunks = numel / 8;
  hipLaunchKernelGGL(relu_kernel, dim3(i2v_ew_grid(chunks, EW_THREADS, EW_MAX_BLOCKS)), dim3(EW_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(src), reinterpret_cast<f16*>(dst), chunks);
  return i2v_check_launch("i2v_relu_f16");
}

extern "C" int i2v_add_broadcast_residual_f16(const void* x, const void* x_lo, const void* feat, void* dst, void* dst_lo, int64_t numel,
                                              int64_t feat_numel, const float* scale_table, int32_t scale_rows, const int32_t* step_idx,
                                              i2v_stream_t stream) {
  I2V_CHECK_ARG(x && feat && dst, "i2v_add_broadcast_residual_f16: null pointer (x / feat / dst)");
  I2V_CHECK_ARG((x_lo == nullptr) == (dst_lo == nullptr),
                "i2v_add_broadcast_residual_f16: x_lo and dst_lo come together (a low half in means a low half out)");
  I2V_CHECK_ARG(numel > 0 && feat_numel > 0 && feat_numel % 8 == 0,
                "i2v_add_broadcast_residual_f16: numel %lld, feat_numel %lld: feat_numel must be a positive multiple of 8", (long long)numel,
                (long long)feat_numel);
  I2V_CHECK_ARG(numel % feat_numel == 0, "i2v_add_broadcast_residual_f16: numel %lld is not a multiple of feat_numel %lld", (long long)numel,
                (long long)feat_numel);
  I2V_CHECK_ARG(i2v_al16(x) && i2v_al16(x_lo) && i2v_al16(feat) && i2v_al16(dst) && i2v_al16(dst_lo),
                "i2v_add_broadcast_residual_f16: the operands must be 16-byte aligned");
  I2V_CHECK_ARG(scale_table == nullptr || scale_rows >= 1, "i2v_add_broadcast_residual_f16: a scale table of %d rows", scale_rows);
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(scale_table) & 3) == 0 && (reinterpret_cast<uintptr_t>(step_idx) & 3) == 0,
                "i2v_add_broadcast_residual_f16: scale_table / step_idx must be 4-byte aligned");
  I2V_CHECK_ARG(dst_lo == nullptr || dst_lo != dst, "i2v_add_broadcast_residual_f16: dst and dst_lo are the same memory");
  I2V_CHECK_ARG(!i2v_overlap(dst, numel * 2, feat, feat_numel * 2) && (dst_lo == nullptr || !i2v_overlap(dst_lo, numel * 2, feat, feat_numel * 2)),
                "i2v_add_broadcast_residual_f16: dst overlaps feat (every repetition reads all of feat)");
  AbArgs a;
  a.chunks = numel / 8;
  const int64_t fchunks = feat_numel / 8;
  const int64_t tiles = i2v_cdiv(a.chunks, AB_TILE);
  I2V_CHECK_ARG(fchunks < ((int64_t)1 << 31) && tiles < ((int64_t)1 << 31), "i2v_add_broadcast_residual_f16: problem too large");
  a.dst = reinterpret_cast<f16*>(dst);
  a.dst_lo = reinterpret_cast<f16*>(dst_lo);
  a.x = reinterpret_cast<const f16*>(x);
  a.x_lo = reinterpret_cast<const f16*>(x_lo);
  a.feat = reinterpret_cast<const f16*>(feat);
  a.fchunks = (uint32_t)fchunks;
  a.tiles = (uint32_t)tiles;
  a.scale_rows = scale_rows;
  a.scale_table = scale_table;
  a.step_idx = step_idx;
  const unsigned grid = (unsigned)(tiles < AB_MAX_BLOCKS ? tiles : AB_MAX_BLOCKS);
  hipLaunchKernelGGL(add_broadcast_residual_kernel, dim3(grid), dim3(AB_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  return i2v_check_launch("i2v_add_broadcast_residual_f16");
}
