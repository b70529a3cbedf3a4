// Hires fix (pipeline `enable_hires_fix`): the latent upscale between the two passes, with the second pass's re-noise fused in.
//   i2v_resize_renoise_f32   out[p, Y, X] = a * sum_ky sum_kx wy[Y, ky] * wx[X, kx] * src[p, iy[Y, ky], ix[X, kx]]  +  b * noise[p, Y, X]
// p runs over the batch * frames * channels planes; src is [planes, h, w], out and noise are [planes, H, W], H >= h and W >= w.  Upscaling
// needs at most four taps per axis in every mode (nearest, bilinear, bicubic, the anti-aliased pair), so a mode is nothing but two tap
// tables -- four source indices and four fp32 weights per output row, and the same per output column -- built on the host in fp64 and
// rounded once (hires_fix.resize_tables).  The kernel does no coordinate arithmetic of its own.
//
// Arithmetic, all fp32, nothing contracted (the pragma below): the term of (ky, kx) is (wy * wx) * src, the 16 terms are added in the
// order ky = 0..3 outer, kx = 0..3 inner, starting from the first term (15 additions); then out = a * r without noise (r's bits for
// a == 1) and (a * r) + (b * noise) with it -- the two products and the sum of i2v_axpby_f32, so the fused launch gives the bits of
// resize followed by axpby.  Against fp64 from the same fp32 tables: |error| <= 2^-19 (|a| sum |wy| |wx| |src| + |b| |noise|).
// A tap of weight 0 contributes 0 * src: an unused tap needs a valid index and a finite source.  A weight of exactly 1 beside zeros
// (the nearest modes, every mode at H == h / W == w) returns the source's bits.
//
// Memory- and latency-bound: 16 gathered 4-byte reads per output value, served by the vector L1 / L2 (neighbouring outputs share their
// sources), one 16-byte store, one 16-byte noise load.  The output is walked as a flat array of 16-byte chunks, one per lane and
// RZ_UNROLL per lane and tile.  With W % 4 == 0 a chunk lies inside one output row: one row of the row table per chunk, four
// consecutive rows of the column table.  Otherwise (odd widths such as 13 or 31) a chunk may straddle two rows or planes and every
// value finds its own row and column; the last numel % 4 values take a scalar path.  Indices are clamped into the source plane before
// they are used, so a damaged table reads wrong values and never out of bounds.
#include "common.h"

namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

constexpr int RZ_THREADS = 256;
constexpr int RZ_UNROLL = 2;
constexpr int RZ_TILE = RZ_THREADS * RZ_UNROLL;      // 16-byte chunks per tile
constexpr int RZ_MAX_BLOCKS = 4096;

struct RzArgs {
  const float* src;
  float* out;
  const float* noise;                                  // may be null: then `b` is not used and nothing is read for it
  const i32x4* iy;                                     // [H] rows of four source-row indices
  const f32x4* wy;
  const i32x4* ix;                                     // [W] rows of four source-column indices
  const f32x4* wx;
  float a, b;
  uint32_t h, w, H, W;
  uint32_t numel;                                      // planes * H * W < 2^31 - 2^19 (host check)
  uint32_t chunks;                                     // numel / 4
  uint32_t tiles;
};

#pragma clang fp contract(off)

__device__ __forceinline__ i32x4 rz_clamp(i32x4 i, uint32_t n) {
  i32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = min(max(i[k], 0), (int32_t)n - 1);
  return o;
}

// the 16-term sum of one output value: sp = the source plane, ry = the four source-row offsets (index * w, clamped)
__device__ __forceinline__ float rz_value(const float* __restrict__ sp, const uint32_t (&ry)[4], f32x4 wy, i32x4 cx, f32x4 wx) {
  float r = 0.0f;
#pragma unroll
  for (int ky = 0; ky < 4; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) {
      const float t = (wy[ky] * wx[kx]) * sp[ry[ky] + (uint32_t)cx[kx]];
      r = (ky == 0 && kx == 0) ? t : r + t;
    }
  }
  return r;
}

__device__ __forceinline__ float rz_finish(float r, float n, float a, float b, bool has_noise) {
  const float ar = a * r;
  return has_noise ? ar + b * n : ar;
}

// the output value at flat element e = (p * H + Y) * W + X, every index found for itself
__device__ __forceinline__ float rz_at(const RzArgs& a, uint32_t e, float n) {
  const uint32_t row = e / a.W, X = e - row * a.W;
  const uint32_t p = row / a.H, Y = row - p * a.H;
  const i32x4 cy = rz_clamp(a.iy[Y], a.h), cx = rz_clamp(a.ix[X], a.w);
  uint32_t ry[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) ry[k] = (uint32_t)cy[k] * a.w;
  return rz_finish(rz_value(a.src + (size_t)p * a.h * a.w, ry, a.wy[Y], cx, a.wx[X]), n, a.a, a.b, a.noise != nullptr);
}

template <bool ALIGNED>
__device__ __forceinline__ void rz_tile(const RzArgs& a, uint32_t base) {
  const bool has_noise = a.noise != nullptr;
#pragma unroll
  for (int u = 0; u < RZ_UNROLL; ++u) {
    const uint32_t q = base + threadIdx.x + u * RZ_THREADS;
    if (q >= a.chunks) continue;
    const uint32_t e = q * 4;
    f32x4 n = {0.0f, 0.0f, 0.0f, 0.0f};
    if (has_noise) n = *reinterpret_cast<const f32x4*>(a.noise + e);
    f32x4 o;
    if (ALIGNED) {
      // W % 4 == 0: the chunk lies inside one output row
      const uint32_t row = e / a.W, X = e - row * a.W;
      const uint32_t p = row / a.H, Y = row - p * a.H;
      const float* sp = a.src + (size_t)p * a.h * a.w;
      const i32x4 cy = rz_clamp(a.iy[Y], a.h);
      const f32x4 wy = a.wy[Y];
      uint32_t ry[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) ry[k] = (uint32_t)cy[k] * a.w;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = rz_finish(rz_value(sp, ry, wy, rz_clamp(a.ix[X + j], a.w), a.wx[X + j]), n[j], a.a, a.b, has_noise);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = rz_at(a, e + j, n[j]);
    }
    *reinterpret_cast<f32x4*>(a.out + e) = o;
  }
}

__global__ __launch_bounds__(RZ_THREADS) void resize_renoise_kernel(const RzArgs a) {
  const bool aligned = (a.W & 3) == 0;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {      // tiles < 2^21: no wrap
    if (aligned)
      rz_tile<true>(a, tile * RZ_TILE);
    else
      rz_tile<false>(a, tile * RZ_TILE);
  }
  // the last numel % 4 values (only with W % 4 != 0): scalar
  if (blockIdx.x == 0) {
    const uint32_t e = a.chunks * 4 + threadIdx.x;
    if (e < a.numel) a.out[e] = rz_at(a, e, a.noise != nullptr ? a.noise[e] : 0.0f);
  }
}

}  // namespace

extern "C" int i2v_resize_renoise_f32(const float* src, float* out, const float* noise, const int32_t* iy, const float* wy,
                                      const int32_t* ix, const float* wx, float a, float b, int64_t planes, int32_t h, int32_t w,
                                      int32_t H, int32_t W, i2v_stream_t stream) {
  I2V_CHECK_ARG(src && out && iy && wy && ix && wx, "i2v_resize_renoise_f32: null pointer");
  I2V_CHECK_ARG(planes >= 1 && h >= 1 && w >= 1, "i2v_resize_renoise_f32: planes %lld, h %d, w %d must be positive", (long long)planes, h,
                w);
  I2V_CHECK_ARG(H >= h && W >= w, "i2v_resize_renoise_f32: %d x %d -> %d x %d is a downscale: upscaling only (H >= h and W >= w)", h, w, H,
                W);
  I2V_CHECK_ARG(i2v_al16(out) && (!noise || i2v_al16(noise)) && i2v_al16(iy) && i2v_al16(wy) && i2v_al16(ix) && i2v_al16(wx),
                "i2v_resize_renoise_f32: out, noise and the four tables must be 16-byte aligned");
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(src) & 3) == 0, "i2v_resize_renoise_f32: src must be 4-byte aligned");
  const int64_t limit = ((int64_t)1 << 31) - ((int64_t)1 << 19);
  I2V_CHECK_ARG(planes < limit && (int64_t)H * W < limit && planes * ((int64_t)H * W) < limit,
                "i2v_resize_renoise_f32: problem too large (planes * H * W must stay below 2^31 - 2^19)");
  const int64_t numel = planes * (int64_t)H * W, in_bytes = planes * (int64_t)h * w * 4;
  I2V_CHECK_ARG(!i2v_overlap(out, numel * 4, src, in_bytes) && !(noise && i2v_overlap(out, numel * 4, noise, numel * 4)) &&
                    !i2v_overlap(out, numel * 4, iy, (int64_t)H * 16) && !i2v_overlap(out, numel * 4, wy, (int64_t)H * 16) &&
                    !i2v_overlap(out, numel * 4, ix, (int64_t)W * 16) && !i2v_overlap(out, numel * 4, wx, (int64_t)W * 16),
                "i2v_resize_renoise_f32: out overlaps src, noise or a table");
  RzArgs r;
  r.src = src;
  r.out = out;
  r.noise = noise;
  r.iy = reinterpret_cast<const i32x4*>(iy);
  r.wy = reinterpret_cast<const f32x4*>(wy);
  r.ix = reinterpret_cast<const i32x4*>(ix);
  r.wx = reinterpret_cast<const f32x4*>(wx);
  r.a = a;
  r.b = b;
  r.h = (uint32_t)h;
  r.w = (uint32_t)w;
  r.H = (uint32_t)H;
  r.W = (uint32_t)W;
  r.numel = (uint32_t)numel;
  r.chunks = (uint32_t)(numel / 4);
  r.tiles = (uint32_t)i2v_cdiv(numel / 4, RZ_TILE);
  const unsigned grid = r.tiles < 1 ? 1u : (r.tiles < (uint32_t)RZ_MAX_BLOCKS ? r.tiles : (unsigned)RZ_MAX_BLOCKS);
  hipLaunchKernelGGL(resize_renoise_kernel, dim3(grid), dim3(RZ_THREADS), 0, reinterpret_cast<hipStream_t>(stream), r);
  return i2v_check_launch("i2v_resize_renoise_f32");
}
