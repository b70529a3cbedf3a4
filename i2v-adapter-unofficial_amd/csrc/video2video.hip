// Video-to-video with a mask (diffusers' inpainting update for a 4-channel UNet, pipeline `mask_image=`): the one launch that runs
// inside a denoising step, after the scheduler-step kernel.
//   i2v_masked_renoise_f32   latents[n, c, p] = m * latents[n, c, p] + (1 - m) * (a * source[n, c, p] + b * noise[n, c, p])
//                            m = mask[n, p] (one plane for all channels), (a, b) = coef[r], r = clamp(step_idx[0], 0, coef_rows - 1)
// m = 1 regenerates (the latent stays), m = 0 keeps the source at the noise level the NEXT step expects.
//
// Table convention: the scheduler-step kernels have already advanced the step counter when this kernel reads it, and they wrap it to
// 0 after the last row.  So row 0 of `coef` is (1, 0) -- the clean source, after the last step -- and row r >= 1 is
// (sqrt(abar), sqrt(1 - abar)) of timesteps[r], the level of the step that comes next.  A one-step schedule falls on row 0.  The
// kernel READS the counter and never writes it.
//
// Exact cases: where m == 1 the latent's bits are stored back as they were loaded (nothing is computed: -0 and NaN payloads survive,
// and whatever source / noise hold does not reach the output); where m == 0 the result is t = (b == 0 ? a * source : fma(b, noise,
// a * source)) with a * source = source for a == 1, so with the row (1, 0) it is the source's bits.  Otherwise
// fma(1 - m, t, m * latent): all fp32.
//
// Memory-bound: three reads and one write over the latents, the mask read once per pixel.  The latents are walked as a flat array of
// 16-byte chunks (4 fp32), MR_UNROLL independent chunks of every operand in flight per lane, 16 KB tiles, a capped grid that strides.
// With hw % 4 == 0 a chunk lies inside one plane and its mask values are one 16-byte load; otherwise (odd planes such as 5 x 7) a
// chunk may straddle two planes and every value finds its own mask value.  The last numel % 4 values take a scalar path.
#include "common.h"

namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_UNROLL = 4;
constexpr int MR_TILE = MR_THREADS * MR_UNROLL;      // 16-byte chunks per tile: 16 KB of each operand
constexpr int MR_MAX_BLOCKS = 2048;

struct MrArgs {
  float* latents;
  const float* source;
  const float* noise;
  const float* mask;
  const float* coef;
  const int32_t* step_idx;
  int32_t coef_rows;
  uint32_t numel;                                      // images * channels * hw < 2^31 - 2^19 (host check)
  uint32_t chunks;                                     // numel / 4
  uint32_t tiles;
  uint32_t channels;
  uint32_t hw;
};

__device__ __forceinline__ float mr_blend(float l, float s, float n, float m, float a, float b) {
  if (m == 1.0f) return l;
  const float as = a == 1.0f ? s : a * s;             // (the source's bits whatever the denormal mode)
  const float t = b == 0.0f ? as : fmaf(b, n, as);
  if (m == 0.0f) return t;
  return fmaf(1.0f - m, t, m * l);
}

// the mask value of the flat element e = (n * channels + c) * hw + p
__device__ __forceinline__ float mr_mask_at(const MrArgs& a, uint32_t e) {
  const uint32_t row = e / a.hw, p = e - row * a.hw;
  return a.mask[(row / a.channels) * a.hw + p];       // < images * hw <= numel
}

template <bool ALIGNED>
__device__ __forceinline__ void mr_tile(const MrArgs& a, uint32_t base, float ca, float cb) {
  f32x4 l[MR_UNROLL], s[MR_UNROLL], n[MR_UNROLL], m[MR_UNROLL];
#pragma unroll
  for (int u = 0; u < MR_UNROLL; ++u) {
    const uint32_t q = base + threadIdx.x + u * MR_THREADS;
    if (q < a.chunks) {
      const uint32_t e = q * 4;
      l[u] = *reinterpret_cast<const f32x4*>(a.latents + e);
      s[u] = *reinterpret_cast<const f32x4*>(a.source + e);
      n[u] = *reinterpret_cast<const f32x4*>(a.noise + e);
      if (ALIGNED) {
        // hw % 4 == 0: the chunk lies inside one plane, and its mask values are 16-byte aligned too
        const uint32_t row = e / a.hw, p = e - row * a.hw;
        m[u] = *reinterpret_cast<const f32x4*>(a.mask + (row / a.channels) * a.hw + p);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) m[u][j] = mr_mask_at(a, e + j);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < MR_UNROLL; ++u) {
    const uint32_t q = base + threadIdx.x + u * MR_THREADS;
    if (q < a.chunks) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = mr_blend(l[u][j], s[u][j], n[u][j], m[u][j], ca, cb);
      *reinterpret_cast<f32x4*>(a.latents + q * 4) = o;
    }
  }
}

__global__ __launch_bounds__(MR_THREADS) void masked_renoise_kernel(const MrArgs a) {
  int row = a.step_idx[0];
  row = row < 0 ? 0 : (row > a.coef_rows - 1 ? a.coef_rows - 1 : row);
  const float ca = a.coef[2 * row], cb = a.coef[2 * row + 1];
  const bool aligned = (a.hw & 3) == 0;
  for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {      // tiles <= 2^19: no wrap
    if (aligned)
      mr_tile<true>(a, tile * MR_TILE, ca, cb);
    else
      mr_tile<false>(a, tile * MR_TILE, ca, cb);
  }
  // the last numel % 4 values (only with hw % 4 != 0): scalar
  if (blockIdx.x == 0) {
    const uint32_t e = a.chunks * 4 + threadIdx.x;
    if (e < a.numel) a.latents[e] = mr_blend(a.latents[e], a.source[e], a.noise[e], mr_mask_at(a, e), ca, cb);
  }
}

}  // namespace

extern "C" int i2v_masked_renoise_f32(float* latents, const float* source, const float* noise, const float* mask, const float* coef,
                                      int32_t coef_rows, const int32_t* step_idx, int64_t images, int32_t channels, int32_t hw,
                                      i2v_stream_t stream) {
  I2V_CHECK_ARG(latents && source && noise && mask && coef && step_idx, "i2v_masked_renoise_f32: null pointer");
  I2V_CHECK_ARG(images >= 1 && channels >= 1 && hw >= 1 && coef_rows >= 1,
                "i2v_masked_renoise_f32: images %lld, channels %d, hw %d, coef_rows %d must be positive", (long long)images, channels, hw,
                coef_rows);
  I2V_CHECK_ARG(i2v_al16(latents) && i2v_al16(source) && i2v_al16(noise) && i2v_al16(mask),
                "i2v_masked_renoise_f32: latents, source, noise and mask must be 16-byte aligned");
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(coef) & 3) == 0 && (reinterpret_cast<uintptr_t>(step_idx) & 3) == 0,
                "i2v_masked_renoise_f32: coef / step_idx must be 4-byte aligned");
  const int64_t limit = ((int64_t)1 << 31) - ((int64_t)1 << 19);
  I2V_CHECK_ARG(images < limit && (int64_t)channels * hw < limit && images * ((int64_t)channels * hw) < limit,
                "i2v_masked_renoise_f32: problem too large (images * channels * hw must stay below 2^31 - 2^19)");
  const int64_t numel = images * (int64_t)channels * hw;
  I2V_CHECK_ARG(!i2v_overlap(latents, numel * 4, source, numel * 4) && !i2v_overlap(latents, numel * 4, noise, numel * 4) &&
                    !i2v_overlap(latents, numel * 4, mask, images * hw * 4),
                "i2v_masked_renoise_f32: latents overlaps source, noise or mask");
  MrArgs a;
  a.latents = latents;
  a.source = source;
  a.noise = noise;
  a.mask = mask;
  a.coef = coef;
  a.step_idx = step_idx;
  a.coef_rows = coef_rows;
  a.numel = (uint32_t)numel;
  a.chunks = (uint32_t)(numel / 4);
  a.tiles = (uint32_t)i2v_cdiv(numel / 4, MR_TILE);
  a.channels = (uint32_t)channels;
  a.hw = (uint32_t)hw;
  const unsigned grid = a.tiles < 1 ? 1u : (a.tiles < (uint32_t)MR_MAX_BLOCKS ? a.tiles : (unsigned)MR_MAX_BLOCKS);
  hipLaunchKernelGGL(masked_renoise_kernel, dim3(grid), dim3(MR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  return i2v_check_launch("i2v_masked_renoise_f32");
}
