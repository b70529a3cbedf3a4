// FreeU (diffusers 0.24 apply_freeu / fourier_filter, threshold 1) on the operands of an up block's skip concatenation, token layout
// [N, H, W, C] fp16.  One launch, two ranges of the grid:
//
//  * skip:   skip' = Re(ifftn(ifftshift(mask * fftshift(fftn(skip))))) over (H, W), mask = s on the 2 x 2 box around the centre of the
//            shifted spectrum and 1 elsewhere.  The box holds exactly the frequencies (k, l) in {0, -1}^2, so with th = 2 pi h / H,
//            tw = 2 pi w / W
//              skip'[h, w] = skip[h, w] + (s - 1) / (H W) * ( S0 + Ah cos th + Bh sin th + Aw cos tw + Bw sin tw
//                                                             + Ad cos(th + tw) + Bd sin(th + tw) )
//              S0 = sum x,  (Ah, Bh) = sum x (cos th, sin th),  (Aw, Bw) = sum x (cos tw, sin tw),  (Ad, Bd) = sum x (cos, sin)(th + tw)
//            -- seven real sums per (image, channel) plane and a rank-4 correction, no FFT.  (H = 1 or W = 1 is refused: the
//            reference's box slice wraps there and the identity does not hold.)
//  * hidden: channels < C1 / 2 times b (fp32, one rounding), the rest copied bit for bit.  With a low half (the precise residual
//            stream's hi + lo pair) the product is taken of hi + lo and written as a pair again; the copied channels keep both halves.
//
// A workgroup of the skip range owns one image x 64 channels: a lane holds 8 consecutive channels (16-byte loads / stores, 8 lanes
// = one 128-byte line per pixel), the 32 lane groups of the workgroup stride over the H W pixels.  The per-lane sums are combined
// across the 8 lane groups of a wave by lane exchanges and across the 4 waves through LDS; a second pass over the same pixels
// (L2-resident: one plane set is <= 74 KB) applies the correction and rounds to fp16 once.  cos / sin come from a table of H + W
// entries built once per workgroup in LDS (sincospif), not from a per-pixel transcendental.
#include "common.h"

namespace {

constexpr int FU_THREADS = 256;
constexpr int FU_CH = 64;            // channels per workgroup of the skip range (8 lanes x 8)
constexpr int FU_GROUPS = 32;        // pixel lane-groups per workgroup
constexpr int FU_MAX_DIM = 256;      // H, W of the twiddle table
constexpr int FU_SUMS = 7;
constexpr int FU_MAX_HIDDEN_BLOCKS = 2048;

template <bool HAS_LO>
__device__ __forceinline__ void freeu_hidden_range(const f16* __restrict__ hid, const f16* __restrict__ hid_lo, f16* __restrict__ out,
                                                   f16* __restrict__ out_lo, int64_t vecs, int c1, float b, int block, int nblocks) {
  const int c8 = c1 >> 3, half = c1 >> 1;
  for (int64_t i = (int64_t)block * FU_THREADS + threadIdx.x; i < vecs; i += (int64_t)nblocks * FU_THREADS) {
    const int cb = (int)(i % c8) * 8;
    f16x8 v = *reinterpret_cast<const f16x8*>(hid + 8 * i);
    f16x8 l = zero8();
    if constexpr (HAS_LO) l = *reinterpret_cast<const f16x8*>(hid_lo + 8 * i);
    if (cb < half) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (cb + j < half) {
          const float x = HAS_LO ? (float)v[j] + (float)l[j] : (float)v[j];
          const float y = x * b;
          v[j] = (f16)y;
          if constexpr (HAS_LO) l[j] = (f16)(y - (float)v[j]);
        }
      }
    }
    *reinterpret_cast<f16x8*>(out + 8 * i) = v;
    if constexpr (HAS_LO) *reinterpret_cast<f16x8*>(out_lo + 8 * i) = l;
  }
}

template <bool HAS_LO>
__global__ __launch_bounds__(FU_THREADS) void freeu_kernel(const f16* __restrict__ hid, const f16* __restrict__ hid_lo,
                                                           f16* __restrict__ hid_out, f16* __restrict__ hid_out_lo,
                                                           const f16* __restrict__ skip, f16* __restrict__ skip_out, int n, int hh,
                                                           int ww, int c1, int c2, float b, float s, int skip_blocks, int chunks) {
  __shared__ float tw_cos_h[FU_MAX_DIM], tw_sin_h[FU_MAX_DIM], tw_cos_w[FU_MAX_DIM], tw_sin_w[FU_MAX_DIM];
  __shared__ __attribute__((aligned(16))) float part[FU_THREADS / I2V_WAVE][FU_SUMS][FU_CH];
  const int hw = hh * ww;
  if ((int)blockIdx.x >= skip_blocks) {      // (uniform per workgroup)
    freeu_hidden_range<HAS_LO>(hid, hid_lo, hid_out, hid_out_lo, (int64_t)n * hw * (c1 >> 3), c1, b, (int)blockIdx.x - skip_blocks,
                               (int)gridDim.x - skip_blocks);
    return;
  }
  const int tid = threadIdx.x;
  for (int i = tid; i < hh; i += FU_THREADS) sincospif(2.0f * (float)i / (float)hh, &tw_sin_h[i], &tw_cos_h[i]);
  for (int i = tid; i < ww; i += FU_THREADS) sincospif(2.0f * (float)i / (float)ww, &tw_sin_w[i], &tw_cos_w[i]);
  __syncthreads();

  const int img = (int)blockIdx.x / chunks, chunk = (int)blockIdx.x - img * chunks;
  const int cl = tid & 7, grp = tid >> 3;              // channel lane (8 channels), pixel lane-group
  const int ch = chunk * FU_CH + cl * 8;
  const bool live = ch < c2;                            // (c2 % 8 == 0: a lane is inside or outside as a whole)
  const f16* src = skip + (int64_t)img * hw * c2 + ch;
  f16* dst = skip_out + (int64_t)img * hw * c2 + ch;

  float acc[FU_SUMS][8];
#pragma unroll
  for (int k = 0; k < FU_SUMS; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
  if (live) {
    for (int p = grp; p < hw; p += FU_GROUPS) {
      const int ph = p / ww, pw = p - ph * ww;
      const float chh = tw_cos_h[ph], shh = tw_sin_h[ph], cww = tw_cos_w[pw], sww = tw_sin_w[pw];
      const float cd = chh * cww - shh * sww, sd = shh * cww + chh * sww;
      const f16x8 v = *reinterpret_cast<const f16x8*>(src + (int64_t)p * c2);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = (float)v[j];
        acc[0][j] += x;
        acc[1][j] = fmaf(x, chh, acc[1][j]);
        acc[2][j] = fmaf(x, shh, acc[2][j]);
        acc[3][j] = fmaf(x, cww, acc[3][j]);
        acc[4][j] = fmaf(x, sww, acc[4][j]);
        acc[5][j] = fmaf(x, cd, acc[5][j]);
        acc[6][j] = fmaf(x, sd, acc[6][j]);
      }
    }
  }
  // lanes l, l ^ 8, l ^ 16, l ^ 32 of a wave hold the same channels: sum them, then the four waves through LDS
#pragma unroll
  for (int k = 0; k < FU_SUMS; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float x = acc[k][j];
      x += __shfl_xor(x, 8);
      x += __shfl_xor(x, 16);
      x += __shfl_xor(x, 32);
      acc[k][j] = x;
    }
  const int wave = tid >> 6;
  if ((tid & 63) < 8) {
#pragma unroll
    for (int k = 0; k < FU_SUMS; ++k) {
      *reinterpret_cast<f32x4*>(&part[wave][k][cl * 8]) = f32x4{acc[k][0], acc[k][1], acc[k][2], acc[k][3]};
      *reinterpret_cast<f32x4*>(&part[wave][k][cl * 8 + 4]) = f32x4{acc[k][4], acc[k][5], acc[k][6], acc[k][7]};
    }
  }
  __syncthreads();
  if (!live) return;
  const float g = (s - 1.0f) / (float)hw;
#pragma unroll
  for (int k = 0; k < FU_SUMS; ++k) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      f32x4 t = *reinterpret_cast<const f32x4*>(&part[0][k][cl * 8 + 4 * q]);
#pragma unroll
      for (int wv = 1; wv < FU_THREADS / I2V_WAVE; ++wv) t += *reinterpret_cast<const f32x4*>(&part[wv][k][cl * 8 + 4 * q]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[k][4 * q + j] = t[j] * g;
    }
  }
  for (int p = grp; p < hw; p += FU_GROUPS) {
    const int ph = p / ww, pw = p - ph * ww;
    const float chh = tw_cos_h[ph], shh = tw_sin_h[ph], cww = tw_cos_w[pw], sww = tw_sin_w[pw];
    const float cd = chh * cww - shh * sww, sd = shh * cww + chh * sww;
    f16x8 v = *reinterpret_cast<const f16x8*>(src + (int64_t)p * c2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float corr = acc[0][j];
      corr = fmaf(acc[1][j], chh, corr);
      corr = fmaf(acc[2][j], shh, corr);
      corr = fmaf(acc[3][j], cww, corr);
      corr = fmaf(acc[4][j], sww, corr);
      corr = fmaf(acc[5][j], cd, corr);
      corr = fmaf(acc[6][j], sd, corr);
      v[j] = (f16)((float)v[j] + corr);
    }
    *reinterpret_cast<f16x8*>(dst + (int64_t)p * c2) = v;
  }
}

}  // namespace

extern "C" int i2v_freeu_f16(const void* hidden, const void* hidden_lo, void* hidden_out, void* hidden_out_lo, const void* skip,
                             void* skip_out, int32_t n, int32_t h, int32_t w, int32_t c1, int32_t c2, float b, float s,
                             i2v_stream_t stream) {
  I2V_CHECK_ARG(hidden && hidden_out && skip && skip_out, "i2v_freeu_f16: null pointer");
  I2V_CHECK_ARG((hidden_lo == nullptr) == (hidden_out_lo == nullptr),
                "i2v_freeu_f16: hidden_lo and hidden_out_lo come together (a low half in means a low half out)");
  I2V_CHECK_ARG(n > 0 && h > 0 && w > 0 && c1 > 0 && c2 > 0, "i2v_freeu_f16: n %d h %d w %d c1 %d c2 %d", n, h, w, c1, c2);
  I2V_CHECK_ARG(h >= 2 && w >= 2, "i2v_freeu_f16: not implemented for this problem (h %d, w %d: the Fourier box needs h, w >= 2)", h, w);
  I2V_CHECK_ARG(h <= FU_MAX_DIM && w <= FU_MAX_DIM, "i2v_freeu_f16: not implemented for this problem (h %d, w %d: at most %d)", h, w,
                FU_MAX_DIM);
  I2V_CHECK_ARG(c1 % 8 == 0 && c2 % 8 == 0, "i2v_freeu_f16: not implemented for this problem (c1 %d, c2 %d: multiples of 8)", c1, c2);
  I2V_CHECK_ARG(hidden != hidden_out && skip != skip_out && (hidden_lo == nullptr || hidden_lo != hidden_out_lo),
                "i2v_freeu_f16: the outputs are new tensors (not in place)");
  I2V_CHECK_ARG(i2v_al16(hidden) && i2v_al16(hidden_out) && i2v_al16(skip) && i2v_al16(skip_out) && i2v_al16(hidden_lo) &&
                    i2v_al16(hidden_out_lo),
                "i2v_freeu_f16: operands must be 16-byte aligned");
  I2V_CHECK_ARG((int64_t)n * h * w * (int64_t)(c1 > c2 ? c1 : c2) < (int64_t)1 << 40, "i2v_freeu_f16: problem too large");
  const int chunks = (int)i2v_cdiv(c2, FU_CH);
  const int64_t skip_blocks = (int64_t)n * chunks;
  I2V_CHECK_ARG(skip_blocks < (int64_t)1 << 30, "i2v_freeu_f16: n %d x %d channel chunks exceed the grid", n, chunks);
  const int64_t hv = i2v_cdiv((int64_t)n * h * w * (c1 / 8), FU_THREADS);
  const int hidden_blocks = (int)(hv < FU_MAX_HIDDEN_BLOCKS ? hv : FU_MAX_HIDDEN_BLOCKS);
  const dim3 grid((unsigned)(skip_blocks + hidden_blocks));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hidden_lo)
    hipLaunchKernelGGL(freeu_kernel<true>, grid, dim3(FU_THREADS), 0, st, reinterpret_cast<const f16*>(hidden),
                       reinterpret_cast<const f16*>(hidden_lo), reinterpret_cast<f16*>(hidden_out), reinterpret_cast<f16*>(hidden_out_lo),
                       reinterpret_cast<const f16*>(skip), reinterpret_cast<f16*>(skip_out), n, h, w, c1, c2, b, s, (int)skip_blocks,
                       chunks);
  else
    hipLaunchKernelGGL(freeu_kernel<false>, grid, dim3(FU_THREADS), 0, st, reinterpret_cast<const f16*>(hidden),
                       static_cast<const f16*>(nullptr), reinterpret_cast<f16*>(hidden_out), static_cast<f16*>(nullptr),
                       reinterpret_cast<const f16*>(skip), reinterpret_cast<f16*>(skip_out), n, h, w, c1, c2, b, s, (int)skip_blocks,
                       chunks);
  return i2v_check_launch("i2v_freeu_f16");
}
