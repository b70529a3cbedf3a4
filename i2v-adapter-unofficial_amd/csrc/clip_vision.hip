// The CLIP vision tower's two own kernels (transformers CLIPVisionModelWithProjection as the pipeline's encode_image calls it, pipe:323-345;
// IP-Adapter's image encoder is OpenCLIP ViT-H/14: 32 pre-LN layers, width 1280, 16 heads of 80, 16 x 16 patches of 14 px + a class token
// = 257 tokens).  Everything else of the tower -- the patch embedding itself, the q|k|v / out / fc1 / fc2 projections, the LayerNorms,
// the visual projection -- runs on the GEMM and LayerNorm entry points the UNet uses, its bidirectional attention on the kernel it
// shares with the text tower (short_attention.hip).
//
//   patchify     pixel_values [B, C, S, S] -> rows [B * (S/p)^2, ld]: row b P + py (S/p) + px is patch (py, px) in column order (c, dy, dx)
//                (the order of patch_embedding.weight.flatten(1)), columns C p p .. ld - 1 written as zero: the im2col of the strided
//                convolution, so that the patch embedding is one GEMM against the weight zero-padded to the same ld
//   embed        out[b, 0, :] = fp16(float(cls) + float(pos[0])), out[b, 1 + t, :] = fp16(float(patch[b P + t]) + float(pos[1 + t])):
//                one 16-byte chunk of one row per lane
//
// None of this is per-step work: an image is encoded once per sample.  The kernels are written to be obviously inside their operands,
// not to be fast.
#include "common.h"

namespace {

constexpr int CV_THREADS = 256;
constexpr int CV_MAX_BLOCKS = 256 * 8;

__global__ __launch_bounds__(CV_THREADS) void clip_patchify_kernel(const f16* __restrict__ px, f16* __restrict__ out, int64_t ld, int ch_row,
                                                                   int chans, int size, int patch, int grid, int64_t total) {
  const int kk = chans * patch * patch, pp = patch * patch;
  for (int64_t i = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CV_THREADS) {
    const int64_t row = i / ch_row;
    const int ch = (int)(i - row * ch_row);
    const int b = (int)(row / (grid * grid)), t = (int)(row - (int64_t)b * grid * grid);
    const int py = t / grid, pxi = t - py * grid;
    const f16* img = px + (int64_t)b * chans * size * size + (int64_t)(py * patch) * size + pxi * patch;
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = 8 * ch + e;
      f16 v = (f16)0.f;
      if (col < kk) {
        const int c = col / pp, r = col - c * pp, dy = r / patch, dx = r - dy * patch;
        v = img[((int64_t)c * size + dy) * size + dx];
      }
      o[e] = v;
    }
    *reinterpret_cast<f16x8*>(out + row * ld + 8 * ch) = o;
  }
}

__global__ __launch_bounds__(CV_THREADS) void clip_vision_embed_kernel(const f16* __restrict__ cls, const f16* __restrict__ patch, int64_t ldp,
                                                                       const f16* __restrict__ pos, f16* __restrict__ out, int patches,
                                                                       int chunks, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * CV_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CV_THREADS) {
    const int64_t row = i / chunks;
    const int ch = (int)(i - row * chunks);
    const int b = (int)(row / (patches + 1)), l = (int)(row - (int64_t)b * (patches + 1));
    const f16x8 x = l == 0 ? ld_global_16B(cls + 8 * ch) : ld_global_16B(patch + ((int64_t)b * patches + l - 1) * ldp + 8 * ch);
    const f16x8 p = ld_global_16B(pos + ((int64_t)l * chunks + ch) * 8);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)((float)x[e] + (float)p[e]);
    *reinterpret_cast<f16x8*>(out + i * 8) = o;
  }
}

}  // namespace

extern "C" int i2v_clip_patchify_f16(const void* pixel_values, void* out, int64_t ld_out, int32_t batch, int32_t channels, int32_t size,
                                     int32_t patch, i2v_stream_t stream) {
  I2V_CHECK_ARG(pixel_values && out, "i2v_clip_patchify_f16: null pointer");
  I2V_CHECK_ARG(batch > 0 && channels > 0 && size > 0 && patch > 0, "i2v_clip_patchify_f16: batch %d channels %d size %d patch %d must be positive",
                batch, channels, size, patch);
  I2V_CHECK_ARG(size <= 4096 && patch <= 256 && channels <= 64, "i2v_clip_patchify_f16: size %d patch %d channels %d too large", size, patch, channels);
  I2V_CHECK_ARG(size % patch == 0, "i2v_clip_patchify_f16: image size %d is not a multiple of the patch size %d", size, patch);
  const int grid = size / patch;
  const int64_t kk = (int64_t)channels * patch * patch, rows = (int64_t)batch * grid * grid;
  I2V_CHECK_ARG(ld_out % 8 == 0 && ld_out >= kk && ld_out < ((int64_t)1 << 24),
                "i2v_clip_patchify_f16: out row stride %lld must be a multiple of 8, at least channels * patch * patch = %lld", (long long)ld_out,
                (long long)kk);
  I2V_CHECK_ARG(rows < ((int64_t)1 << 31) && (int64_t)batch * channels * size * size < ((int64_t)1 << 40), "i2v_clip_patchify_f16: problem too large");
  I2V_CHECK_ARG((reinterpret_cast<uintptr_t>(pixel_values) & 1) == 0 && i2v_al16(out),
                "i2v_clip_patchify_f16: pixel_values must be 2-byte, out 16-byte aligned");
  I2V_CHECK_ARG(!i2v_overlap(out, rows * ld_out * 2, pixel_values, (int64_t)batch * channels * size * size * 2),
                "i2v_clip_patchify_f16: out is a new tensor (it must not overlap pixel_values)");
  const int ch_row = (int)(ld_out / 8);
  const int64_t total = rows * ch_row;
  hipLaunchKernelGGL(clip_patchify_kernel, dim3(i2v_ew_grid(total, CV_THREADS, CV_MAX_BLOCKS)), dim3(CV_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(pixel_values), reinterpret_cast<f16*>(out), ld_out, ch_row, channels, size, patch, grid, total);
  return i2v_check_launch("i2v_clip_patchify_f16");
}

extern "C" int i2v_clip_vision_embed_f16(const void* cls, const void* patch, int64_t ld_patch, const void* pos, void* out, int32_t batch,
                                         int32_t patches, int32_t hidden, i2v_stream_t stream) {
  I2V_CHECK_ARG(cls && patch && pos && out, "i2v_clip_vision_embed_f16: null pointer");
  I2V_CHECK_ARG(batch > 0 && patches > 0, "i2v_clip_vision_embed_f16: batch %d patches %d must be positive", batch, patches);
  I2V_CHECK_ARG(hidden > 0 && hidden % 8 == 0, "i2v_clip_vision_embed_f16: hidden %d must be a positive multiple of 8", hidden);
  I2V_CHECK_ARG(ld_patch % 8 == 0 && ld_patch >= hidden && ld_patch < ((int64_t)1 << 24),
                "i2v_clip_vision_embed_f16: patch row stride %lld must be a multiple of 8, at least hidden", (long long)ld_patch);
  I2V_CHECK_ARG((int64_t)batch * (patches + 1) < ((int64_t)1 << 31), "i2v_clip_vision_embed_f16: problem too large (%lld rows)",
                (long long)batch * (patches + 1));
  I2V_CHECK_ARG(i2v_al16(cls) && i2v_al16(patch) && i2v_al16(pos) && i2v_al16(out), "i2v_clip_vision_embed_f16: pointers must be 16-byte aligned");
  const int64_t rows = (int64_t)batch * (patches + 1), out_bytes = rows * hidden * 2;
  I2V_CHECK_ARG(!i2v_overlap(out, out_bytes, cls, (int64_t)hidden * 2) && !i2v_overlap(out, out_bytes, pos, (int64_t)(patches + 1) * hidden * 2) &&
                    !i2v_overlap(out, out_bytes, patch, (((int64_t)batch * patches - 1) * ld_patch + hidden) * 2),
                "i2v_clip_vision_embed_f16: out is a new tensor (it must not overlap the class token, the patches or the position table)");
  const int chunks = hidden / 8;
  const int64_t total = rows * chunks;
  hipLaunchKernelGGL(clip_vision_embed_kernel, dim3(i2v_ew_grid(total, CV_THREADS, CV_MAX_BLOCKS)), dim3(CV_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(cls), reinterpret_cast<const f16*>(patch), ld_patch, reinterpret_cast<const f16*>(pos),
                     reinterpret_cast<f16*>(out), patches, chunks, total);
  return i2v_check_launch("i2v_clip_vision_embed_f16");
}
