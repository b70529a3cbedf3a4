// The CLIP text tower's two own kernels (transformers CLIPTextModel as the pipeline calls it, pipe:412-453): everything else of the
// tower -- the QKV / out / fc1 / fc2 projections, the LayerNorms -- runs on the GEMM and LayerNorm entry points the UNet uses, its
// causal attention on the kernel it shares with the vision tower (short_attention.hip).
//
//   embed        out[b*L + l, :] = fp16(float(tok[ids[b, l], :]) + float(pos[l, :]))      one 16-byte chunk of one row per lane
//   quick-GELU   y = fp16(x * sigmoid(1.702 x)) in fp32, any n, in place or not
//
// None of this is per-step work: a prompt is encoded once per sample, 2 x 77 tokens.  The kernels are written to be obviously inside
// their operands, not to be fast -- the whole tower is launch-latency bound.
#include "common.h"

namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_MAX_BLOCKS = 256 * 8;

__global__ __launch_bounds__(CT_THREADS) void clip_embed_kernel(const f16* __restrict__ tok, const f16* __restrict__ pos,
                                                                const int32_t* __restrict__ ids, f16* __restrict__ out, int len, int vocab,
                                                                int chunks, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CT_THREADS) {
    const int row = (int)(i / chunks), ch = (int)(i - (int64_t)row * chunks);
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);      // the host has checked its copy; a device table that differs cannot leave tok
    const int l = row % len;
    const f16x8 t = ld_global_16B(tok + ((int64_t)id * chunks + ch) * 8);
    const f16x8 p = ld_global_16B(pos + ((int64_t)l * chunks + ch) * 8);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)((float)t[e] + (float)p[e]);
    *reinterpret_cast<f16x8*>(out + i * 8) = o;
  }
}

__device__ __forceinline__ float quick_gelu_f(float x) { return x / (1.0f + __expf(-1.702f * x)); }

// nvec 16-byte chunks on the vector path (0 when a pointer is not 16-byte aligned), the rest one value per lane
__global__ __launch_bounds__(CT_THREADS) void quick_gelu_kernel(const f16* x, f16* y, int64_t nvec, int64_t n) {
  const int64_t t0 = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x, step = (int64_t)gridDim.x * CT_THREADS;
  for (int64_t i = t0; i < nvec; i += step) {
    const f16x8 v = ld_global_16B(x + i * 8);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)quick_gelu_f((float)v[e]);
    *reinterpret_cast<f16x8*>(y + i * 8) = o;
  }
  for (int64_t i = nvec * 8 + t0; i < n; i += step) y[i] = (f16)quick_gelu_f((float)x[i]);
}

}  // namespace

extern "C" int i2v_clip_embed_f16(const void* tok, const void* pos, const int32_t* ids, const int32_t* ids_host, void* out, int32_t batch,
                                  int32_t len, int32_t vocab, int32_t max_positions, int32_t hidden, i2v_stream_t stream) {
  I2V_CHECK_ARG(tok && pos && ids && ids_host && out, "i2v_clip_embed_f16: null pointer");
  I2V_CHECK_ARG(batch > 0 && len > 0 && vocab > 0 && max_positions > 0, "i2v_clip_embed_f16: batch %d len %d vocab %d max_positions %d must be positive",
                batch, len, vocab, max_positions);
  I2V_CHECK_ARG(len <= max_positions, "i2v_clip_embed_f16: %d tokens for a position table of %d rows", len, max_positions);
  I2V_CHECK_ARG(hidden > 0 && hidden % 8 == 0, "i2v_clip_embed_f16: hidden %d must be a positive multiple of 8", hidden);
  I2V_CHECK_ARG((int64_t)batch * len < ((int64_t)1 << 31), "i2v_clip_embed_f16: problem too large (%lld rows)", (long long)batch * len);
  I2V_CHECK_ARG(i2v_al16(tok) && i2v_al16(pos) && i2v_al16(out), "i2v_clip_embed_f16: pointers must be 16-byte aligned");
  const int64_t rows = (int64_t)batch * len;
  for (int64_t i = 0; i < rows; ++i)
    I2V_CHECK_ARG(ids_host[i] >= 0 && ids_host[i] < vocab, "i2v_clip_embed_f16: token id %d at (%lld, %lld) is outside the vocabulary of %d",
                  ids_host[i], (long long)(i / len), (long long)(i % len), vocab);
  const int64_t out_bytes = rows * hidden * 2;
  I2V_CHECK_ARG(!i2v_overlap(out, out_bytes, tok, (int64_t)vocab * hidden * 2) && !i2v_overlap(out, out_bytes, pos, (int64_t)max_positions * hidden * 2) &&
                    !i2v_overlap(out, out_bytes, ids, rows * 4),
                "i2v_clip_embed_f16: out is a new tensor (it must not overlap the tables or the ids)");
  const int chunks = hidden / 8;
  const int64_t total = rows * chunks;
  hipLaunchKernelGGL(clip_embed_kernel, dim3(i2v_ew_grid(total, CT_THREADS, CT_MAX_BLOCKS)), dim3(CT_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(tok), reinterpret_cast<const f16*>(pos), ids, reinterpret_cast<f16*>(out), len, vocab, chunks,
                     total);
  return i2v_check_launch("i2v_clip_embed_f16");
}

extern "C" int i2v_quick_gelu_f16(const void* x, void* y, int64_t n, i2v_stream_t stream) {
  I2V_CHECK_ARG(x && y, "i2v_quick_gelu_f16: null pointer");
  I2V_CHECK_ARG(n > 0 && n < ((int64_t)1 << 40), "i2v_quick_gelu_f16: n %lld must be in [1, 2^40)", (long long)n);
  I2V_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 1) == 0, "i2v_quick_gelu_f16: pointers must be 2-byte aligned");
  I2V_CHECK_ARG(x == y || !i2v_overlap(x, n * 2, y, n * 2), "i2v_quick_gelu_f16: y is x (in place) or does not overlap it");
  const int64_t nvec = (i2v_al16(x) && i2v_al16(y)) ? n / 8 : 0;
  const int64_t items = nvec > n - nvec * 8 ? nvec : n - nvec * 8;
  hipLaunchKernelGGL(quick_gelu_kernel, dim3(i2v_ew_grid(items, CT_THREADS, CT_MAX_BLOCKS)), dim3(CT_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(x), reinterpret_cast<f16*>(y), nvec, n);
  return i2v_check_launch("i2v_quick_gelu_f16");
}
