// Backward kernels of the adapter training step (reference loop src/train_image_to_video.py:839-884, trainable
// set unet:979-1026 = i2v_adapter.to_q / to_out only): what the backward of one I2VAdapterTransformerBlock needs beside
// i2v_gemm_f16 (dgrad = the same GEMM over transposed weights, wgrad = the same GEMM over transposed activations) and the
// flash-attention backward (attention_bwd.hip):
//
//   * the channel-major operand copies of the attention backward (i2v_transpose_f16), rowsum(dO o O) per head;
//   * LayerNorm backward (input gradient only: the norms are frozen), GEGLU backward, column sums (bias gradient),
//     the masked-MSE seed gradient (loss without the first frame, train_image_to_video.py:848-856);
//   * the permutes, pools and the optimiser step (sum of squares, AdamW, axpby).
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ small kernels
// dst[b][c][r] = src[b][r][c]; columns r in [rows, rows8) of dst are zero-filled
__global__ __launch_bounds__(256) void transpose_kernel(const f16* __restrict__ src, int64_t src_bs, int64_t ld_src,
                                                        f16* __restrict__ dst, int64_t dst_bs, int64_t ld_dst, int rows,
                                                        int cols, int rows8) {
  __shared__ f16 tile[64][66];
  const int b = blockIdx.z, r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const f16* s = src + (int64_t)b * src_bs;
  f16* t = dst + (int64_t)b * dst_bs;
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i, cc = c0 + tx;
    tile[i][tx] = (r < rows && cc < cols) ? s[(int64_t)r * ld_src + cc] : (f16)0.f;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int cc = c0 + i, r = r0 + tx;
    if (cc < cols && r < rows8) t[(int64_t)cc * ld_dst + r] = tile[tx][i];
  }
}

// out[(b * heads + h) * L + l] = sum_i a[b][l][h d + i] * bm[b][l][h d + i]
__global__ __launch_bounds__(256) void rowdot_kernel(const f16* __restrict__ a, int64_t lda, const f16* __restrict__ bm,
                                                     int64_t ldb, float* __restrict__ out, int64_t rows, int L, int heads,
                                                     int d) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * heads) return;
  const int64_t row = idx / heads;
  const int h = (int)(idx - row * heads);
  const f16* pa = a + row * lda + h * d;
  const f16* pb = bm + row * ldb + h * d;
  float s = 0.f;
  for (int i = 0; i < d; i += 8) {
    const f16x8 x = ld_global_16B(pa + i), y = ld_global_16B(pb + i);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += (float)x[e] * (float)y[e];
  }
  const int64_t b = row / L, l = row - b * L;
  out[(b * heads + h) * L + l] = s;
}

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// LayerNorm backward, input gradient only: with xh = (x - mean) rstd and gy = dn o gamma,
//   dx = rstd (gy - mean(gy) - xh mean(gy o xh))  (+ add: the gradient arriving over the residual path)
__global__ __launch_bounds__(256) void ln_bwd_kernel(const f16* __restrict__ x, int64_t ldx, const f16* __restrict__ dn,
                                                     int64_t lddn, const f16* __restrict__ gamma, const f16* __restrict__ add,
                                                     int64_t ldadd, f16* __restrict__ dx, int64_t lddx, int rows, int C,
                                                     float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const f16* xr = x + (int64_t)row * ldx;
  const f16* dr = dn + (int64_t)row * lddn;
  const int nvec = C / 8;
  float s = 0.f;
  for (int v = lane; v < nvec; v += 64) {
    const f16x8 a = ld_global_16B(xr + 8 * v);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += (float)a[e];
  }
  const float mean = wave_sum64(s) / (float)C;
  float q = 0.f;
  for (int v = lane; v < nvec; v += 64) {
    const f16x8 a = ld_global_16B(xr + 8 * v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = (float)a[e] - mean;
      q += t * t;
    }
  }
  const float rstd = rsqrtf(wave_sum64(q) / (float)C + eps);
  float s1 = 0.f, s2 = 0.f;
  for (int v = lane; v < nvec; v += 64) {
    const f16x8 a = ld_global_16B(xr + 8 * v), dd = ld_global_16B(dr + 8 * v), ga = ld_global_16B(gamma + 8 * v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gy = (float)dd[e] * (float)ga[e];
      s1 += gy;
      s2 += gy * ((float)a[e] - mean) * rstd;
    }
  }
  s1 = wave_sum64(s1) / (float)C;
  s2 = wave_sum64(s2) / (float)C;
  for (int v = lane; v < nvec; v += 64) {
    const f16x8 a = ld_global_16B(xr + 8 * v), dd = ld_global_16B(dr + 8 * v), ga = ld_global_16B(gamma + 8 * v);
    f16x8 up = zero8();
    if (add) up = ld_global_16B(add + (int64_t)row * ldadd + 8 * v);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = ((float)a[e] - mean) * rstd;
      o[e] = (f16)(rstd * ((float)dd[e] * (float)ga[e] - s1 - xh * s2) + (float)up[e]);
    }
    *reinterpret_cast<f16x8*>(dx + (int64_t)row * lddx + 8 * v) = o;
  }
}

// GEGLU backward: h [rows][2 inner] interleaved (value_i, gate_i) (the pre-activation of the I2V_EPI_GEGLU GEMM),
// dy [rows][inner] -> dh[.., 2 i] = dy gelu(g), dh[.., 2 i + 1] = dy a (Phi(g) + g phi(g))
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const f16* __restrict__ hh, int64_t ldh, const f16* __restrict__ dy,
                                                        int64_t lddy, f16* __restrict__ dh, int64_t lddh, int64_t rows,
                                                        int inner) {
  const int nvec = inner / 4;    // 4 outputs = 8 interleaved inputs per thread
  const int64_t total = rows * nvec;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / nvec;
    const int v = (int)(idx - row * nvec);
    const f16x8 hv = ld_global_16B(hh + row * ldh + 8 * v);
    const f16x4 d4 = *reinterpret_cast<const f16x4*>(dy + row * lddy + 4 * v);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = (float)hv[2 * e], gt = (float)hv[2 * e + 1], dd = (float)d4[e];
      const float phi = 0.5f * (1.0f + erff(gt * 0.70710678118654752440f));
      const float pdf = 0.39894228040143267794f * __expf(-0.5f * gt * gt);
      o[2 * e] = (f16)(dd * gt * phi);
      o[2 * e + 1] = (f16)(dd * a * (phi + gt * pdf));
    }
    *reinterpret_cast<f16x8*>(dh + row * lddh + 8 * v) = o;
  }
}

// GEGLU forward from the stored pre-activation: y[.., i] = h[.., 2 i] gelu(h[.., 2 i + 1]) (the training forward keeps h for the
// backward and derives y from it, instead of running the projection GEMM a second time with the fused GEGLU epilogue)
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const f16* __restrict__ hh, int64_t ldh, f16* __restrict__ y, int64_t ldy,
                                                        int64_t rows, int inner) {
  const int nvec = inner / 8;    // 8 outputs = 16 interleaved inputs per thread
  const int64_t total = rows * nvec;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / nvec;
    const int v = (int)(idx - row * nvec);
    const f16x8 h0 = ld_global_16B(hh + row * ldh + 16 * v), h1 = ld_global_16B(hh + row * ldh + 16 * v + 8);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = (f16)((float)h0[2 * e] * gelu_erf((float)h0[2 * e + 1]));
      o[4 + e] = (f16)((float)h1[2 * e] * gelu_erf((float)h1[2 * e + 1]));
    }
    *reinterpret_cast<f16x8*>(y + row * ldy + 8 * v) = o;
  }
}

// out[c] += sum_r x[r][c] (fp32 atomics over row chunks; out is zeroed / accumulated by the caller)
__global__ __launch_bounds__(256) void colsum_kernel(const f16* __restrict__ x, int64_t ldx, float* __restrict__ out,
                                                     int64_t rows, int cols, int64_t rows_per_block) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  float s = 0.f;
  if (c < cols)
    for (int64_t r = r0 + rl; r < r1; r += 4) s += (float)x[r * ldx + c];
  red[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && c < cols) atomicAdd(out + c, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// out[c] += sum_r a[r][c] b[r][c]: the gain gradient of a LayerNorm / GroupNorm (d gamma = sum dy o xhat)
__global__ __launch_bounds__(256) void colsum_prod_kernel(const f16* __restrict__ a, int64_t lda, const f16* __restrict__ b,
                                                          int64_t ldb, float* __restrict__ out, int64_t rows, int cols,
                                                          int64_t rows_per_block) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  float s = 0.f;
  if (c < cols)
    for (int64_t r = r0 + rl; r < r1; r += 4) s += (float)a[r * lda + c] * (float)b[r * ldb + c];
  red[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && c < cols) atomicAdd(out + c, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// The same sums with a run-to-run identical result (the atomics above make bias / gain gradients depend on block
// scheduling): every 256-row block writes its partial, one thread per column adds the partials in block order.
__global__ __launch_bounds__(256) void colsum_partial_kernel(const f16* __restrict__ a, int64_t lda, const f16* __restrict__ b,
                                                             int64_t ldb, float* __restrict__ partial, int64_t rows, int cols,
                                                             int64_t rows_per_block) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  float s = 0.f;
  if (c < cols) {
    if (b != nullptr)
      for (int64_t r = r0 + rl; r < r1; r += 4) s += (float)a[r * lda + c] * (float)b[r * ldb + c];
    else
      for (int64_t r = r0 + rl; r < r1; r += 4) s += (float)a[r * lda + c];
  }
  red[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && c < cols)
    partial[(int64_t)blockIdx.y * cols + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ partial, float* __restrict__ out, int nblocks,
                                                           int cols) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  float s = 0.f;
  for (int i = 0; i < nblocks; ++i) s += partial[(int64_t)i * cols + c];
  out[c] += s;
}

// g[m][c] = coef (y[m][c] - t[m][c]) for tokens of frames >= 1, 0 for the first frame of every clip
__global__ __launch_bounds__(256) void mse_grad_kernel(const f16* __restrict__ y, const f16* __restrict__ t,
                                                       f16* __restrict__ gout, int64_t n_img, int L, int C, int frames,
                                                       float coef) {
  const int nvec = C / 8;
  const int64_t total = n_img * L * nvec;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t row = idx / nvec;
    const int64_t img = row / L;
    const bool first = (img % frames) == 0;
    const f16x8 a = ld_global_16B(y + idx * 8), b = ld_global_16B(t + idx * 8);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = first ? (f16)0.f : (f16)(coef * ((float)a[e] - (float)b[e]));
    *reinterpret_cast<f16x8*>(gout + idx * 8) = o;
  }
}

// the same seed from an fp32 prediction and an fp32 target (F.mse_loss(model_pred.float(), target.float()),
// train_image_to_video.py:848): only the emitted gradient is fp16; rowsq[m] = sum_c (y - t)^2 of the unmasked rows (0 on the
// first frame of a clip) is the loss's numerator, summed by the caller in a fixed order
__global__ __launch_bounds__(256) void mse_grad_f32_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                           f16* __restrict__ gout, float* __restrict__ rowsq, int64_t n_img, int L,
                                                           int C, int frames, float coef) {
  const int64_t rows = n_img * L;
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < rows; row += (int64_t)gridDim.x * 256) {
    const bool first = ((row / L) % frames) == 0;
    float sq = 0.f;
    for (int c0 = 0; c0 < C; c0 += 8) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(y + row * C + c0), a1 = *reinterpret_cast<const f32x4*>(y + row * C + c0 + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(t + row * C + c0), b1 = *reinterpret_cast<const f32x4*>(t + row * C + c0 + 4);
      f16x8 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d0 = first ? 0.f : a0[e] - b0[e], d1 = first ? 0.f : a1[e] - b1[e];
        sq = fmaf(d0, d0, fmaf(d1, d1, sq));
        o[e] = (f16)(coef * d0);
        o[4 + e] = (f16)(coef * d1);
      }
      *reinterpret_cast<f16x8*>(gout + row * C + c0) = o;
    }
    rowsq[row] = sq;
  }
}

// out = a + b (gradients meeting at a skip connection / a residual branch)
__global__ __launch_bounds__(256) void add_kernel(const f16* __restrict__ a, const f16* __restrict__ b, f16* __restrict__ out,
                                                  int64_t nvec) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const f16x8 x = ld_global_16B(a + 8 * i), y = ld_global_16B(b + 8 * i);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)((float)x[e] + (float)y[e]);
    *reinterpret_cast<f16x8*>(out + 8 * i) = o;
  }
}

// rows (b, f, p) <-> (b, p, f): to_pixel_major = 1 reads row (b f + f') hw + p and writes row (b hw + p) F + f'
__global__ __launch_bounds__(256) void permute_rows_kernel(const f16* __restrict__ src, f16* __restrict__ dst, int64_t batches,
                                                           int frames, int hw, int C, int to_pixel_major) {
  const int nvec = C / 8;
  const int64_t total = batches * frames * hw * nvec;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int v = (int)(idx % nvec);
    const int64_t row = idx / nvec;                       // destination row
    const int64_t per = (int64_t)frames * hw, b = row / per, rem = row - b * per;
    int64_t srow;
    if (to_pixel_major) {
      const int64_t p = rem / frames, f = rem - p * frames;
      srow = b * per + f * hw + p;
    } else {
      const int64_t f = rem / hw, p = rem - f * hw;
      srow = b * per + p * frames + f;
    }
    *reinterpret_cast<f16x8*>(dst + row * C + 8 * v) = ld_global_16B(src + srow * C + 8 * v);
  }
}

// dst [n, 2h, 2w, C]: dst[2y][2x] = src[y][x], zero elsewhere (the input-gradient of a stride-2 convolution is the
// stride-1 convolution of this with the flipped, transposed weights)
__global__ __launch_bounds__(256) void zero_insert_kernel(const f16* __restrict__ src, f16* __restrict__ dst, int64_t n, int h,
                                                          int w, int C) {
  const int nvec = C / 8;
  const int64_t total = n * (2 * h) * (2 * w) * nvec;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int v = (int)(idx % nvec);
    int64_t r = idx / nvec;
    const int xx = (int)(r % (2 * w));
    r /= 2 * w;
    const int yy = (int)(r % (2 * h));
    const int64_t img = r / (2 * h);
    f16x8 o = zero8();
    if (((xx | yy) & 1) == 0) o = ld_global_16B(src + ((img * h + (yy >> 1)) * w + (xx >> 1)) * C + 8 * v);
    *reinterpret_cast<f16x8*>(dst + idx * 8) = o;
  }
}

// dst [n, h, w, C] = sum of the 2 x 2 blocks of src [n, 2h, 2w, C] (input-gradient of the nearest-2x upsampling)
__global__ __launch_bounds__(256) void sum_pool_kernel(const f16* __restrict__ src, f16* __restrict__ dst, int64_t n, int h, int w,
                                                       int C) {
  const int nvec = C / 8;
  const int64_t total = n * h * w * nvec;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int v = (int)(idx % nvec);
    int64_t r = idx / nvec;
    const int xx = (int)(r % w);
    r /= w;
    const int yy = (int)(r % h);
    const int64_t img = r / h;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const f16x8 t = ld_global_16B(src + ((img * 2 * h + 2 * yy + dy) * (2 * w) + 2 * xx + dx) * C + 8 * v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (float)t[e];
      }
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)acc[e];
    *reinterpret_cast<f16x8*>(dst + idx * 8) = o;
  }
}

// out[0] += sum x^2 (global gradient norm for clip_grad_norm_, train_image_to_video.py:878-879)
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += x[i] * x[i];
  s = wave_sum64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// torch.optim.AdamW (decoupled weight decay) over one flat fp32 bucket; grad_coef folds 1 / loss_scale, the data-parallel
// mean and the clip coefficient: g = grad * min(1, max_norm / (*norm_sq)^0.5 / ...) is applied by the caller through it,
// except the clip, which reads the DEVICE value *norm_sq (no host round trip): g *= min(1, max_norm / (sqrt(norm_sq) grad_coef'))
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                    float* __restrict__ m, float* __restrict__ v, int64_t n, float lr, float b1,
                                                    float b2, float eps, float wd, float bc1, float bc2, float grad_coef,
                                                    const float* __restrict__ norm_sq, float max_norm) {
  float coef = grad_coef;
  if (norm_sq != nullptr && max_norm > 0.f) {
    const float total = sqrtf(*norm_sq) * grad_coef;          // norm of the un-scaled, averaged gradient
    coef *= fminf(1.0f, max_norm / (total + 1e-6f));           // clip_grad_norm_'s coefficient
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float g = grad[i] * coef;
    float p = param[i] * (1.0f - lr * wd);
    const float mi = b1 * m[i] + (1.0f - b1) * g;
    const float vi = b2 * v[i] + (1.0f - b2) * g * g;
    m[i] = mi;
    v[i] = vi;
    p -= lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
    param[i] = p;
  }
}

// Run-to-run identical, rank-to-rank identical gradient norm + the overflow guard of a mixed-precision step:
// sumsq_partials_kernel writes one partial per workgroup (no atomics); adamw_prepare_kernel (ONE workgroup) sums them in a
// fixed order, publishes the total, and decides the step: a non-finite norm (an inf / NaN anywhere in the fp16-scaled
// gradients) sets *found_inf and leaves the applied-step counter alone, otherwise the counter advances.
// adamw_guarded_kernel is a no-op under *found_inf -- parameters, both moments and the bias-correction step stay as they
// were, which is what accelerate's GradScaler does for the reference's fp16 run (train_image_to_video.py:306-308, 876-882).
__global__ __launch_bounds__(256) void sumsq_partials_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ partials) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += x[i] * x[i];
  s = wave_sum64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void adamw_prepare_kernel(const float* __restrict__ partials, int n_partials,
                                                            float* __restrict__ norm_sq, int32_t* __restrict__ applied_steps,
                                                            int32_t* __restrict__ found_inf) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n_partials; i += 256) s += partials[i];   // fixed order per thread, fixed tree below
  s = wave_sum64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float total = (red[0] + red[1]) + (red[2] + red[3]);
    *norm_sq = total;
    // inf or NaN, tested on the BITS (exponent all ones): this library is built with -fno-honor-nans, under which the compiler
    // rewrites !(|x| <= c) as |x| > c -- false for NaN (the first form of this test let a NaN gradient through)
    // (and on bits the optimiser cannot trace back to a float: it recognises the mask-and-compare as an fpclass test and, told
    //  that NaNs do not exist, narrows it to "is infinite" -- measured: inf caught, NaN let through)
    uint32_t bits = __builtin_bit_cast(uint32_t, total);
    asm volatile("" : "+v"(bits));
    const bool bad = (bits & 0x7f800000u) == 0x7f800000u;
    *found_inf = bad ? 1 : 0;
    if (!bad) *applied_steps += 1;
  }
}

__global__ __launch_bounds__(256) void adamw_guarded_kernel(float* __restrict__ param, const float* __restrict__ grad,
                                                            float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                            float b1, float b2, float eps, float wd, float grad_coef,
                                                            const float* __restrict__ norm_sq, float max_norm,
                                                            const int32_t* __restrict__ applied_steps,
                                                            const int32_t* __restrict__ found_inf) {
  if (*found_inf) return;                                       // overflowed gradients: the whole update is skipped
  const float step = (float)*applied_steps;
  const float bc1 = 1.0f - powf(b1, step), bc2 = 1.0f - powf(b2, step);
  float coef = grad_coef;
  if (max_norm > 0.f) {
    const float total = sqrtf(*norm_sq) * grad_coef;
    coef *= fminf(1.0f, max_norm / (total + 1e-6f));
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float g = grad[i] * coef;
    float p = param[i] * (1.0f - lr * wd);
    const float mi = b1 * m[i] + (1.0f - b1) * g;
    const float vi = b2 * v[i] + (1.0f - b2) * g * g;
    m[i] = mi;
    v[i] = vi;
    p -= lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
    param[i] = p;
  }
}

inline int ew_grid(int64_t n) {
  const int64_t b = i2v_cdiv(n, 256);
  return (int)(b < 65535 * 4 ? (b > 0 ? b : 1) : 65535 * 4);
}

}  // namespace

extern "C" int i2v_transpose_f16(const void* src, int64_t src_batch_stride, int64_t ld_src, void* dst,
                                 int64_t dst_batch_stride, int64_t ld_dst, int32_t batches, int32_t rows, int32_t cols,
                                 i2v_stream_t stream) {
  const int rows8 = (rows + 7) & ~7;
  I2V_CHECK_ARG(src && dst && batches > 0 && rows > 0 && cols > 0 && ld_src >= cols && ld_dst >= rows8 && batches <= 65535,
                "i2v_transpose_f16: bad arguments (ld_dst must cover rows rounded up to 8)");
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)i2v_cdiv(rows8, 64), (unsigned)i2v_cdiv(cols, 64), batches), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(src), src_batch_stride, ld_src,
                     reinterpret_cast<f16*>(dst), dst_batch_stride, ld_dst, rows, cols, rows8);
  return i2v_check_launch("i2v_transpose_f16");
}

extern "C" int i2v_rowdot_heads_f32(const void* a, int64_t lda, const void* b, int64_t ldb, float* out, int64_t rows,
                                    int32_t rows_per_batch, int32_t heads, int32_t head_dim, i2v_stream_t stream) {
  I2V_CHECK_ARG(a && b && out && rows > 0 && rows_per_batch > 0 && rows % rows_per_batch == 0 && heads > 0 && head_dim > 0 &&
                    head_dim % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && i2v_al16(a) && i2v_al16(b),
                "i2v_rowdot_heads_f32: bad arguments");
  hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)i2v_cdiv(rows * heads, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(a), lda,
                     reinterpret_cast<const f16*>(b), ldb, out, rows, rows_per_batch, heads, head_dim);
  return i2v_check_launch("i2v_rowdot_heads_f32");
}

extern "C" int i2v_layernorm_bwd_f16(const void* x, int64_t ldx, const void* dn, int64_t lddn, const void* gamma,
                                     const void* add, int64_t ldadd, void* dx, int64_t lddx, int32_t rows, int32_t C, float eps,
                                     i2v_stream_t stream) {
  I2V_CHECK_ARG(x && dn && gamma && dx && rows > 0 && C > 0 && C % 8 == 0 && ldx % 8 == 0 && lddn % 8 == 0 && lddx % 8 == 0 &&
                    (!add || ldadd % 8 == 0) && i2v_al16(x) && i2v_al16(dn) && i2v_al16(gamma) && i2v_al16(dx) && (!add || i2v_al16(add)),
                "i2v_layernorm_bwd_f16: bad arguments (C and the strides must be multiples of 8, pointers 16-byte aligned)");
  hipLaunchKernelGGL(ln_bwd_kernel, dim3((unsigned)i2v_cdiv(rows, 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(x), ldx, reinterpret_cast<const f16*>(dn), lddn,
                     reinterpret_cast<const f16*>(gamma), reinterpret_cast<const f16*>(add), ldadd, reinterpret_cast<f16*>(dx),
                     lddx, rows, C, eps);
  return i2v_check_launch("i2v_layernorm_bwd_f16");
}

extern "C" int i2v_geglu_bwd_f16(const void* h, int64_t ldh, const void* dy, int64_t lddy, void* dh, int64_t lddh, int64_t rows,
                                 int32_t inner, i2v_stream_t stream) {
  I2V_CHECK_ARG(h && dy && dh && rows > 0 && inner > 0 && inner % 4 == 0 && ldh % 8 == 0 && lddh % 8 == 0 && lddy % 4 == 0 &&
                    i2v_al16(h) && i2v_al16(dh) && (reinterpret_cast<uintptr_t>(dy) & 7) == 0,
                "i2v_geglu_bwd_f16: bad arguments");
  hipLaunchKernelGGL(geglu_bwd_kernel, dim3(ew_grid(rows * (inner / 4))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(h), ldh, reinterpret_cast<const f16*>(dy), lddy, reinterpret_cast<f16*>(dh),
                     lddh, rows, inner);
  return i2v_check_launch("i2v_geglu_bwd_f16");
}

extern "C" int i2v_geglu_f16(const void* h, int64_t ldh, void* y, int64_t ldy, int64_t rows, int32_t inner, i2v_stream_t stream) {
  I2V_CHECK_ARG(h && y && rows > 0 && inner > 0 && inner % 8 == 0 && ldh % 8 == 0 && ldy % 8 == 0 && ldh >= 2 * inner &&
                    ldy >= inner && i2v_al16(h) && i2v_al16(y),
                "i2v_geglu_f16: bad arguments");
  hipLaunchKernelGGL(geglu_fwd_kernel, dim3(ew_grid(rows * (inner / 8))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(h), ldh, reinterpret_cast<f16*>(y), ldy, rows, inner);
  return i2v_check_launch("i2v_geglu_f16");
}

extern "C" int i2v_colsum_f32(const void* x, int64_t ldx, float* out, int64_t rows, int32_t cols, i2v_stream_t stream) {
  I2V_CHECK_ARG(x && out && rows > 0 && cols > 0 && ldx >= cols, "i2v_colsum_f32: bad arguments");
  const int64_t rpb = 256;
  hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)i2v_cdiv(cols, 64), (unsigned)i2v_cdiv(rows, rpb)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(x), ldx, out, rows, cols, rpb);
  return i2v_check_launch("i2v_colsum_f32");
}

extern "C" int i2v_colsum_prod_f32(const void* a, int64_t lda, const void* b, int64_t ldb, float* out, int64_t rows, int32_t cols,
                                   i2v_stream_t stream) {
  I2V_CHECK_ARG(a && b && out && rows > 0 && cols > 0 && lda >= cols && ldb >= cols, "i2v_colsum_prod_f32: bad arguments");
  const int64_t rpb = 256;
  hipLaunchKernelGGL(colsum_prod_kernel, dim3((unsigned)i2v_cdiv(cols, 64), (unsigned)i2v_cdiv(rows, rpb)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(a), lda, reinterpret_cast<const f16*>(b),
                     ldb, out, rows, cols, rpb);
  return i2v_check_launch("i2v_colsum_prod_f32");
}

extern "C" int64_t i2v_colsum_workspace_bytes(int64_t rows, int32_t cols) {
  return rows > 0 && cols > 0 ? i2v_cdiv(rows, 256) * (int64_t)cols * (int64_t)sizeof(float) : 0;
}

extern "C" int i2v_colsum_det_f32(const void* a, int64_t lda, const void* b, int64_t ldb, float* out, int64_t rows, int32_t cols,
                                  void* workspace, i2v_stream_t stream) {
  I2V_CHECK_ARG(a && out && workspace && rows > 0 && cols > 0 && lda >= cols && (b == nullptr || ldb >= cols) &&
                    i2v_cdiv(rows, 256) < (1 << 30), "i2v_colsum_det_f32: bad arguments");
  const int64_t rpb = 256, nb = i2v_cdiv(rows, rpb);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(colsum_partial_kernel, dim3((unsigned)i2v_cdiv(cols, 64), (unsigned)nb), dim3(256), 0, s,
                     reinterpret_cast<const f16*>(a), lda, reinterpret_cast<const f16*>(b), ldb, reinterpret_cast<float*>(workspace),
                     rows, cols, rpb);
  hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)i2v_cdiv(cols, 256)), dim3(256), 0, s,
                     reinterpret_cast<const float*>(workspace), out, (int)nb, cols);
  return i2v_check_launch("i2v_colsum_det_f32");
}

extern "C" int i2v_masked_mse_grad_f16(const void* y, const void* target, void* grad, int64_t n_img, int32_t tokens,
                                       int32_t channels, int32_t frames, float coef, i2v_stream_t stream) {
  I2V_CHECK_ARG(y && target && grad && n_img > 0 && tokens > 0 && channels > 0 && channels % 8 == 0 && frames > 0 &&
                    n_img % frames == 0 && i2v_al16(y) && i2v_al16(target) && i2v_al16(grad),
                "i2v_masked_mse_grad_f16: bad arguments");
  hipLaunchKernelGGL(mse_grad_kernel, dim3(ew_grid(n_img * tokens * (channels / 8))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(y),
                     reinterpret_cast<const f16*>(target), reinterpret_cast<f16*>(grad), n_img, tokens, channels, frames, coef);
  return i2v_check_launch("i2v_masked_mse_grad_f16");
}

extern "C" int i2v_masked_mse_grad_f32(const float* y, const float* target, void* grad, float* rowsq, int64_t n_img, int32_t tokens,
                                       int32_t channels, int32_t frames, float coef, i2v_stream_t stream) {
  I2V_CHECK_ARG(y && target && grad && rowsq && n_img > 0 && tokens > 0 && channels > 0 && channels % 8 == 0 && frames > 0 &&
                    n_img % frames == 0 && i2v_al16(y) && i2v_al16(target) && i2v_al16(grad),
                "i2v_masked_mse_grad_f32: bad arguments");
  hipLaunchKernelGGL(mse_grad_f32_kernel, dim3(ew_grid(n_img * tokens)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), y, target,
                     reinterpret_cast<f16*>(grad), rowsq, n_img, tokens, channels, frames, coef);
  return i2v_check_launch("i2v_masked_mse_grad_f32");
}

extern "C" int i2v_add_f16(const void* a, const void* b, void* out, int64_t n, i2v_stream_t stream) {
  I2V_CHECK_ARG(a && b && out && n > 0 && n % 8 == 0 && i2v_al16(a) && i2v_al16(b) && i2v_al16(out), "i2v_add_f16: bad arguments");
  hipLaunchKernelGGL(add_kernel, dim3(ew_grid(n / 8)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f16*>(a), reinterpret_cast<const f16*>(b), reinterpret_cast<f16*>(out), n / 8);
  return i2v_check_launch("i2v_add_f16");
}

extern "C" int i2v_permute_rows_f16(const void* src, void* dst, int64_t batches, int32_t frames, int32_t hw, int32_t channels,
                                    int32_t to_pixel_major, i2v_stream_t stream) {
  I2V_CHECK_ARG(src && dst && src != dst && batches > 0 && frames > 0 && hw > 0 && channels > 0 && channels % 8 == 0 &&
                    i2v_al16(src) && i2v_al16(dst), "i2v_permute_rows_f16: bad arguments");
  hipLaunchKernelGGL(permute_rows_kernel, dim3(ew_grid(batches * frames * hw * (channels / 8))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(src), reinterpret_cast<f16*>(dst),
                     batches, frames, hw, channels, to_pixel_major);
  return i2v_check_launch("i2v_permute_rows_f16");
}

extern "C" int i2v_zero_insert2x_f16(const void* src, void* dst, int64_t n_img, int32_t h, int32_t w, int32_t channels,
                                     i2v_stream_t stream) {
  I2V_CHECK_ARG(src && dst && n_img > 0 && h > 0 && w > 0 && channels > 0 && channels % 8 == 0 && i2v_al16(src) && i2v_al16(dst),
                "i2v_zero_insert2x_f16: bad arguments");
  hipLaunchKernelGGL(zero_insert_kernel, dim3(ew_grid(n_img * 4 * h * w * (channels / 8))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(src), reinterpret_cast<f16*>(dst), n_img, h,
                     w, channels);
  return i2v_check_launch("i2v_zero_insert2x_f16");
}

extern "C" int i2v_sum_pool2x_f16(const void* src, void* dst, int64_t n_img, int32_t h, int32_t w, int32_t channels,
                                  i2v_stream_t stream) {
  I2V_CHECK_ARG(src && dst && n_img > 0 && h > 0 && w > 0 && channels > 0 && channels % 8 == 0 && i2v_al16(src) && i2v_al16(dst),
                "i2v_sum_pool2x_f16: bad arguments");
  hipLaunchKernelGGL(sum_pool_kernel, dim3(ew_grid(n_img * h * w * (channels / 8))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16*>(src), reinterpret_cast<f16*>(dst), n_img, h,
                     w, channels);
  return i2v_check_launch("i2v_sum_pool2x_f16");
}

extern "C" int i2v_sumsq_f32(const float* x, int64_t n, float* out, i2v_stream_t stream) {
  I2V_CHECK_ARG(x && out && n > 0, "i2v_sumsq_f32: bad arguments");
  const int64_t b = i2v_cdiv(n, 256);
  hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)(b < 1024 ? b : 1024)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, n, out);
  return i2v_check_launch("i2v_sumsq_f32");
}

// y = a y + b x over a flat fp32 bucket: gradient accumulation (a = 1, b = 1 / accumulation steps) and the EMA of the trained
// weights (a = decay, b = 1 - decay)
__global__ __launch_bounds__(256) void axpby_kernel(float* __restrict__ y, const float* __restrict__ x, float a, float b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = a * y[i] + b * x[i];
}

extern "C" int i2v_axpby_f32(float* y, const float* x, float a, float b, int64_t n, i2v_stream_t stream) {
  I2V_CHECK_ARG(y && x && n > 0, "i2v_axpby_f32: bad arguments");
  const int64_t blk = i2v_cdiv(n, 256);
  hipLaunchKernelGGL(axpby_kernel, dim3((unsigned)(blk < 4096 ? blk : 4096)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), y, x,
                     a, b, n);
  return i2v_check_launch("i2v_axpby_f32");
}

extern "C" int i2v_adamw_guarded_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, float grad_coef, float max_norm,
                                     float* partials, int32_t n_partials, float* norm_sq, int32_t* applied_steps,
                                     int32_t* found_inf, i2v_stream_t stream) {
  I2V_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && n > 0, "i2v_adamw_guarded_f32: bad arguments");
  I2V_CHECK_ARG(partials && norm_sq && applied_steps && found_inf && n_partials >= 1 && n_partials <= 1024,
                "i2v_adamw_guarded_f32: partials[1..1024], norm_sq, applied_steps and found_inf are required");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t b = i2v_cdiv(n, 256);
  const int np = (int)(b < n_partials ? b : n_partials);
  hipLaunchKernelGGL(sumsq_partials_kernel, dim3(np), dim3(256), 0, s, grad, n, partials);
  hipLaunchKernelGGL(adamw_prepare_kernel, dim3(1), dim3(256), 0, s, partials, np, norm_sq, applied_steps, found_inf);
  hipLaunchKernelGGL(adamw_guarded_kernel, dim3((unsigned)(b < 4096 ? b : 4096)), dim3(256), 0, s, param, grad, exp_avg, exp_avg_sq,
                     n, lr, beta1, beta2, eps, weight_decay, grad_coef, norm_sq, max_norm, applied_steps, found_inf);
  return i2v_check_launch("i2v_adamw_guarded_f32");
}

extern "C" int i2v_adamw_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int32_t step, float grad_coef, const float* norm_sq,
                             float max_norm, i2v_stream_t stream) {
  I2V_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && n > 0 && step >= 1, "i2v_adamw_f32: bad arguments");
  const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
  const int64_t b = i2v_cdiv(n, 256);
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)(b < 4096 ? b : 4096)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), param,
                     grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, grad_coef, norm_sq, max_norm);
  return i2v_check_launch("i2v_adamw_f32");
}
