// Backward kernels of the adapter training step (reference loop src/train_image_to_video.py:839-884, trainable
// set unet:979-1026 = i2v_adapter.to_q / to_out only): what the backward of one I2VAdapterTransformerBlock needs beside
// i2v_gemm_f16 (dgrad = the same GEMM over transposed weights, wgrad = the same GEMM over transposed activations):
//
//   * flash-attention backward on MFMA, recomputing P from Q, K and the forward's log-sum-exp (never the L x L scores):
//       dQ   kernel: a wave owns 16 queries, sweeps the keys:   S^T = K Q^T, dP^T = V dO^T (key on the MFMA row, so the
//                    accumulators ARE the B operand of)           dQ^T += K^T dS^T
//       dK/dV kernel: a wave owns 16 keys, sweeps the queries of every batch entry that shares them (kv_group: the F
//                    frames of a clip read the frame-0 K / V, i2v:483-492 -- dK0 / dV0 are summed over the frames here,
//                    in registers):                              S = Q K^T, dP = dO V^T (query on the MFMA row), then
//                                                                 dV^T += dO^T P,  dK^T += Q^T dS
//     two sweeps (7 products instead of 5) buy: no atomics, no cross-workgroup sum, run-to-run identical gradients.
//     The K^T / Q^T / dO^T operands are channel-major copies ([batch][channel][token], the V^T layout of the forward)
//     made by i2v_transpose_f16;
//   * the log-sum-exp of a forward attention (the inference kernel does not keep it), rowsum(dO o O) per head;
//   * LayerNorm backward (input gradient only: the norms are frozen), GEGLU backward, column sums (bias gradient),
//     the masked-MSE seed gradient (loss without the first frame, train_image_to_video.py:848-856).
//
// MFMA orientation (v_mfma_f32_16x16x32_f16, D = A B): A lane (row = l & 15, k = 8 (l >> 4) + 0..7), B lane
// (k = 8 (l >> 4) + 0..7, col = l & 15), D lane (row = 4 (l >> 4) + r, col = l & 15).  Rows of a 32-row block are
// dealt to the two 16-row MFMAs so that D rows 4 g + r of tiles t = 0, 1 are block rows 8 g + 4 t + r: a lane's 8
// values are block rows 8 g .. 8 g + 7 = one B-operand fragment of the next product, no lane movement (as attention.hip).
#include <cstdlib>

#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ int perm_row(int l15, int t) { return 8 * (l15 >> 2) + 4 * t + (l15 & 3); }

// the fragments of one token row over the (zero-padded) head dim: chunk s holds channels 32 s + 8 g .. + 7
template <int KS>
__device__ __forceinline__ void row_frags(f16x8 (&f)[KS], const f16* row_ptr, bool row_ok, int g, int d) {
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int dd = 32 * s + 8 * g;
    f[s] = (row_ok && dd < d) ? ld_global_16B(row_ptr + dd) : zero8();
  }
}

template <int KS>
__device__ __forceinline__ f32x4 chain(const f16x8 (&a)[KS], const f16x8 (&b)[KS]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < KS; ++s) acc = mfma16x16x32(a[s], b[s], acc);
  return acc;
}

__device__ __forceinline__ f16x8 pack8(const float (&lo)[4], const float (&hi)[4]) {
  f16x8 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    o[r] = (f16)lo[r];
    o[4 + r] = (f16)hi[r];
  }
  return o;
}

__device__ __forceinline__ float group_max(float v) {   // over the 4 lane groups holding the same column
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// ------------------------------------------------------------------------------------------------ log-sum-exp
// lse[bq][h][q] = log2 sum_j exp2(c s_qj), c = scale log2 e: the statistic the backward recomputes P from.
template <int KS>
__global__ __launch_bounds__(256) void attn_lse_kernel(const i2v_attn_params p, const float c, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
  const int h = blockIdx.y, bq = blockIdx.z, bkv = bq / p.kv_group, d = p.head_dim;
  const int q = blockIdx.x * 64 + wave * 16 + l15;
  const f16* Q = reinterpret_cast<const f16*>(p.q) + (int64_t)bq * p.q_batch_stride + h * d;
  const f16* Kg = reinterpret_cast<const f16*>(p.k) + (int64_t)bkv * p.k_batch_stride + h * d;
  f16x8 qf[KS];
  row_frags<KS>(qf, Q + (int64_t)q * p.q_row_stride, q < p.lq, g, d);
  float m = -INFINITY, l = 0.f;
  for (int kb = 0; kb < p.lk; kb += 32) {
    float v[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = kb + perm_row(l15, t);
      f16x8 kf[KS];
      row_frags<KS>(kf, Kg + (int64_t)key * p.k_row_stride, key < p.lk, g, d);
      const f32x4 s = chain<KS>(kf, qf);   // rows = keys kb + 8 g + 4 t + r, column = query l15
#pragma unroll
      for (int r = 0; r < 4; ++r) v[t][r] = (kb + 8 * g + 4 * t + r < p.lk) ? c * s[r] : -INFINITY;
    }
    float mx = fmaxf(fmaxf(fmaxf(v[0][0], v[0][1]), fmaxf(v[0][2], v[0][3])),
                     fmaxf(fmaxf(v[1][0], v[1][1]), fmaxf(v[1][2], v[1][3])));
    mx = group_max(mx);
    const float mn = fmaxf(m, mx);      // finite: every 32-key block holds at least one key < lk
    float add = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) add += __builtin_amdgcn_exp2f(v[t][r] - mn);
    l = l * __builtin_amdgcn_exp2f(m - mn) + add;
    m = mn;
  }
  l = group_sum(l);
  if (g == 0 && q < p.lq) lse[((int64_t)bq * p.heads + h) * p.lq + q] = m + __log2f(l);
}

// the same statistic with the 32-key K blocks staged once per workgroup in LDS and two query tiles per wave (long sequences)
template <int KS, int U>
__global__ __launch_bounds__(256) void attn_lse_lds_kernel(const i2v_attn_params p, const float c, float* __restrict__ lse) {
  constexpr int RS = KS * 32 + 8, QCH = 32 * KS * 4, NQ = (QCH + 255) / 256;
  __shared__ __attribute__((aligned(16))) f16 lds[2 * 32 * RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const int h = blockIdx.y, bq = blockIdx.z, bkv = bq / p.kv_group, d = p.head_dim;
  const int q0 = blockIdx.x * (64 * U) + wave * (16 * U);
  const f16* Q = reinterpret_cast<const f16*>(p.q) + (int64_t)bq * p.q_batch_stride + h * d;
  const f16* Kg = reinterpret_cast<const f16*>(p.k) + (int64_t)bkv * p.k_batch_stride + h * d;
  f16x8 qf[U][KS];
  float m[U], l[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = q0 + 16 * u + l15;
    row_frags<KS>(qf[u], Q + (int64_t)q * p.q_row_stride, q < p.lq, g, d);
    m[u] = -INFINITY;
    l[u] = 0.f;
  }
  const int nit = (p.lk + 31) / 32;
  f16x8 rk[NQ];
  auto fetch = [&](int it) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int t = tid + 256 * i, row = t / (KS * 4), ch = t - row * (KS * 4);
      const bool ok = t < QCH && 32 * it + row < p.lk && 8 * ch < d;
      rk[i] = ok ? ld_global_16B(Kg + (int64_t)(32 * it + row) * p.k_row_stride + 8 * ch) : zero8();
    }
  };
  auto commit = [&](int stage) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int t = tid + 256 * i, row = t / (KS * 4), ch = t - row * (KS * 4);
      if (t < QCH) *reinterpret_cast<f16x8*>(lds + stage * 32 * RS + row * RS + 8 * ch) = rk[i];
    }
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int it = 0; it < nit; ++it) {
    if (it + 1 < nit) fetch(it + 1);
    const f16* sk = lds + (it & 1) * 32 * RS;
    float v[U][2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int r = perm_row(l15, t);
      f16x8 kf[KS];
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) kf[s2] = *reinterpret_cast<const f16x8*>(sk + r * RS + 32 * s2 + 8 * g);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const f32x4 s = chain<KS>(kf, qf[u]);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) v[u][t][r4] = (32 * it + 8 * g + 4 * t + r4 < p.lk) ? c * s[r4] : -INFINITY;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float mx = fmaxf(fmaxf(fmaxf(v[u][0][0], v[u][0][1]), fmaxf(v[u][0][2], v[u][0][3])),
                       fmaxf(fmaxf(v[u][1][0], v[u][1][1]), fmaxf(v[u][1][2], v[u][1][3])));
      mx = group_max(mx);
      const float mn = fmaxf(m[u], mx);
      float add = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) add += __builtin_amdgcn_exp2f(v[u][t][r4] - mn);
      l[u] = l[u] * __builtin_amdgcn_exp2f(m[u] - mn) + add;
      m[u] = mn;
    }
    if (it + 1 < nit) commit((it + 1) & 1);
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = q0 + 16 * u + l15;
    const float lt = group_sum(l[u]);
    if (g == 0 && q < p.lq) lse[((int64_t)bq * p.heads + h) * p.lq + q] = m[u] + __log2f(lt);
  }
}

// ------------------------------------------------------------------------------------------------ dQ
// U = 16-row tiles per wave (1 or 2): the K / V / K^T fragments a key block needs are fetched once and used for both of a
// wave's query tiles.  This form reads its fragments straight from L2 (short sequences); long ones take the LDS-staged form below.
template <int KS, int DT, int U>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const i2v_attn_bwd_params p, const float c) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
  const int h = blockIdx.y, bq = blockIdx.z, bkv = bq / p.kv_group, d = p.head_dim;
  const int q0 = blockIdx.x * (64 * U) + wave * (16 * U);
  const f16* Q = reinterpret_cast<const f16*>(p.q) + (int64_t)bq * p.q_batch_stride + h * d;
  const f16* DO = reinterpret_cast<const f16*>(p.dout) + (int64_t)bq * p.do_batch_stride + h * d;
  const f16* Kg = reinterpret_cast<const f16*>(p.k) + (int64_t)bkv * p.k_batch_stride + h * d;
  const f16* Vg = reinterpret_cast<const f16*>(p.v) + (int64_t)bkv * p.v_batch_stride + h * d;
  const f16* KT = reinterpret_cast<const f16*>(p.kt) + (int64_t)bkv * p.kt_batch_stride + (int64_t)h * d * p.kt_row_stride;
  f16x8 qf[U][KS], dof[U][KS];
  float lse_q[U], del_q[U];
  f32x4 acc[U][DT];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = q0 + 16 * u + l15;
    const bool qok = q < p.lq;
    row_frags<KS>(qf[u], Q + (int64_t)q * p.q_row_stride, qok, g, d);
    row_frags<KS>(dof[u], DO + (int64_t)q * p.do_row_stride, qok, g, d);
    const int64_t stat = ((int64_t)bq * p.heads + h) * p.lq + (qok ? q : 0);
    lse_q[u] = qok ? p.lse[stat] : 0.f;
    del_q[u] = qok ? p.delta[stat] : 0.f;
#pragma unroll
    for (int i = 0; i < DT; ++i) acc[u][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int lk8 = (p.lk + 7) & ~7;     // K^T rows are zero-filled up to the next multiple of 8 keys (i2v_transpose_f16)
  for (int kb = 0; kb < p.lk; kb += 32) {
    float ds[U][2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = kb + perm_row(l15, t);
      f16x8 kf[KS], vf[KS];
      row_frags<KS>(kf, Kg + (int64_t)key * p.k_row_stride, key < p.lk, g, d);
      row_frags<KS>(vf, Vg + (int64_t)key * p.v_row_stride, key < p.lk, g, d);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const f32x4 s = chain<KS>(kf, qf[u]);     // S^T : rows = keys kb + 8 g + 4 t + r, column = query l15
        const f32x4 dp = chain<KS>(vf, dof[u]);   // dP^T
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pr = (kb + 8 * g + 4 * t + r < p.lk) ? __builtin_amdgcn_exp2f(c * s[r] - lse_q[u]) : 0.f;
          ds[u][t][r] = pr * (dp[r] - del_q[u]);
        }
      }
    }
    f16x8 dsb[U];                                  // B operands: keys kb + 8 g .. + 7 of query l15
#pragma unroll
    for (int u = 0; u < U; ++u) dsb[u] = pack8(ds[u][0], ds[u][1]);
    const int kcol = kb + 8 * g;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int row = 16 * i + l15;          // channel of the head
      const f16x8 a = (row < d && kcol < lk8) ? ld_global_16B(KT + (int64_t)row * p.kt_row_stride + kcol) : zero8();
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u][i] = mfma16x16x32(a, dsb[u], acc[u][i]);   // dQ^T: rows = channels, column = query
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = q0 + 16 * u + l15;
    if (q >= p.lq) continue;
    f16* DQ = reinterpret_cast<f16*>(p.dq) + (int64_t)bq * p.dq_batch_stride + (int64_t)q * p.dq_row_stride + h * d;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int dd = 16 * i + 4 * g;
      if (dd >= d) continue;
      f16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (f16)(acc[u][i][r] * p.scale);
      *reinterpret_cast<f16x4*>(DQ + dd) = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------ dK, dV
template <int KS, int DT, int U>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const i2v_attn_bwd_params p, const float c) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, l15 = lane & 15;
  // blockIdx.z = (K / V batch entry, partition of its kv_group query batches: i2v_attn_bwd_params.kv_partitions)
  const int parts = p.kv_partitions > 1 ? p.kv_partitions : 1;
  const int h = blockIdx.y, bkv = blockIdx.z / parts, part = blockIdx.z - bkv * parts, d = p.head_dim;
  const int fpp = p.kv_group / parts;
  const int key0 = blockIdx.x * (64 * U) + wave * (16 * U);
  const f16* Kg = reinterpret_cast<const f16*>(p.k) + (int64_t)bkv * p.k_batch_stride + h * d;
  const f16* Vg = reinterpret_cast<const f16*>(p.v) + (int64_t)bkv * p.v_batch_stride + h * d;
  f16x8 kf[U][KS], vf[U][KS];
  f32x4 dk[U][DT], dv[U][DT];
  bool kok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int key = key0 + 16 * u + l15;
    kok[u] = key < p.lk;
    row_frags<KS>(kf[u], Kg + (int64_t)key * p.k_row_stride, kok[u], g, d);
    row_frags<KS>(vf[u], Vg + (int64_t)key * p.v_row_stride, kok[u], g, d);
#pragma unroll
    for (int i = 0; i < DT; ++i) dk[u][i] = dv[u][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int f = part * fpp; f < (part + 1) * fpp; ++f) {   // this workgroup's share of the batch entries that attend to this K / V
    const int bq = bkv * p.kv_group + f;
    const f16* Q = reinterpret_cast<const f16*>(p.q) + (int64_t)bq * p.q_batch_stride + h * d;
    const f16* DO = reinterpret_cast<const f16*>(p.dout) + (int64_t)bq * p.do_batch_stride + h * d;
    const f16* QT = reinterpret_cast<const f16*>(p.qt) + (int64_t)bq * p.qt_batch_stride + (int64_t)h * d * p.qt_row_stride;
    const f16* DOT = reinterpret_cast<const f16*>(p.doutt) + (int64_t)bq * p.dot_batch_stride + (int64_t)h * d * p.dot_row_stride;
    const float* lse = p.lse + ((int64_t)bq * p.heads + h) * p.lq;
    const float* del = p.delta + ((int64_t)bq * p.heads + h) * p.lq;
    const int lq8 = (p.lq + 7) & ~7;                // Q^T / dO^T rows are zero-filled up to the next multiple of 8 queries
    for (int qb = 0; qb < p.lq; qb += 32) {
      float pv[U][2][4], ds[U][2][4];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int qrow = qb + perm_row(l15, t);
        f16x8 qa[KS], da[KS];
        row_frags<KS>(qa, Q + (int64_t)qrow * p.q_row_stride, qrow < p.lq, g, d);
        row_frags<KS>(da, DO + (int64_t)qrow * p.do_row_stride, qrow < p.lq, g, d);
        float l4[4], d4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qi = qb + 8 * g + 4 * t + r;
          l4[r] = lse[qi < p.lq ? qi : 0];
          d4[r] = del[qi < p.lq ? qi : 0];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const f32x4 s = chain<KS>(qa, kf[u]);     // S : rows = queries qb + 8 g + 4 t + r, column = key l15
          const f32x4 dp = chain<KS>(da, vf[u]);    // dP
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool ok = kok[u] && (qb + 8 * g + 4 * t + r < p.lq);   // (short sequences: the frames of one pixel)
            const float pr = ok ? __builtin_amdgcn_exp2f(c * s[r] - l4[r]) : 0.f;
            pv[u][t][r] = pr;
            ds[u][t][r] = ok ? pr * (dp[r] - d4[r]) : 0.f;
          }
        }
      }
      f16x8 pb[U], dsb[U];                          // B operands: queries qb + 8 g .. + 7, key l15
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pb[u] = pack8(pv[u][0], pv[u][1]);
        dsb[u] = pack8(ds[u][0], ds[u][1]);
      }
      const int qcol = qb + 8 * g;
#pragma unroll
      for (int i = 0; i < DT; ++i) {
        const int row = 16 * i + l15;
        const bool in = row < d && qcol < lq8;
        const f16x8 a1 = in ? ld_global_16B(DOT + (int64_t)row * p.dot_row_stride + qcol) : zero8();
        const f16x8 a2 = in ? ld_global_16B(QT + (int64_t)row * p.qt_row_stride + qcol) : zero8();
#pragma unroll
        for (int u = 0; u < U; ++u) {
          dv[u][i] = mfma16x16x32(a1, pb[u], dv[u][i]);    // dV^T : rows = channels, column = key l15
          dk[u][i] = mfma16x16x32(a2, dsb[u], dk[u][i]);   // dK^T
        }
      }
    }
  }
  if (parts > 1) {   // fp32 partials [2][parts][batch_kv * lk][heads * d]; dkv_sum_kernel adds them in a fixed order
    const int64_t rows_kv = (int64_t)(p.batch_q / p.kv_group) * p.lk, cc = (int64_t)p.heads * d;
    float* wk = p.dkv_partial + ((int64_t)part * rows_kv) * cc;
    float* wv = wk + (int64_t)parts * rows_kv * cc;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!kok[u]) continue;
      const int64_t row = (int64_t)bkv * p.lk + key0 + 16 * u + l15;
#pragma unroll
      for (int i = 0; i < DT; ++i) {
        const int dd = 16 * i + 4 * g;
        if (dd >= d) continue;
        *reinterpret_cast<f32x4*>(wk + row * cc + h * d + dd) = dk[u][i] * p.scale;
        *reinterpret_cast<f32x4*>(wv + row * cc + h * d + dd) = dv[u][i];
      }
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!kok[u]) continue;
    const int key = key0 + 16 * u + l15;
    f16* DK = reinterpret_cast<f16*>(p.dk) + (int64_t)bkv * p.dk_batch_stride + (int64_t)key * p.dk_row_stride + h * d;
    f16* DV = reinterpret_cast<f16*>(p.dv) + (int64_t)bkv * p.dv_batch_stride + (int64_t)key * p.dv_row_stride + h * d;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int dd = 16 * i + 4 * g;
      if (dd >= d) continue;
      f16x4 ok4, ov4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ok4[r] = (f16)(dk[u][i][r] * p.scale);
        ov4[r] = (f16)dv[u][i][r];
      }
      *reinterpret_cast<f16x4*>(DK + dd) = ok4;
      *reinterpret_cast<f16x4*>(DV + dd) = ov4;
    }
  }
}

// ------------------------------------------------------------------------------------------------ dK, dV, LDS-staged
// The same sweep with the query-side operands of a 32-query block (Q, dO rows; Q^T, dO^T rows; lse, delta) staged ONCE per
// workgroup in LDS (two stages, the next block's chunks in flight in registers under the current block's MFMAs) instead of
// fetched from L2 by each of the four waves: a quarter of the L2 traffic, and no load round trip inside an iteration.
// QB: queries per staged block (one barrier per block): 32, or 64 = two 32-query contraction steps per barrier
template <int KS, int DT, int U, int QB = 32>
__global__ __launch_bounds__(256) void attn_bwd_dkv_lds_kernel(const i2v_attn_bwd_params p, const float c) {
  constexpr int RS = KS * 32 + 8;                    // LDS row stride of the Q / dO tiles (halfs)
  constexpr int TS = QB + 8;                         // ... of the Q^T / dO^T tiles
  constexpr int QCH = QB * KS * 4;                   // 16-byte chunks of a [QB][KS * 32] tile
  constexpr int TCH = DT * 16 * (QB / 8);            // ... of a [DT * 16][QB] tile
  constexpr int NQ = (QCH + 255) / 256, NT = (TCH + 255) / 256;
  constexpr int STAGE_H = 2 * QB * RS + 2 * DT * 16 * TS;     // halfs per stage (+ 2 QB floats of lse / delta)
  __shared__ __attribute__((aligned(16))) f16 lds[2 * (STAGE_H + 4 * QB)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  // blockIdx.z = (K / V batch entry, partition of its kv_group query batches)
  const int parts = p.kv_partitions > 1 ? p.kv_partitions : 1;
  const int h = blockIdx.y, bkv = blockIdx.z / parts, part = blockIdx.z - bkv * parts, d = p.head_dim;
  const int fpp = p.kv_group / parts, f0 = part * fpp;          // this workgroup's query batches: f0 .. f0 + fpp - 1
  const int key0 = blockIdx.x * (64 * U) + wave * (16 * U);
  const f16* Kg = reinterpret_cast<const f16*>(p.k) + (int64_t)bkv * p.k_batch_stride + h * d;
  const f16* Vg = reinterpret_cast<const f16*>(p.v) + (int64_t)bkv * p.v_batch_stride + h * d;
  f16x8 kf[U][KS], vf[U][KS];
  f32x4 dk[U][DT], dv[U][DT];
  bool kok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int key = key0 + 16 * u + l15;
    kok[u] = key < p.lk;
    row_frags<KS>(kf[u], Kg + (int64_t)key * p.k_row_stride, kok[u], g, d);
    row_frags<KS>(vf[u], Vg + (int64_t)key * p.v_row_stride, kok[u], g, d);
#pragma unroll
    for (int i = 0; i < DT; ++i) dk[u][i] = dv[u][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int nqb = (p.lq + QB - 1) / QB, nit = fpp * nqb;
  const int lq8 = (p.lq + 7) & ~7;
  f16x8 rq[NQ], rdo[NQ], rqt[NT], rdot[NT];
  float rl = 0.f, rd = 0.f;
  auto fetch = [&](int it) {
    const int f = it / nqb, qb = (it - f * nqb) * QB;
    const int bq = bkv * p.kv_group + f0 + f;
    const f16* Q = reinterpret_cast<const f16*>(p.q) + (int64_t)bq * p.q_batch_stride + h * d;
    const f16* DO = reinterpret_cast<const f16*>(p.dout) + (int64_t)bq * p.do_batch_stride + h * d;
    const f16* QT = reinterpret_cast<const f16*>(p.qt) + (int64_t)bq * p.qt_batch_stride + (int64_t)h * d * p.qt_row_stride;
    const f16* DOT = reinterpret_cast<const f16*>(p.doutt) + (int64_t)bq * p.dot_batch_stride + (int64_t)h * d * p.dot_row_stride;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int t = tid + 256 * i, row = t / (KS * 4), ch = t - row * (KS * 4);
      const bool ok = t < QCH && qb + row < p.lq && 8 * ch < d;
      rq[i] = ok ? ld_global_16B(Q + (int64_t)(qb + row) * p.q_row_stride + 8 * ch) : zero8();
      rdo[i] = ok ? ld_global_16B(DO + (int64_t)(qb + row) * p.do_row_stride + 8 * ch) : zero8();
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int t = tid + 256 * i, row = t / (QB / 8), ch = t - row * (QB / 8);
      const bool ok = t < TCH && row < d && qb + 8 * ch < lq8;
      rqt[i] = ok ? ld_global_16B(QT + (int64_t)row * p.qt_row_stride + qb + 8 * ch) : zero8();
      rdot[i] = ok ? ld_global_16B(DOT + (int64_t)row * p.dot_row_stride + qb + 8 * ch) : zero8();
    }
    if (tid < QB) {
      const int64_t st = ((int64_t)bq * p.heads + h) * p.lq + min(qb + tid, p.lq - 1);
      rl = p.lse[st];
      rd = p.delta[st];
    }
  };
  auto commit = [&](int stage) {
    f16* sq = lds + stage * (STAGE_H + 4 * QB);
    f16* sdo = sq + QB * RS;
    f16* sqt = sdo + QB * RS;
    f16* sdot = sqt + DT * 16 * TS;
    float* sst = reinterpret_cast<float*>(sdot + DT * 16 * TS);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int t = tid + 256 * i, row = t / (KS * 4), ch = t - row * (KS * 4);
      if (t < QCH) {
        *reinterpret_cast<f16x8*>(sq + row * RS + 8 * ch) = rq[i];
        *reinterpret_cast<f16x8*>(sdo + row * RS + 8 * ch) = rdo[i];
      }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int t = tid + 256 * i, row = t / (QB / 8), ch = t - row * (QB / 8);
      if (t < TCH) {
        *reinterpret_cast<f16x8*>(sqt + row * TS + 8 * ch) = rqt[i];
        *reinterpret_cast<f16x8*>(sdot + row * TS + 8 * ch) = rdot[i];
      }
    }
    if (tid < QB) {
      sst[tid] = rl;
      sst[QB + tid] = rd;
    }
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int it = 0; it < nit; ++it) {
    if (it + 1 < nit) fetch(it + 1);
    const f16* sq0 = lds + (it & 1) * (STAGE_H + 4 * QB);
    const f16* sdo0 = sq0 + QB * RS;
    const f16* sqt0 = sdo0 + QB * RS;
    const f16* sdot0 = sqt0 + DT * 16 * TS;
    const float* sst0 = reinterpret_cast<const float*>(sdot0 + DT * 16 * TS);
#pragma unroll
    for (int sb = 0; sb < QB / 32; ++sb) {   // 32-query contraction steps of the staged block
    const int qb = (it % nqb) * QB + 32 * sb;
    const f16* sq = sq0 + 32 * sb * RS;
    const f16* sdo = sdo0 + 32 * sb * RS;
    const f16* sqt = sqt0 + 32 * sb;
    const f16* sdot = sdot0 + 32 * sb;
    const float* sst = sst0 + 32 * sb;
    float pv[U][2][4], ds[U][2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int r = perm_row(l15, t);
      f16x8 qa[KS], da[KS];
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) {
        qa[s2] = *reinterpret_cast<const f16x8*>(sq + r * RS + 32 * s2 + 8 * g);
        da[s2] = *reinterpret_cast<const f16x8*>(sdo + r * RS + 32 * s2 + 8 * g);
      }
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(sst + 8 * g + 4 * t);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(sst + QB + 8 * g + 4 * t);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const f32x4 s = chain<KS>(qa, kf[u]);
        const f32x4 dp = chain<KS>(da, vf[u]);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const bool ok = kok[u] && (qb + 8 * g + 4 * t + r4 < p.lq);
          const float pr = ok ? __builtin_amdgcn_exp2f(c * s[r4] - l4[r4]) : 0.f;
          pv[u][t][r4] = pr;
          ds[u][t][r4] = ok ? pr * (dp[r4] - d4[r4]) : 0.f;
        }
      }
    }
    f16x8 pb[U], dsb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      pb[u] = pack8(pv[u][0], pv[u][1]);
      dsb[u] = pack8(ds[u][0], ds[u][1]);
    }
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const f16x8 a1 = *reinterpret_cast<const f16x8*>(sdot + (16 * i + l15) * TS + 8 * g);
      const f16x8 a2 = *reinterpret_cast<const f16x8*>(sqt + (16 * i + l15) * TS + 8 * g);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        dv[u][i] = mfma16x16x32(a1, pb[u], dv[u][i]);
        dk[u][i] = mfma16x16x32(a2, dsb[u], dk[u][i]);
      }
    }
    }   // sb
    if (it + 1 < nit) commit((it + 1) & 1);     // the other stage was last read in iteration it - 1 (closed by its barrier)
    __syncthreads();
  }
  if (parts > 1) {   // fp32 partials [2][parts][batch_kv * lk][heads * d]; dkv_sum_kernel adds them in a fixed order
    const int64_t rows_kv = (int64_t)(p.batch_q / p.kv_group) * p.lk, cc = (int64_t)p.heads * d;
    float* wk = p.dkv_partial + ((int64_t)part * rows_kv) * cc;
    float* wv = wk + (int64_t)parts * rows_kv * cc;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!kok[u]) continue;
      const int64_t row = (int64_t)bkv * p.lk + key0 + 16 * u + l15;
#pragma unroll
      for (int i = 0; i < DT; ++i) {
        const int dd = 16 * i + 4 * g;
        if (dd >= d) continue;
        *reinterpret_cast<f32x4*>(wk + row * cc + h * d + dd) = dk[u][i] * p.scale;
        *reinterpret_cast<f32x4*>(wv + row * cc + h * d + dd) = dv[u][i];
      }
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!kok[u]) continue;
    const int key = key0 + 16 * u + l15;
    f16* DK = reinterpret_cast<f16*>(p.dk) + (int64_t)bkv * p.dk_batch_stride + (int64_t)key * p.dk_row_stride + h * d;
    f16* DV = reinterpret_cast<f16*>(p.dv) + (int64_t)bkv * p.dv_batch_stride + (int64_t)key * p.dv_row_stride + h * d;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int dd = 16 * i + 4 * g;
      if (dd >= d) continue;
      f16x4 ok4, ov4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ok4[r] = (f16)(dk[u][i][r] * p.scale);
        ov4[r] = (f16)dv[u][i][r];
      }
      *reinterpret_cast<f16x4*>(DK + dd) = ok4;
      *reinterpret_cast<f16x4*>(DV + dd) = ov4;
    }
  }
}

// dk / dv (fp16) = sum over the partitions of the fp32 partials, partition 0 first
__global__ __launch_bounds__(256) void dkv_sum_kernel(const i2v_attn_bwd_params p) {
  const int parts = p.kv_partitions, d = p.head_dim;
  const int64_t rows_kv = (int64_t)(p.batch_q / p.kv_group) * p.lk, cc = (int64_t)p.heads * d, n4 = rows_kv * (cc / 4);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / (cc / 4);
    const int c4 = (int)(i - row * (cc / 4)) * 4;
    const int b = (int)(row / p.lk), key = (int)(row - (int64_t)b * p.lk);
    const float* wk = p.dkv_partial + row * cc + c4;
    const float* wv = wk + (int64_t)parts * rows_kv * cc;
    f32x4 sk = *reinterpret_cast<const f32x4*>(wk), sv = *reinterpret_cast<const f32x4*>(wv);
    for (int q = 1; q < parts; ++q) {
      sk += *reinterpret_cast<const f32x4*>(wk + (int64_t)q * rows_kv * cc);
      sv += *reinterpret_cast<const f32x4*>(wv + (int64_t)q * rows_kv * cc);
    }
    f16x4 ok4, ov4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ok4[r] = (f16)sk[r];
      ov4[r] = (f16)sv[r];
    }
    *reinterpret_cast<f16x4*>(reinterpret_cast<f16*>(p.dk) + (int64_t)b * p.dk_batch_stride + (int64_t)key * p.dk_row_stride + c4) = ok4;
    *reinterpret_cast<f16x4*>(reinterpret_cast<f16*>(p.dv) + (int64_t)b * p.dv_batch_stride + (int64_t)key * p.dv_row_stride + c4) = ov4;
  }
}

// ------------------------------------------------------------------------------------------------ dQ, LDS-staged
// The dQ sweep with the key-side operands of a 32-key block (K, V rows; K^T rows) staged once per workgroup (as above).
template <int KS, int DT, int U>
__global__ __launch_bounds__(256) void attn_bwd_dq_lds_kernel(const i2v_attn_bwd_params p, const float c) {
  constexpr int RS = KS * 32 + 8, TS = 32 + 8;
  constexpr int QCH = 32 * KS * 4, TCH = DT * 16 * 4;
  constexpr int NQ = (QCH + 255) / 256, NT = (TCH + 255) / 256;
  constexpr int STAGE_H = 2 * 32 * RS + DT * 16 * TS;
  __shared__ __attribute__((aligned(16))) f16 lds[2 * STAGE_H];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const int h = blockIdx.y, bq = blockIdx.z, bkv = bq / p.kv_group, d = p.head_dim;
  const int q0 = blockIdx.x * (64 * U) + wave * (16 * U);
  const f16* Q = reinterpret_cast<const f16*>(p.q) + (int64_t)bq * p.q_batch_stride + h * d;
  const f16* DO = reinterpret_cast<const f16*>(p.dout) + (int64_t)bq * p.do_batch_stride + h * d;
  const f16* Kg = reinterpret_cast<const f16*>(p.k) + (int64_t)bkv * p.k_batch_stride + h * d;
  const f16* Vg = reinterpret_cast<const f16*>(p.v) + (int64_t)bkv * p.v_batch_stride + h * d;
  const f16* KT = reinterpret_cast<const f16*>(p.kt) + (int64_t)bkv * p.kt_batch_stride + (int64_t)h * d * p.kt_row_stride;
  f16x8 qf[U][KS], dof[U][KS];
  float lse_q[U], del_q[U];
  f32x4 acc[U][DT];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = q0 + 16 * u + l15;
    const bool qok = q < p.lq;
    row_frags<KS>(qf[u], Q + (int64_t)q * p.q_row_stride, qok, g, d);
    row_frags<KS>(dof[u], DO + (int64_t)q * p.do_row_stride, qok, g, d);
    const int64_t stat = ((int64_t)bq * p.heads + h) * p.lq + (qok ? q : 0);
    lse_q[u] = qok ? p.lse[stat] : 0.f;
    del_q[u] = qok ? p.delta[stat] : 0.f;
#pragma unroll
    for (int i = 0; i < DT; ++i) acc[u][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int lk8 = (p.lk + 7) & ~7, nit = (p.lk + 31) / 32;
  f16x8 rk[NQ], rv[NQ], rkt[NT];
  auto fetch = [&](int it) {
    const int kb = 32 * it;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int t = tid + 256 * i, row = t / (KS * 4), ch = t - row * (KS * 4);
      const bool ok = t < QCH && kb + row < p.lk && 8 * ch < d;
      rk[i] = ok ? ld_global_16B(Kg + (int64_t)(kb + row) * p.k_row_stride + 8 * ch) : zero8();
      rv[i] = ok ? ld_global_16B(Vg + (int64_t)(kb + row) * p.v_row_stride + 8 * ch) : zero8();
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int t = tid + 256 * i, row = t >> 2, ch = t & 3;
      const bool ok = t < TCH && row < d && kb + 8 * ch < lk8;
      rkt[i] = ok ? ld_global_16B(KT + (int64_t)row * p.kt_row_stride + kb + 8 * ch) : zero8();
    }
  };
  auto commit = [&](int stage) {
    f16* sk = lds + stage * STAGE_H;
    f16* sv = sk + 32 * RS;
    f16* skt = sv + 32 * RS;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int t = tid + 256 * i, row = t / (KS * 4), ch = t - row * (KS * 4);
      if (t < QCH) {
        *reinterpret_cast<f16x8*>(sk + row * RS + 8 * ch) = rk[i];
        *reinterpret_cast<f16x8*>(sv + row * RS + 8 * ch) = rv[i];
      }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int t = tid + 256 * i, row = t >> 2, ch = t & 3;
      if (t < TCH) *reinterpret_cast<f16x8*>(skt + row * TS + 8 * ch) = rkt[i];
    }
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int it = 0; it < nit; ++it) {
    if (it + 1 < nit) fetch(it + 1);
    const int kb = 32 * it;
    const f16* sk = lds + (it & 1) * STAGE_H;
    const f16* sv = sk + 32 * RS;
    const f16* skt = sv + 32 * RS;
    float ds[U][2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int r = perm_row(l15, t);
      f16x8 kf[KS], vf[KS];
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) {
        kf[s2] = *reinterpret_cast<const f16x8*>(sk + r * RS + 32 * s2 + 8 * g);
        vf[s2] = *reinterpret_cast<const f16x8*>(sv + r * RS + 32 * s2 + 8 * g);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const f32x4 s = chain<KS>(kf, qf[u]);
        const f32x4 dp = chain<KS>(vf, dof[u]);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const float pr = (kb + 8 * g + 4 * t + r4 < p.lk) ? __builtin_amdgcn_exp2f(c * s[r4] - lse_q[u]) : 0.f;
          ds[u][t][r4] = pr * (dp[r4] - del_q[u]);
        }
      }
    }
    f16x8 dsb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) dsb[u] = pack8(ds[u][0], ds[u][1]);
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const f16x8 a = *reinterpret_cast<const f16x8*>(skt + (16 * i + l15) * TS + 8 * g);
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u][i] = mfma16x16x32(a, dsb[u], acc[u][i]);
    }
    if (it + 1 < nit) commit((it + 1) & 1);
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = q0 + 16 * u + l15;
    if (q >= p.lq) continue;
    f16* DQ = reinterpret_cast<f16*>(p.dq) + (int64_t)bq * p.dq_batch_stride + (int64_t)q * p.dq_row_stride + h * d;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int dd = 16 * i + 4 * g;
      if (dd >= d) continue;
      f16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (f16)(acc[u][i][r] * p.scale);
      *reinterpret_cast<f16x4*>(DQ + dd) = o;
    }
  }
}

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

// tests/attn_bwd_reference.py forms() mirrors these choices (and i2v_attention_lse_f32's, the (KS, DT) classes): it must follow them
template <int KS, int DT>
int launch_bwd(const i2v_attn_bwd_params& p, hipStream_t s) {
  const float c = p.scale * LOG2E;
  // two 16-row tiles per wave where the sequence is long enough to still fill the chip (halves the fragment loads per FLOP)
  const bool two_q = p.lq >= 512 && DT <= 6, two_k = p.lk >= 512 && DT <= 6;
  const dim3 gq((unsigned)i2v_cdiv(p.lq, two_q ? 128 : 64), p.heads, p.batch_q);
  static const int lds_off_q = getenv("I2V_ATTN_BWD_LDS") ? (atoi(getenv("I2V_ATTN_BWD_LDS")) == 0) : 0;
  if (two_q && !lds_off_q && p.lk >= 64) hipLaunchKernelGGL((attn_bwd_dq_lds_kernel<KS, DT, 2>), gq, dim3(256), 0, s, p, c);
  else if (two_q) hipLaunchKernelGGL((attn_bwd_dq_kernel<KS, DT, 2>), gq, dim3(256), 0, s, p, c);
  else hipLaunchKernelGGL((attn_bwd_dq_kernel<KS, DT, 1>), gq, dim3(256), 0, s, p, c);
  int rc = i2v_check_launch("i2v_attention_bwd_f16(dQ)");
  if (rc < 0) return rc;
  if (p.dk != nullptr) {
    static const int lds_off = getenv("I2V_ATTN_BWD_LDS") ? (atoi(getenv("I2V_ATTN_BWD_LDS")) == 0) : 0;
    const int parts = p.kv_partitions > 1 ? p.kv_partitions : 1;   // (every form of the sweep deals the group out)
    const dim3 gk((unsigned)i2v_cdiv(p.lk, two_k ? 128 : 64), p.heads, (p.batch_q / p.kv_group) * parts);
    // 64 staged queries per barrier (two 32-query contraction steps): the 32-query loop has 28 MFMAs per wave between barriers.
    // Same box, 16 frames x 4096 tokens, d = 40 (tools/attn_bwd_probe.py): self-attention backward 2.95 -> 2.73 ms per call, the
    // cross-frame form (one K / V for 16 frames: 256 workgroups walking 1024 blocks each) 3.72 -> 3.16.  I2V_ATTN_BWD_QB=32: off.
    static const int qb64 = getenv("I2V_ATTN_BWD_QB") ? (atoi(getenv("I2V_ATTN_BWD_QB")) == 64) : 1;
    bool done = false;
    if constexpr (DT <= 6) {   // (two_k implies it; the 64-query stages of wider heads would not fit LDS)
      if (two_k && !lds_off && p.lq >= 128 && qb64) {
        hipLaunchKernelGGL((attn_bwd_dkv_lds_kernel<KS, DT, 2, 64>), gk, dim3(256), 0, s, p, c);
        done = true;
      }
    }
    if (done) {
    } else if (two_k && !lds_off && p.lq >= 64) hipLaunchKernelGGL((attn_bwd_dkv_lds_kernel<KS, DT, 2>), gk, dim3(256), 0, s, p, c);
    else if (two_k) hipLaunchKernelGGL((attn_bwd_dkv_kernel<KS, DT, 2>), gk, dim3(256), 0, s, p, c);
    else hipLaunchKernelGGL((attn_bwd_dkv_kernel<KS, DT, 1>), gk, dim3(256), 0, s, p, c);
    if (parts > 1) {
      const int64_t n4 = (int64_t)(p.batch_q / p.kv_group) * p.lk * ((int64_t)p.heads * p.head_dim / 4);
      hipLaunchKernelGGL(dkv_sum_kernel, dim3(ew_grid(n4)), dim3(256), 0, s, p);
    }
    rc = i2v_check_launch("i2v_attention_bwd_f16(dK, dV)");
  }
  return rc;
}

}  // namespace

extern "C" int i2v_attention_lse_f32(const i2v_attn_params* pp, float* lse, i2v_stream_t stream) {
  I2V_CHECK_ARG(pp && lse, "i2v_attention_lse_f32: null argument");
  const i2v_attn_params& p = *pp;
  I2V_CHECK_ARG(p.q && p.k, "i2v_attention_lse_f32: null q / k");
  I2V_CHECK_ARG(p.batch_q > 0 && p.kv_group > 0 && p.batch_q % p.kv_group == 0 && p.heads > 0 && p.lq > 0 && p.lk > 0,
                "i2v_attention_lse_f32: bad sizes");
  I2V_CHECK_ARG(p.head_dim > 0 && p.head_dim % 8 == 0 && p.head_dim <= 160, "i2v_attention_lse_f32: head_dim (%d) must be a "
                "multiple of 8 and <= 160", p.head_dim);
  I2V_CHECK_ARG(p.q_row_stride % 8 == 0 && p.k_row_stride % 8 == 0 && p.q_batch_stride % 8 == 0 && p.k_batch_stride % 8 == 0 &&
                    i2v_al16(p.q) && i2v_al16(p.k), "i2v_attention_lse_f32: q / k strides must be multiples of 8 elements, 16-byte aligned");
  I2V_CHECK_ARG(p.heads <= 65535 && p.batch_q <= 65535, "i2v_attention_lse_f32: heads / batch_q exceed the grid limits");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float c = p.scale * LOG2E;
  const int ks = (p.head_dim + 31) / 32;
  const dim3 block(256);
  static const int lds_off = getenv("I2V_ATTN_BWD_LDS") ? (atoi(getenv("I2V_ATTN_BWD_LDS")) == 0) : 0;
  if (!lds_off && p.lq >= 512 && p.lk >= 64 && ks <= 3) {   // long sequences: K staged in LDS, two query tiles per wave
    const dim3 grid2((unsigned)i2v_cdiv(p.lq, 128), p.heads, p.batch_q);
    if (ks == 1) hipLaunchKernelGGL((attn_lse_lds_kernel<1, 2>), grid2, block, 0, s, p, c, lse);
    else if (ks == 2) hipLaunchKernelGGL((attn_lse_lds_kernel<2, 2>), grid2, block, 0, s, p, c, lse);
    else hipLaunchKernelGGL((attn_lse_lds_kernel<3, 2>), grid2, block, 0, s, p, c, lse);
    return i2v_check_launch("i2v_attention_lse_f32");
  }
  const dim3 grid((unsigned)i2v_cdiv(p.lq, 64), p.heads, p.batch_q);
  if (ks == 1) hipLaunchKernelGGL((attn_lse_kernel<1>), grid, block, 0, s, p, c, lse);
  else if (ks == 2) hipLaunchKernelGGL((attn_lse_kernel<2>), grid, block, 0, s, p, c, lse);
  else if (ks == 3) hipLaunchKernelGGL((attn_lse_kernel<3>), grid, block, 0, s, p, c, lse);
  else if (ks == 4) hipLaunchKernelGGL((attn_lse_kernel<4>), grid, block, 0, s, p, c, lse);
  else hipLaunchKernelGGL((attn_lse_kernel<5>), grid, block, 0, s, p, c, lse);
  return i2v_check_launch("i2v_attention_lse_f32");
}

extern "C" int i2v_attention_bwd_f16(const i2v_attn_bwd_params* pp, i2v_stream_t stream) {
  I2V_CHECK_ARG(pp != nullptr, "i2v_attention_bwd_f16: null params");
  const i2v_attn_bwd_params& p = *pp;
  I2V_CHECK_ARG(p.q && p.k && p.v && p.kt && p.dout && p.lse && p.delta && p.dq, "i2v_attention_bwd_f16: null pointer");
  I2V_CHECK_ARG(p.batch_q > 0 && p.kv_group > 0 && p.batch_q % p.kv_group == 0 && p.heads > 0 && p.lq > 0 && p.lk > 0,
                "i2v_attention_bwd_f16: bad sizes");
  I2V_CHECK_ARG(p.head_dim > 0 && p.head_dim % 8 == 0 && p.head_dim <= 160, "i2v_attention_bwd_f16: head_dim (%d) must be a "
                "multiple of 8 and <= 160", p.head_dim);
  I2V_CHECK_ARG(p.heads <= 65535 && p.batch_q <= 65535, "i2v_attention_bwd_f16: heads / batch_q exceed the grid limits");
  const int lk8 = (p.lk + 7) & ~7;
  I2V_CHECK_ARG(p.kt_row_stride >= lk8 && p.kt_row_stride % 8 == 0, "i2v_attention_bwd_f16: kt_row_stride must be a multiple "
                "of 8 and >= lk rounded up to 8 (zero-filled: i2v_transpose_f16)");
  const int64_t strides[] = {p.q_row_stride, p.q_batch_stride, p.k_row_stride, p.k_batch_stride, p.v_row_stride,
                             p.v_batch_stride, p.kt_batch_stride, p.do_row_stride, p.do_batch_stride, p.dq_row_stride,
                             p.dq_batch_stride};
  for (int64_t st : strides) I2V_CHECK_ARG(st % 8 == 0, "i2v_attention_bwd_f16: strides must be multiples of 8 elements");
  I2V_CHECK_ARG(i2v_al16(p.q) && i2v_al16(p.k) && i2v_al16(p.v) && i2v_al16(p.kt) && i2v_al16(p.dout) && i2v_al16(p.dq) && i2v_al16(p.lse) && i2v_al16(p.delta),
                "i2v_attention_bwd_f16: pointers must be 16-byte aligned");
  I2V_CHECK_ARG(p.kv_partitions >= 0, "i2v_attention_bwd_f16: kv_partitions must be >= 0");
  if (p.dk != nullptr && p.kv_partitions > 1)
    I2V_CHECK_ARG(p.dkv_partial != nullptr && i2v_al16(p.dkv_partial) && p.kv_group % p.kv_partitions == 0 &&
                      (p.heads * p.head_dim) % 4 == 0,
                  "i2v_attention_bwd_f16: kv_partitions (%d) needs the dkv_partial scratch and must divide kv_group (%d)",
                  p.kv_partitions, p.kv_group);
  if (p.dk != nullptr) {
    I2V_CHECK_ARG(p.dv && p.qt && p.doutt, "i2v_attention_bwd_f16: dk needs dv, qt and doutt");
    const int lq8 = (p.lq + 7) & ~7;
    I2V_CHECK_ARG(p.qt_row_stride >= lq8 && p.qt_row_stride % 8 == 0 && p.dot_row_stride >= lq8 && p.dot_row_stride % 8 == 0 &&
                      p.qt_batch_stride % 8 == 0 && p.dot_batch_stride % 8 == 0 && p.dk_row_stride % 8 == 0 &&
                      p.dk_batch_stride % 8 == 0 && p.dv_row_stride % 8 == 0 && p.dv_batch_stride % 8 == 0 && i2v_al16(p.qt) &&
                      i2v_al16(p.doutt) && i2v_al16(p.dk) && i2v_al16(p.dv),
                  "i2v_attention_bwd_f16: Q^T / dO^T / dK / dV strides and alignment");
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int d = p.head_dim;
  if (d <= 32) return launch_bwd<1, 2>(p, s);
  if (d <= 48) return launch_bwd<2, 3>(p, s);
  if (d <= 64) return launch_bwd<2, 4>(p, s);
  if (d <= 80) return launch_bwd<3, 5>(p, s);
  if (d <= 96) return launch_bwd<3, 6>(p, s);
  if (d <= 128) return launch_bwd<4, 8>(p, s);
  return launch_bwd<5, 10>(p, s);
}

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
