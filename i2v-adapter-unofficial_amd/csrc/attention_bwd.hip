// Flash-attention backward of the adapter training step on MFMA (i2v_attention_bwd_f16) and the log-sum-exp of a forward attention
// (i2v_attention_lse_f32: the inference kernel does not keep it), recomputing P from Q, K and that log-sum-exp (never the L x L scores):
//       dQ   kernel: a wave owns 16 queries, sweeps the keys:   S^T = K Q^T, dP^T = V dO^T (key on the MFMA row, so the
//                    accumulators ARE the B operand of)           dQ^T += K^T dS^T
//       dK/dV kernel: a wave owns 16 keys, sweeps the queries of every batch entry that shares them (kv_group: the F
//                    frames of a clip read the frame-0 K / V, i2v:483-492 -- dK0 / dV0 are summed over the frames here,
//                    in registers):                              S = Q K^T, dP = dO V^T (query on the MFMA row), then
//                                                                 dV^T += dO^T P,  dK^T += Q^T dS
//     two sweeps (7 products instead of 5) buy: no atomics, no cross-workgroup sum, run-to-run identical gradients.
//     The K^T / Q^T / dO^T operands are channel-major copies ([batch][channel][token], the V^T layout of the forward)
//     made by i2v_transpose_f16 (backward.hip).
// Which kernel runs a problem is decided in ONE place, dispatch() below, over ONE launch table; the launches and the host queries
// (i2v_attention_bwd_route, i2v_attention_bwd_last_route, i2v_attn_bwd_kernel_exists) walk both.
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

using Route = struct i2v_attn_bwd_route;   // (include/i2v_hip.h)

// ---- THE launch table: every instantiation the library holds.  The launches (i2v_attention_bwd_f16, i2v_attention_lse_f32) and the
// existence query (i2v_attn_bwd_kernel_exists) both walk this array; a class or a form added here is launchable and visible at once.
struct Entry {
  int kind, ks, dt, form;   // I2V_ATTN_BWD_KIND_*, the head-dim class (dt 0: the log-sum-exp kernels have none), the form of that kind
  void (*sweep)(const i2v_attn_bwd_params& p, float c, dim3 grid, hipStream_t s);           // kinds DQ, DKV
  void (*lse)(const i2v_attn_params& p, float c, float* lse, dim3 grid, hipStream_t s);     // kind LSE
};
#define SWEEP(KIND, KS, DT, FORM, ...)                                                                           \
  {I2V_ATTN_BWD_KIND_##KIND, KS, DT, I2V_ATTN_BWD_##FORM,                                                         \
   [](const i2v_attn_bwd_params& p, float c, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((__VA_ARGS__), grid, dim3(256), 0, s, p, c); }, \
   nullptr}
#define LSE(KS, FORM, ...)                                                          \
  {I2V_ATTN_BWD_KIND_LSE, KS, 0, FORM, nullptr, [](const i2v_attn_params& p, float c, float* lse, dim3 grid, hipStream_t s) { \
     hipLaunchKernelGGL((__VA_ARGS__), grid, dim3(256), 0, s, p, c, lse);           \
   }}
#define ONE_TILE(KS, DT) SWEEP(DQ, KS, DT, DQ1, attn_bwd_dq_kernel<KS, DT, 1>), SWEEP(DKV, KS, DT, DKV1, attn_bwd_dkv_kernel<KS, DT, 1>)
#define TWO_TILE(KS, DT)                                                                                              \
  SWEEP(DQ, KS, DT, DQ2, attn_bwd_dq_kernel<KS, DT, 2>), SWEEP(DQ, KS, DT, DQ2_LDS, attn_bwd_dq_lds_kernel<KS, DT, 2>), \
  SWEEP(DKV, KS, DT, DKV2, attn_bwd_dkv_kernel<KS, DT, 2>), SWEEP(DKV, KS, DT, DKV2_LDS32, attn_bwd_dkv_lds_kernel<KS, DT, 2, 32>), \
  SWEEP(DKV, KS, DT, DKV2_LDS64, attn_bwd_dkv_lds_kernel<KS, DT, 2, 64>)
#define LSE_PLAIN(KS) LSE(KS, I2V_ATTN_LSE, attn_lse_kernel<KS>)
#define LSE_STAGED(KS) LSE(KS, I2V_ATTN_LSE_LDS, attn_lse_lds_kernel<KS, 2>)
// head-dim classes <KS 32-channel contraction steps, DT 16-channel output tiles> in ascending order: a head_dim takes the first
// class whose 16 DT channels hold it.  Two 16-row tiles per wave exist up to DT 6 (wider heads: the accumulators of two tiles and
// the 64-query stages do not fit), the LDS-staged log-sum-exp up to KS 3.
const Entry TABLE[] = {ONE_TILE(1, 2), ONE_TILE(2, 3), ONE_TILE(2, 4), ONE_TILE(3, 5), ONE_TILE(3, 6), ONE_TILE(4, 8), ONE_TILE(5, 10),
                       TWO_TILE(1, 2), TWO_TILE(2, 3), TWO_TILE(2, 4), TWO_TILE(3, 5), TWO_TILE(3, 6),
                       LSE_PLAIN(1),   LSE_PLAIN(2),   LSE_PLAIN(3),   LSE_PLAIN(4),   LSE_PLAIN(5),
                       LSE_STAGED(1),  LSE_STAGED(2),  LSE_STAGED(3)};
#undef SWEEP
#undef LSE
#undef ONE_TILE
#undef TWO_TILE
#undef LSE_PLAIN
#undef LSE_STAGED
constexpr int MAX_HEAD_DIM = 160, TWO_TILE_MAX_DT = 6, LSE_LDS_MAX_KS = 3;

const Entry* find_entry(int kind, int ks, int dt, int form) {
  for (const Entry& e : TABLE)
    if (e.kind == kind && e.ks == ks && e.dt == dt && e.form == form) return &e;
  return nullptr;
}

// the sizes of a problem: what the route depends on
struct Shape {
  int batch_q, kv_group, heads, head_dim, lq, lk;
};

// what the kernels assume of the sizes
int check_shape(int batch_q, int kv_group, int heads, int head_dim, int lq, int lk, const char* who) {
  I2V_CHECK_ARG(batch_q > 0 && kv_group > 0 && batch_q % kv_group == 0 && heads > 0 && lq > 0 && lk > 0, "%s: bad sizes", who);
  I2V_CHECK_ARG(head_dim > 0 && head_dim % 8 == 0 && head_dim <= MAX_HEAD_DIM, "%s: head_dim (%d) must be a multiple of 8 and <= %d",
                who, head_dim, MAX_HEAD_DIM);
  I2V_CHECK_ARG(heads <= 65535 && batch_q <= 65535, "%s: heads / batch_q exceed the grid limits", who);
  return I2V_OK;
}

bool env_is(const char* name, int value, bool unset) { return getenv(name) ? atoi(getenv(name)) == value : unset; }

// THE dispatch rule: which instantiations run a problem that passed check_shape.  i2v_attention_bwd_f16 and i2v_attention_lse_f32
// launch what this answers and i2v_attention_bwd_route reports it; pure host arithmetic.
Route dispatch(const Shape& s, bool need_dkv) {
  Route r{};
  for (const Entry& e : TABLE)
    if (e.kind == I2V_ATTN_BWD_KIND_DQ && s.head_dim <= 16 * e.dt) {
      r.ks = e.ks, r.dt = e.dt;
      break;
    }
  // the environment switches, read once per process: I2V_ATTN_BWD_LDS=0 turns the LDS-staged forms off, I2V_ATTN_BWD_QB=32 the
  // 64-query stage of the dK / dV sweep
  static const bool lds = !env_is("I2V_ATTN_BWD_LDS", 0, false), qb64 = env_is("I2V_ATTN_BWD_QB", 64, true);
  // two 16-row tiles per wave where the sequence is long enough to still fill the chip (halves the fragment loads per FLOP)
  const bool two_q = s.lq >= 512 && r.dt <= TWO_TILE_MAX_DT, two_k = s.lk >= 512 && r.dt <= TWO_TILE_MAX_DT;
  r.dq_form = !two_q ? I2V_ATTN_BWD_DQ1 : (lds && s.lk >= 64) ? I2V_ATTN_BWD_DQ2_LDS : I2V_ATTN_BWD_DQ2;
  r.dq_blocks = (int32_t)i2v_cdiv(s.lq, two_q ? 128 : 64);
  const int32_t key_blocks = (int32_t)i2v_cdiv(s.lk, two_k ? 128 : 64);
  r.dkv_form = -1;
  if (need_dkv) {
    // 64 staged queries per barrier (two 32-query contraction steps): the 32-query loop has 28 MFMAs per wave between barriers.
    // Same box, 16 frames x 4096 tokens, d = 40 (tools/attn_bwd_probe.py): self-attention backward 2.95 -> 2.73 ms per call, the
    // cross-frame form (one K / V for 16 frames: 256 workgroups walking 1024 blocks each) 3.72 -> 3.16.  I2V_ATTN_BWD_QB=32: off.
    r.dkv_form = !two_k                          ? I2V_ATTN_BWD_DKV1
                 : (lds && s.lq >= 128 && qb64) ? I2V_ATTN_BWD_DKV2_LDS64
                 : (lds && s.lq >= 64)          ? I2V_ATTN_BWD_DKV2_LDS32
                                                : I2V_ATTN_BWD_DKV2;
    r.dkv_blocks = key_blocks;
  }
  // long sequences: K staged in LDS, two query tiles per wave
  r.lse_form = (lds && s.lq >= 512 && s.lk >= 64 && r.ks <= LSE_LDS_MAX_KS) ? I2V_ATTN_LSE_LDS : I2V_ATTN_LSE;
  // how many workgroups share the frames of one K / V in the dK / dV sweep: the cross-frame form has too few (key block, head)
  // workgroups for the chip, so the group is dealt out -- a power of two dividing kv_group that brings the sweep to about one thousand
  r.kv_partitions = 1;
  if (s.kv_group >= 2 && s.lq >= 32) {
    const int64_t blocks = (int64_t)key_blocks * s.heads * (s.batch_q / s.kv_group);
    const int most = s.kv_group < 8 ? s.kv_group : 8;
    int parts = 1;
    while (parts * 2 <= most && s.kv_group % (parts * 2) == 0 && blocks * parts < 1024) parts *= 2;
    r.kv_partitions = parts;
  }
  return r;
}

thread_local Route last_route;
thread_local bool have_last_route = false;
thread_local int last_lse_form = -1;

}  // namespace

extern "C" int i2v_attention_bwd_route(int32_t batch_q, int32_t kv_group, int32_t heads, int32_t head_dim, int32_t lq, int32_t lk,
                                       int32_t need_dkv, Route* route) {
  I2V_CHECK_ARG(route != nullptr, "i2v_attention_bwd_route: null argument");
  if (const int rc = check_shape(batch_q, kv_group, heads, head_dim, lq, lk, "i2v_attention_bwd_route")) return rc;
  *route = dispatch(Shape{batch_q, kv_group, heads, head_dim, lq, lk}, need_dkv != 0);
  return I2V_OK;
}

extern "C" int i2v_attention_bwd_last_route(Route* route) {
  I2V_CHECK_ARG(route != nullptr, "i2v_attention_bwd_last_route: null argument");
  I2V_CHECK_ARG(have_last_route, "i2v_attention_bwd_last_route: this thread has launched no i2v_attention_bwd_f16 yet");
  *route = last_route;
  route->lse_form = last_lse_form;
  return I2V_OK;
}

extern "C" int i2v_attn_bwd_kernel_exists(int32_t kind, const Route* r) {
  if (r == nullptr) return 0;
  const Entry* e = kind == I2V_ATTN_BWD_KIND_DQ    ? find_entry(kind, r->ks, r->dt, r->dq_form)
                   : kind == I2V_ATTN_BWD_KIND_DKV ? find_entry(kind, r->ks, r->dt, r->dkv_form)
                   : kind == I2V_ATTN_BWD_KIND_LSE ? find_entry(kind, r->ks, 0, r->lse_form)
                                                   : nullptr;
  return e != nullptr ? 1 : 0;
}

extern "C" int i2v_attention_lse_f32(const i2v_attn_params* pp, float* lse, i2v_stream_t stream) {
  I2V_CHECK_ARG(pp && lse, "i2v_attention_lse_f32: null argument");
  const i2v_attn_params& p = *pp;
  I2V_CHECK_ARG(p.q && p.k, "i2v_attention_lse_f32: null q / k");
  if (const int rc = check_shape(p.batch_q, p.kv_group, p.heads, p.head_dim, p.lq, p.lk, "i2v_attention_lse_f32")) return rc;
  I2V_CHECK_ARG(p.q_row_stride % 8 == 0 && p.k_row_stride % 8 == 0 && p.q_batch_stride % 8 == 0 && p.k_batch_stride % 8 == 0 &&
                    i2v_al16(p.q) && i2v_al16(p.k), "i2v_attention_lse_f32: q / k strides must be multiples of 8 elements, 16-byte aligned");
  const Route r = dispatch(Shape{p.batch_q, p.kv_group, p.heads, p.head_dim, p.lq, p.lk}, false);
  const Entry* e = find_entry(I2V_ATTN_BWD_KIND_LSE, r.ks, 0, r.lse_form);
  if (e == nullptr) I2V_FAIL(I2V_ERR_UNSUPPORTED, "i2v_attention_lse_f32: no kernel for form %d, KS %d", r.lse_form, r.ks);
  const dim3 grid((unsigned)i2v_cdiv(p.lq, r.lse_form == I2V_ATTN_LSE_LDS ? 128 : 64), p.heads, p.batch_q);
  e->lse(p, p.scale * LOG2E, lse, grid, reinterpret_cast<hipStream_t>(stream));
  last_lse_form = r.lse_form;
  return i2v_check_launch("i2v_attention_lse_f32");
}

extern "C" int i2v_attention_bwd_f16(const i2v_attn_bwd_params* pp, i2v_stream_t stream) {
  I2V_CHECK_ARG(pp != nullptr, "i2v_attention_bwd_f16: null params");
  const i2v_attn_bwd_params& p = *pp;
  I2V_CHECK_ARG(p.q && p.k && p.v && p.kt && p.dout && p.lse && p.delta && p.dq, "i2v_attention_bwd_f16: null pointer");
  if (const int rc = check_shape(p.batch_q, p.kv_group, p.heads, p.head_dim, p.lq, p.lk, "i2v_attention_bwd_f16")) return rc;
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
  const bool need_dkv = p.dk != nullptr;
  if (need_dkv && p.kv_partitions > 1)
    I2V_CHECK_ARG(p.dkv_partial != nullptr && i2v_al16(p.dkv_partial) && p.kv_group % p.kv_partitions == 0 &&
                      (p.heads * p.head_dim) % 4 == 0,
                  "i2v_attention_bwd_f16: kv_partitions (%d) needs the dkv_partial scratch and must divide kv_group (%d)",
                  p.kv_partitions, p.kv_group);
  if (need_dkv) {
    I2V_CHECK_ARG(p.dv && p.qt && p.doutt, "i2v_attention_bwd_f16: dk needs dv, qt and doutt");
    const int lq8 = (p.lq + 7) & ~7;
    I2V_CHECK_ARG(p.qt_row_stride >= lq8 && p.qt_row_stride % 8 == 0 && p.dot_row_stride >= lq8 && p.dot_row_stride % 8 == 0 &&
                      p.qt_batch_stride % 8 == 0 && p.dot_batch_stride % 8 == 0 && p.dk_row_stride % 8 == 0 &&
                      p.dk_batch_stride % 8 == 0 && p.dv_row_stride % 8 == 0 && p.dv_batch_stride % 8 == 0 && i2v_al16(p.qt) &&
                      i2v_al16(p.doutt) && i2v_al16(p.dk) && i2v_al16(p.dv),
                  "i2v_attention_bwd_f16: Q^T / dO^T / dK / dV strides and alignment");
  }
  Route r = dispatch(Shape{p.batch_q, p.kv_group, p.heads, p.head_dim, p.lq, p.lk}, need_dkv);
  const Entry* eq = find_entry(I2V_ATTN_BWD_KIND_DQ, r.ks, r.dt, r.dq_form);
  const Entry* ek = need_dkv ? find_entry(I2V_ATTN_BWD_KIND_DKV, r.ks, r.dt, r.dkv_form) : nullptr;
  if (eq == nullptr || (need_dkv && ek == nullptr))
    I2V_FAIL(I2V_ERR_UNSUPPORTED, "i2v_attention_bwd_f16: no kernel for dQ form %d / dK dV form %d, class <%d, %d>", r.dq_form, r.dkv_form,
             r.ks, r.dt);
  // the route recommends a partition count; the launch runs with the one the caller passed (it sized the dkv_partial scratch)
  r.kv_partitions = need_dkv && p.kv_partitions > 1 ? p.kv_partitions : 1;   // (every form of the sweep deals the group out)
  last_route = r;
  have_last_route = true;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float c = p.scale * LOG2E;
  eq->sweep(p, c, dim3((unsigned)r.dq_blocks, p.heads, p.batch_q), s);
  int rc = i2v_check_launch("i2v_attention_bwd_f16(dQ)");
  if (rc < 0 || !need_dkv) return rc;
  ek->sweep(p, c, dim3((unsigned)r.dkv_blocks, p.heads, (p.batch_q / p.kv_group) * r.kv_partitions), s);
  if (r.kv_partitions > 1) {
    const int64_t n4 = (int64_t)(p.batch_q / p.kv_group) * p.lk * ((int64_t)p.heads * p.head_dim / 4);
    hipLaunchKernelGGL(dkv_sum_kernel, dim3(i2v_ew_grid(n4, 256, 65535 * 4)), dim3(256), 0, s, p);
  }
  return i2v_check_launch("i2v_attention_bwd_f16(dK, dV)");
}
