// out = in + s * r on one 16-byte chunk: the arithmetic that i2v_add_residuals_f16, i2v_add_multi_residuals_f16 (controlnet.hip) and
// i2v_add_broadcast_residual_f16 (t2i_adapter.hip) share, so that the kernels give the same bits for the same operands.
#pragma once
#include "common.h"

// one chunk, NETS residuals: p_k = s_k * r_k, acc = p_0 + p_1 + ... in net order, sum = in + acc -- fp32 arithmetic, every product and
// every sum rounded on its own, then one rounding to fp16 (and the rounding's remainder as the new low half).  Where every product is
// exactly zero the skip's bits (and its low half's) stay as they are: s = 0 switches the control off bit for bit, -0 included.
//
// Contraction is OFF in here.  The bit-level contracts hang on it: a product fused into the sum that follows it is not rounded, so
// fma(s, r, in) (one net) and in + (s * r + 0 * r') (the same net beside a silent one) would differ in their last bit, and which
// products are fused would be the compiler's choice per instantiation.  With every product rounded, a product that is exactly zero
// adds nothing to acc (x + 0 = x; acc = -0 only where all products are zero), so a silent net changes no bit, and one net is the
// same expression in every kernel that includes this header.
template <int NETS, bool HAS_LO>
__device__ __forceinline__ void ar_multi_chunk(const f16x8 hi, const f16x8 lo, const f16x8 (&r)[NETS], const float (&s)[NETS], f16x8& out,
                                               f16x8& out_lo) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float acc = s[0] * (float)r[0][j];
    bool zero = acc == 0.0f;
#pragma unroll
    for (int k = 1; k < NETS; ++k) {
      const float p = s[k] * (float)r[k][j];
      zero = zero && p == 0.0f;
      acc = acc + p;
    }
    if (HAS_LO) {
      const float sum = ((float)hi[j] + (float)lo[j]) + acc;
      const f16 h = (f16)sum;
      const f16 l = (f16)(sum - (float)h);
      out[j] = zero ? hi[j] : h;
      out_lo[j] = zero ? lo[j] : l;
    } else {
      out[j] = zero ? hi[j] : (f16)((float)hi[j] + acc);
    }
  }
}

// one residual: the single-net form of the above
template <bool HAS_LO>
__device__ __forceinline__ void ar_chunk(const f16x8 hi, const f16x8 lo, const f16x8 r, float s, f16x8& out, f16x8& out_lo) {
  const f16x8 rs[1] = {r};
  const float ss[1] = {s};
  ar_multi_chunk<1, HAS_LO>(hi, lo, rs, ss, out, out_lo);
}
