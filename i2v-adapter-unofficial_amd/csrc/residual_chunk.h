// out = in + s * r on one 16-byte chunk: the arithmetic that i2v_add_residuals_f16 (controlnet.hip) and i2v_add_broadcast_residual_f16
// (t2i_adapter.hip) share, so that the two kernels give the same bits for the same operands.
#pragma once
#include "common.h"

// one chunk: fp32 arithmetic, one rounding to fp16 (and the rounding's remainder as the new low half).  A product that is exactly
// zero leaves the skip's bits (and its low half's) as they are: s = 0 switches the control off bit for bit, -0 included.
template <bool HAS_LO>
__device__ __forceinline__ void ar_chunk(const f16x8 hi, const f16x8 lo, const f16x8 r, float s, f16x8& out, f16x8& out_lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float p = s * (float)r[j];
    if (HAS_LO) {
      const float sum = ((float)hi[j] + (float)lo[j]) + p;
      const f16 h = (f16)sum;
      const f16 l = (f16)(sum - (float)h);
      out[j] = p == 0.0f ? hi[j] : h;
      out_lo[j] = p == 0.0f ? lo[j] : l;
    } else {
      out[j] = p == 0.0f ? hi[j] : (f16)((float)hi[j] + p);
    }
  }
}
