"""The per-element error bound of `i2v_weight_embeds_f16` against float64, derived the way tests/gemm_bounds.py and
tests/tattn_bounds.py derive theirs: from the precision of the formats and the kernel's documented order of operations
(include/i2v_hip.h), never from what the kernel returns.

The kernel computes, for an element x (fp16, exact) of prompt p with weight w (fp32, exact),

    out = fl16( fl32( fl32(x * w) * r ) ),      r = fl32( S0^ / S1^ ),   S0^ ~ sum x,   S1^ ~ sum fl32(w x)

with u32 = 2^-24 and u16 = 2^-11 the unit roundoffs.  Against the exact y = x w R, R = sum x / sum w x:

  * The sums.  Their order is fixed: a lane adds the 8 values of each of its 16-byte chunks q = lane, lane + 1024, ... in turn, the wave
    adds its 64 lanes in a 6-level butterfly, the workgroup adds the 16 waves' partials in turn.  A value therefore passes through at
    most  d = 8 * ceil(chunks / 1024) + 6 + 16  additions (chunks = tokens * dim / 8), and the computed sum of terms t_i is
    sum t_i (1 + e_i) with |e_i| <= (1 + u32)^d - 1 =: g(d)  (Higham, Accuracy and Stability, eq. 4.4: every addition a term passes
    through contributes one factor).  The terms of S1 carry one more factor for the product's rounding: g(d + 1).
        |S0^ - S0| <= g(d) sum|x|,            |S1^ - S1| <= g(d + 1) sum|w x|
    Relative to the sums themselves that is  a = g(d) sum|x| / |sum x|  and  b = g(d + 1) sum|w x| / |sum w x|: the bound widens by
    itself when a mean is badly conditioned, and is infinite once b >= 1 (the computed S1 may be zero).
  * The ratio.  r = (S0^ / S1^)(1 + e), |e| <= u32 (the division is correctly rounded), so
        |r / R - 1| <= (1 + a)(1 + u32) / (1 - b) - 1 =: e_r
  * The element.  Two fp32 multiplies and the rounding to fp16, plus 2^-25 where the result is subnormal in fp16 (half the spacing
    2^-24 of the subnormals):
        |out - y| <= |y| ((1 + e_r)(1 + u32)^2 (1 + u16) - 1) + 2^-25

Without restore_mean r is exactly 1 and e_r = 0.  Inputs whose results leave fp16's range are not covered (an embedding is O(1))."""
import math

import torch

U32, U16 = 2.0 ** -24, 2.0 ** -11
THREADS, WAVE = 1024, 64          # the kernel's workgroup, from the header's description of the order of the sums


# (P, tokens, dim): one chunk; a prompt; two and three chunks of 77 (more than one pass of the 1024 lanes); odd sizes; a width that is
# no multiple of 64
CASES = [(1, 1, 8), (1, 77, 768), (3, 154, 768), (2, 231, 768), (5, 7, 24), (2, 33, 1032)]


def case_inputs(p, t, d, seed=0, offset=0.5):
    """embedding-like fp16 values with an offset (a well conditioned mean; 0.02 makes it ill conditioned), and weights as a prompt has
    them: bos 1, the rest spread over [0.2, 2]"""
    g = torch.Generator().manual_seed(seed + 131 * p + 17 * t + d)
    x = (torch.randn(p, t, d, generator=g) + offset).half()
    w = torch.ones(p, t)
    w[:, 1:] = (1.0 + 0.4 * torch.randn(p, max(t - 1, 0), generator=g)).clamp(0.2, 2.0)
    if t == 1:
        w[:] = 1.3
    return x, w.float()


def sum_depth(tokens, dim):
    chunks = tokens * (dim // 8)
    return 8 * math.ceil(chunks / THREADS) + int(math.log2(WAVE)) + THREADS // WAVE


def g(d):
    return (1.0 + U32) ** d - 1.0


def ratio_error(x, w, restore_mean=True):
    """e_r per prompt (float64 [P]); inf where the weighted mean is too badly conditioned for any statement"""
    x, w = x.double(), w.double()
    if not restore_mean:
        return torch.zeros(x.shape[0], dtype=torch.float64)
    d = sum_depth(x.shape[1], x.shape[2])
    y = x * w[:, :, None]
    a = g(d) * x.abs().sum((1, 2)) / x.sum((1, 2)).abs()
    b = g(d + 1) * y.abs().sum((1, 2)) / y.sum((1, 2)).abs()
    e = (1 + a) * (1 + U32) / (1 - b) - 1
    return torch.where((b < 1) & torch.isfinite(a), e, torch.full_like(e, float("inf")))


def bound(x, w, restore_mean=True):
    """the bound for every element: float64 [P, T, D]"""
    from tests.prompt_weight_reference import weight_ref64
    y, _ = weight_ref64(x, w, restore_mean)
    e_r = ratio_error(x, w, restore_mean)[:, None, None]
    return y.abs() * ((1 + e_r) * (1 + U32) ** 2 * (1 + U16) - 1) + 2.0 ** -25


def check(out, x, w, restore_mean=True):
    """(worst error / bound over ALL elements, every element within its bound).  A NaN anywhere fails."""
    from tests.prompt_weight_reference import weight_ref64
    y, _ = weight_ref64(x, w, restore_mean)
    b = bound(x, w, restore_mean)
    err = (out.double() - y).abs()
    ok = bool((err <= b).all())
    return float((err / b).max()), ok
