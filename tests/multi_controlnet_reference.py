"""What the Multi-ControlNet tests share: `i2v_add_multi_residuals_f16` evaluated in fp64, its per-element bounds (derived in the header
of tests/test_multi_controlnet_gpu.py), an fp32 restatement of the kernel's arithmetic on the CPU (with and without a fused
multiply-add chain), the kernel test's problem -- tests.controlnet_reference.kernel_case()'s tensors with residual sets from further
seeds -- and a restatement of diffusers' broadcasting rule for the per-net scale and window arguments."""
import torch

from tests import controlnet_reference as R

NETS_MAX = 4
# per-net scales of the kernel test: at least 0.5 apart, one of them 0 (so that a swap, a dropped net and the neighbouring row separate);
# for two nets also a pair without a zero, so that two products are summed everywhere
SCALES = {1: ((-0.75,),), 2: ((1.0, 0.0), (1.0, -0.75)), 3: ((1.0, 0.0, -0.75),), 4: ((1.0, 0.0, -0.75, 0.5),)}
ROWS, ROW = 3, R.KERNEL_ROW


def table(scales):
    """fp32 [N, 3]: net k's row is (s_k + 2, s_k + 0.5, s_k) -- read at row 2; the neighbouring row differs by 0.5 for every net"""
    return torch.tensor([[s + 2.0, s + 0.5, s] for s in scales], dtype=torch.float32)


_cases = {}


def case(n_nets):
    """(skips, lows, [N residual lists]): kernel_case()'s skips and lows; set 0 is its residuals, set k comes from seed 3 + 10 k.
    Computed once per N and shared: do not write to the tensors."""
    if n_nets not in _cases:
        skips, lows, ress = R.kernel_case()
        sets = [ress] + [R.kernel_case(seed=3 + 10 * k)[2] for k in range(1, n_nets)]
        _cases[n_nets] = (skips, lows, sets)
    return _cases[n_nets]


def fp64(skip, ress, scales, lo=None):
    """skip (+ lo) + sum_k s_k res_k in fp64; the tensors are fp16, the scales python floats that are exact in fp32"""
    ref = skip.double()
    if lo is not None:
        ref = ref + lo.double()
    for s, r in zip(scales, ress):
        ref = ref + float(s) * r.double()
    return ref


def bound(skip, ress, scales, lo=None):
    """the per-element bounds of tests/test_multi_controlnet_gpu.py's header"""
    n = len(ress)
    sp = sum((float(s) * r.double()).abs() for s, r in zip(scales, ress))
    ref = fp64(skip, ress, scales, lo).abs()
    if lo is None:
        return 2.0 ** -11 * ref + 2.0 ** -24 * (skip.double().abs() + (n + 1) * sp) + 2.0 ** -24
    return 2.0 ** -22 * ref + 2.0 ** -23 * (skip.double().abs() + lo.double().abs()) + 2.0 ** -24 * (n + 1) * sp + 2.0 ** -24


def _fma32(a, b, c):
    """fma(a, b, c) on fp32 tensors: the product of two fp32 values is exact in fp64, the sum is rounded there and then to fp32"""
    return (a.double() * b.double() + c.double()).float()


def restate(skip, ress, scales, lo=None, fma=False):
    """the kernel's arithmetic in fp32 on the CPU -> the value hi' (+ lo') stands for, in fp64.  fma=False: every product and every sum
    rounded on its own (what the kernel does).  fma=True: every product after the first fused into the running sum and the first one
    into nothing (what a contracting compiler may make of the same expression): the bounds hold for both."""
    sc = [torch.tensor(float(s), dtype=torch.float32) for s in scales]
    acc = sc[0] * ress[0].float()
    zero = acc == 0
    for s, r in zip(sc[1:], ress[1:]):
        p = s * r.float()
        zero = zero & (p == 0)
        acc = _fma32(s.expand_as(p), r.float(), acc) if fma else acc + p
    base = skip.float() if lo is None else skip.float() + lo.float()
    total = base + acc
    hi = total.half()
    if lo is None:
        return torch.where(zero, skip, hi).double()
    new_lo = (total - hi.float()).half()
    return torch.where(zero, skip, hi).double() + torch.where(zero, lo, new_lo).double()


def diffusers_broadcast(n_nets, scale, start, end):
    """diffusers' StableDiffusionControlNetPipeline.__call__ (the lines that align control_guidance_start / _end and
    controlnet_conditioning_scale with a MultiControlNetModel's nets), restated: -> (scales, starts, ends), three lists of n_nets"""
    if not isinstance(start, list) and isinstance(end, list):
        start = len(end) * [start]
    elif not isinstance(end, list) and isinstance(start, list):
        end = len(start) * [end]
    elif not isinstance(start, list) and not isinstance(end, list):
        start, end = n_nets * [start], n_nets * [end]
    if isinstance(scale, float):
        scale = [scale] * n_nets
    return list(scale), start, end
