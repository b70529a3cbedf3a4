"""Nearest-2x up-sampling folded into the conv weights (blocks.pack_upconv_fold, i2v_gemm_params.upsample = 2): the parts that
need no GPU -- the algebra and layout of the pack, the host query, the argument checks and the accounting.

Exactness of the algebra test: the operands are drawn on grids that fp16 represents exactly (x multiples of 2^-6 below 8, w
multiples of 2^-8 below 8), so every product is a multiple of 2^-14 and every partial sum of the <= 9 * 128 products stays below
2^17: all of it is exact in fp64 whatever the order of summation, and so are the pre-summed weights (sums of <= 4 such w).  The
folded form must therefore equal the reference convolution with max-abs error 0, not merely closely."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F


def _grid(shape, g, scale, step):
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale / step).round().clamp(-8 / step + 1, 8 / step - 1) * step


def unpack(f, cin, kblock):
    """[4, Cout, 4 Cin] in the packer's contraction order -> [phase, Cout, Cin, ty, tx], written from the documented index rule"""
    co = f.shape[1]
    out = torch.empty(4, co, cin, 2, 2, dtype=f.dtype)
    for t in range(4):
        for ci in range(cin):
            k = ((ci // 64) * 4 + t) * 64 + ci % 64 if kblock else t * cin + ci
            out[:, :, ci, t >> 1, t & 1] = f[:, :, k]
    return out


def folded_conv(x, f5, b):
    """the four 2x2 convolutions of the source image, interleaved into the up-sampled output"""
    n, _, h, w = x.shape
    out = torch.empty(n, f5.shape[1], 2 * h, 2 * w, dtype=x.dtype)
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        # output (2 i + py, 2 j + px) reads source rows i + py - 1, i + py and columns j + px - 1, j + px; outside = zero
        out[:, :, py::2, px::2] = F.conv2d(F.pad(x, (1 - px, px, 1 - py, py)), f5[ph], b)
    return out


@pytest.mark.parametrize("cin,cout,h,w", [(8, 5, 1, 1), (24, 6, 3, 5), (16, 4, 4, 4), (64, 7, 1, 1), (128, 3, 5, 3), (64, 9, 4, 6)])
def test_pack_algebra_is_exact(cin, cout, h, w):
    from i2v_adapter_unofficial_amd import blocks, kernels
    g = torch.Generator().manual_seed(cin * 100 + h * 10 + w)
    x, wt, b = _grid((2, cin, h, w), g, 1.0, 2.0 ** -6), _grid((cout, cin, 3, 3), g, 0.5, 2.0 ** -8), _grid((cout,), g, 1.0, 2.0 ** -6)
    assert (x.half().double() == x).all() and (wt.half().double() == wt).all()          # fp16-representable operands
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt, b, padding=1)
    kblock = bool(kernels.conv_k_block(cin))
    assert kblock == (cin % 64 == 0)
    f = blocks.pack_upconv_fold(wt, dtype=torch.float64)
    assert tuple(f.shape) == (4, cout, 4 * cin) and f.is_contiguous()
    got = folded_conv(x, unpack(f, cin, kblock), b)
    assert (got - ref).abs().max().item() == 0.0
    # the operand the kernel reads: the same sums formed in fp32 and rounded to fp16 once
    f16 = blocks.pack_upconv_fold(wt.float())
    assert f16.dtype == torch.float16 and torch.equal(f16, f.float().half())


def test_pack_sums_are_rounded_once():
    """a sum of four taps that fp16 cannot hold tap by tap: rounding after every addition would lose it"""
    from i2v_adapter_unofficial_amd import blocks
    wt = torch.zeros(1, 8, 3, 3)
    wt[0, 0, 1:, 1:] = torch.tensor([[1.0, 2.0 ** -11], [2.0 ** -11, 2.0 ** -11]])      # phase (0, 0), tap (1, 1): 1 + 3 * 2^-11
    f = blocks.pack_upconv_fold(wt)
    assert f[0, 0, 3 * 8].item() == torch.tensor(1.0 + 3 * 2.0 ** -11).half().item() == 1.0 + 2.0 ** -9


def _lib():
    import i2v_adapter_unofficial_amd as pkg
    import os
    import sys
    if not os.path.exists(pkg._lib.LIB_PATH):
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import __graft_entry__
        __graft_entry__.build()
    return pkg._lib


def test_query_accepts_the_step_shapes_and_refuses_what_the_kernel_cannot_do():
    from i2v_adapter_unofficial_amd import kernels as K
    lib = _lib()
    for shape, cout in (((32, 32, 32, 640), 640), ((32, 16, 16, 1280), 1280), ((32, 8, 8, 1280), 1280), ((12, 32, 32, 64), 320),
                        ((4, 32, 32, 128), 128), ((20, 16, 16, 640), 1280)):
        assert K.upconv_fold_supported(shape, cout), (shape, cout)
    # a phase that is not whole 256-row tiles, too few tiles for the 8-wave kernel, channel counts without a column tile / K tile
    for shape, cout in (((3, 7, 5, 64), 320), ((1, 8, 8, 64), 320), ((32, 16, 16, 1280), 1288), ((32, 16, 16, 72), 320)):
        assert not K.upconv_fold_supported(shape, cout), (shape, cout)
    h = lib.load()
    p = lib.GemmParams()
    K._upconv_fold_params(p, 32, 16, 16, 1280, 1280)
    p.a = p.w = p.c = p.bias = 1 << 40
    assert h.i2v_gemm_upconv_fold_supported(C.byref(p)) == 1 and h.i2v_gemm_workspace_bytes(C.byref(p)) == 0
    assert h.i2v_gemm_gn_partial_rows(C.byref(p)) == 0
    for field, value in (("residual", 1 << 41), ("rowvec", 1 << 41), ("c_lo", 1 << 41), ("out_h", 31), ("rows_per_w", 4096), ("upsample", 1),
                         ("K", 9 * 1280), ("a_perm_frames", 16)):
        q = lib.GemmParams.from_buffer_copy(p)
        setattr(q, field, value)
        if field == "rowvec":
            q.ld_rowvec, q.rows_per_vec = 1280, 1024
        assert h.i2v_gemm_upconv_fold_supported(C.byref(q)) == 0, field


def test_bad_folded_problems_are_refused_on_the_host():
    from i2v_adapter_unofficial_amd import kernels as K
    lib = _lib()
    h = lib.load()
    p = lib.GemmParams()
    K._upconv_fold_params(p, 3, 7, 5, 64, 320)           # no whole tiles per phase: no kernel runs it
    p.a = p.w = p.c = 1 << 40
    assert h.i2v_gemm_f16(C.byref(p), None) == -1 and b"i2v_gemm_upconv_fold_supported" in h.i2v_last_error()
    p.upsample = 3
    assert h.i2v_gemm_f16(C.byref(p), None) == -1 and b"upsample must be" in h.i2v_last_error()
    p.upsample, p.K, p.ldw = 2, 9 * 64, 9 * 64
    assert h.i2v_gemm_f16(C.byref(p), None) == -1 and b"4 cin" in h.i2v_last_error()


def test_profile_counts_the_executed_work():
    from i2v_adapter_unofficial_amd import profiling
    x, out = torch.empty(2, 4, 4, 64), torch.empty(2, 8, 8, 320)
    w9, wf = torch.empty(320, 9 * 64), torch.empty(4, 320, 4 * 64)
    cls, flops, _, detail = profiling._work_conv((x, w9), dict(upsample=True, w_folded=wf), out)
    assert (cls, flops, detail) == ("conv3x3", 2.0 * 128 * 320 * 256, "128x320x256 up4")
    cls, flops, _, detail = profiling._work_conv((x, w9), dict(upsample=True), out)
    assert (cls, flops, detail) == ("conv3x3", 2.0 * 128 * 320 * 576, "128x320x576 up")
