"""The folded up-sampling convolution on the GPU (K.conv3x3(..., w_folded=), i2v_gemm_params.upsample = 2): four pre-summed taps
per output parity instead of nine gathered ones.

Reference: the exact fp64 convolution of the fp16-rounded operands, F.conv2d(F.interpolate(x, 2, "nearest"), w, b, padding=1), with the
`close` rule of tests/test_kernels_gpu.py (rel 3e-3, as test_conv3x3_big_tiles).  Every output element is compared.  Against the kernel
it replaces: on the same inputs the folded route's rms error may be at most 1.5 x the 9-tap route's (the weight rounding of the
pre-summed taps adds 2.0e-4 rms to the 2.7 - 3.1e-4 of the fp16 output rounding both have: 1.20 - 1.24 x expected)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import _pack_conv, close

pytestmark = pytest.mark.gpu


def h64(t):
    return t.half().double()


def _mods():
    import i2v_adapter_unofficial_amd as pkg
    return pkg.kernels, pkg.blocks


def _run(dev, x, w, b, fold):
    """x [n, cin, h, w], w [cout, cin, 3, 3], b [cout] (fp16-representable) -> NCHW result of the folded / the 9-tap route"""
    K, blocks = _mods()
    xt = x.permute(0, 2, 3, 1).contiguous().half().to(dev)
    wp, bd = _pack_conv(w.float()).to(dev), b.half().to(dev)
    if fold:
        assert K.upconv_fold_supported(xt.shape, w.shape[0])
        out = K.conv3x3(xt, wp, bd, upsample=True, w_folded=blocks.pack_upconv_fold(w.float()).to(dev))
    else:
        out = K.conv3x3(xt, wp, bd, upsample=True)
    return out.permute(0, 3, 1, 2)


def _ref(x, w, b):
    return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)


def _rms(t):
    return t.double().pow(2).mean().sqrt().item()


# the three up-samplers of the denoising step, the shapes test_conv3x3_big_tiles runs with up=True (320- and 128-column tiles), batches
# that are not 32 (128-row tiles of the 320-column form; the 256-column tile), 256-row and 128-row tiles of the 8 x 8 -> 16 x 16 problem
SHAPES = [(32, 32, 32, 640, 640), (32, 16, 16, 1280, 1280), (32, 8, 8, 1280, 1280), (12, 32, 32, 64, 320), (4, 32, 32, 128, 128),
          (20, 16, 16, 640, 1280), (4, 64, 64, 256, 256), (24, 8, 8, 320, 1280)]


@pytest.mark.parametrize("n,hh,ww,cin,cout", SHAPES)
def test_folded_route_matches_the_exact_convolution_and_the_kernel_it_replaces(dev, n, hh, ww, cin, cout):
    g = torch.Generator().manual_seed(cin + cout + n)
    x = h64(torch.randn(n, cin, hh, ww, generator=g))
    w = h64(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin))
    b = h64(torch.randn(cout, generator=g))
    ref = _ref(x, w, b)
    got, old = _run(dev, x, w, b, True).cpu(), _run(dev, x, w, b, False).cpu()
    e_new, e_old = _rms(got.double() - ref), _rms(old.double() - ref)
    print(f"upconv fold {n}x{hh}x{ww} {cin}->{cout}: rms err folded {e_new:.3e}, 9-tap {e_old:.3e}, ratio {e_new / e_old:.3f}, "
          f"out rms {_rms(ref):.3f}, max err folded {(got.double() - ref).abs().max().item():.3e}")
    close(got, ref, name="folded up-sampling conv")
    assert e_new <= 1.5 * e_old, (e_new, e_old)


@pytest.mark.parametrize("n,hh,ww,cin,cout", [(12, 32, 32, 64, 320), (32, 8, 8, 1280, 1280), (4, 32, 32, 128, 128)])
def test_impulses_on_every_border_and_corner(dev, n, hh, ww, cin, cout):
    """single source pixels on each border and corner (and one inside), every other pixel zero: what each of the 3 x 3 output
    neighbourhoods of an impulse receives is one pre-summed tap of one phase, and at the border part of it must fall off the image"""
    g = torch.Generator().manual_seed(7 + cin)
    w = h64(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin))
    b = h64(torch.randn(cout, generator=g) * 0.1)
    spots = [(0, 0), (0, ww - 1), (hh - 1, 0), (hh - 1, ww - 1), (0, ww // 2), (hh - 1, ww // 2), (hh // 2, 0), (hh // 2, ww - 1),
             (hh // 2, ww // 2)]
    x = torch.zeros(n, cin, hh, ww, dtype=torch.float64)
    for i in range(n):                    # one impulse per image (cycling through the spots), the last image carries all of them
        for (sy, sx) in (spots if i == n - 1 else [spots[i % len(spots)]]):
            x[i, :, sy, sx] = h64(torch.randn(cin, generator=g))
    ref = _ref(x, w, b)
    close(_run(dev, x, w, b, True), ref, name="folded up-sampling conv, border impulses")
    # the images' first / last rows and columns on their own, so that an error there cannot hide behind the tolerance's max|ref| term
    got = _run(dev, x, w, b, True).cpu()
    for sl in ((..., 0, slice(None)), (..., -1, slice(None)), (..., slice(None), 0), (..., slice(None), -1)):
        close(got[sl], ref[sl], name=f"border {sl[1:]}")


def _upsampler(dev, channels, seed):
    _, blocks = _mods()
    torch.manual_seed(seed)
    return blocks.Upsample2D(channels).half().to(dev)


def _spy(monkeypatch):
    K, _ = _mods()
    calls, real = [], K.conv3x3

    def conv3x3(*a, **kw):
        calls.append(kw.get("w_folded") is not None)
        return real(*a, **kw)
    monkeypatch.setattr(K, "conv3x3", conv3x3)
    return calls, real


def test_module_takes_the_folded_route_and_the_switch_restores_the_nine_taps(dev, monkeypatch):
    K, blocks = _mods()
    up = _upsampler(dev, 640, 3)
    x = torch.randn(16, 16, 16, 640, generator=torch.Generator().manual_seed(1)).half().to(dev)
    calls, real = _spy(monkeypatch)
    p = up.packed()
    nine = real(x, p["w"], p["b"], upsample=True)
    monkeypatch.setattr(blocks, "UPCONV_FOLD", True)
    y = up._fwd(x)
    y2 = up._fwd(x, (32, 32))
    assert calls == [True, True] and torch.equal(y, y2)
    ref = _ref(x.permute(0, 3, 1, 2).double().cpu(), up.conv.weight.double().cpu(), up.conv.bias.double().cpu())
    close(y.permute(0, 3, 1, 2), ref, name="Upsample2D, folded")
    monkeypatch.setattr(blocks, "UPCONV_FOLD", False)           # I2V_UPCONV_FOLD=0: the 9-tap kernel, bit for bit
    assert torch.equal(up._fwd(x), nine) and calls[-1] is False


@pytest.mark.parametrize("n,hh,ww,c,size", [(16, 16, 16, 640, (31, 32)), (16, 16, 16, 640, (32, 31)), (16, 16, 16, 640, (31, 31)),
                                            (3, 7, 5, 64, None), (1, 8, 8, 320, None), (2, 9, 9, 40, (17, 18))])
def test_fallbacks_stay_on_the_nine_tap_kernel_bit_for_bit(dev, monkeypatch, n, hh, ww, c, size):
    """2x - 1 output sizes (forward_upsample_size) and shapes the query refuses: the same call as before, the same bits"""
    K, blocks = _mods()
    monkeypatch.setattr(blocks, "UPCONV_FOLD", True)
    up = _upsampler(dev, c, 5)
    x = torch.randn(n, hh, ww, c, generator=torch.Generator().manual_seed(2)).half().to(dev)
    calls, real = _spy(monkeypatch)
    p = up.packed()
    want = real(x, p["w"], p["b"], upsample=True, output_size=size)
    got = up._fwd(x, size)
    assert calls == [False] and torch.equal(got, want)
    assert "w_fold" not in dict.keys(p)                         # the lazy pack was not built for a route that does not read it


def test_wrapper_refuses_what_the_folded_form_cannot_express(dev):
    K, blocks = _mods()
    up = _upsampler(dev, 640, 3)
    p = up.packed()
    x = torch.zeros(16, 16, 16, 640, dtype=torch.float16, device=dev)
    with pytest.raises(ValueError, match="exactly"):
        K.conv3x3(x, p["w"], p["b"], upsample=True, w_folded=p["w_fold"], output_size=(31, 32))
    with pytest.raises(ValueError, match="bias only"):
        K.conv3x3(x, p["w"], p["b"], upsample=True, w_folded=p["w_fold"], out_scale=0.5)
    with pytest.raises(ValueError, match="w_folded must be"):
        K.conv3x3(x, p["w"], p["b"], upsample=True, w_folded=p["w_fold"][:, :, :-8].contiguous())
