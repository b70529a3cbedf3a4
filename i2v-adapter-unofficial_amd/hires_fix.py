"""Hires fix (the two-pass "hires fix" of the AnimateDiff / A1111 / ComfyUI front ends): host side.  The tap tables the HIP latent upscale
reads (`kernels.resize_renoise`, csrc/resize.hip), the settings of `I2VAdapterPipeline.enable_hires_fix`, the size rule of the second pass
and the argument checks.

The specification of a table is torch's own `torch.nn.functional.interpolate(x, size=(H, W), mode=..., align_corners=False,
antialias=...)` on the CPU: SIZE-based, so the scale of an axis is n_in / n_out (not 1 / scale_factor).  Upscaling only (n_out >= n_in):
every mode then reads at most four source values per axis, and a table is four indices and four weights per output position.  The weights
are evaluated in float64 and rounded to fp32 once, here; the kernel does no coordinate arithmetic of its own."""
import collections
import math

import numpy as np
import torch

UPSCALERS = ("nearest", "nearest-exact", "bilinear", "bicubic", "bilinear-antialiased", "bicubic-antialiased")
TAPS = 4
DEFAULT_SCALE = 1.5
_device_tables = {}


def _cubic1(x, a):
    """the cubic convolution kernel for |x| <= 1"""
    return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0


def _cubic2(x, a):
    """the cubic convolution kernel for 1 < |x| < 2"""
    return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a


def _aa_filter(x, cubic):
    """torch's anti-alias filters: the triangle, or the cubic with A = -0.5"""
    x = abs(x)
    if not cubic:
        return 1.0 - x if x < 1.0 else 0.0
    if x < 1.0:
        return _cubic1(x, -0.5)
    if x < 2.0:
        return _cubic2(x, -0.5)
    return 0.0


def resize_tables(n_in, n_out, mode, dtype=np.float32):
    """-> (idx int32 [n_out, 4], w float32 [n_out, 4]) numpy arrays: output position d of an axis is sum_k w[d, k] * source[idx[d, k]].
    The weights are evaluated in float64 and rounded once to `dtype` (np.float64 returns them unrounded: what the tests compare with torch).
    `mode` is one of UPSCALERS; n_out >= n_in >= 1.  With s = n_in / n_out:
        nearest                 min(floor(d s), n_in - 1)                               (s and the product in fp32, as torch evaluates them)
        nearest-exact           min(floor((d + 0.5) s), n_in - 1)                       (likewise)
        bilinear                x = max(s (d + 0.5) - 0.5, 0), i0 = min(floor(x), n_in - 1), i1 = min(i0 + 1, n_in - 1), weights (1 - l, l)
        bicubic                 x = s (d + 0.5) - 0.5 NOT clamped, i = floor(x), t = x - i, indices clamp(i - 1 + k, 0, n_in - 1), the cubic
                                convolution weights with A = -0.75
        *-antialiased           torch's separable anti-alias path, whose support is not widened when upscaling: c = s (d + 0.5), support 1
                                (bilinear) or 2 (bicubic), taps lo = max(int(c - sup + 0.5), 0) .. hi = min(int(c + sup + 0.5), n_in), the
                                weight of tap j is filter(j + lo - c + 0.5) -- the triangle, or the cubic with A = -0.5 --, normalised by
                                their sum; hi - lo <= 4 for n_out >= n_in
    An unused tap has weight 0 and a valid index.  n_out == n_in gives weight exactly 1 on the own index in every mode."""
    n_in, n_out = int(n_in), int(n_out)
    if mode not in UPSCALERS:
        raise ValueError(f"unknown upscaler {mode!r}: one of {', '.join(UPSCALERS)}")
    if n_in < 1 or n_out < n_in:
        raise ValueError(f"resize_tables: {n_in} -> {n_out} is not an upscale (n_out >= n_in >= 1): downscaling is not supported")
    idx = np.zeros((n_out, TAPS), dtype=np.int64)
    w = np.zeros((n_out, TAPS), dtype=np.float64)
    s = n_in / n_out
    for d in range(n_out):
        if mode in ("nearest", "nearest-exact"):
            if n_out == n_in:
                i = d
            else:
                s32 = np.float32(n_in) / np.float32(n_out)
                pos = np.float32(d) if mode == "nearest" else np.float32(d) + np.float32(0.5)
                i = min(int(np.floor(np.float32(pos * s32))), n_in - 1)
            idx[d, :], w[d, 0] = i, 1.0
        elif mode == "bilinear":
            x = max(s * (d + 0.5) - 0.5, 0.0)
            i0 = min(int(math.floor(x)), n_in - 1)
            lam = min(max(x - i0, 0.0), 1.0)
            i1 = min(i0 + 1, n_in - 1)
            idx[d, :] = i0
            idx[d, 1] = i1
            w[d, 0], w[d, 1] = 1.0 - lam, lam
        elif mode == "bicubic":
            x = s * (d + 0.5) - 0.5
            i = int(math.floor(x))
            t = x - i
            a = -0.75
            w[d] = (_cubic2(t + 1.0, a), _cubic1(t, a), _cubic1(1.0 - t, a), _cubic2(2.0 - t, a))
            idx[d] = [min(max(i - 1 + k, 0), n_in - 1) for k in range(TAPS)]
        else:
            cubic = mode == "bicubic-antialiased"
            sup = 2.0 if cubic else 1.0
            c = s * (d + 0.5)
            lo = max(int(c - sup + 0.5), 0)
            hi = min(int(c + sup + 0.5), n_in)
            if not 1 <= hi - lo <= TAPS:
                raise AssertionError(f"resize_tables: {hi - lo} taps at {n_in} -> {n_out}, position {d}")
            taps = [_aa_filter(j + lo - c + 0.5, cubic) for j in range(hi - lo)]
            total = sum(taps)
            idx[d, :] = lo
            for j, v in enumerate(taps):
                idx[d, j], w[d, j] = lo + j, v / total
    return idx.astype(np.int32), w.astype(dtype)


def device_tables(h, w, height, width, mode, device):
    """(iy, wy, ix, wx) of an [h, w] -> [height, width] resize on `device`, the operands of `kernels.resize_renoise`: int32 / fp32
    [height, 4] and [width, 4], kept per (sizes, mode, device)"""
    key = (int(h), int(w), int(height), int(width), mode, str(device))
    hit = _device_tables.get(key)
    if hit is None:
        iy, wy = resize_tables(h, height, mode)
        ix, wx = resize_tables(w, width, mode)
        hit = tuple(torch.from_numpy(t).contiguous().to(device) for t in (iy, wy, ix, wx))
        if len(_device_tables) >= 16:       # a handful of sizes per process; never grows without bound
            _device_tables.clear()
        _device_tables[key] = hit
    return hit


HiresFixSettings = collections.namedtuple("HiresFixSettings", "scale size strength num_inference_steps upscaler")


def check_hires_fix_args(scale, size, strength, num_inference_steps, upscaler):
    """the argument checks of `enable_hires_fix` -> HiresFixSettings.  Exactly one of `scale` (>= 1) and `size` = (height, width),
    multiples of 8; `strength` in (0, 1]; `num_inference_steps` None (the call's) or an integer with int(steps * strength) >= 1."""
    if (scale is None) == (size is None):
        raise ValueError("hires fix: pass exactly one of `scale` and `size`" + (" (both were given)" if scale is not None else ""))
    if scale is not None:
        scale = float(scale)
        if not math.isfinite(scale) or scale < 1.0:
            raise ValueError(f"hires fix: `scale` = {scale} < 1 is a downscale; the second pass runs at the first pass's size or above")
    else:
        try:
            whole = all(int(v) == v for v in size)
            size = tuple(int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"hires fix: `size` must be (height, width), got {size!r}") from None
        if len(size) != 2 or not whole:
            raise ValueError(f"hires fix: `size` must be (height, width) in whole pixels, got {size!r}")
        if min(size) < 8 or size[0] % 8 or size[1] % 8:
            raise ValueError(f"hires fix: `size` = {size} must be positive multiples of 8 (the VAE's factor)")
    strength = float(strength)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"hires fix: `strength` should be in (0.0, 1.0] but is {strength}")
    if upscaler not in UPSCALERS:
        raise ValueError(f"hires fix: unknown upscaler {upscaler!r}: one of {', '.join(UPSCALERS)} -- pixel-space upscalers (decode, "
                         "resize, encode) and ESRGAN-class networks are not implemented: latent upscalers only")
    if num_inference_steps is not None:
        if int(num_inference_steps) != num_inference_steps or num_inference_steps < 1:
            raise ValueError(f"hires fix: `num_inference_steps` must be an integer >= 1, got {num_inference_steps!r}")
        num_inference_steps = int(num_inference_steps)
        second_pass_steps(num_inference_steps, strength)
    return HiresFixSettings(scale, size if scale is None else None, strength, num_inference_steps, upscaler)


def second_pass_steps(num_inference_steps, strength):
    """the steps the second pass executes: the last int(steps * strength) of a `num_inference_steps` schedule (video-to-video's rule)"""
    steps = min(int(num_inference_steps * strength), num_inference_steps)
    if steps < 1:
        raise ValueError(f"hires fix: after adjusting the num_inference_steps {num_inference_steps} by strength {strength} the second pass "
                         f"has {steps} steps, which is < 1")
    return steps


def target_size(height, width, settings):
    """the size of the second pass for a first pass of height x width: `size` as given, or 8 * round(side * scale / 8) per side.  A target
    side below the base side (a downscale) or not a multiple of 8 is a ValueError; the base size itself is allowed."""
    if settings.size is not None:
        h2, w2 = settings.size
    else:
        h2, w2 = (8 * int(round(side * settings.scale / 8)) for side in (height, width))
    if h2 % 8 or w2 % 8:
        raise ValueError(f"hires fix: the target {h2} x {w2} has to be divisible by 8")
    if h2 < height or w2 < width:
        raise ValueError(f"hires fix: the target {h2} x {w2} is below the first pass's {height} x {width}: downscaling is not supported")
    return h2, w2
