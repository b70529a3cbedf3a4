"""The yardsticks of the hires fix's latent upscale (tests/test_hires_fix.py on the host, tests/test_hires_fix_gpu.py on the GPU).

The truth is torch's own `F.interpolate(x, size=(H, W), mode=..., align_corners=False, antialias=...)` on float64 CPU tensors
(`truth`).  `apply` evaluates a pair of tap tables in float64 with numpy -- what i2v_resize_renoise_f32 computes, without its roundings.
`bound` is the kernel's error bound against `apply` on the SAME fp32 tables:

    E = 2^-19 (|a| sum |wy| |wx| |src| + |b| |noise|)

2^-19 = 32 * 2^-24: two weight roundings, two product roundings, at most 15 additions and the three roundings of the final a r + b n,
each at most 2^-24 relative on a partial sum that sum |wy| |wx| |src| bounds -- 22 roundings, with room.

`variant_tables` restates the table arithmetic with its decisions exposed, so that the tests can build the WRONG evaluations the bound
has to reject: the other cubic constant, unnormalised anti-alias weights, align_corners=True coordinates, a clamped bicubic coordinate,
1 / scale_factor coordinates."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# (h, w -> H, W)
SHAPE_PAIRS = [(1, 1, 3, 2), (2, 3, 5, 4), (3, 5, 3, 13), (5, 3, 7, 7), (8, 8, 12, 12), (7, 9, 10, 31), (4, 6, 16, 24), (9, 5, 11, 6),
               (6, 6, 6, 6), (8, 8, 9, 8)]
MODES = ("nearest", "nearest-exact", "bilinear", "bicubic", "bilinear-antialiased", "bicubic-antialiased")
REL = 2.0 ** -19
FP64_NOISE = 1e-12


def pair_id(p):
    return f"{p[0]}x{p[1]}-{p[2]}x{p[3]}"


def truth(src, height, width, mode, align_corners=False):
    """src float64 [planes, h, w] (numpy) -> float64 [planes, height, width]: torch's CPU interpolate"""
    x = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float64))[None]
    base = mode.replace("-antialiased", "")
    if base.startswith("nearest"):
        return F.interpolate(x, size=(height, width), mode=base)[0].numpy()
    return F.interpolate(x, size=(height, width), mode=base, align_corners=align_corners, antialias=mode.endswith("-antialiased"))[0].numpy()


def apply(src, row_table, col_table):
    """sum_ky sum_kx wy[Y, ky] wx[X, kx] src[p, iy[Y, ky], ix[X, kx]] in float64; tables are (idx [n, 4], w [n, 4])"""
    (iy, wy), (ix, wx) = row_table, col_table
    src = np.asarray(src, dtype=np.float64)
    g = src[:, iy.astype(np.int64)][:, :, :, ix.astype(np.int64)]                # [p, Y, ky, X, kx]
    return np.einsum("yk,xl,pykxl->pyx", np.asarray(wy, dtype=np.float64), np.asarray(wx, dtype=np.float64), g)


def bound(src, row_table, col_table, a=1.0, b=0.0, noise=None):
    """E per output element, float64, from the fp32 tables the kernel reads"""
    (iy, wy), (ix, wx) = row_table, col_table
    e = abs(a) * apply(np.abs(src), (iy, np.abs(np.asarray(wy, dtype=np.float64))), (ix, np.abs(np.asarray(wx, dtype=np.float64))))
    if noise is not None:
        e = e + abs(b) * np.abs(np.asarray(noise, dtype=np.float64))
    return REL * e


def _cubic(x, a):
    x = abs(x)
    if x <= 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a
    return 0.0


def variant_tables(n_in, n_out, mode, cubic_a=None, normalise=True, clamp_cubic=False, scale=None, align_corners=False):
    """float64 tables of one axis with the decisions of hires_fix.resize_tables exposed (the defaults restate it for the four
    interpolating modes): `cubic_a` the cubic constant (default -0.75 for bicubic, -0.5 for bicubic-antialiased), `normalise` the division
    of the anti-alias weights by their sum, `clamp_cubic` clamping bicubic's source coordinate at 0, `scale` the scale of the axis
    (default n_in / n_out), `align_corners` the align_corners=True coordinate d (n_in - 1) / (n_out - 1)."""
    s = n_in / n_out if scale is None else scale
    idx, w = np.zeros((n_out, 4), dtype=np.int32), np.zeros((n_out, 4), dtype=np.float64)
    for d in range(n_out):
        if align_corners:
            x = d * ((n_in - 1) / (n_out - 1)) if n_out > 1 else 0.0
        else:
            x = s * (d + 0.5) - 0.5
        if mode == "bilinear":
            x = max(x, 0.0)
            i0 = min(int(math.floor(x)), n_in - 1)
            lam = min(max(x - i0, 0.0), 1.0)
            idx[d], w[d, 0], w[d, 1] = (i0, min(i0 + 1, n_in - 1), i0, i0), 1.0 - lam, lam
        elif mode == "bicubic":
            a = -0.75 if cubic_a is None else cubic_a
            if clamp_cubic:
                x = max(x, 0.0)
            i = int(math.floor(x))
            t = x - i
            idx[d] = [min(max(i - 1 + k, 0), n_in - 1) for k in range(4)]
            w[d] = [_cubic(t + 1.0, a), _cubic(t, a), _cubic(1.0 - t, a), _cubic(2.0 - t, a)]
        else:
            cubic = mode == "bicubic-antialiased"
            a = -0.5 if cubic_a is None else cubic_a
            sup = 2.0 if cubic else 1.0
            c = s * (d + 0.5)
            lo, hi = max(int(c - sup + 0.5), 0), min(int(c + sup + 0.5), n_in)
            taps = [(_cubic(j + lo - c + 0.5, a) if cubic else max(1.0 - abs(j + lo - c + 0.5), 0.0)) for j in range(min(hi - lo, 4))]
            total = sum(taps) if normalise else 1.0
            idx[d] = lo
            for j, v in enumerate(taps):
                idx[d, j], w[d, j] = lo + j, v / total
    return idx, w
