"""The hires fix on the host: the tap tables against torch's own interpolate in float64, the error bound the GPU test holds the kernel to
-- shown here to pass a faithful fp32 evaluation and to reject eight wrong ones --, the size rule and every refusal before anything is
encoded, the switches, the driver's flags, the handle's refusal and the ABI of i2v_resize_renoise_f32 with its host-side argument checks.
No kernel is launched."""
import os
import re

import numpy as np
import pytest
import torch

from tests import hires_bounds as HB
from tests.parity import ROOT, SMALL_UNET


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def HF():
    from i2v_adapter_unofficial_amd import hires_fix
    return hires_fix


def _src(pair, seed=3, planes=3):
    return np.random.RandomState(seed).randn(planes, pair[0], pair[1])


def _tables(pair, mode, dtype=np.float32):
    h, w, H, W = pair
    return HF().resize_tables(h, H, mode, dtype=dtype), HF().resize_tables(w, W, mode, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("mode", HB.MODES)
@pytest.mark.parametrize("pair", HB.SHAPE_PAIRS, ids=HB.pair_id)
def test_tables_against_torch_in_float64(pair, mode):
    h, w, H, W = pair
    src = _src(pair)
    rows, cols = _tables(pair, mode, np.float64)
    diff = np.abs(HB.apply(src, rows, cols) - HB.truth(src, H, W, mode)).max()
    print(f"{HB.pair_id(pair)} {mode}: max |tables - torch| = {diff:.3e}")
    assert diff <= HB.FP64_NOISE
    for (idx, wt), n_in, n_out in ((rows, h, H), (cols, w, W)):
        assert idx.shape == wt.shape == (n_out, 4) and idx.dtype == np.int32 and wt.dtype == np.float64
        assert idx.min() >= 0 and idx.max() < n_in


@pytest.mark.parametrize("mode", HB.MODES)
def test_the_fp32_tables_rows_sum_to_one_and_the_exact_cases(mode):
    for n_in, n_out in sorted({(p[0], p[2]) for p in HB.SHAPE_PAIRS} | {(p[1], p[3]) for p in HB.SHAPE_PAIRS} | {(64, 96), (64, 128)}):
        idx, wt = HF().resize_tables(n_in, n_out, mode)
        assert idx.dtype == np.int32 and wt.dtype == np.float32 and idx.shape == wt.shape == (n_out, 4)
        assert idx.min() >= 0 and idx.max() < n_in
        assert np.abs(wt.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22
        exact, _ = HF().resize_tables(n_in, n_out, mode, dtype=np.float64)
        assert np.array_equal(exact, idx)
        if mode.startswith("nearest"):
            assert np.array_equal(np.sort(wt, axis=1), np.tile(np.float32([0, 0, 0, 1]), (n_out, 1)))
        if n_in == n_out:
            # the identity: weight exactly 1 on the own index, in every mode
            one = wt == 1.0
            assert np.array_equal(one.sum(axis=1), np.ones(n_out)) and np.array_equal((wt != 0).sum(axis=1), np.ones(n_out))
            assert np.array_equal(idx[one], np.arange(n_out))


def test_resize_tables_refusals():
    with pytest.raises(ValueError, match="unknown upscaler 'lanczos'"):
        HF().resize_tables(4, 8, "lanczos")
    for n_in, n_out in ((8, 4), (0, 4), (5, 4)):
        with pytest.raises(ValueError, match="downscaling is not supported"):
            HF().resize_tables(n_in, n_out, "bilinear")


# ---------------------------------------------------------------------------------------------------------- the bound
def _fp32_evaluation(src, rows, cols, a, b, noise):
    """the kernel's arithmetic in numpy fp32: (wy * wx) * src, added in the order ky outer, kx inner, then a r (+ b n)"""
    (iy, wy), (ix, wx) = rows, cols
    f32 = np.float32
    s = src.astype(f32)
    r = None
    for ky in range(4):
        for kx in range(4):
            t = (wy[:, ky][None, :, None] * wx[:, kx][None, None, :]).astype(f32) * s[:, iy[:, ky]][:, :, ix[:, kx]]
            r = t if r is None else (r + t).astype(f32)
    out = (f32(a) * r).astype(f32)
    return out if noise is None else (out + (f32(b) * noise.astype(f32)).astype(f32)).astype(f32)


@pytest.mark.parametrize("mode", HB.MODES)
@pytest.mark.parametrize("pair", HB.SHAPE_PAIRS + [(64, 64, 96, 96)], ids=HB.pair_id)
def test_the_bound_passes_a_faithful_fp32_evaluation(pair, mode):
    src = _src(pair).astype(np.float32).astype(np.float64)
    rows, cols = _tables(pair, mode)
    noise = np.random.RandomState(5).randn(src.shape[0], pair[2], pair[3]).astype(np.float32).astype(np.float64)
    for a, b, z in ((1.0, 0.0, None), (0.6, 0.8, noise)):
        a, b = float(np.float32(a)), float(np.float32(b))
        got = _fp32_evaluation(src, rows, cols, a, b, z).astype(np.float64)
        ref = a * HB.apply(src, rows, cols) + (b * z if z is not None else 0.0)
        e = HB.bound(src, rows, cols, a, b, z)
        assert (np.abs(got - ref) <= e).all(), float((np.abs(got - ref) / np.maximum(e, 1e-300)).max())


def _wrong_forms():
    """name -> (modes it applies to, wrong(src, pair, mode) -> float64 output)"""
    v = HB.variant_tables

    def by_variant(**kw):
        return lambda src, p, mode: HB.apply(src, v(p[0], p[2], mode, **kw), v(p[1], p[3], mode, **kw))

    def other_scale(src, p, mode):
        # the coordinates of interpolate(scale_factor=f) with f = (n_out + 0.5) / n_in: the same output size, scale 1 / f
        return HB.apply(src, v(p[0], p[2], mode, scale=p[0] / (p[2] + 0.5)), v(p[1], p[3], mode, scale=p[1] / (p[3] + 0.5)))

    def transposed_gather(src, p, mode):
        # the row table indexing columns and the column table rows (clamped into the plane, as the kernel clamps)
        (iy, wy), (ix, wx) = _tables(p, mode, np.float64)
        g = src[:, np.minimum(ix, p[0] - 1)][:, :, :, np.minimum(iy, p[1] - 1)]          # [p, X, kx, Y, ky]
        return np.einsum("yk,xl,pxlyk->pyx", wy, wx, g)

    return {
        "bicubic with A = -0.5": (("bicubic",), by_variant(cubic_a=-0.5)),
        "antialiased bicubic with A = -0.75": (("bicubic-antialiased",), by_variant(cubic_a=-0.75)),
        "unnormalised antialiased weights": (("bilinear-antialiased", "bicubic-antialiased"), by_variant(normalise=False)),
        "align_corners=True coordinates": (("bilinear", "bicubic"), lambda src, p, mode: HB.truth(src, p[2], p[3], mode, align_corners=True)),
        "nearest where nearest-exact was asked": (("nearest-exact",), lambda src, p, mode: HB.truth(src, p[2], p[3], "nearest")),
        "bicubic's x clamped at 0": (("bicubic",), by_variant(clamp_cubic=True)),
        "row and column tables swapped": (HB.MODES, transposed_gather),
        "scale = 1 / scale_factor coordinates": (("bilinear", "bicubic", "bilinear-antialiased", "bicubic-antialiased"), other_scale),
    }


def test_the_variant_tables_restate_the_product_tables():
    for pair in HB.SHAPE_PAIRS:
        for mode in HB.MODES[2:]:
            for n_in, n_out in ((pair[0], pair[2]), (pair[1], pair[3])):
                idx, wt = HF().resize_tables(n_in, n_out, mode, dtype=np.float64)
                vi, vw = HB.variant_tables(n_in, n_out, mode)
                sel = vw != 0
                assert np.array_equal(wt != 0, sel) and np.array_equal(idx[sel], vi[sel]) and np.array_equal(wt, vw)


@pytest.mark.parametrize("form", sorted(_wrong_forms()))
def test_the_bound_rejects_the_wrong_evaluation(form):
    modes, wrong = _wrong_forms()[form]
    for mode in modes:
        coincide = []
        for pair in HB.SHAPE_PAIRS:
            src = _src(pair, seed=11).astype(np.float32).astype(np.float64)
            ref = HB.truth(src, pair[2], pair[3], mode)
            got = wrong(src, pair, mode)
            diff = np.abs(got - ref)
            if diff.max() <= HB.FP64_NOISE:
                coincide.append(pair)           # (asserted: the wrong form IS the right one on this case, an identity for example)
                continue
            e = HB.bound(src, *_tables(pair, mode))
            assert (diff > e).any(), f"{form}, {mode}, {HB.pair_id(pair)}: off by {diff.max():.3e} and inside the bound"
        print(f"{form} / {mode}: coincides with the truth on {[HB.pair_id(p) for p in coincide]}")
        if form == "nearest where nearest-exact was asked":
            # three, not two, and by arithmetic: one source pixel, the identity, and the integer factor 4 on both axes, where
            # floor(d / 4) == floor((d + 0.5) / 4) for every d -- `nearest` IS `nearest-exact` on exactly these
            assert coincide == [(1, 1, 3, 2), (4, 6, 16, 24), (6, 6, 6, 6)]
        else:
            assert len(coincide) <= 2, (form, mode, coincide)


# ---------------------------------------------------------------------------------------------------------- settings, sizes, refusals
def _cpu_pipe():
    p = pkg()
    return p.I2VAdapterPipeline(unet=p.UNetMotionCrossFrameAttnModel(**SMALL_UNET))


def _call(pipe, **kw):
    base = dict(condition_image_latents=torch.zeros(1, 4, 8, 8), num_frames=3, num_inference_steps=4, output_type="latent",
                prompt_embeds=torch.zeros(1, 7, 64), negative_prompt_embeds=torch.zeros(1, 7, 64))
    return pipe(**{**base, **kw})


def test_the_size_rule():
    S, target = HF().check_hires_fix_args, HF().target_size
    assert target(512, 512, S(1.5, None, 0.6, None, "bicubic")) == (768, 768)
    assert target(512, 320, S(2.0, None, 0.6, None, "bicubic")) == (1024, 640)
    assert target(64, 72, S(1.3, None, 0.6, None, "bicubic")) == (8 * round(64 * 1.3 / 8), 8 * round(72 * 1.3 / 8)) == (80, 96)
    assert target(64, 64, S(1.0, None, 0.6, None, "bicubic")) == (64, 64)                     # the base size is allowed
    assert target(64, 64, S(None, (96, 128), 0.6, None, "bicubic")) == (96, 128)
    assert target(64, 64, S(None, [64, 64], 0.6, None, "bicubic")) == (64, 64)
    with pytest.raises(ValueError, match="downscaling is not supported"):
        target(128, 64, S(None, (96, 96), 0.6, None, "bicubic"))


def test_enable_disable_and_every_refusal_of_enable():
    pipe = _cpu_pipe()
    assert pipe.hires_fix_enabled is False
    pipe.enable_hires_fix()
    assert pipe.hires_fix_enabled and pipe._hires_fix == (1.5, None, 0.6, None, "bicubic-antialiased")
    pipe.enable_hires_fix(size=(96, 96), strength=0.5, num_inference_steps=6, upscaler="nearest-exact")
    assert pipe._hires_fix == (None, (96, 96), 0.5, 6, "nearest-exact")
    pipe.disable_hires_fix()
    assert pipe.hires_fix_enabled is False and pipe._hires_fix is None
    with pytest.raises(ValueError, match="exactly one of `scale` and `size`.*both"):
        pipe.enable_hires_fix(scale=2.0, size=(96, 96))
    with pytest.raises(ValueError, match="exactly one of `scale` and `size`"):
        pipe.enable_hires_fix(scale=None, size=None)
    for bad in (0.5, 0.99, -2.0, float("nan")):
        with pytest.raises(ValueError, match="downscale|`scale`"):
            pipe.enable_hires_fix(scale=bad)
    for bad in ((100, 96), (96, 0), (96,), 96, (96.5, 96)):
        with pytest.raises(ValueError, match="`size`"):
            pipe.enable_hires_fix(size=bad)
    for bad in (0.0, -0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"`strength` should be in \(0.0, 1.0\]"):
            pipe.enable_hires_fix(strength=bad)
    with pytest.raises(ValueError, match="the second pass has 0 steps"):
        pipe.enable_hires_fix(strength=0.3, num_inference_steps=3)                             # int(3 * 0.3) = 0
    with pytest.raises(ValueError, match="integer >= 1"):
        pipe.enable_hires_fix(num_inference_steps=0)
    with pytest.raises(ValueError, match="unknown upscaler 'area'"):
        pipe.enable_hires_fix(upscaler="area")
    with pytest.raises(ValueError, match="pixel-space upscalers .* ESRGAN-class networks are not implemented"):
        pipe.enable_hires_fix(upscaler="R-ESRGAN 4x+")
    assert pipe.hires_fix_enabled is False                                                    # a refused enable changes nothing


def test_the_calls_refusals_come_before_anything_is_encoded():
    pipe = _cpu_pipe()                # no VAE, no GPU: anything behind the checks would raise something else
    pipe.enable_hires_fix(size=(56, 96))
    with pytest.raises(ValueError, match="56 x 96 is below the first pass's 64 x 64"):
        _call(pipe)
    with pytest.raises(ValueError, match="below the first pass's 128 x 128"):
        _call(pipe, height=128, width=128, condition_image=object())                            # (the size from the arguments)
    pipe.enable_hires_fix(scale=1.5, strength=0.2)
    with pytest.raises(ValueError, match="the second pass has 0 steps"):
        _call(pipe)                                                                            # int(4 * 0.2) = 0 with the call's steps
    pipe.enable_hires_fix(scale=1.5)
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):                        # a valid call goes on to the missing GPU
        _call(pipe)
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        pipe.upscale_latents(torch.zeros(1, 3, 4, 8, 8), 96, 96)
    with pytest.raises(ValueError, match="downscale"):
        pipe.upscale_latents(torch.zeros(1, 3, 4, 8, 8), 96, 56)
    with pytest.raises(ValueError, match="unknown upscaler"):
        pipe.upscale_latents(torch.zeros(1, 3, 4, 8, 8), 96, 96, upscaler="lanczos")
    with pytest.raises(ValueError, match="divisible by 8"):
        pipe.upscale_latents(torch.zeros(1, 3, 4, 8, 8), 100, 96)
    with pytest.raises(ValueError, match=r"\[B, F, C, h, w\]"):
        pipe.upscale_latents(torch.zeros(3, 4, 8, 8), 96, 96)
    pipe.disable_hires_fix()
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        _call(pipe)


def test_the_wrapper_refuses_host_tensors():
    z = torch.zeros(2, 4, 4)
    tables = tuple(torch.from_numpy(t) for pair in (HF().resize_tables(4, 6, "bilinear"), HF().resize_tables(4, 6, "bilinear")) for t in pair)
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        pkg().kernels.resize_renoise(z, tables)


def test_the_c_handle_refuses_a_pipeline_with_the_hires_fix():
    from i2v_adapter_unofficial_amd import handle
    pipe = _cpu_pipe()
    pipe.enable_hires_fix()
    st = dict(latents=torch.zeros(1, 4, 4, 16, 16), copies=2, ctx_text=torch.zeros(2, 7, 64, dtype=torch.float16), ctx_ip=None)
    for fn in (handle.record_step_plan, handle.record_prepare_plan):
        with pytest.raises(NotImplementedError, match=fn.__name__ + ".*hires fix"):
            fn(pipe, st)
    with pytest.raises(NotImplementedError, match="export_denoiser.*hires fix"):
        handle.export_denoiser(pipe, "unused", num_frames=4, latent_height=16, latent_width=16)


def test_driver_flags():
    P = pkg().pipeline_i2v_adapter
    parser = P.build_parser()
    a = parser.parse_args(["--task_name", "t"])
    assert a.hires_scale is None and a.hires_size is None and a.hires_strength == 0.6 and a.hires_steps is None
    assert a.hires_upscaler == "bicubic-antialiased"
    a = parser.parse_args(["--task_name", "t", "--hires_scale", "1.5", "--hires_strength", "0.5", "--hires_steps", "20", "--hires_upscaler",
                           "bilinear"])
    assert (a.hires_scale, a.hires_strength, a.hires_steps, a.hires_upscaler) == (1.5, 0.5, 20, "bilinear")
    assert parser.parse_args(["--task_name", "t", "--hires_size", "768", "1024"]).hires_size == [768, 1024]
    # refused before anything is loaded
    assert P.main(["--task_name", "t", "--hires_scale", "1.5", "--hires_size", "768", "768"]) == -1
    assert P.main(["--task_name", "t", "--hires_scale", "0.5"]) == -1
    assert P.main(["--task_name", "t", "--hires_size", "100", "96"]) == -1
    assert P.main(["--task_name", "t", "--hires_scale", "2", "--hires_upscaler", "esrgan"]) == -1
    assert P.main(["--task_name", "t", "--hires_scale", "2", "--hires_strength", "0.1", "--hires_steps", "5"]) == -1


# ---------------------------------------------------------------------------------------------------------- the ABI
NAME = "i2v_resize_renoise_f32"


def test_abi_30_declares_exports_and_binds_the_symbol():
    lib = pkg()._lib
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 30
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    from i2v_adapter_unofficial_amd import handle as H
    assert re.search(rf"\bint {NAME}\(", src) and NAME in lib.SIGNATURES and hasattr(h, NAME)
    assert NAME not in H.ENTRY_IDS                              # the C handle's plan format is unchanged: it refuses the hires fix
    assert len(lib.SIGNATURES[NAME][1]) == 15
    assert callable(pkg().kernels.resize_renoise)
    assert os.path.exists(os.path.join(ROOT, "i2v-adapter-unofficial_amd", "csrc", "resize.hip"))


def test_bad_arguments_are_refused_on_the_host():
    """I2V_ERR_INVALID_ARG before anything is launched: callable without a GPU (the pointers are never dereferenced)"""
    h = pkg()._lib.load()
    S, O, N, IY, WY, IX, WX = (1 << 40) + 4, 1 << 41, 1 << 42, 1 << 43, (1 << 43) + 4096, (1 << 43) + 8192, (1 << 43) + 12288
    ok = dict(src=S, out=O, noise=N, iy=IY, wy=WY, ix=IX, wx=WX, a=0.6, b=0.8, planes=24, h=5, w=7, H=9, W=13)
    out_bytes = 24 * 9 * 13 * 4
    cases = [(dict(src=None), b"null"), (dict(out=None), b"null"), (dict(iy=None), b"null"), (dict(wy=None), b"null"),
             (dict(ix=None), b"null"), (dict(wx=None), b"null"),
             (dict(H=4), b"downscale"), (dict(W=6), b"downscale"), (dict(h=10, w=14), b"downscale"),
             (dict(planes=0), b"positive"), (dict(h=0), b"positive"), (dict(w=-1), b"positive"),
             (dict(out=O + 4), b"16-byte"), (dict(noise=N + 8), b"16-byte"), (dict(iy=IY + 4), b"16-byte"), (dict(wx=WX + 8), b"16-byte"),
             (dict(src=S + 2), b"4-byte"),
             (dict(src=O + 16), b"overlaps"), (dict(src=O - 24 * 5 * 7 * 4 + 16), b"overlaps"), (dict(noise=O + out_bytes - 16), b"overlaps"),
             (dict(iy=O + 32), b"overlaps"), (dict(wx=O + out_bytes - 16), b"overlaps"),
             (dict(planes=1 << 31), b"too large"), (dict(planes=1 << 20, H=1 << 6, W=1 << 6), b"too large"),
             (dict(H=1 << 16, W=1 << 16), b"too large")]
    for kw, msg in cases:
        args = tuple({**ok, **kw}.values())
        assert getattr(h, NAME)(*args, None) == -1, kw
        assert NAME.encode() in h.i2v_last_error() and msg in h.i2v_last_error(), (kw, h.i2v_last_error())
