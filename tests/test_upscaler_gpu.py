"""The Real-ESRGAN compact upscaler on the GPU against tests/srvgg_reference.py.

* i2v_conv3x3_c64_prelu_f16: every case of LAYER_CASES (tests/taesd_reference.SIZES x {bias, none} x {plain, own residual + closing
  ReLU} x pixel strides 64 / 72) against the fp64 layer with its per-element bound, inside NaN-poisoned buffers with guard rows; the
  multi-tile walk, slope 0 = ReLU and slope 1 = plain bit for bit, and the argument errors.  tests/test_upscaler.py shows that the
  bound rejects four wrong evaluations of every case.
* i2v_pixel_shuffle_add_f32: every case of EXIT_CASES against fp64 within 2^-22 (|y| + |base| + 1), the output between NaN guards.
* the "unit_clamp" entry map of i2v_taesd_prep_f16.
* the model: teacher-forced (binding: every launch against its layer's bound given the launch's own input), end to end against the
  fp32 restatement with the fp16-storage variant as the yardstick, batch = frames bit for bit.
* the pipeline and the driver.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import gemm_bounds as B
from tests import srvgg_reference as R
from tests import taesd_reference as T

pytestmark = pytest.mark.gpu
GUARD = 24       # guard pixels on either side of a token-major buffer
f16 = torch.float16


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def K():
    return pkg().kernels


def _strided(values, ld, dev, shape=None):
    """(NaN-filled buffer [GUARD + pixels + GUARD, ld], its [N, H, W, 64] view holding `values` (or left NaN))"""
    n, h, w, c = shape if values is None else values.shape
    buf = torch.full((n * h * w + 2 * GUARD, ld), float("nan"), dtype=f16, device=dev)
    view = buf[GUARD: GUARD + n * h * w, :c].view(n, h, w, c)
    if values is not None:
        view.copy_(values.to(dev))
    return buf, view


def _outside_is_nan(buf, n_pix, c=64):
    inner = buf[GUARD: GUARD + n_pix]
    return (bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n_pix:]).all())
            and bool(torch.isnan(inner[:, c:]).all()) and not bool(torch.isnan(inner[:, :c]).any()))


# ------------------------------------------------------------------------------------------------------------- the PReLU launch
@functools.lru_cache(maxsize=None)
def _layer_ref(case):
    x, w, b, slope, r = R.layer_case_inputs(case)
    return (x, w, b, slope, r) + R.layer_fp64(x, w, b, slope, r, case[1][2])


def _launch(case, dev, slope=None, **kw):
    (n, h, w), (name, bias, res_out, ldx, ldo) = case
    x, wt, b, sl, r, ref, tol = _layer_ref(case)
    xbuf, xv = _strided(x, ldx, dev)
    obuf, ov = _strided(None, ldo, dev, shape=(n, h, w, 64))
    out = K().conv3x3_c64(xv, K().pack_conv_c64(wt.to(dev)), None if b is None else b.to(dev), relu_out=res_out,
                          residual=None if r is None else r.to(dev), out=ov, slope=(sl if slope is None else slope).to(dev), **kw)
    assert out is ov
    return xbuf, obuf, ov


@pytest.mark.parametrize("case", R.LAYER_CASES, ids=R.layer_case_id)
def test_prelu_conv_obeys_the_bound_and_stays_inside_its_buffers(dev, case):
    (n, h, w), cfg = case
    x, wt, b, sl, r, ref, tol = _layer_ref(case)
    xbuf, obuf, ov = _launch(case, dev)
    got = ov.cpu()
    ex = B.excess(got, ref, tol)
    print(f"{R.layer_case_id(case)}: largest excess {float(ex.max()):.3e} (<= 0 passes), max |err| {float((got.double() - ref).abs().max()):.3e}")
    assert bool(torch.isfinite(got.float()).all())
    assert not bool((ex > 0).any()), f"{int((ex > 0).sum())}/{ex.numel()} elements miss the bound, largest excess {float(ex.max()):.3e}"
    assert _outside_is_nan(obuf, n * h * w), "the kernel wrote outside its 64 channels / pixels, or left a NaN inside"
    assert _outside_is_nan(xbuf, n * h * w) and torch.equal(xbuf[GUARD: GUARD + n * h * w, :64].cpu().view(n, h, w, 64), x)


@pytest.mark.parametrize("cfg", R.LAYER_CONFIGS, ids=[c[0] for c in R.LAYER_CONFIGS])
def test_prelu_multi_tile_walk_is_bit_equal(dev, cfg):
    """(3, 9, 17) is 12 tiles: max_workgroups 5 and 1, and a repeat, give the unconstrained launch's bits"""
    case = ((3, 9, 17), cfg)
    free = _launch(case, dev)[2].clone()
    walk = _launch(case, dev, max_workgroups=5)
    again = _launch(case, dev, max_workgroups=5)[2]
    one = _launch(case, dev, max_workgroups=1)[2]
    assert torch.equal(walk[2], free) and torch.equal(again, free) and torch.equal(one, free)
    assert _outside_is_nan(walk[1], 3 * 9 * 17)


@pytest.mark.parametrize("case", [c for c in R.LAYER_CASES if c[0] in ((3, 9, 17), (1, 1, 1))], ids=R.layer_case_id)
def test_slope_zero_is_the_relu_launch_and_slope_one_the_plain_one(dev, case):
    (n, h, w), (name, bias, res_out, ldx, ldo) = case
    x, wt, b, sl, r, ref, tol = _layer_ref(case)
    k = K()
    args = (x.to(dev), k.pack_conv_c64(wt.to(dev)), None if b is None else b.to(dev))
    kw = dict(relu_out=res_out, residual=None if r is None else r.to(dev))
    relu, plain = k.conv3x3_c64(*args, relu_mid=True, **kw), k.conv3x3_c64(*args, **kw)
    assert torch.equal(k.conv3x3_c64(*args, slope=torch.zeros(64, device=dev), **kw), relu)
    assert torch.equal(k.conv3x3_c64(*args, slope=torch.ones(64, device=dev), **kw), plain)
    assert not torch.equal(relu, plain)


def test_prelu_bad_operands_are_the_librarys_argument_error(dev):
    k, E = K(), pkg().HipLibraryError
    w = k.pack_conv_c64(torch.zeros(64, 64, 3, 3, device=dev))
    x = torch.zeros((2, 8, 16, 64), dtype=f16, device=dev)
    slope = torch.zeros(64, device=dev)
    sentinel = torch.full((2, 8, 16, 64), 7.0, dtype=f16, device=dev)
    with pytest.raises(E, match="i2v_conv3x3_c64_prelu_f16.*out overlaps x"):
        k.conv3x3_c64(x, w, out=x, slope=slope)
    mis = torch.zeros(2 * 8 * 16 * 64 + 8, dtype=f16, device=dev)[4: 4 + 2 * 8 * 16 * 64].view(2, 8, 16, 64)
    with pytest.raises(E, match="16-byte"):
        k.conv3x3_c64(mis, w, out=sentinel, slope=slope)
    with pytest.raises(E, match="64 -> 64"):
        k.conv3x3_c64(torch.zeros((2, 8, 16, 32), dtype=f16, device=dev), w, slope=slope)
    with pytest.raises(E, match="pixel strides"):
        k.conv3x3_c64(torch.zeros((2, 8, 16, 68), dtype=f16, device=dev)[..., :64], w, out=sentinel, slope=slope)
    with pytest.raises(E, match="slope"):
        k.conv3x3_c64(x, w, out=sentinel, slope=torch.zeros(66, device=dev)[2:])                 # 8-byte aligned
    with pytest.raises(E, match="relu_mid must be 0"):
        k.conv3x3_c64(x, w, out=sentinel, slope=slope, relu_mid=True)
    with pytest.raises(E, match="out overlaps slope"):
        k.conv3x3_c64(x, w, out=sentinel, slope=sentinel.view(torch.float32).view(-1)[:64])
    with pytest.raises(ValueError, match="slope"):
        k.conv3x3_c64(x, w, out=sentinel, slope=torch.zeros(32, device=dev))
    with pytest.raises(TypeError, match="slope"):
        k.conv3x3_c64(x, w, out=sentinel, slope=torch.zeros(64, dtype=f16, device=dev))
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())                      # nothing was launched


# ------------------------------------------------------------------------------------------------------------- the exit
@pytest.mark.parametrize("case", R.EXIT_CASES, ids=R.exit_case_id)
def test_exit_obeys_the_bound_and_stays_inside_its_buffer(dev, case):
    (n, h, w), s, f32, signed, ld = case
    y, src = R.exit_case_inputs(case)
    ref, tol = R.exit_fp64(y, src, s, unit_in=signed, clamp=True, signed_out=signed)
    raw, _ = R.exit_fp64(y, src, s, unit_in=signed, clamp=False, signed_out=False)
    assert bool((raw > 1).any()) and bool((raw < 0).any())                   # the clamp has work on both sides
    ybuf, yv = _strided(y, ld, dev)
    numel, g = n * 3 * s * h * s * w, 64
    obuf = torch.full((g + numel + g,), float("nan"), dtype=torch.float32, device=dev)
    ov = obuf[g: g + numel].view(n, 3, s * h, s * w)
    out = K().pixel_shuffle_add(yv, src.to(dev), s, unit_in=signed, clamp=True, signed_out=signed, out=ov)
    assert out is ov
    got = ov.cpu()
    assert bool(torch.isfinite(got).all()) and bool(torch.isnan(obuf[:g]).all()) and bool(torch.isnan(obuf[g + numel:]).all())
    ex = (got.double() - ref).abs() - tol
    print(f"{R.exit_case_id(case)}: largest excess {float(ex.max()):.3e} (<= 0 passes)")
    assert not bool((ex > 0).any()), f"{int((ex > 0).sum())}/{ex.numel()} elements miss the bound, largest excess {float(ex.max()):.3e}"
    assert _outside_is_nan(ybuf, n * h * w)
    # the unclamped / mixed forms are the same kernel
    free = K().pixel_shuffle_add(yv, src.to(dev), s, unit_in=signed, clamp=False, signed_out=False).cpu()
    assert not bool(((free.double() - raw).abs() > tol).any())


def test_exit_bad_operands_are_the_librarys_argument_error(dev):
    k, E = K(), pkg().HipLibraryError
    y = torch.zeros((2, 5, 7, 64), dtype=f16, device=dev)
    src = torch.zeros((2, 3, 5, 7), device=dev)
    sentinel = torch.full((2, 3, 20, 28), 7.0, device=dev)
    for s in (0, 5):
        with pytest.raises(E, match=f"s {s}"):
            k.pixel_shuffle_add(y, src, s, out=torch.full((2, 3, 5 * s, 7 * s), 7.0, device=dev))
    with pytest.raises(E, match="pixel stride"):
        k.pixel_shuffle_add(torch.zeros((2, 5, 7, 68), dtype=f16, device=dev)[..., :64], src, 4, out=sentinel)
    with pytest.raises(E, match="aligned"):
        k.pixel_shuffle_add(torch.zeros(2 * 5 * 7 * 64 + 8, dtype=f16, device=dev)[4: 4 + 2 * 5 * 7 * 64].view(2, 5, 7, 64), src, 4, out=sentinel)
    with pytest.raises(E, match="overlaps"):
        k.pixel_shuffle_add(y, sentinel.view(-1)[: 2 * 3 * 5 * 7].view(2, 3, 5, 7), 4, out=sentinel)
    with pytest.raises(ValueError, match="src"):
        k.pixel_shuffle_add(y, src[:, :2], 4, out=sentinel)
    with pytest.raises(ValueError, match="out"):
        k.pixel_shuffle_add(y, src, 2, out=sentinel)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())                      # nothing was launched


# ------------------------------------------------------------------------------------------------------------- the entry mover
@pytest.mark.parametrize("dtype", (torch.float32, f16), ids=("f32", "f16"))
@pytest.mark.parametrize("shape", ((1, 3, 1, 1), (2, 4, 5, 3), (3, 3, 40, 24), (1, 64, 3, 5), (2, 13, 7, 9)), ids=str)
def test_taesd_prep_unit_clamp(dev, shape, dtype):
    """min(max((v + 1) / 2, 0), 1) against fp64: |got - ref| <= (2^-11 + 2^-23) |ref| + 2^-25 -- one rounded add in fp32 (the halving
    and the clamps are exact) and the rounding to fp16, as for the "unit" map; the padding channels are zeros"""
    g = torch.Generator().manual_seed(shape[1] * 100 + shape[2])
    n, c, h, w = shape
    src = (torch.randn(shape, generator=g) * 2).to(dtype)
    src.view(-1)[0] = 0.0
    ref = ((src.double().permute(0, 2, 3, 1) + 1) / 2).clamp(0, 1)
    assert bool((ref == 0).any()) or n * h * w == 1
    for ld in (64, 72):
        buf, view = _strided(None, ld, dev, shape=(n, h, w, 64))
        out = K().taesd_prep(src.to(dev), "unit_clamp", out=view)
        assert out is view and _outside_is_nan(buf, n * h * w)
        got = view.cpu()
        assert bool((got[..., c:] == 0).all())
        ex = (got[..., :c].double() - ref).abs() - ((2.0 ** -11 + 2.0 ** -23) * ref.abs() + 2.0 ** -25)
        assert not bool((ex > 0).any()), float(ex.max())
        assert float(got[..., :c].min()) >= 0 and float(got[..., :c].max()) <= 1


# ------------------------------------------------------------------------------------------------------------- the model
MODELS = ((2, 2), (16, 4))
FRAMES = ((2, 3, 9, 17), (1, 3, 16, 32))


@functools.lru_cache(maxsize=None)
def _pair(num_conv, s):
    ref = R.seeded_reference(num_conv, s)
    hv = pkg().SRVGGNetCompact.from_pretrained(ref.state_dict())
    return ref, hv.to(torch.device("cuda:0"))


def _frames(shape):
    g = torch.Generator().manual_seed(shape[2] * 100 + shape[3])
    return torch.rand(shape, generator=g) * 2 - 1


@pytest.mark.parametrize("num_conv,s", MODELS)
def test_every_launch_binds_teacher_forced(dev, num_conv, s):
    ref, hv = _pair(num_conv, s)
    for shape in FRAMES:
        t = _frames(shape)
        hv._trace = []
        try:
            hv(t.to(dev), signed=True)
        finally:
            trace, hv._trace = hv._trace, None
        kinds = [e[1] for e in trace]
        assert kinds == ["prep"] + ["prelu"] * (1 + num_conv) + ["exit_conv", "exit"]
        for name, kind, x, y, extra in trace:
            x, y = x.cpu(), y.cpu()
            if kind == "prep":
                want = R.entry_map(x.double()).permute(0, 2, 3, 1)
                assert bool((y[..., 3:] == 0).all())
                y = y[..., :3]
                ex = (y.double() - want).abs() - ((2.0 ** -11 + 2.0 ** -23) * want.abs() + 2.0 ** -25)
            elif kind == "exit":
                want, tol = R.exit_fp64(x, extra.cpu(), s, unit_in=True, clamp=True, signed_out=True)
                ex = (y.double() - want).abs() - tol
            else:
                conv = ref.get_submodule(name)
                w16 = conv.weight.detach().half()
                w16 = torch.nn.functional.pad(w16, (0, 0, 0, 0, 0, 64 - w16.shape[1], 0, 64 - w16.shape[0]))
                b16 = torch.nn.functional.pad(conv.bias.detach().half(), (0, 64 - conv.bias.shape[0]))
                slope = None
                if kind == "prelu":
                    slope = ref.get_submodule(f"body.{int(name.split('.')[1]) + 1}").weight.detach()
                    assert torch.equal(extra.cpu(), slope)
                else:
                    assert bool((y[..., 3 * s * s:] == 0).all())                # the padding channels of the exit convolution
                want, tol = R.layer_fp64(x, w16, b16, slope)
                ex = B.excess(y, want, tol)
            assert tuple(y.shape) == tuple(want.shape), name
            assert bool(torch.isfinite(y.float()).all()) and not bool((ex > 0).any()), \
                f"{name} ({kind}) at {tuple(x.shape)}: {int((ex > 0).sum())}/{ex.numel()} elements miss the bound, largest excess {float(ex.max()):.3e}"


@pytest.mark.parametrize("num_conv,s", MODELS)
def test_end_to_end_within_twice_the_fp16_storage_error(dev, num_conv, s):
    """max-abs and rms error of the HIP model against the fp32 restatement, each at most twice what the CPU fp16-storage variant
    (fp32 accumulation) makes on the same input: the summation order differs and ties round either way; a wrong slope or channel is
    orders of magnitude above.  At most 10 % of the reference's outputs saturate, so the clamp cannot hide an error.
    Measured on one MI355X (HIP max / rms, yardstick max / rms): see DESIGN 4.18."""
    ref, hv = _pair(num_conv, s)
    for shape in FRAMES:
        t = _frames(shape)
        x = R.entry_map(t)
        with torch.no_grad():
            assert R.saturated_fraction(ref, x) <= 0.10
            exact = R.leave_map(ref(x), True)
            yard = R.leave_map(R.run_fp16_storage(ref, x), True) - exact
        got = hv(t.to(dev), signed=True).cpu()
        assert got.dtype == torch.float32 and got.shape == exact.shape == (shape[0], 3, s * shape[2], s * shape[3])
        err = got - exact
        pairs = (float(err.abs().max()), float(err.pow(2).mean().sqrt())), (float(yard.abs().max()), float(yard.pow(2).mean().sqrt()))
        print(f"num_conv {num_conv} s {s} {shape}: HIP vs fp32 max {pairs[0][0]:.3e} rms {pairs[0][1]:.3e}; fp16-storage vs fp32 "
              f"max {pairs[1][0]:.3e} rms {pairs[1][1]:.3e}")
        assert bool(torch.isfinite(got).all()) and float(got.min()) >= -1 and float(got.max()) <= 1
        assert pairs[0][0] <= 2 * pairs[1][0] and pairs[0][1] <= 2 * pairs[1][1], pairs
        # [0, 1] in and out is the same network
        with torch.no_grad():
            exact_u = R.leave_map(ref(x), False)
            yard_u = float((R.leave_map(R.run_fp16_storage(ref, x), False) - exact_u).abs().max())
        assert float((hv(x.to(dev), signed=False).cpu() - exact_u).abs().max()) <= 2 * yard_u


@pytest.mark.parametrize("num_conv,s", MODELS)
def test_a_batch_is_its_frames(dev, num_conv, s):
    _, hv = _pair(num_conv, s)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand((3, 3, 9, 17), generator=g) * 2 - 1).to(dev)
    whole = hv(x)
    for i in range(3):
        assert torch.equal(whole[i: i + 1], hv(x[i: i + 1])), i
    assert torch.equal(hv(x.half()), hv(x.half().float()))                   # an fp16 source is read as it is


def test_relu_and_leakyrelu_are_the_same_epilogue(dev):
    ref = R.seeded_reference(2, 2)
    bare = {k: v for k, v in ref.state_dict().items() if v.dim() != 1 or k.endswith("bias")}
    x = torch.rand((1, 3, 9, 17), generator=torch.Generator().manual_seed(2))
    for act in ("relu", "leakyrelu"):
        cpu = R.SRVGGReference(num_conv=2, upscale=2, act_type=act).eval()
        cpu.load_state_dict(bare)
        hv = pkg().SRVGGNetCompact.from_pretrained(bare, act_type=act).to(dev)
        with torch.no_grad():
            exact = cpu(x).clamp(0, 1)
            yard = float((R.run_fp16_storage(cpu, x).clamp(0, 1) - exact).abs().max())
        assert float((hv(x.to(dev), signed=False).cpu() - exact).abs().max()) <= 2 * yard


# ------------------------------------------------------------------------------------------------------------- the pipeline
def _small_pipe(dev):
    from tests.parity import hip_unet_from_oracle, oracle_small_unet
    hv = pkg().AutoencoderTiny()
    hv.load_state_dict(T.seeded_reference(0).state_dict())
    return pkg().I2VAdapterPipeline(vae=hv.to(dev).eval(), unet=hip_unet_from_oracle(oracle_small_unet(), dev))


def _call_args():
    g = torch.Generator().manual_seed(3)
    h = lambda t: t.half().float()
    kw = dict(prompt_embeds=h(torch.randn(1, 7, 64, generator=g)), negative_prompt_embeds=h(torch.randn(1, 7, 64, generator=g)),
              condition_image_latents=h(torch.randn(1, 4, 8, 8, generator=g)), num_frames=3, num_inference_steps=2, guidance_scale=7.5,
              frame_similarity_sample_ratio=1.0)
    gens = lambda: dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                        prior_noise_generator=torch.Generator().manual_seed(7))
    return kw, gens


def test_pipeline_upscales_the_decoded_frames(dev):
    from tests.parity import host_threads
    host_threads()
    pipe = _small_pipe(dev)
    kw, gens = _call_args()
    plain = pipe(output_type="pt", **kw, **gens()).frames
    assert plain.shape == (1, 3, 3, 64, 64)
    pipe.enable_upscaler(R.seeded_reference(2, 2).state_dict())
    assert pipe.upscaler_enabled and pipe._upscaler[0].device.type == "cuda"
    up = pipe(output_type="pt", **kw, **gens()).frames
    assert up.shape == (1, 3, 3, 128, 128) and up.dtype == torch.float32 and bool(torch.isfinite(up).all())
    assert torch.equal(up, pipe.upscale_frames(plain)) and torch.equal(up[0], pipe.upscale_frames(plain[0]))
    assert float(up.min()) >= -1 and float(up.max()) <= 1 and not torch.equal(up[..., ::2, ::2], plain)
    with pytest.raises(ValueError, match="output_type='latent' with the upscaler enabled"):
        pipe(output_type="latent", **kw, **gens())
    pipe.enable_upscaler(pipe._upscaler[0], frames_per_batch=1)
    assert torch.equal(pipe(output_type="pt", **kw, **gens()).frames, up)
    pipe.enable_upscaler(pipe._upscaler[0], frames_per_batch=2)
    assert torch.equal(pipe.upscale_frames(plain), up)
    pipe.enable_upscaler(pipe._upscaler[0])
    pipe.enable_vae_slicing()
    assert torch.equal(pipe(output_type="pt", **kw, **gens()).frames, up)
    pipe.disable_vae_slicing()
    pil = pipe(output_type="pil", **kw, **gens()).frames
    assert len(pil) == 1 and len(pil[0]) == 3 and all(im.size == (128, 128) for im in pil[0])
    pipe.disable_upscaler()
    assert torch.equal(pipe(output_type="pt", **kw, **gens()).frames, plain)
    assert pipe(output_type="latent", **kw, **gens()).frames.shape == (1, 3, 4, 8, 8)


def test_eval_driver_with_an_upscaler(dev, tmp_path):
    """`--upscaler FILE` on a one-row CSV: the GIF is `upscale` x the size"""
    import PIL.Image
    from safetensors.torch import save_file
    import i2v_adapter_unofficial_amd as p
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    from i2v_adapter_unofficial_amd.pipeline_i2v_adapter import main
    root = str(tmp_path)
    ch = (32, 64, 128, 128)
    kw = dict(sample_size=8, block_out_channels=ch, attention_head_dim=4, norm_num_groups=8, cross_attention_dim=64)
    init_random_weights_(p.UNet2DConditionModel(**kw), seed=1).save_pretrained(os.path.join(root, "sd", "unet"))
    init_random_weights_(p.AutoencoderKL(block_out_channels=(32, 64, 64, 64), norm_num_groups=8), seed=2) \
        .save_pretrained(os.path.join(root, "sd", "vae"))
    p.DDIMScheduler().save_pretrained(os.path.join(root, "sd", "scheduler"))
    init_random_weights_(p.MotionAdapter(block_out_channels=ch, motion_num_attention_heads=4, motion_norm_num_groups=8),
                         seed=3).save_pretrained(os.path.join(root, "motion"))
    init_random_weights_(p.I2VAdapterModule(2, ch, 4), seed=4).save_pretrained(
        os.path.join(root, "checkpoint", "demo", "epoch_3", "i2v_adapter"))
    torch.save({"params_ema": R.seeded_reference(2, 2).state_dict()}, os.path.join(root, "realesr-tiny.pth"))
    rs = np.random.RandomState(0)
    data = os.path.join(root, "data")
    os.makedirs(os.path.join(data, "images"))
    PIL.Image.fromarray((rs.rand(70, 90, 3) * 255).astype("uint8")).save(os.path.join(data, "images", "0.png"))
    with open(os.path.join(data, "eval.csv"), "w") as f:
        f.write('image_path,name\nimages/0.png,"a cat on a boat"\n')
    g = torch.Generator().manual_seed(5)
    save_file({"prompt_embeds": torch.randn(1, 7, 64, generator=g), "negative_prompt_embeds": torch.randn(1, 7, 64, generator=g)},
              os.path.join(root, "embeds.safetensors"))
    common = ["--task_name", "demo", "--checkpoint_epoch", "3", "--eval_data_path", os.path.join(data, "eval.csv"),
              "--embeds", os.path.join(root, "embeds.safetensors"), "--model_path", os.path.join(root, "sd"),
              "--motion_adapter_path", os.path.join(root, "motion"), "--checkpoint_root", os.path.join(root, "checkpoint"),
              "--samples_root", os.path.join(root, "samples"), "--num_frames", "3", "--num_inference_steps", "2"]
    assert main(common + ["--upscaler", os.path.join(root, "realesr-tiny.pth")]) == 0
    out = PIL.Image.open(os.path.join(root, "samples", "demo", "epoch_3", "a cat on a boat.gif"))
    assert out.n_frames == 3 and out.size == (128, 128)
