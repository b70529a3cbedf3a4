"""The hires fix on the GPU: the kernel i2v_resize_renoise_f32 against the float64 evaluation of its own fp32 tables under the bound of
tests/hires_bounds.py and in its exact cases, and the pipeline's second pass on the small UNet -- bit-equal to the two calls it stands
for (a latent call, `upscale_latents`, the condition at the target size, a `video_latents=` call) under five samplers and next to a
ControlNet, a T2I-Adapter, a mask, per-frame prompts, FreeNoise and FreeInit; the graph cache; the output's shapes; the callback.

Yardsticks.  |got - ref| <= E = 2^-19 (|a| sum |wy| |wx| |src| + |b| |noise|) per element (tests/hires_bounds.py).  Bit-equal: the
nearest modes with (a, b) = (1, 0) to the gather, identity sizes in every mode to the source, two runs to each other, and the fused launch
to the unfused pair resize + `K.axpby`.  Every launch writes into the middle of a NaN-filled buffer whose margins must stay NaN."""
import numpy as np
import pytest
import torch

from tests import controlnet_reference as CR
from tests import hires_bounds as HB
from tests import t2i_adapter_reference as TR
from tests.parity import hip_unet_from_oracle, oracle_small_unet

pytestmark = pytest.mark.gpu

f16 = torch.float16
PLANES = (2, 3, 4)               # B, F, C
GUARD = 64                       # fp32 values of NaN on either side of the output
COEFS = ((1.0, 0.0), (0.6, 0.8))


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def HF():
    from i2v_adapter_unofficial_amd import hires_fix
    return hires_fix


def bits(t):
    return t.contiguous().view(torch.int32)


def h16(t):
    return t.half().float()


# ---------------------------------------------------------------------------------------------------------- the kernel
def _launch(dev, src, tables, noise, a, b):
    """through the ABI into the middle of a NaN-filled buffer: the margins stay NaN, the interior has none.  Returns the host result."""
    K, L = pkg().kernels, pkg()._lib
    height, width = tables[0].shape[0], tables[2].shape[0]
    planes = src.numel() // (src.shape[-2] * src.shape[-1])
    numel = planes * height * width
    buf = torch.full((numel + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    out = buf[GUARD: GUARD + numel]
    L.check(L.load().i2v_resize_renoise_f32(src.data_ptr(), out.data_ptr(), noise.data_ptr() if noise is not None else None,
                                            *(t.data_ptr() for t in tables), a, b, planes, src.shape[-2], src.shape[-1], height, width,
                                            K._stream()), "i2v_resize_renoise_f32")
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool(host[:GUARD].isnan().all()) and bool(host[GUARD + numel:].isnan().all()), "written outside the output"
    assert not bool(host[GUARD: GUARD + numel].isnan().any()), "an output value was not written"
    return host[GUARD: GUARD + numel].view(*src.shape[:-2], height, width)


@pytest.mark.parametrize("pair", HB.SHAPE_PAIRS + [(64, 64, 96, 96)], ids=HB.pair_id)
def test_kernel_against_float64_in_every_mode(dev, pair):
    K = pkg().kernels
    h, w, H, W = pair
    g = torch.Generator().manual_seed(7)
    src, noise = torch.randn(*PLANES, h, w, generator=g), torch.randn(*PLANES, H, W, generator=g)
    d_src, d_noise = src.to(dev), noise.to(dev)
    s64, n64 = src.reshape(-1, h, w).double().numpy(), noise.reshape(-1, H, W).double().numpy()
    for mode in HB.MODES:
        rows, cols = HF().resize_tables(h, H, mode), HF().resize_tables(w, W, mode)
        tables = HF().device_tables(h, w, H, W, mode, dev)
        assert all(torch.equal(t.cpu(), torch.from_numpy(x)) for t, x in zip(tables, rows + cols))
        base = HB.apply(s64, rows, cols)
        for a, b in COEFS:
            a32, b32 = float(np.float32(a)), float(np.float32(b))
            for z in (None, d_noise):
                got = _launch(dev, d_src, tables, z, a, b)
                ref = a32 * base + (b32 * n64 if z is not None else 0.0)
                e = HB.bound(s64, rows, cols, a32, b32, n64 if z is not None else None)
                err = np.abs(got.reshape(-1, H, W).double().numpy() - ref)
                worst = float((err / np.maximum(e, 1e-300)).max())
                print(f"resize_renoise {HB.pair_id(pair)} {mode} a={a} b={b} noise={z is not None}: worst |err| / E = {worst:.3f}")
                assert (err <= e).all(), (mode, a, b, worst)
                # two runs are bit-equal, and so is the wrapper's own allocation
                assert torch.equal(bits(_launch(dev, d_src, tables, z, a, b)), bits(got))
                assert torch.equal(bits(K.resize_renoise(d_src, tables, z, a, b).cpu()), bits(got))
                if z is not None:
                    # the fused launch against resize followed by axpby
                    two = K.axpby(K.resize_renoise(d_src, tables), d_noise, a, b).cpu()
                    assert torch.equal(bits(two), bits(got)), (mode, a, b)
                elif a == 1.0:
                    if mode.startswith("nearest"):
                        gather = src[..., torch.from_numpy(rows[0][:, 0]).long(), :][..., torch.from_numpy(cols[0][:, 0]).long()]
                        assert torch.equal(bits(gather), bits(got)), mode
                    if (h, w) == (H, W):
                        assert torch.equal(bits(src), bits(got)), mode
        assert torch.equal(d_src.cpu(), src) and torch.equal(d_noise.cpu(), noise)


def test_wrapper_refusals(dev):
    K = pkg().kernels
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
    tables = HF().device_tables(5, 7, 9, 13, "bilinear", dev)
    assert K.resize_renoise(z(2, 5, 7), tables).shape == (2, 9, 13)
    with pytest.raises(ValueError, match="downscale"):
        K.resize_renoise(z(2, 10, 7), tables)
    with pytest.raises(ValueError, match="noise must be"):
        K.resize_renoise(z(2, 5, 7), tables, z(2, 9, 12))
    with pytest.raises(ValueError, match="contiguous"):
        K.resize_renoise(z(2, 5, 14)[..., ::2], tables)
    with pytest.raises(ValueError, match=r"\[n_out, 4\] table"):
        K.resize_renoise(z(2, 5, 7), (tables[0], tables[1][:, :3], tables[2], tables[3]))
    with pytest.raises(TypeError, match="float32"):
        K.resize_renoise(z(2, 5, 7).half(), tables)
    with pytest.raises(TypeError, match="int32"):
        K.resize_renoise(z(2, 5, 7), (tables[0].long(),) + tables[1:])


# ---------------------------------------------------------------------------------------------------------- the pipeline
FRAMES, BASE, TARGET, STEPS = 3, 64, 96, 4


@pytest.fixture(scope="module")
def small(dev):
    ou = oracle_small_unet()
    return ou, hip_unet_from_oracle(ou, dev)


@pytest.fixture(scope="module")
def vae(dev):
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    return init_random_weights_(pkg().AutoencoderKL(block_out_channels=(32, 64, 64, 64), norm_num_groups=8), seed=2).to(dev, f16).eval()


def _pil(t):
    import PIL.Image
    return PIL.Image.fromarray((t.permute(1, 2, 0).numpy() * 255).round().astype("uint8"))


def _image(seed=21):
    return _pil(torch.rand(3, BASE, BASE, generator=torch.Generator().manual_seed(seed)))


def _control(seed=41):
    return [_pil(f) for f in torch.rand(FRAMES, 3, BASE, BASE, generator=torch.Generator().manual_seed(seed))]


def _embeds(seed=31, per_frame=False, frames=FRAMES):
    g = torch.Generator().manual_seed(seed)
    shape = (1, frames, 7, 64) if per_frame else (1, 7, 64)
    return dict(prompt_embeds=h16(torch.randn(*shape, generator=g)), negative_prompt_embeds=h16(torch.randn(*shape, generator=g)),
                num_frames=frames, guidance_scale=7.5, num_inference_steps=STEPS, output_type="latent")


def _gens():
    return dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _sched(kind):
    p = pkg()
    return {"ddim": p.DDIMScheduler, "dpmsolver++": p.DPMSolverMultistepScheduler, "lcm": p.LCMScheduler,
            "euler_discrete": p.EulerDiscreteScheduler, "euler_ancestral": p.EulerAncestralDiscreteScheduler}[kind]()


def _both_routes(pipe, kw, extra=None, free_init=False, image=None, target=(TARGET, TARGET)):
    """-> (hires, manual): the call with the fix enabled, and the two calls it stands for with the same generator objects re-seeded
    identically.  `extra`: the arguments both passes share beside `kw` (control frames, a mask)."""
    extra, image = dict(extra or {}), image if image is not None else _image()
    first_source = {k: extra.pop(k) for k in ("video_latents", "strength") if k in extra}
    pipe.enable_hires_fix(size=target, strength=0.5)
    hires = pipe(**kw, **extra, **first_source, condition_image=image, height=BASE, width=BASE, **_gens()).frames
    pipe.disable_hires_fix()
    gens = _gens()
    first = pipe(**kw, **extra, **first_source, condition_image=image, height=BASE, width=BASE, **gens).frames
    source = pipe.upscale_latents(first, *target, upscaler="bicubic-antialiased")
    cond = pipe.encode_condition_image(image, *target, gens["generator"])
    if free_init:
        pipe.disable_free_init()
    manual = pipe(**kw, **extra, video_latents=source, strength=0.5, condition_image_latents=cond, height=target[0], width=target[1],
                  **gens).frames
    return hires, manual


@pytest.mark.parametrize("kind", ["ddim", "dpmsolver++", "lcm", "euler_discrete", "euler_ancestral"])
def test_the_hires_call_is_the_two_calls_it_stands_for(dev, small, vae, kind):
    pipe = pkg().I2VAdapterPipeline(vae=vae, unet=small[1], scheduler=_sched(kind))
    hires, manual = _both_routes(pipe, _embeds())
    assert hires.shape == (1, FRAMES, 4, TARGET // 8, TARGET // 8) and bool(torch.isfinite(hires).all())
    assert torch.equal(bits(hires), bits(manual))
    assert len(pipe._graph_cache) == 2                         # the two sizes, captured once each and replayed by the manual route


def test_next_to_a_controlnet(dev, small, vae):
    cn = pkg().ControlNetModel(**CR.small_config())
    cn.load_state_dict(CR.small_reference().state_dict())
    pipe = pkg().I2VAdapterPipeline(vae=vae, unet=small[1], controlnet=cn.to(dev, f16).eval())
    hires, manual = _both_routes(pipe, _embeds(), dict(control_image=_control()))
    assert torch.equal(bits(hires), bits(manual))
    pipe.enable_hires_fix(size=(TARGET, TARGET), strength=0.5)
    off = pipe(**_embeds(), control_image=_control(), controlnet_conditioning_scale=0.0, condition_image=_image(), height=BASE, width=BASE,
               **_gens()).frames
    assert not torch.equal(off, hires), "the control does not reach the result"


def test_next_to_a_t2i_adapter(dev, small, vae):
    ad = pkg().T2IAdapter(**TR.small_config(3))
    ad.load_state_dict(TR.small_reference(3).state_dict())
    pipe = pkg().I2VAdapterPipeline(vae=vae, unet=small[1], t2i_adapter=ad.to(dev, f16).eval())
    hires, manual = _both_routes(pipe, _embeds(), dict(adapter_image=_control(43)))
    assert torch.equal(bits(hires), bits(manual))


def test_with_a_mask_the_second_pass_keeps_the_upscaled_first_pass(dev, small, vae):
    pipe = pkg().I2VAdapterPipeline(vae=vae, unet=small[1])
    mask = torch.zeros(BASE // 8, BASE // 8)
    mask[:, BASE // 16:] = 1.0                                 # the right half is regenerated, the left half keeps the source
    clip = torch.randn(1, FRAMES, 4, BASE // 8, BASE // 8, generator=torch.Generator().manual_seed(9))
    hires, manual = _both_routes(pipe, _embeds(), dict(mask_image=mask, video_latents=clip, strength=1.0))
    assert torch.equal(bits(hires), bits(manual))
    # the kept half of frames 1.. is the upscaled first pass, bit for bit (the mask's last row is the clean source)
    first = pipe(**_embeds(), mask_image=mask, video_latents=clip, strength=1.0, condition_image=_image(), height=BASE, width=BASE,
                 **_gens()).frames
    up = pipe.upscale_latents(first, TARGET, TARGET, upscaler="bicubic-antialiased")
    half = TARGET // 16
    assert torch.equal(bits(hires[:, 1:, :, :, :half]), bits(up[:, 1:, :, :, :half]))
    assert not torch.equal(hires[:, 1:, :, :, half:], up[:, 1:, :, :, half:])


def test_with_per_frame_prompts(dev, small, vae):
    pipe = pkg().I2VAdapterPipeline(vae=vae, unet=small[1])
    hires, manual = _both_routes(pipe, _embeds(per_frame=True))
    assert torch.equal(bits(hires), bits(manual))


def test_under_free_noise(dev, small, vae):
    """6 frames with context_length 4: both passes' initial noise is FreeNoise's reschedule of the prior's draw"""
    pipe = pkg().I2VAdapterPipeline(vae=vae, unet=small[1])
    pipe.enable_free_noise(context_length=4, context_stride=2)
    try:
        hires, manual = _both_routes(pipe, _embeds(frames=6))
    finally:
        pipe.disable_free_noise()
    assert hires.shape == (1, 6, 4, TARGET // 8, TARGET // 8) and torch.equal(bits(hires), bits(manual))


def test_free_init_belongs_to_the_first_pass(dev, small, vae):
    pipe = pkg().I2VAdapterPipeline(vae=vae, unet=small[1])
    pipe.enable_free_init(num_iters=2)
    hires, manual = _both_routes(pipe, _embeds(), free_init=True)
    assert not pipe.free_init_enabled and torch.equal(bits(hires), bits(manual))
    plain, _ = _both_routes(pipe, _embeds())
    assert not torch.equal(plain, hires), "FreeInit's second round did not run"


def test_condition_latents_that_were_passed_in_are_upscaled(dev, small):
    pipe = pkg().I2VAdapterPipeline(unet=small[1])
    cond = torch.randn(1, 4, BASE // 8, BASE // 8, generator=torch.Generator().manual_seed(3))
    pipe.enable_hires_fix(size=(TARGET, TARGET), strength=0.5, upscaler="bilinear")
    hires = pipe(**_embeds(), condition_image_latents=cond, **_gens()).frames
    pipe.disable_hires_fix()
    gens = _gens()
    first = pipe(**_embeds(), condition_image_latents=cond, **gens).frames
    cond2 = pipe.upscale_latents(cond[:, None], TARGET, TARGET, upscaler="bilinear")[:, 0]
    manual = pipe(**_embeds(), video_latents=pipe.upscale_latents(first, TARGET, TARGET, upscaler="bilinear"), strength=0.5,
                  condition_image_latents=cond2, **gens).frames
    assert torch.equal(bits(hires), bits(manual)) and torch.equal(bits(hires[:, 0]), bits(cond2))


def test_the_graph_cache_holds_the_two_sizes_and_a_plain_call_is_what_it_was(dev, small, vae):
    pipe = pkg().I2VAdapterPipeline(vae=vae, unet=small[1])
    call = lambda seed=31: pipe(**_embeds(seed), condition_image=_image(), height=BASE, width=BASE, **_gens()).frames
    before = call()
    plain_graph = pipe._graph
    pipe._graph_cache.clear()
    pipe.enable_hires_fix(size=(TARGET, TARGET), strength=0.5)
    first = call()
    assert len(pipe._graph_cache) == 2
    keys, graphs = list(pipe._graph_cache), [g for g, _ in pipe._graph_cache.values()]
    second = call(77)                                          # other embeds: replayed, nothing captured
    assert len(pipe._graph_cache) == 2 and set(pipe._graph_cache) == set(keys)
    assert all(any(g is old for old in graphs) for g, _ in pipe._graph_cache.values())
    assert not torch.equal(second, first) and torch.equal(call(), first)
    pipe.disable_hires_fix()
    after = call()
    assert torch.equal(bits(after), bits(before)) and any(pipe._graph is g for g in graphs), "a plain call captured a new graph"
    assert len(pipe._graph_cache) == 2 and plain_graph is not None
    # while the fix is off the cache holds one shape at a time again
    pipe(**_embeds(), condition_image=_image(), height=BASE, width=2 * BASE, **_gens())
    assert len(pipe._graph_cache) == 1


def test_output_shapes_the_identity_target_and_the_callback(dev, small, vae):
    pipe = pkg().I2VAdapterPipeline(vae=vae, unet=small[1])
    kw = dict(_embeds(), condition_image=_image(), height=BASE, width=BASE)
    plain = pipe(**kw, **_gens()).frames
    pipe.enable_hires_fix(size=(TARGET, 128), strength=0.5)
    assert pipe(**kw, **_gens()).frames.shape == (1, FRAMES, 4, TARGET // 8, 16)              # a non-square target
    frames = pipe(**dict(kw, output_type="pt"), **_gens()).frames
    assert frames.shape == (1, FRAMES, 3, TARGET, 128) and bool(torch.isfinite(frames).all())
    # a target equal to the base size: the resize is an identity and the second pass still runs
    pipe.enable_hires_fix(scale=1.0, strength=0.5)
    same = pipe(**kw, **_gens()).frames
    assert same.shape == plain.shape and not torch.equal(same, plain)
    # the callback sees both passes, the second pass's indices after the first's; eager steps, the same bits
    pipe.enable_hires_fix(size=(TARGET, TARGET), strength=0.5)
    seen = []
    eager = pipe(**kw, callback=lambda i, t, x: seen.append((i, int(t), tuple(x.shape[-2:]))), **_gens()).frames
    assert [i for i, _, _ in seen] == list(range(STEPS + int(STEPS * 0.5)))
    assert [s for _, _, s in seen] == [(BASE // 8,) * 2] * STEPS + [(TARGET // 8,) * 2] * int(STEPS * 0.5)
    assert torch.equal(bits(eager), bits(pipe(**kw, **_gens()).frames))
