"""Video-to-video and masked editing on the GPU: the kernel i2v_masked_renoise_f32 against the fp32 restatement
(tests/video2video_reference.py) and in its exact cases, and the pipeline's `video=` / `video_latents=` / `strength=` / `mask_image=` on
the small UNet -- the initial latents, the DDIM trajectory against the reference loop on the oracle UNet, graph == eager under the three
schedulers, the mask's exact cases, the step count under `strength`, the captured graph's reuse, `encode_video` with both VAEs, a
ControlNet and FreeNoise next to it, and the driver.

Yardsticks.  The kernel is held per element to |got - ref| <= 4 * 2^-24 * (|m l| + |1 - m| (|a s| + |b n|)) against the float64 blend
of its fp32 operands: the result is a handful of fp32 roundings of those terms, whatever the contraction.  m == 1, and m == 0 at the
row (1, 0), are bit-exact.  `prepare_video_latents` is two products and one sum: 2 * 2^-24 of each term.  The trajectory uses the
existing gate, tests/parity.REL_TOL_TRAJECTORY of max|latent|.
"""
import os

import numpy as np
import pytest
import torch

from tests import controlnet_reference as CR
from tests import video2video_reference as R
from tests.parity import REL_TOL_TRAJECTORY, compare, hip_unet_from_oracle, oracle_small_unet

pytestmark = pytest.mark.gpu

f16 = torch.float16
SHAPES = [(3, 4, 35),            # an odd 5 x 7 plane: the scalar tail, planes not 16-byte aligned to each other
          (2, 4, 256),
          (5, 4, 4096 + 4)]      # more than one 1024-chunk tile per plane, and a tile that straddles two planes
TABLE = [[1.0, 0.0], [0.8, 0.6], [0.3125, 0.95], [0.05, 0.9987]]


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h16(t):
    return t.half().float()


def bits(t):
    return t.contiguous().view(torch.int32)


def _operands(shape, seed=9):
    """latents, source, noise [n, c, hw] and a soft mask [n, 1, hw] with exact zeros and ones in it"""
    g = torch.Generator().manual_seed(seed)
    n, c, hw = shape
    l, s, z = (torch.randn(n, c, hw, generator=g) for _ in range(3))
    m = torch.rand(n, 1, hw, generator=g)
    pick = torch.rand(n, 1, hw, generator=g)
    m[pick < 0.2] = 0.0
    m[pick > 0.8] = 1.0
    return l, s, z, m


def _launch(dev, shape, l, s, z, m, counter, table=TABLE):
    """through the wrapper, on the 5-D view [1, n, c, 1, hw]; returns (result on the host, the counter after the launch)"""
    n, c, hw = shape
    lat = l.to(dev).view(1, n, c, 1, hw).clone()
    idx = torch.tensor([counter], dtype=torch.int32, device=dev)
    out = pkg().kernels.masked_renoise(lat, s.to(dev).view(1, n, c, 1, hw), z.to(dev).view(1, n, c, 1, hw), m.to(dev).view(1, n, 1, 1, hw),
                                       torch.tensor(table, dtype=torch.float32, device=dev), idx)
    assert out is lat
    return lat.cpu().view(n, c, hw), int(idx.item())


# ---------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_reference_and_the_row_follows_the_counter(dev, shape):
    l, s, z, m = _operands(shape)
    table = torch.tensor(TABLE, dtype=torch.float32)
    results = {}
    for counter, row in ((0, 0), (2, 2), (9, 3), (-4, 0)):          # the first row, a middle row, past the table and below it: clamped
        got, after = _launch(dev, shape, l, s, z, m, counter)
        assert after == counter, "the kernel advanced the step counter"
        a, b = table[row]
        worst, ok = R.check_blend(got, l, s, z, m, a, b)
        print(f"masked_renoise {shape} counter {counter} -> row {row}: worst |err| / bound {worst:.3f}")
        assert ok, f"counter {counter}: worst |err| / bound = {worst}"
        results[counter] = got
    assert torch.equal(bits(results[-4]), bits(results[0]))
    # the bound tells a right result from two wrong ones: the neighbouring pixel's mask, the next table row
    a, b = table[2]
    wrong_mask = R.blend(l, s, z, torch.roll(m, 1, dims=-1), float(a), float(b))
    wrong_row = R.blend(l, s, z, m, float(table[3][0]), float(table[3][1]))
    for wrong in (wrong_mask, wrong_row):
        worst, ok = R.check_blend(wrong, l, s, z, m, a, b)
        assert not ok and worst > 100, worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_exact_cases(dev, shape):
    l, s, z, m = _operands(shape, seed=13)
    special = torch.tensor([0.0, -0.0, 1e-42, -1e-42, 3.4e38, -3.4e38, 1.0, -1.0])       # zeros, subnormals, the largest
    l[0, 0, :8], s[-1, -1, -8:] = special, special
    inf = torch.full_like(z, float("inf"))
    # m == 1 everywhere: the latent's bits, whatever source and noise hold
    got, _ = _launch(dev, shape, l, inf, -inf, torch.ones_like(m), 1)
    assert torch.equal(bits(got), bits(l)), "m == 1 does not keep the latent's bits"
    # m == 0 at the row (1, 0): the source's bits, whatever the latents and the noise hold
    for counter in (0, -1):
        got, _ = _launch(dev, shape, inf, s, -inf, torch.zeros_like(m), counter)
        assert torch.equal(bits(got), bits(s)), "m == 0 at row 0 is not the source's bits"
    # a binary mask at row 0: each element is one or the other
    binary = (m >= 0.5).float()
    got, _ = _launch(dev, shape, l, s, z, binary, 0)
    assert torch.equal(bits(got), bits(torch.where(binary.bool().expand_as(l), l, s)))


GUARD = 64          # fp32 values of poison on either side of the latents


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_stays_inside_the_latents_and_is_deterministic(dev, shape):
    """through the ABI with the test's own buffers: poisoned guard bands before and after the latents stay intact, the inputs are not
    written, the counter is unchanged, and two launches on equal inputs are bit-equal"""
    K, L = pkg().kernels, pkg()._lib
    l, s, z, m = _operands(shape, seed=17)
    n, c, hw = shape
    numel = n * c * hw
    d_s, d_z, d_m = s.to(dev), z.to(dev), m.to(dev)
    table, idx = torch.tensor(TABLE, dtype=torch.float32, device=dev), torch.tensor([1], dtype=torch.int32, device=dev)
    outs = []
    for _ in range(2):
        buf = torch.full((numel + 2 * GUARD,), 777.0, dtype=torch.float32, device=dev)
        lat = buf[GUARD: GUARD + numel]
        lat.copy_(l.reshape(-1))
        L.check(L.load().i2v_masked_renoise_f32(lat.data_ptr(), d_s.data_ptr(), d_z.data_ptr(), d_m.data_ptr(), table.data_ptr(), len(TABLE),
                                                idx.data_ptr(), n, c, hw, K._stream()), "i2v_masked_renoise_f32")
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool((host[:GUARD] == 777.0).all()) and bool((host[GUARD + numel:] == 777.0).all()), "written outside the latents"
        outs.append(host[GUARD: GUARD + numel])
    assert torch.equal(bits(outs[0]), bits(outs[1]))
    assert not torch.equal(outs[0], l.reshape(-1))
    assert int(idx.item()) == 1 and torch.equal(d_s.cpu(), s) and torch.equal(d_z.cpu(), z) and torch.equal(d_m.cpu(), m)
    assert R.check_blend(outs[0].view(n, c, hw), l, s, z, m, *TABLE[1])[1]


def test_wrapper_refusals(dev):
    K = pkg().kernels
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
    lat, mask, coef, idx = z(1, 2, 4, 5, 7), z(1, 2, 1, 5, 7), z(3, 2), z(1, dtype=torch.int32)
    assert K.masked_renoise(lat, z(1, 2, 4, 5, 7), z(1, 2, 4, 5, 7), mask, coef, idx) is lat
    with pytest.raises(ValueError, match="must have the latents' shape"):
        K.masked_renoise(lat, z(1, 2, 4, 5, 8), z(1, 2, 4, 5, 7), mask, coef, idx)
    with pytest.raises(ValueError, match="mask must be"):
        K.masked_renoise(lat, z(1, 2, 4, 5, 7), z(1, 2, 4, 5, 7), z(1, 2, 4, 5, 7), coef, idx)
    with pytest.raises(ValueError, match=r"coef must be \[rows >= 1, 2\]"):
        K.masked_renoise(lat, z(1, 2, 4, 5, 7), z(1, 2, 4, 5, 7), mask, z(3, 4), idx)
    with pytest.raises(ValueError, match="contiguous"):
        K.masked_renoise(lat, z(1, 2, 4, 5, 14)[..., ::2], z(1, 2, 4, 5, 7), mask, coef, idx)
    with pytest.raises(TypeError, match="float32"):
        K.masked_renoise(lat.half(), z(1, 2, 4, 5, 7), z(1, 2, 4, 5, 7), mask, coef, idx)
    with pytest.raises(TypeError, match="int32"):
        K.masked_renoise(lat, z(1, 2, 4, 5, 7), z(1, 2, 4, 5, 7), mask, coef, idx.long())
    with pytest.raises(pkg()._lib.HipLibraryError, match="overlaps"):
        K.masked_renoise(lat, lat, z(1, 2, 4, 5, 7), mask, coef, idx)


# ---------------------------------------------------------------------------------------------------------- the pipeline
FRAMES, HW = 3, 16


@pytest.fixture(scope="module")
def small(dev):
    ou = oracle_small_unet()
    return ou, hip_unet_from_oracle(ou, dev)


def _problem(seed=31, frames=FRAMES, hw=HW):
    g = torch.Generator().manual_seed(seed)
    kw = dict(prompt_embeds=h16(torch.randn(1, 7, 64, generator=g)), negative_prompt_embeds=h16(torch.randn(1, 7, 64, generator=g)),
              condition_image_latents=torch.randn(1, 4, hw, hw, generator=g), num_frames=frames, guidance_scale=7.5, output_type="latent")
    return kw, torch.randn(1, frames, 4, hw, hw, generator=g)


def _gens():
    return dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _noise(frames=FRAMES, hw=HW):
    """the initial noise of a call under `_gens()`: the prior's draw, from `prior_noise_generator`"""
    return torch.randn((1, frames, 4, hw, hw), generator=torch.Generator().manual_seed(7), dtype=torch.float32)


def _half_mask(hw=HW):
    m = torch.zeros(hw, hw)
    m[:, hw // 2:] = 1.0           # the right half is regenerated, the left half keeps the source
    return m


def _sched(kind):
    p = pkg()
    return {"ddim": p.DDIMScheduler, "dpmsolver++": p.DPMSolverMultistepScheduler, "lcm": p.LCMScheduler}[kind]()


def test_prepare_video_latents_against_the_reference(dev, small):
    pipe = pkg().I2VAdapterPipeline(unet=small[1])
    _, src = _problem()
    noise = _noise()
    ac = R.alphas_cumprod()
    for t in (999, 481, 1):
        keep = src.to(dev)
        got = pipe.prepare_video_latents(keep, noise.to(dev), torch.tensor(t)).cpu()
        assert torch.equal(keep.cpu(), src), "the source was overwritten: the blend needs it again"
        sa, sb = R.noise_level(ac, t)
        ref = sa * src.double() + sb * noise.double()
        bound = 2 * R.EPS32 * ((sa * src.double()).abs() + (sb * noise.double()).abs())
        assert bool(((got.double() - ref).abs() <= bound).all())
        assert bool(((R.initial_latents(src, noise, ac, t).double() - ref).abs() <= bound).all())       # (the fp32 restatement too)


@pytest.fixture(scope="module")
def reference_runs(small):
    """the reference loop on the oracle UNet, once: 3 of 4 DDIM steps (strength 0.75), without and with the half-plane mask, with the
    latents after every step"""
    ou = small[0]
    kw, src = _problem()
    noise = _noise()
    runs = {}
    for name, mask in (("plain", None), ("masked", _half_mask()[None, None, None].expand(1, FRAMES, 1, HW, HW))):
        seen = {}
        out = R.sample(ou, kw["prompt_embeds"], kw["negative_prompt_embeds"], kw["condition_image_latents"], src, noise, 4, 0.75,
                       guidance_scale=7.5, mask=mask, callback=lambda i, t, lat: seen.__setitem__(i, (int(t), lat)))
        runs[name] = (out, seen)
    return runs


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_trajectory_against_the_reference_loop(dev, small, reference_runs, masked):
    kw, src = _problem()
    ref, _ = reference_runs["masked" if masked else "plain"]
    extra = dict(mask_image=_half_mask()) if masked else {}
    pipe = pkg().I2VAdapterPipeline(unet=small[1])
    got = pipe(**kw, video_latents=src, num_inference_steps=4, strength=0.75, **extra, **_gens()).frames
    assert got.shape == (1, FRAMES, 4, HW, HW) and torch.equal(got[:, 0].cpu(), kw["condition_image_latents"])
    err, scale = compare(got, ref, rel=REL_TOL_TRAJECTORY, name=f"video-to-video DDIM trajectory (3 of 4 steps, masked={masked})")
    print(f"video-to-video trajectory masked={masked}: max abs err {err:.3e} (max|ref| {scale:.3e}, rel {err / scale:.3e})")
    # the source reaches the result: another clip, another trajectory; and it is not the prior's trajectory
    other = pipe(**kw, video_latents=src.flip(1), num_inference_steps=4, strength=0.75, **extra, **_gens()).frames
    prior = pipe(**kw, num_inference_steps=4, **_gens()).frames
    assert (other - got).abs().max().item() > 10 * REL_TOL_TRAJECTORY * scale
    assert (prior - got).abs().max().item() > 10 * REL_TOL_TRAJECTORY * scale


@pytest.mark.parametrize("kind", ["ddim", "dpmsolver++", "lcm"])
def test_graph_equals_eager_with_a_mask(dev, small, kind):
    kw, src = _problem()
    if kind == "lcm":
        kw["guidance_scale"] = 1.5
    pipe = pkg().I2VAdapterPipeline(unet=small[1], scheduler=_sched(kind))
    call = lambda **k: pipe(**kw, video_latents=src, num_inference_steps=4, strength=0.75, **k, **_gens()).frames
    graph = call(mask_image=_half_mask())
    eager = call(mask_image=_half_mask(), use_graph=False)
    assert torch.isfinite(graph).all() and torch.equal(graph, eager)
    assert len(pipe._graph_cache) == 1, "the masked step did not stay one captured graph"
    assert not torch.equal(graph, call()), "the mask does not reach the result"
    # the kept half of the frames behind the first is the source, bit for bit, under every scheduler
    assert torch.equal(bits(graph[:, 1:, :, :, : HW // 2].cpu()), bits(src[:, 1:, :, :, : HW // 2]))


def test_mask_of_ones_is_the_call_without_a_mask_and_mask_of_zeros_returns_the_source(dev, small):
    kw, src = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=small[1])
    call = lambda **k: pipe(**kw, video_latents=src, num_inference_steps=3, strength=1.0, **k, **_gens()).frames
    plain = call()
    assert torch.equal(call(mask_image=torch.ones(HW, HW)), plain)
    assert torch.equal(call(mask_image=torch.ones(HW, HW), use_graph=False), plain)
    kept = call(mask_image=torch.zeros(HW, HW)).cpu()
    assert torch.equal(bits(kept[:, 1:]), bits(src[:, 1:])), "mask == 0 does not return the source latents"
    assert torch.equal(kept[:, 0], kw["condition_image_latents"])
    # a soft mask at the latent resolution is taken as it is: neither of the two
    soft = call(mask_image=torch.full((FRAMES, 1, HW, HW), 0.5))
    assert torch.isfinite(soft).all() and not torch.equal(soft, plain) and not torch.equal(soft[:, 1:].cpu(), src[:, 1:])
    # without a condition image the source's first frame is the condition
    kw2 = {k: v for k, v in kw.items() if k != "condition_image_latents"}
    first = pipe(**kw2, video_latents=src, num_inference_steps=3, **_gens()).frames
    assert torch.equal(first[:, 0].cpu(), src[:, 0])


def test_the_kept_half_follows_add_noise_at_every_step(dev, small, reference_runs):
    """through `callback`: after step i the kept half of the frames behind the first is add_noise(source, noise, t_{i+1}) within the
    kernel's bound, after the last step the source bit for bit; the regenerated half follows the reference loop"""
    kw, src = _problem()
    noise = _noise()
    ref, ref_seen = reference_runs["masked"]
    pipe = pkg().I2VAdapterPipeline(unet=small[1])
    seen = {}
    out = pipe(**kw, video_latents=src, num_inference_steps=4, strength=0.75, mask_image=_half_mask(),
               callback=lambda i, t, lat: seen.__setitem__(i, (int(t), lat.detach().cpu().clone())), **_gens()).frames.cpu()
    assert sorted(seen) == [0, 1, 2] and [seen[i][0] for i in range(3)] == [ref_seen[i][0] for i in range(3)]
    ac = R.alphas_cumprod()
    ts = [seen[i][0] for i in range(3)]
    half = (slice(None), slice(1, None), slice(None), slice(None), slice(0, HW // 2))
    s64, n64 = src[half].double(), noise[half].double()
    for i in range(2):
        a, b = R.noise_level(ac, ts[i + 1])
        want = a * s64 + b * n64
        bound = 4 * R.EPS32 * ((a * s64).abs() + (b * n64).abs())
        err = (seen[i][1][half].double() - want).abs()
        assert bool((err <= bound).all()), f"after step {i}: worst |err| / bound {float((err / bound).max())}"
        compare(seen[i][1], ref_seen[i][1], rel=REL_TOL_TRAJECTORY, name=f"masked video-to-video, latents after step {i}")
    assert torch.equal(bits(seen[2][1][half]), bits(src[half])) and torch.equal(bits(out[half]), bits(src[half]))
    graph = pipe(**kw, video_latents=src, num_inference_steps=4, strength=0.75, mask_image=_half_mask(), **_gens()).frames.cpu()
    assert torch.equal(graph, out)


def test_strength_decides_the_number_of_unet_forwards(dev, small):
    kw, src = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=small[1])
    for strength, steps in ((0.5, 2), (None, 3), (1.0, 4)):             # None is 0.8: int(4 * 0.8) = 3
        seen = []
        pipe(**kw, video_latents=src, num_inference_steps=4, strength=strength, callback=lambda i, t, lat: seen.append(int(t)), **_gens())
        pipe.scheduler.set_timesteps(4)
        assert seen == [int(t) for t in pipe.scheduler.timesteps[4 - steps:]], (strength, seen)


def test_a_video_call_replays_the_plain_calls_graph_and_a_masked_call_captures_once(dev, small):
    kw, src = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=small[1])
    pipe(**kw, num_inference_steps=3, **_gens())
    plain_graph = pipe._graph
    assert plain_graph is not None
    video = pipe(**kw, video_latents=src, num_inference_steps=3, strength=1.0, **_gens()).frames
    assert pipe._graph is plain_graph and len(pipe._graph_cache) == 1, "a source clip without a mask re-captured the step"
    assert torch.equal(video, pipe(**kw, video_latents=src, num_inference_steps=3, strength=1.0, use_graph=False, **_gens()).frames)
    first = pipe(**kw, video_latents=src, num_inference_steps=3, strength=1.0, mask_image=_half_mask(), **_gens()).frames
    masked_graph = pipe._graph
    assert masked_graph is not plain_graph and len(pipe._graph_cache) == 1
    kw2, src2 = _problem(seed=77)
    mask2 = _half_mask().t().contiguous()
    again = pipe(**kw2, video_latents=src2, num_inference_steps=3, strength=1.0, mask_image=mask2, **_gens()).frames
    assert pipe._graph is masked_graph and len(pipe._graph_cache) == 1, "a second masked sample of the same shape re-captured the step"
    eager = pipe(**kw2, video_latents=src2, num_inference_steps=3, strength=1.0, mask_image=mask2, use_graph=False, **_gens()).frames
    assert torch.equal(again, eager) and not torch.equal(again, first)
    assert torch.equal(bits(again[:, 1:, :, : HW // 2].cpu()), bits(src2[:, 1:, :, : HW // 2]))       # the second mask keeps the upper half


# ---------------------------------------------------------------------------------------------------------- encode_video
def _frames(n, hw, seed=3):
    return torch.rand(n, 3, hw, hw, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("tiny", [False, True], ids=["AutoencoderKL", "AutoencoderTiny"])
def test_encode_video_and_the_first_frame_as_condition(dev, small, tiny):
    p = pkg()
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    if tiny:
        from tests import taesd_reference as TR
        vae = p.AutoencoderTiny()
        vae.load_state_dict(TR.seeded_reference(0).state_dict())
        vae = vae.to(dev).eval()
    else:
        vae = init_random_weights_(p.AutoencoderKL(block_out_channels=(32, 64, 64, 64), norm_num_groups=8), seed=2).to(dev, f16).eval()
    pipe = p.I2VAdapterPipeline(vae=vae, unet=small[1])
    frames = _frames(FRAMES, 64)
    sf = vae.config["scaling_factor"]
    got = pipe.encode_video(frames, 64, 64, generator=torch.Generator().manual_seed(5))
    assert got.shape == (1, FRAMES, 4, 8, 8) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    pre = pipe.image_processor.preprocess(frames).to(dev)
    encs = [vae.encode(pre[i: i + 1]) for i in range(FRAMES)]
    if tiny:
        want = torch.cat([e.latents for e in encs]) * sf
    else:
        from i2v_adapter_unofficial_amd.vae import DiagonalGaussianDistribution
        moments = torch.cat([e.latent_dist.parameters for e in encs])
        want = DiagonalGaussianDistribution(moments).sample(torch.Generator().manual_seed(5)) * sf       # ONE draw over all frames
    assert torch.equal(got[0], want)
    pipe.enable_vae_slicing()
    assert torch.equal(pipe.encode_video(frames, 64, 64, generator=torch.Generator().manual_seed(5)), got)
    pipe.disable_vae_slicing()
    # PIL frames and a [B, F, 3, H, W] tensor are the same clip; a list of generators draws each sample's frames from its own
    import PIL.Image
    pil = [PIL.Image.fromarray((f.permute(1, 2, 0).numpy() * 255).round().astype("uint8")) for f in frames]
    as_pil = pipe.encode_video(pil, 64, 64, generator=torch.Generator().manual_seed(5))
    quant = torch.stack([torch.from_numpy(np.asarray(im, dtype=np.float32) / 255).permute(2, 0, 1) for im in pil])
    assert torch.equal(as_pil, pipe.encode_video(quant[None], 64, 64, generator=torch.Generator().manual_seed(5)))
    # (frame by frame, so that the encoder sees the same batch -- a batch of 6 frames may take other kernel routes than one of 3)
    pipe.enable_vae_slicing()
    two = pipe.encode_video(torch.stack([frames, frames.flip(0)]), 64, 64, generator=[torch.Generator().manual_seed(5), torch.Generator().manual_seed(9)])
    assert two.shape == (2, FRAMES, 4, 8, 8) and torch.equal(two[0], got[0])
    assert torch.equal(two[1:], pipe.encode_video(frames.flip(0), 64, 64, generator=torch.Generator().manual_seed(9)))
    pipe.disable_vae_slicing()
    # a call with `video=` and no condition image: the source's first frame is the condition.  Draws from `generator`: the video's
    # sample, then prepare_latents'
    kw, _ = _problem()
    kw.pop("condition_image_latents")
    out = pipe(**kw, video=frames, height=64, width=64, num_inference_steps=3, **_gens()).frames
    assert out.shape == (1, FRAMES, 4, 8, 8) and torch.equal(out[:, 0], got[:, 0])
    longer = pipe(**kw, video=torch.cat([frames, frames[:1]]), height=64, width=64, num_inference_steps=3, **_gens()).frames
    assert torch.equal(longer, out), "a frame beyond num_frames was not dropped before the encode"
    by_latents = pipe(**kw, video_latents=got, num_inference_steps=3, **_gens()).frames     # (nothing else of the call reads `generator`)
    assert torch.equal(by_latents, out)


# ---------------------------------------------------------------------------------------------------------- next to the rest
def test_next_to_a_controlnet(dev, small):
    ref = CR.small_reference()
    cn = pkg().ControlNetModel(**CR.small_config())
    cn.load_state_dict(ref.state_dict())
    cn = cn.to(dev, f16).eval()
    kw, src = _problem()
    control = torch.rand(FRAMES, 3, 8 * HW, 8 * HW, generator=torch.Generator().manual_seed(41))
    pipe = pkg().I2VAdapterPipeline(unet=small[1], controlnet=cn)
    call = lambda **k: pipe(**kw, video_latents=src, num_inference_steps=3, strength=1.0, mask_image=_half_mask(), **k, **_gens()).frames
    graph = call(control_image=control)
    eager = call(control_image=control, use_graph=False)
    assert torch.isfinite(graph).all() and torch.equal(graph, eager) and len(pipe._graph_cache) == 1
    assert not torch.equal(graph, call(control_image=control, controlnet_conditioning_scale=0.0)), "the control does not reach the result"
    assert torch.equal(bits(graph[:, 1:, :, :, : HW // 2].cpu()), bits(src[:, 1:, :, :, : HW // 2]))


def test_under_free_noise(dev, small):
    """6 frames with context_length 4: the initial noise is FreeNoise's reschedule of the prior's draw, and the blend re-noises the kept
    region with that same noise"""
    kw, src = _problem(frames=6)
    pipe = pkg().I2VAdapterPipeline(unet=small[1])
    pipe.enable_free_noise(context_length=4, context_stride=2)
    try:
        call = lambda **k: pipe(**kw, video_latents=src, num_inference_steps=3, strength=1.0, **k, **_gens()).frames
        graph = call(mask_image=_half_mask())
        eager = call(mask_image=_half_mask(), use_graph=False)
        plain = call()
    finally:
        pipe.disable_free_noise()
    assert graph.shape == (1, 6, 4, HW, HW) and torch.isfinite(graph).all()
    assert torch.equal(graph, eager) and not torch.equal(graph, plain)
    assert torch.equal(bits(graph[:, 1:, :, :, : HW // 2].cpu()), bits(src[:, 1:, :, :, : HW // 2]))


# ---------------------------------------------------------------------------------------------------------- the driver
def test_eval_driver_with_a_video_and_a_mask(dev, tmp_path, monkeypatch):
    """`--video_column COL --mask_column COL --strength S` on a two-row CSV: a directory of frames with one mask image, an animated GIF
    with a directory of masks"""
    import PIL.Image
    from safetensors.torch import save_file
    import i2v_adapter_unofficial_amd as p
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    from i2v_adapter_unofficial_amd.pipeline_i2v_adapter import I2VAdapterPipeline, main
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
    rs = np.random.RandomState(0)
    img = lambda h, w: PIL.Image.fromarray((rs.rand(h, w, 3) * 255).astype("uint8"))
    data = os.path.join(root, "data")
    for d in ("images", "clip0", "masks1"):
        os.makedirs(os.path.join(data, d))
    for j in range(5):                                    # more frames than the clip needs: the first four in sorted order
        img(48, 80).save(os.path.join(data, "clip0", f"{j:03d}.png"))
    for j in range(4):
        img(64, 64).convert("L").save(os.path.join(data, "masks1", f"{j:03d}.png"))
    gif = [img(64, 64) for _ in range(4)]
    gif[0].save(os.path.join(data, "clip1.gif"), save_all=True, append_images=gif[1:], duration=100, loop=0)
    img(32, 32).convert("L").save(os.path.join(data, "mask0.png"))
    names = ["a cat on a boat", "a dog in the snow"]
    with open(os.path.join(data, "eval.csv"), "w") as f:
        f.write("image_path,name,clip,mask\n")
        for i, (clip, mask) in enumerate((("clip0", "mask0.png"), ("clip1.gif", "masks1"))):
            img(70, 90).save(os.path.join(data, "images", f"{i}.png"))
            f.write(f'images/{i}.png,"{names[i]}",{clip},{mask}\n')
    g = torch.Generator().manual_seed(5)
    save_file({"prompt_embeds": torch.randn(2, 7, 64, generator=g), "negative_prompt_embeds": torch.randn(1, 7, 64, generator=g)},
              os.path.join(root, "embeds.safetensors"))
    seen = []
    call = I2VAdapterPipeline.__call__

    def spy(self, *a, **k):
        mask = k.get("mask_image")
        seen.append((len(k["video"]), k["video"][0].size, k["strength"], k["frame_similarity_sample_ratio"],
                     None if mask is None else (len(mask), mask[0].size) if isinstance(mask, list) else (mask.mode, mask.size)))
        return call(self, *a, **k)
    monkeypatch.setattr(I2VAdapterPipeline, "__call__", spy)
    common = ["--task_name", "demo", "--checkpoint_epoch", "3", "--eval_data_path", os.path.join(data, "eval.csv"),
              "--embeds", os.path.join(root, "embeds.safetensors"), "--model_path", os.path.join(root, "sd"),
              "--motion_adapter_path", os.path.join(root, "motion"), "--checkpoint_root", os.path.join(root, "checkpoint"),
              "--samples_root", os.path.join(root, "samples"), "--num_frames", "4", "--num_inference_steps", "4"]
    assert main(common + ["--video_column", "clip", "--mask_column", "mask", "--strength", "0.5"]) == 0
    assert seen == [(4, (80, 48), 0.5, 1, ("L", (32, 32))), (4, (64, 64), 0.5, 1, (4, (64, 64)))]
    for name in names:
        out = PIL.Image.open(os.path.join(root, "samples", "demo", "epoch_3", f"{name}.gif"))
        assert out.n_frames == 4 and out.size == (64, 64)
    del seen[:]
    assert main(common + ["--video_column", "clip"]) == 0                                  # no mask, the default strength
    assert seen == [(4, (80, 48), None, 1, None), (4, (64, 64), None, 1, None)]
    assert main(common + ["--mask_column", "mask"]) == -1                                  # a mask needs a clip
