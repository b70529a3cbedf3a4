"""The captured step's per-sample inputs on the GPU (small UNet, 2 frames, 16 x 16 latents): a graph-cache hit that replaces EVERY
per-sample input at once, the schedule tables from both of their callers under FreeInit's fast sampling, and the per-call switches
(`precise_stream=`, `cross_attention_kwargs={"scale": s}`), set for one call and restored after it.  Everything is bit equality
between two routes through the same kernels: no tolerance.  The host side is tests/test_pipeline_state.py's."""
import pytest
import torch

from tests import controlnet_reference as CR
from tests import t2i_adapter_reference as R
from tests.parity import hip_unet_from_oracle, oracle_small_unet

pytestmark = pytest.mark.gpu

f16 = torch.float16
FRAMES, HW = 2, 16


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h16(t):
    return t.half().float()


@pytest.fixture(scope="module")
def parts(dev):
    """(HIP UNet, ControlNet, T2I-Adapter) with the small references' weights"""
    hu = hip_unet_from_oracle(oracle_small_unet(), dev)
    cn = pkg().ControlNetModel(**CR.small_config())
    cn.load_state_dict(CR.small_reference().state_dict())
    ad = pkg().T2IAdapter(**R.small_config(3))
    ad.load_state_dict(R.small_reference(3).state_dict())
    return hu, cn.to(dev, f16).eval(), ad.to(dev, f16).eval()


def _sample(seed, guidance=1.5):
    """every per-sample input of a call from one seed: embeds, condition latents, control frames, adapter frames, both scales, source
    clip, mask and the three generators"""
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros(HW, HW)
    mask[:, seed % 5 + 4:] = 1.0
    return dict(prompt_embeds=h16(torch.randn(1, 7, 64, generator=g)), negative_prompt_embeds=h16(torch.randn(1, 7, 64, generator=g)),
                condition_image_latents=torch.randn(1, 4, HW, HW, generator=g), num_frames=FRAMES, guidance_scale=guidance,
                output_type="latent", control_image=torch.rand(FRAMES, 3, 8 * HW, 8 * HW, generator=g),
                adapter_image=torch.rand(FRAMES, 3, 8 * HW, 8 * HW, generator=g),
                controlnet_conditioning_scale=0.5 + seed % 7 / 10, adapter_conditioning_scale=0.4 + seed % 3 / 10,
                generator=torch.Generator().manual_seed(seed + 1), prior_mask_generator=torch.Generator().manual_seed(seed + 2),
                prior_noise_generator=torch.Generator().manual_seed(seed + 3)), \
        dict(video_latents=torch.randn(1, FRAMES, 4, HW, HW, generator=g), mask_image=mask, strength=0.75)


def test_a_cache_hit_replaces_every_per_sample_input(dev, parts):
    """ControlNet + T2I-Adapter + LCM's noise table + a masked source clip in one captured step: sample B differs from sample A in
    every per-sample input and replays A's graph; its result is B's own eager run on a fresh pipeline"""
    hu, cn, ad = parts
    make = lambda: pkg().I2VAdapterPipeline(unet=hu, controlnet=cn, t2i_adapter=ad, scheduler=pkg().LCMScheduler())
    pipe = make()
    a = pipe(**_sample(11)[0], **_sample(11)[1], num_inference_steps=4).frames
    first = pipe._graph
    assert first is not None and len(pipe._graph_cache) == 1
    gst = next(iter(pipe._graph_cache.values()))[1]
    held = {n for n in pkg().pipeline_i2v_adapter.SAMPLE_INPUTS if gst.get(n) is not None}
    assert held == set(pkg().pipeline_i2v_adapter.SAMPLE_INPUTS) - {"ctx_ip"}, "the step does not read every declared input"
    b = pipe(**_sample(24)[0], **_sample(24)[1], num_inference_steps=4).frames
    assert pipe._graph is first and len(pipe._graph_cache) == 1, "a second sample of the same shape re-captured the step"
    eager = make()(**_sample(24)[0], **_sample(24)[1], num_inference_steps=4, use_graph=False).frames
    assert torch.isfinite(b).all() and torch.equal(b, eager), "a replayed graph read something of the previous sample"
    assert not torch.equal(b, a)
    # each of B's inputs reaches the replayed graph on its own: B with one of A's in its place is another result
    for name in ("prompt_embeds", "condition_image_latents", "control_image", "adapter_image", "controlnet_conditioning_scale",
                 "adapter_conditioning_scale", "generator", "prior_noise_generator", "video_latents", "mask_image"):
        kw, clip = _sample(24)
        src = _sample(11)
        (kw if name in kw else clip)[name] = (src[0] if name in src[0] else src[1])[name]
        mixed = pipe(**kw, **clip, num_inference_steps=4).frames
        assert pipe._graph is first and not torch.equal(mixed, b), name


def test_free_init_fast_sampling_with_both_windows_graph_equals_eager(dev, parts):
    """FreeInit's fast sampling gives round 0 two steps and round 1 four: `_schedule_tables` runs from `__call__` and from
    `_free_init_round`, the ControlNet's window 0.0 .. 0.5 and the adapter's factor 0.5 over each round's own step count"""
    hu, cn, ad = parts
    pipe = pkg().I2VAdapterPipeline(unet=hu, controlnet=cn, t2i_adapter=ad, scheduler=pkg().DPMSolverMultistepScheduler())
    pipe.enable_free_init(num_iters=2, use_fast_sampling=True)
    windows = dict(control_guidance_start=0.0, control_guidance_end=0.5, adapter_conditioning_factor=0.5)
    call = lambda **k: pipe(**_sample(11, guidance=7.5)[0], num_inference_steps=4, **windows, **k).frames
    graph = call()
    gst = next(iter(pipe._graph_cache.values()))[1]
    kw = _sample(11)[0]                 # (the cache holds the last round's capture: 4 steps, each table over its first half)
    half = lambda s: torch.tensor([s, s, 0.0, 0.0], dtype=torch.float32)
    assert gst["t_table"].shape == (4,) and torch.equal(gst["cn_scale"].cpu(), half(kw["controlnet_conditioning_scale"]))
    assert torch.equal(gst["t2i_scale"].cpu(), half(kw["adapter_conditioning_scale"]))
    eager = call(use_graph=False)
    assert torch.isfinite(graph).all() and torch.equal(graph, eager)
    whole = pipe(**_sample(11, guidance=7.5)[0], num_inference_steps=4).frames
    assert not torch.equal(graph, whole), "the windows did not reach the steps"
    pipe.disable_free_init()
    assert not torch.equal(call(), graph)


def test_precise_stream_is_set_for_one_call_and_restored(dev, parts):
    from i2v_adapter_unofficial_amd import blocks
    hu = parts[0]
    pipe = pkg().I2VAdapterPipeline(unet=hu)
    kw = {k: v for k, v in _sample(11, guidance=7.5)[0].items() if "control" not in k and "adapter" not in k}
    call = lambda **k: pipe(**dict(kw, **{n: torch.Generator().manual_seed(5) for n in kw if "generator" in n}), num_inference_steps=3, **k)
    was = blocks.precise_stream()
    try:
        for before in (False, True):
            blocks.set_precise_stream(before)
            seen = []
            per_call = call(precise_stream=True, callback=lambda i, t, lat: seen.append(blocks.precise_stream())).frames
            assert seen == [True] * 3 and blocks.precise_stream() is before
            plain = call(precise_stream=False).frames
            assert blocks.precise_stream() is before
            with pytest.raises(ValueError, match="`strength` = 0.5 was passed without a source clip"):
                call(precise_stream=not before, strength=0.5)
            assert blocks.precise_stream() is before, "a call that raised left its stream mode behind"
            blocks.set_precise_stream(True)
            assert torch.equal(call().frames, per_call) and torch.equal(call(precise_stream=None).frames, per_call)
            assert not torch.equal(plain, per_call)
    finally:
        blocks.set_precise_stream(was)


def test_the_lora_scale_is_set_for_one_call_and_restored(dev, parts):
    hu = parts[0]
    pipe = pkg().I2VAdapterPipeline(unet=hu)
    kw = {k: v for k, v in _sample(11, guidance=7.5)[0].items() if "control" not in k and "adapter" not in k}
    was = hu.set_lora_scale(0.75)
    try:
        seen = []
        pipe(**kw, num_inference_steps=3, cross_attention_kwargs={"scale": 0.5, "other": 1},
             callback=lambda i, t, lat: seen.append(hu._lora_state()["scale"]))
        assert seen == [0.5] * 3
        assert hu.set_lora_scale(0.75) == 0.75, "the call's scale stuck"
        with pytest.raises(ValueError, match="`strength` = 0.5 was passed without a source clip"):
            pipe(**kw, num_inference_steps=3, cross_attention_kwargs={"scale": 0.25}, strength=0.5)
        assert hu.set_lora_scale(0.75) == 0.75, "a call that raised left its scale behind"
        pipe(**kw, num_inference_steps=3, cross_attention_kwargs={"scale": None}, precise_stream=False,
             callback=lambda i, t, lat: seen.append(hu._lora_state()["scale"]))
        assert seen[3:] == [0.75] * 3 and hu.set_lora_scale(0.75) == 0.75
    finally:
        hu.set_lora_scale(was)
