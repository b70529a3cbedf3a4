"""ControlNet on the host: the model's state-dict keys against diffusers' list, its config, its refusals, the keep table, the
pipeline's control-image preprocessing and argument errors (all raised before any GPU call), `from_unet`, and the power of the kernel
test's bound (tests/test_controlnet_gpu.py) to reject wrong evaluations.  No kernel is launched."""
import os

import numpy as np
import pytest
import torch

from tests import controlnet_reference as R
from tests.parity import GOLDEN_DIR, SMALL_UNET


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _keys(module):
    return sorted(f"{k} {','.join(str(s) for s in v.shape)}" for k, v in module.state_dict().items())


def test_state_dict_keys_are_diffusers():
    p = pkg()
    with torch.device("meta"):
        m = p.ControlNetModel()
        u = p.UNet2DConditionModel()
    golden = open(os.path.join(GOLDEN_DIR, "controlnet_sd15_keys.txt")).read().split("\n")[:-1]
    assert _keys(m) == golden and len(golden) == 340
    assert not any("i2v_adapter" in k or "motion_modules" in k for k in m.state_dict())
    # the down / mid portion coincides with the UNet's keys of the same modules
    shared = ("conv_in.", "time_embedding.", "down_blocks.", "mid_block.")
    assert [k for k in _keys(m) if k.startswith(shared)] == [k for k in _keys(u) if k.startswith(shared)]
    # ... and the reference the GPU tests use carries the same keys (one state dict loads into both)
    small = p.ControlNetModel(**R.small_config())
    assert _keys(small) == _keys(R.small_reference())


def test_config_round_trip(tmp_path):
    p = pkg()
    m = p.ControlNetModel(**R.small_config())
    with torch.no_grad():
        for q in m.parameters():
            q.copy_(torch.randn(q.shape) * 0.1)
    m.save_pretrained(str(tmp_path))
    back = p.ControlNetModel.from_pretrained(str(tmp_path))
    assert dict(back.config) == dict(m.config)
    assert back.config.conditioning_embedding_out_channels == R.SMALL_COND_CHANNELS and back.config.attention_head_dim == 4
    assert back.config.controlnet_conditioning_channel_order == "rgb" and back.config.global_pool_conditions is False
    a, b = m.state_dict(), back.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    # the SD-1.5 defaults are diffusers'
    with torch.device("meta"):
        cfg = pkg().ControlNetModel().config
    assert (cfg.in_channels, cfg.conditioning_channels, cfg.block_out_channels, cfg.layers_per_block) == (4, 3, (320, 640, 1280, 1280), 2)
    assert (cfg.cross_attention_dim, cfg.attention_head_dim, cfg.num_attention_heads, cfg.use_linear_projection) == (768, 8, None, False)
    assert (cfg.norm_num_groups, cfg.norm_eps, cfg.conditioning_embedding_out_channels) == (32, 1e-5, (16, 32, 96, 256))
    assert (cfg.flip_sin_to_cos, cfg.freq_shift, cfg.downsample_padding, cfg.act_fn) == (True, 0, 1, "silu")


@pytest.mark.parametrize("kw,key", [
    (dict(class_embed_type="timestep"), "class_embed_type"), (dict(num_class_embeds=10), "num_class_embeds"),
    (dict(addition_embed_type="text_time"), "addition_embed_type"), (dict(global_pool_conditions=True), "global_pool_conditions"),
    (dict(controlnet_conditioning_channel_order="bgr"), "controlnet_conditioning_channel_order"),
    (dict(only_cross_attention=True), "only_cross_attention"), (dict(only_cross_attention=(False, True, False, False)), "only_cross_attention"),
    (dict(act_fn="gelu"), "act_fn")])
def test_unsupported_config_values_raise_naming_the_key(kw, key):
    with torch.device("meta"):
        with pytest.raises(NotImplementedError, match=key):
            pkg().ControlNetModel(**R.small_config(), **kw)


def test_keep_table():
    keep = pkg().controlnet.controlnet_keep_table
    assert keep(4, 1.0, 0.0, 1.0) == [1.0, 1.0, 1.0, 1.0]
    assert keep(4, 1.0, 0.5, 1.0) == [0.0, 0.0, 1.0, 1.0]           # i / 4 < 0.5 for i = 0, 1
    assert keep(5, 1.0, 0.0, 0.4) == [1.0, 1.0, 0.0, 0.0, 0.0]      # (i + 1) / 5 > 0.4 from i = 2
    assert keep(1, 1.0, 0.0, 1.0) == [1.0]
    assert keep(4, 0.5, 0.5, 1.0) == [0.0, 0.0, 0.5, 0.5] and keep(3, 0.0) == [0.0, 0.0, 0.0]
    for start, end in ((0.5, 0.5), (0.6, 0.4), (-0.1, 1.0), (0.0, 1.1)):
        with pytest.raises(ValueError, match="start"):
            keep(4, 1.0, start, end)


def _cpu_pipe(controlnet=True):
    p = pkg()
    unet = p.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    cn = p.ControlNetModel(**R.small_config()) if controlnet else None
    return p.I2VAdapterPipeline(unet=unet, controlnet=cn)


def test_control_image_preprocessing():
    import PIL.Image
    pipe = _cpu_pipe()
    rs = np.random.RandomState(0)
    imgs = [PIL.Image.fromarray((rs.rand(40, 56, 3) * 255).astype("uint8")) for _ in range(3)]
    t = pipe.prepare_control_image(imgs, 2, 3, 32, 48)
    assert t.shape == (6, 3, 32, 48) and t.dtype == torch.float32
    assert 0.0 <= t.min().item() and t.max().item() <= 1.0 and t.mean().item() > 0.3          # [0, 1]: not normalised to [-1, 1]
    assert torch.equal(t[:3], t[3:])                                                        # one clip shared by the batch
    same = pipe.prepare_control_image([im.resize((48, 32), PIL.Image.LANCZOS) for im in imgs], 1, 3, 32, 48)
    assert torch.equal(same, t[:3])                                                         # resized by the image processor
    f = torch.rand(3, 3, 32, 48)
    assert torch.equal(pipe.prepare_control_image(f, 2, 3, 32, 48), torch.cat([f, f]))
    bf = torch.rand(2, 3, 3, 32, 48)
    assert torch.equal(pipe.prepare_control_image(bf, 2, 3, 32, 48), bf.reshape(6, 3, 32, 48))
    with pytest.raises(ValueError, match="frames"):
        pipe.prepare_control_image(imgs[:2], 1, 3, 32, 48)
    with pytest.raises(ValueError, match="batch"):
        pipe.prepare_control_image(bf, 3, 3, 32, 48)
    with pytest.raises(ValueError, match="already be 32 x 48"):
        pipe.prepare_control_image(torch.rand(3, 3, 16, 48), 1, 3, 32, 48)


def test_argument_errors_come_before_any_gpu_call():
    """every ControlNet argument error is raised on the host with the models on the CPU; only a valid call reaches the no-CPU-path
    error (the order tests/test_clip_text.py checks for the prompt arguments)"""
    p = pkg()
    g = torch.Generator().manual_seed(0)
    kw = dict(prompt_embeds=torch.randn(1, 7, 64, generator=g), negative_prompt_embeds=torch.randn(1, 7, 64, generator=g),
              condition_image_latents=torch.randn(1, 4, 16, 16, generator=g), num_frames=2, num_inference_steps=3)
    frames = torch.rand(2, 3, 128, 128, generator=g)
    pipe = _cpu_pipe()
    with pytest.raises(ValueError, match="`control_image` is required"):
        pipe(**kw)
    with pytest.raises(ValueError, match="holds 3 frames"):
        pipe(**kw, control_image=torch.rand(3, 3, 128, 128))
    with pytest.raises(ValueError, match="holds 1 frames"):
        pipe(**kw, control_image=[frames[0]])
    with pytest.raises(NotImplementedError, match="guess_mode"):
        pipe(**kw, control_image=frames, guess_mode=True)
    for start, end in ((0.5, 0.5), (0.7, 0.2), (-0.5, 1.0), (0.0, 1.5)):
        with pytest.raises(ValueError, match="start"):
            pipe(**kw, control_image=frames, control_guidance_start=start, control_guidance_end=end)
    with pytest.raises(ValueError, match="no `controlnet`"):
        _cpu_pipe(controlnet=False)(**kw, control_image=frames)
    with pytest.raises(NotImplementedError, match="list of ControlNets"):
        p.I2VAdapterPipeline(unet=pipe.unet, controlnet=[pipe.controlnet, pipe.controlnet])
    with pytest.raises(p.HipLibraryError, match="no CPU fallback"):
        pipe(**kw, control_image=frames)
    with pytest.raises(NotImplementedError, match="guess_mode"):
        pipe.controlnet(torch.zeros(2, 4, 16, 16), 1, torch.zeros(1, 7, 64), frames, guess_mode=True)
    # the C handle and the trainer refuse a ControlNet by name
    from i2v_adapter_unofficial_amd import handle
    for fn, args in ((handle.record_step_plan, (pipe, {})), (handle.record_prepare_plan, (pipe, {}))):
        with pytest.raises(NotImplementedError, match="ControlNet"):
            fn(*args)
    with pytest.raises(NotImplementedError, match="ControlNet"):
        handle.export_denoiser(pipe, "unused", num_frames=2, latent_height=16, latent_width=16)


def test_from_unet_copies_the_shared_keys_and_leaves_the_zero_convs_zero():
    p = pkg()
    torch.manual_seed(3)
    sources = [p.UNetMotionCrossFrameAttnModel(**SMALL_UNET),
               p.UNet2DConditionModel(block_out_channels=SMALL_UNET["block_out_channels"], attention_head_dim=4, norm_num_groups=8,
                                      cross_attention_dim=64)]
    for unet in sources:
        cn = p.ControlNetModel.from_unet(unet, conditioning_embedding_out_channels=R.SMALL_COND_CHANNELS)
        usd, csd = unet.state_dict(), cn.state_dict()
        shared = [k for k in csd if k.startswith(("conv_in.", "time_embedding.", "down_blocks.", "mid_block."))]
        assert len(shared) == len(csd) - 16 - 26 and all(torch.equal(csd[k], usd[k]) for k in shared)
        assert any(k.startswith("down_blocks.0.attentions.1.transformer_blocks.0.attn2.") for k in shared)
        zero = [k for k in csd if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block.", "controlnet_cond_embedding.conv_out."))]
        assert len(zero) == 2 * 13 + 2 and all(not csd[k].any() for k in zero)
        assert csd["controlnet_cond_embedding.conv_in.weight"].any()
        assert cn.config.attention_head_dim == 4 and cn.config.conditioning_embedding_out_channels == R.SMALL_COND_CHANNELS


def test_kernel_bound_rejects_wrong_evaluations():
    """the bounds the GPU kernel test asserts (tests/test_controlnet_gpu.py's header), on the very tensors it uses: for every
    tensor and every scale it bounds by (s = 1, -0.75; s = 0 is a bit-equality check there), the fp32 evaluation passes and three wrong
    ones fail -- the neighbouring row of the scale table, the residual of the neighbouring tensor, and (precise pair) a dropped `lo`"""
    skips, lows, ress = R.kernel_case()
    for s in R.KERNEL_SCALES:
        table = R.kernel_table(s)
        assert table[R.KERNEL_ROW].item() == s
        if s == 0.0:
            continue
        wrong_s = table[R.KERNEL_ROW - 1].item()
        for i, (hi, lo, r) in enumerate(zip(skips, lows, ress)):
            for precise in (False, True):
                l = lo if precise else None
                ref, bound = R.add_residuals_fp64(hi, r, s, l), R.add_residuals_bound(hi, r, s, l)
                good32 = hi.float() + (lo.float() if precise else 0.0) + torch.tensor(s) * r.float()
                good = good32.half().double() if not precise else good32.half().double() + (good32 - good32.half().float()).half().double()
                assert bool(((good - ref).abs() <= bound).all()), (i, s, precise)
                fails = lambda v: bool(((v - ref).abs() > bound).any())
                assert fails(R.add_residuals_fp64(hi, r, wrong_s, l)), ("neighbouring row", i, s, precise)
                assert fails(R.add_residuals_fp64(hi, R.neighbour_residual(ress, i), s, l)), ("neighbouring residual", i, s, precise)
                if precise:
                    assert fails(R.add_residuals_fp64(hi, r, s, None)), ("dropped lo", i, s)
