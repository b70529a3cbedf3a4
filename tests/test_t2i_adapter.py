"""T2I-Adapter on the host: the model's state-dict keys against the committed list and the torch restatement
(tests/t2i_adapter_reference.py), its config and refusals, the scale table, the pipeline's and the UNet's argument errors (all raised
before any GPU call), the ABI of the four new entry points and their host-side argument checks, the driver's flags.  No kernel is
launched."""
import os
import re

import numpy as np
import pytest
import torch

from tests import t2i_adapter_reference as R
from tests.parity import GOLDEN_DIR, ROOT, SMALL_UNET


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _keys(module):
    return sorted(f"{k} {','.join(str(s) for s in v.shape)}" for k, v in module.state_dict().items())


def test_state_dict_keys_are_the_committed_list_and_the_reference_modules():
    p = pkg()
    with torch.device("meta"):
        m, ref = p.T2IAdapter(), R.T2IAdapter()
    golden = open(os.path.join(GOLDEN_DIR, "t2i_adapter_keys.txt")).read().split("\n")[:-1]
    assert _keys(m) == golden == _keys(ref) and len(golden) == 38
    assert sum(v.numel() for v in m.state_dict().values()) == 77369280                  # the published 77 M
    names = {k.split(" ")[0] for k in golden}
    assert {"adapter.conv_in.weight", "adapter.body.1.in_conv.weight", "adapter.body.2.in_conv.bias",
            "adapter.body.3.resnets.1.block2.weight"} <= names
    assert not any(k.startswith(("adapter.body.0.in_conv", "adapter.body.3.in_conv")) for k in names)      # 320 -> 320, 1280 -> 1280
    for c in (1, 3):
        assert _keys(p.T2IAdapter(**R.small_config(c))) == _keys(R.T2IAdapter(**R.small_config(c)))
    assert p.T2IAdapter(**R.small_config(1)).state_dict()["adapter.conv_in.weight"].shape == (32, 64, 3, 3)


def test_config_defaults_and_round_trip(tmp_path):
    p = pkg()
    with torch.device("meta"):
        cfg = p.T2IAdapter().config
    assert dict(cfg) == dict(in_channels=3, channels=(320, 640, 1280, 1280), num_res_blocks=2, downscale_factor=8,
                             adapter_type="full_adapter")
    torch.manual_seed(0)
    m = p.T2IAdapter(**R.small_config(1))
    assert m.total_downscale_factor == 64 and m.downscale_factor == 8
    for safe in (True, False):                                # diffusion_pytorch_model.safetensors and .bin
        d = str(tmp_path / ("st" if safe else "bin"))
        m.save_pretrained(d, safe_serialization=safe)
        assert sorted(os.listdir(d)) == ["config.json", "diffusion_pytorch_model." + ("safetensors" if safe else "bin")]
        back = p.T2IAdapter.from_pretrained(d)
        assert dict(back.config) == dict(m.config) and back.config.channels == R.SMALL_CHANNELS and back.config.in_channels == 1
        a, b = m.state_dict(), back.state_dict()
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("kw,exc,key", [
    (dict(adapter_type="light_adapter"), NotImplementedError, "adapter_type"),
    (dict(adapter_type="full_adapter_xl"), NotImplementedError, "adapter_type"),
    (dict(adapter_type="other"), ValueError, "adapter_type"),
    (dict(downscale_factor=16), NotImplementedError, "downscale_factor"),
    (dict(in_channels=4), NotImplementedError, "in_channels"),
    (dict(channels=(32, 64, 128)), NotImplementedError, "channels"),
    (dict(channels=(32, 64, 100, 128)), NotImplementedError, "channels"),
    (dict(num_res_blocks=0), ValueError, "num_res_blocks")])
def test_unsupported_config_values_raise_naming_the_key(kw, exc, key):
    with torch.device("meta"):
        with pytest.raises(exc, match=key):
            pkg().T2IAdapter(**{**R.small_config(), **kw})


@pytest.mark.parametrize("n", [1, 4, 25])
@pytest.mark.parametrize("factor", [0.0, 0.5, 1.0])
def test_scale_table_is_diffusers_rule(n, factor):
    """StableDiffusionAdapterPipeline: the features are added on step i when i < int(num_inference_steps * factor)"""
    table = pkg().t2i_adapter.adapter_scale_table
    got = table(n, 0.75, factor)
    assert got == [0.75 if i < int(n * factor) else 0.0 for i in range(n)] and len(got) == n
    assert sum(v != 0 for v in got) == {0.0: 0, 0.5: n // 2, 1.0: n}[factor]
    assert table(n, 0.0, factor) == [0.0] * n and table(n) == [1.0] * n


def test_scale_table_refusals():
    table = pkg().t2i_adapter.adapter_scale_table
    for factor in (-0.1, 1.5):
        with pytest.raises(ValueError, match="factor"):
            table(4, 1.0, factor)
    with pytest.raises(ValueError, match="num_steps"):
        table(0)


def _cpu_pipe(adapter=True, in_channels=3):
    p = pkg()
    unet = p.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    ad = p.T2IAdapter(**R.small_config(in_channels)) if adapter else None
    return p.I2VAdapterPipeline(unet=unet, t2i_adapter=ad)


def test_adapter_image_preprocessing():
    import PIL.Image
    rs = np.random.RandomState(0)
    imgs = [PIL.Image.fromarray((rs.rand(40, 56, 3) * 255).astype("uint8")) for _ in range(3)]
    pipe = _cpu_pipe()
    t = pipe.prepare_adapter_image(imgs, 2, 3, 32, 48)
    assert t.shape == (6, 3, 32, 48) and t.dtype == torch.float32
    assert 0.0 <= t.min().item() and t.max().item() <= 1.0 and t.mean().item() > 0.3          # [0, 1]: not normalised to [-1, 1]
    assert torch.equal(t[:3], t[3:])                                                        # one clip shared by the batch
    # RGB: what the ControlNet path makes of the same images
    assert torch.equal(t, pipe.prepare_control_image(imgs, 2, 3, 32, 48))
    # a 1-channel adapter converts to "L"
    grey = _cpu_pipe(in_channels=1)
    g = grey.prepare_adapter_image(imgs, 1, 3, 32, 48)
    want = torch.stack([torch.from_numpy(np.asarray(im.convert("L").resize((48, 32), PIL.Image.LANCZOS), dtype=np.float32) / 255.0)[None]
                        for im in imgs])
    assert g.shape == (3, 1, 32, 48) and torch.equal(g, want)
    f = torch.rand(3, 1, 32, 48)
    assert torch.equal(grey.prepare_adapter_image(f, 2, 3, 32, 48), torch.cat([f, f]))
    bf = torch.rand(2, 3, 3, 32, 48)
    assert torch.equal(pipe.prepare_adapter_image(bf, 2, 3, 32, 48), bf.reshape(6, 3, 32, 48))
    with pytest.raises(ValueError, match="frames"):
        pipe.prepare_adapter_image(imgs[:2], 1, 3, 32, 48)
    with pytest.raises(ValueError, match="batch"):
        pipe.prepare_adapter_image(bf, 3, 3, 32, 48)
    with pytest.raises(ValueError, match="already be 32 x 48"):
        pipe.prepare_adapter_image(torch.rand(3, 3, 16, 48), 1, 3, 32, 48)
    with pytest.raises(ValueError, match="channels"):
        grey.prepare_adapter_image(torch.rand(3, 3, 32, 48), 1, 3, 32, 48)


def test_pipeline_argument_errors_come_before_any_gpu_call():
    """every T2I-Adapter argument error is raised on the host with the models on the CPU; only a valid call reaches the no-CPU-path
    error"""
    p = pkg()
    g = torch.Generator().manual_seed(0)
    kw = dict(prompt_embeds=torch.randn(1, 7, 64, generator=g), negative_prompt_embeds=torch.randn(1, 7, 64, generator=g),
              condition_image_latents=torch.randn(1, 4, 16, 16, generator=g), num_frames=2, num_inference_steps=3)
    frames = torch.rand(2, 3, 128, 128, generator=g)
    pipe = _cpu_pipe()
    with pytest.raises(ValueError, match="`adapter_image` is required"):
        pipe(**kw)
    with pytest.raises(ValueError, match="holds 3 frames"):
        pipe(**kw, adapter_image=torch.rand(3, 3, 128, 128))
    with pytest.raises(ValueError, match="holds 1 frames"):
        pipe(**kw, adapter_image=[frames[0]])
    with pytest.raises(ValueError, match="1 channels, the adapter's `in_channels` is 3"):
        pipe(**kw, adapter_image=torch.rand(2, 1, 128, 128))
    with pytest.raises(ValueError, match="must be"):
        pipe(**kw, adapter_image=torch.rand(3, 128, 128))
    with pytest.raises(ValueError, match="list of `num_frames` images or a tensor"):
        pipe(**kw, adapter_image="frames.gif")
    for factor in (-0.25, 1.25):
        with pytest.raises(ValueError, match="factor"):
            pipe(**kw, adapter_image=frames, adapter_conditioning_factor=factor)
    with pytest.raises(ValueError, match="no `t2i_adapter`"):
        _cpu_pipe(adapter=False)(**kw, adapter_image=frames)
    with pytest.raises(NotImplementedError, match="MultiAdapter"):
        p.I2VAdapterPipeline(unet=pipe.unet, t2i_adapter=[pipe.t2i_adapter, pipe.t2i_adapter])
    with pytest.raises(p.HipLibraryError, match="no CPU fallback"):
        pipe(**kw, adapter_image=frames)


def test_model_argument_errors():
    p = pkg()
    m = p.T2IAdapter(**R.small_config())
    for fn in (m.forward, m.embed):
        with pytest.raises(ValueError, match=r"\(N, 3, height, width\)"):
            fn(torch.zeros(2, 1, 64, 64))
        with pytest.raises(ValueError, match="multiples of 8"):
            fn(torch.zeros(2, 3, 60, 64))
        with pytest.raises(p.HipLibraryError, match="no CPU fallback"):
            fn(torch.zeros(2, 3, 64, 64))


def _features(batch, hw=(16, 16), channels=SMALL_UNET["block_out_channels"]):
    h, w = hw
    out = []
    for c in channels:
        out.append(torch.zeros(batch, c, h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def test_unet_forward_argument_errors_name_the_level():
    p = pkg()
    unet = p.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    sample, ctx = torch.zeros(2, 2, 4, 16, 16), torch.zeros(2, 7, 64)
    call = lambda feats, s=sample: unet(s, 10, True, ctx, down_intrablock_additional_residuals=feats)
    with pytest.raises(ValueError, match="3 tensors for 4 down blocks"):
        call(_features(4)[:3])
    bad = _features(4)
    bad[2] = torch.zeros(4, 128, 5, 4)
    with pytest.raises(ValueError, match="level 2 takes .*height 4, width 4, channels 128"):
        call(bad)
    bad = _features(4)
    bad[1] = torch.zeros(4, 32, 8, 8)
    with pytest.raises(ValueError, match="level 1 .*channels 64"):
        call(bad)
    with pytest.raises(ValueError, match="level 0 .*dividing the batch 4"):
        call(_features(3))
    bad = _features(4)
    bad[3] = torch.zeros(128, 2, 2)
    with pytest.raises(ValueError, match="level 3 must be"):
        call(bad)
    # an odd latent size: the levels are the ceil halves (9 x 13 -> 5 x 7 -> 3 x 4 -> 2 x 2)
    odd = torch.zeros(2, 2, 4, 9, 13)
    with pytest.raises(ValueError, match="level 1 takes .*height 5, width 7"):
        call(_features(4, hw=(9, 13))[:1] + _features(4, hw=(8, 12))[1:], odd)
    # valid lists (the full batch, B * F of one CFG half, one frame set shared by all) reach the no-CPU-path error
    for feats, s in ((_features(4), sample), (_features(2), sample), (_features(4, hw=(9, 13)), odd)):
        with pytest.raises(p.HipLibraryError, match="no CPU fallback"):
            call(feats, s)
    with pytest.raises(p.HipLibraryError, match="no CPU fallback"):
        unet(sample, 10, True, ctx)


def test_the_c_handle_and_the_trainer_refuse_an_adapter():
    from i2v_adapter_unofficial_amd import handle, training
    pipe = _cpu_pipe()
    for fn, args in ((handle.record_step_plan, (pipe, {})), (handle.record_prepare_plan, (pipe, {}))):
        with pytest.raises(NotImplementedError, match="T2I-Adapter"):
            fn(*args)
    with pytest.raises(NotImplementedError, match="T2I-Adapter"):
        handle.export_denoiser(pipe, "unused", num_frames=2, latent_height=16, latent_width=16)
    tr = training.UNetAdapterTrainer(pipe.unet)
    with pytest.raises(NotImplementedError, match="T2I-Adapter"):
        tr.forward(torch.zeros(1, 2, 4, 16, 16), 10, torch.zeros(1, 7, 64), down_intrablock_additional_residuals=_features(2))


ENTRY_POINTS = ("i2v_pixel_unshuffle8_f16", "i2v_avgpool2x_f16", "i2v_relu_f16", "i2v_add_broadcast_residual_f16")


def test_abi_declares_exports_and_binds_the_four_entry_points():
    lib = pkg()._lib
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 24
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    from i2v_adapter_unofficial_amd import handle as H
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(", src) and name in lib.SIGNATURES and hasattr(h, name)
        assert name not in H.ENTRY_IDS                          # the C handle's plan format is unchanged: it refuses an adapter
    assert len(lib.SIGNATURES["i2v_add_broadcast_residual_f16"][1]) == 11


def test_bad_arguments_are_refused_on_the_host():
    """null / misaligned / mis-sized / overlapping operands return I2V_ERR_INVALID_ARG before anything is launched: callable without
    a GPU (the pointers are never dereferenced)"""
    h = pkg()._lib.load()
    A, B, D, L = 1 << 40, 1 << 41, 1 << 42, 1 << 43

    def refused(fn, args, msg):
        assert fn(*args, None) == -1, args
        assert msg in h.i2v_last_error(), (args, h.i2v_last_error())

    un = h.i2v_pixel_unshuffle8_f16
    for args, msg in (((None, 1, D, 2, 3, 16, 24), b"null"), ((A, 1, None, 2, 3, 16, 24), b"null"), ((A, 1, D, 2, 2, 16, 24), b"c 2"),
                      ((A, 1, D, 0, 3, 16, 24), b"n 0"), ((A, 1, D, 2, 3, 12, 24), b"multiples of 8"), ((A, 0, D, 2, 1, 16, 20), b"multiples of 8"),
                      ((A, 1, D, 2, 3, 0, 24), b"multiples of 8"), ((A + 8, 1, D, 2, 3, 16, 24), b"16-byte"), ((A, 0, D + 2, 2, 3, 16, 24), b"16-byte"),
                      ((A, 1, A + 1024, 2, 3, 16, 24), b"overlaps")):
        refused(un, args, msg)
    pool = h.i2v_avgpool2x_f16
    for args, msg in (((None, D, 2, 5, 7, 32), b"null"), ((A, None, 2, 5, 7, 32), b"null"), ((A, D, 2, 5, 7, 12), b"multiple of 8"),
                      ((A, D, 2, 5, 7, 0), b"multiple of 8"), ((A, D, 2, 0, 7, 32), b"h 0"), ((A, D, 0, 5, 7, 32), b"n 0"),
                      ((A + 4, D, 2, 5, 7, 32), b"16-byte"), ((A, D + 8, 2, 5, 7, 32), b"16-byte"), ((A, A, 2, 5, 7, 32), b"overlaps")):
        refused(pool, args, msg)
    relu = h.i2v_relu_f16
    for args, msg in (((None, D, 64), b"null"), ((A, None, 64), b"null"), ((A, D, 60), b"multiple of 8"), ((A, D, 0), b"multiple of 8"),
                      ((A + 2, D, 64), b"16-byte"), ((A, D + 8, 64), b"16-byte"), ((A, A + 16, 64), b"without being it")):
        refused(relu, args, msg)
    add = h.i2v_add_broadcast_residual_f16
    ok = dict(x=A, x_lo=None, feat=B, dst=D, dst_lo=None, numel=4200 * 2, feat_numel=4200, table=None, rows=0, idx=None)

    def add_args(**kw):
        return tuple({**ok, **kw}.values())

    for kw, msg in ((dict(x=None), b"null"), (dict(feat=None), b"null"), (dict(dst=None), b"null"), (dict(x_lo=L), b"come together"),
                    (dict(dst_lo=L), b"come together"), (dict(numel=0), b"numel 0"), (dict(feat_numel=0), b"positive multiple of 8"),
                    (dict(feat_numel=4196, numel=8392), b"positive multiple of 8"), (dict(numel=4200 * 2 + 8), b"not a multiple of feat_numel"),
                    (dict(numel=4200 // 2), b"not a multiple of feat_numel"), (dict(x=A + 8), b"16-byte"), (dict(feat=B + 2), b"16-byte"),
                    (dict(dst=D + 4), b"16-byte"), (dict(x_lo=L + 8, dst_lo=L + (1 << 20)), b"16-byte"), (dict(table=L, rows=0), b"0 rows"),
                    (dict(table=L + 2, rows=3), b"4-byte"), (dict(idx=L + 1), b"4-byte"), (dict(x_lo=L, dst_lo=D), b"same memory"),
                    (dict(dst=B), b"overlaps feat"), (dict(dst=B + 4200 * 2 - 16), b"overlaps feat"), (dict(x_lo=L, dst_lo=B), b"overlaps feat")):
        refused(add, add_args(**kw), msg)


def test_driver_flags_parse():
    parser = pkg().pipeline_i2v_adapter.build_parser()
    a = parser.parse_args(["--task_name", "t"])
    assert (a.t2i_adapter, a.adapter_column, a.adapter_scale, a.adapter_factor) == (None, None, 1.0, 1.0)
    a = parser.parse_args(["--task_name", "t", "--t2i_adapter", "/models/t2iadapter_depth_sd15v2", "--adapter_column", "depth",
                           "--adapter_scale", "0.8", "--adapter_factor", "0.5", "--controlnet", "/models/cn", "--control_column", "pose"])
    assert (a.t2i_adapter, a.adapter_column, a.adapter_scale, a.adapter_factor) == ("/models/t2iadapter_depth_sd15v2", "depth", 0.8, 0.5)
    assert (a.controlnet, a.control_column) == ("/models/cn", "pose")
