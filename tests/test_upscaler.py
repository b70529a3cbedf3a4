"""The Real-ESRGAN compact upscaler (upscaler.SRVGGNetCompact) without a GPU: state-dict keys against the plain-torch restatement and
the committed key list, every load format, the inferred configuration and the refusals, the ABI of the new entry points and their
host-side argument checks, the pipeline's host logic, the driver's flags, and what the GPU gates rely on -- `exit_fp64` is
PixelShuffle + nearest base, and the per-element bounds REJECT the wrong evaluations of every kernel case."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_bounds as B
from tests import srvgg_reference as R
from tests.parity import SMALL_UNET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def U():
    return pkg().upscaler


# ------------------------------------------------------------------------------------------------------------- keys and files
def _golden():
    out, cur = {}, None
    for line in open(os.path.join(ROOT, "tests", "golden", "srvgg_keys.txt")).read().split():
        if line.startswith("[num_conv="):
            cur = out.setdefault(int(line[len("[num_conv="):-1]), [])
        else:
            cur.append(line)
    return out


@pytest.mark.parametrize("num_conv", (16, 32))
def test_state_dict_keys_are_the_restatements_and_the_committed_list(num_conv):
    with torch.device("meta"):
        keys = list(pkg().SRVGGNetCompact(num_conv=num_conv).state_dict().keys())
        ref = R.SRVGGReference(num_conv=num_conv)
    assert keys == list(ref.state_dict().keys()) == _golden()[num_conv] and len(keys) == 3 * (num_conv + 1) + 2
    shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    last = 2 * (num_conv + 1)
    assert shapes["body.0.weight"] == (64, 3, 3, 3) and shapes[f"body.{last}.weight"] == (48, 64, 3, 3) and shapes["body.1.weight"] == (64,)
    assert "body.1.bias" not in shapes and f"body.{last}.bias" in shapes and not any(k.startswith("upsampler") for k in shapes)


def test_every_load_format_and_the_round_trip(tmp_path):
    from safetensors.torch import save_file
    ref = R.seeded_reference(2, 2, seed=3)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    S = pkg().SRVGGNetCompact
    torch.save({"params_ema": state, "params": {"junk": torch.zeros(1)}}, str(tmp_path / "ema.pth"))      # params_ema first
    torch.save({"params": state}, str(tmp_path / "params.pth"))
    torch.save(state, str(tmp_path / "bare.pt"))
    save_file({k: v.contiguous() for k, v in state.items()}, str(tmp_path / "m.safetensors"))
    for src in (str(tmp_path / "ema.pth"), str(tmp_path / "params.pth"), str(tmp_path / "bare.pt"), str(tmp_path / "m.safetensors"), state,
                {"params_ema": state}):
        m = S.from_pretrained(src)
        assert (m.num_conv, m.upscale, m.act_type, m.training) == (2, 2, "prelu", False)
        assert all(torch.equal(m.state_dict()[k], v) for k, v in state.items()) and list(m.state_dict()) == list(state)
    m.save_pretrained(str(tmp_path / "again" / "up.safetensors"))
    again = S.from_pretrained(str(tmp_path / "again" / "up.safetensors"))
    assert all(torch.equal(again.state_dict()[k], v) for k, v in state.items())
    with pytest.raises(ValueError, match="safetensors"):
        m.save_pretrained(str(tmp_path / "up.pth"))
    with pytest.raises(EnvironmentError):
        S.from_pretrained(str(tmp_path / "missing.pth"))
    # a dict without PReLU weights says nothing about its activation
    bare = {k: v for k, v in state.items() if v.dim() != 1 or k.endswith("bias")}
    with pytest.raises(ValueError, match="act_type='relu' or 'leakyrelu'"):
        S.from_pretrained(bare)
    for act, cls in (("relu", torch.nn.ReLU), ("leakyrelu", torch.nn.LeakyReLU)):
        m = S.from_pretrained(bare, act_type=act)
        assert m.act_type == act and isinstance(m.body[1], cls) and list(m.state_dict()) == list(bare)
    assert m.body[1].negative_slope == 0.1
    with pytest.raises(ValueError, match="holds PReLU weights"):
        S.from_pretrained(state, act_type="relu")


@pytest.mark.parametrize("num_conv,upscale", ((16, 4), (32, 4), (0, 1), (5, 3)))
def test_the_configuration_is_inferred_from_keys_and_shapes(num_conv, upscale):
    with torch.device("meta"):
        state = R.SRVGGReference(num_conv=num_conv, upscale=upscale).state_dict()
    assert U().infer_config(state) == dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=num_conv, upscale=upscale, act_type="prelu")


def test_refusals_name_the_value():
    S = pkg().SRVGGNetCompact
    with torch.device("meta"):
        for kw, msg in ((dict(num_feat=32), "num_feat=32"), (dict(num_in_ch=1), "num_in_ch=1"), (dict(num_out_ch=4), "num_out_ch=4"),
                        (dict(upscale=5), "upscale=5"), (dict(upscale=0), "upscale=0"), (dict(act_type="gelu"), "act_type='gelu'")):
            with pytest.raises(NotImplementedError, match=msg):
                S(**kw)
        # ... and from a state dict, before anything is built or packed
        for kw, msg in ((dict(num_feat=32), "num_feat=32"), (dict(num_in_ch=4), "num_in_ch=4"), (dict(num_out_ch=1), "num_out_ch=1"),
                        (dict(upscale=5), "upscale=5"), (dict(upscale=8), "upscale=8")):
            with pytest.raises(NotImplementedError, match=msg):
                S.from_pretrained(R.SRVGGReference(num_conv=1, **kw).state_dict())
        good = R.SRVGGReference(num_conv=1, upscale=2).state_dict()
        for extra in ("body.4.running_mean", "upsampler.weight", "conv_first.weight", "body.1.bias"):
            with pytest.raises(NotImplementedError, match=re.escape(f"`{extra}`")):
                S.from_pretrained({**good, extra: torch.zeros(64)})
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        S(num_conv=0, upscale=1)(torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        S(num_conv=0, upscale=1)(torch.zeros(1, 4, 4, 4))


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_declares_exports_and_binds_the_new_entry_points():
    lib = pkg()._lib
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 31
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for name in ("i2v_conv3x3_c64_prelu_f16", "i2v_pixel_shuffle_add_f32"):
        assert re.search(rf"\bint {name}\(", src) and name in lib.SIGNATURES and hasattr(h, name)
    assert lib.SIGNATURES["i2v_conv3x3_c64_prelu_f16"][1] == [C.POINTER(lib.ConvC64Params), C.c_void_p, C.c_void_p]
    assert len(lib.SIGNATURES["i2v_pixel_shuffle_add_f32"][1]) == 13
    assert int(re.search(r"#define I2V_TAESD_PREP_UNIT_CLAMP (\d+)", src).group(1)) == lib.I2V_TAESD_PREP_UNIT_CLAMP
    assert pkg().kernels.TAESD_PREP_MODES["unit_clamp"] == lib.I2V_TAESD_PREP_UNIT_CLAMP
    from i2v_adapter_unofficial_amd import handle as H
    assert not {"i2v_conv3x3_c64_prelu_f16", "i2v_pixel_shuffle_add_f32"} & set(H.ENTRY_IDS)      # the upscaler is in no recorded plan


def test_bad_arguments_are_refused_on_the_host():
    """the new refusals return I2V_ERR_INVALID_ARG before anything is launched: callable without a GPU"""
    lib = pkg()._lib
    h = lib.load()
    SL = 1 << 43
    assert h.i2v_conv3x3_c64_prelu_f16(None, SL, None) == -1 and b"i2v_conv3x3_c64_prelu_f16: null params" in h.i2v_last_error()

    def params(**kw):
        p = lib.ConvC64Params()
        p.x, p.w, p.out, p.ldx, p.ldo = 1 << 40, 1 << 41, 1 << 42, 64, 64
        p.n_img, p.height, p.width, p.cin, p.cout = 2, 9, 17, 64, 64
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    # the existing entry's checks, through the new one ...
    for kw, msg in ((dict(x=None), b"null pointer"), (dict(cin=32), b"64 -> 64"), (dict(ldo=68), b"pixel strides"),
                    (dict(out=(1 << 42) + 2), b"16-byte"), (dict(out=1 << 40), b"out overlaps x"),
                    (dict(residual=(1 << 42) + 128, ldr=64), b"without being it"), (dict(max_workgroups=-1), b"max_workgroups")):
        assert h.i2v_conv3x3_c64_prelu_f16(C.byref(params(**kw)), SL, None) == -1, kw
        assert msg in h.i2v_last_error(), (kw, h.i2v_last_error())
    # ... and its own
    for kw, slope, msg in ((dict(), None, b"slope"), (dict(), SL + 4, b"slope"), (dict(relu_mid=1), SL, b"relu_mid must be 0"),
                           (dict(), (1 << 42) + 256, b"out overlaps slope"), (dict(), (1 << 42) - 128, b"out overlaps slope")):
        assert h.i2v_conv3x3_c64_prelu_f16(C.byref(params(**kw)), slope, None) == -1, (kw, slope)
        assert msg in h.i2v_last_error(), (kw, slope, h.i2v_last_error())
    Y, S, O = 1 << 40, 1 << 41, 1 << 42
    ok = dict(y=Y, ld=64, src=S, f32=1, out=O, n=2, h=5, w=7, s=4, mode=lib.I2V_TAESD_PREP_UNIT_CLAMP, clamp=1, signed=1)
    for kw, msg in ((dict(y=None), b"null"), (dict(src=None), b"null"), (dict(out=None), b"null"), (dict(s=0), b"s 0"), (dict(s=5), b"s 5"),
                    (dict(ld=60), b"pixel stride"), (dict(ld=68), b"pixel stride"), (dict(y=Y + 8), b"aligned"), (dict(out=O + 4), b"aligned"),
                    (dict(src=S + 2), b"aligned"), (dict(mode=1), b"entry_mode 1"), (dict(mode=3), b"entry_mode 3"), (dict(h=0), b"h 0"),
                    (dict(out=Y), b"overlaps"), (dict(out=S + 16), b"overlaps"), (dict(out=Y - 16), b"overlaps")):
        a = {**ok, **kw}
        assert h.i2v_pixel_shuffle_add_f32(a["y"], a["ld"], a["src"], a["f32"], a["out"], a["n"], a["h"], a["w"], a["s"], a["mode"],
                                           a["clamp"], a["signed"], None) == -1, kw
        assert msg in h.i2v_last_error(), (kw, h.i2v_last_error())
    # an fp16 source needs 2-byte alignment only
    a = {**ok, "src": S + 2, "f32": 0, "s": 9}
    assert h.i2v_pixel_shuffle_add_f32(a["y"], 64, a["src"], 0, a["out"], 2, 5, 7, 9, a["mode"], 1, 1, None) == -1 and b"s 9" in h.i2v_last_error()


# ------------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("s", (1, 2, 3, 4))
def test_exit_fp64_is_pixel_shuffle_plus_the_nearest_base(s):
    g = torch.Generator().manual_seed(s)
    y = torch.randn((2, 5, 7, 64), generator=g).half()
    src = torch.rand((2, 3, 5, 7), generator=g)
    body = y[..., : 3 * s * s].double().permute(0, 3, 1, 2)
    want = F.pixel_shuffle(body, s) + F.interpolate(src.double(), scale_factor=s, mode="nearest")
    got, tol = R.exit_fp64(y, src, s, unit_in=False, clamp=False, signed_out=False)
    assert torch.equal(got, want) and tuple(got.shape) == (2, 3, 5 * s, 7 * s) and bool((tol >= R.U22).all())
    assert torch.equal(R.exit_fp64(y, src, s, clamp=True, signed_out=True)[0], want.clamp(0, 1) * 2 - 1)
    signed = src * 2.4 - 1.2
    assert torch.equal(R.exit_fp64(y, signed, s, unit_in=True, clamp=False)[0],
                       F.pixel_shuffle(body, s) + F.interpolate(R.entry_map(signed.double()), scale_factor=s, mode="nearest"))


def test_the_restatement_is_the_documented_forward():
    ref = R.seeded_reference(2, 3, seed=1)
    x = torch.rand(1, 3, 6, 5, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        h = x
        for i, m in enumerate(ref.body):
            h = m(h)
        want = F.pixel_shuffle(h, 3) + F.interpolate(x, scale_factor=3, mode="nearest")
        assert torch.equal(ref(x), want)
        # fp16 storage tracks it, and another accumulation stays within the end-to-end gate's factor
        yard = float((R.run_fp16_storage(ref, x) - want).abs().max())
        other = float((R.run_fp16_storage(ref, x, accumulate=torch.float64) - want).abs().max())
        assert 0 < yard < 5e-3 and other <= 2 * yard
    for m in ref.body:
        if isinstance(m, torch.nn.PReLU):
            a = m.weight.detach()
            assert float(a[5]) == 0.0 and float(a[37]) == 1.0 and float(a.min()) > -0.3 and float(a.max()) < 1.3 and float(a.min()) < 0


@pytest.mark.parametrize("case", R.LAYER_CASES, ids=R.layer_case_id)
def test_layer_bound_rejects_wrong_evaluations(case):
    """the per-element bound accepts the layer rounded to fp16 (from fp64 and through fp32) and rejects the slopes rotated by 8
    channels, their 32-channel halves swapped, the slope applied after the residual, and ReLU in place of PReLU"""
    _, (name, bias, res_out, _, _) = case
    x, w, b, slope, r = R.layer_case_inputs(case)
    ref, tol = R.layer_fp64(x, w, b, slope, r, res_out)
    assert not bool((B.excess(ref.half(), ref, tol) > 0).any()) and not bool((B.excess(ref.float().half(), ref, tol) > 0).any())
    muts = R.layer_mutants_of(case[1])
    assert set(muts) <= set(R.LAYER_MUTANTS) and len(muts) >= 3
    for mut in muts:
        wrong, _ = R.layer_fp64(x, w, b, slope, r, res_out, mutant=mut)
        assert bool((B.excess(wrong.half(), ref, tol) > 0).any()), mut
    # slope 0 is the ReLU layer and slope 1 the plain one of tests/taesd_reference.py
    from tests import taesd_reference as T
    assert torch.equal(R.layer_fp64(x, w, b, torch.zeros(64), r, res_out)[0], T.layer_fp64(x, w, b, r, True, res_out)[0])
    assert torch.equal(R.layer_fp64(x, w, b, torch.ones(64), r, res_out)[0], T.layer_fp64(x, w, b, r, False, res_out)[0])


@pytest.mark.parametrize("case", R.EXIT_CASES, ids=R.exit_case_id)
def test_exit_bound_rejects_wrong_evaluations(case):
    """the exit's bound accepts the fp32 evaluation and rejects dy / dx transposed, colour-minor channels, a missing base, a bilinear
    base and the clamp after the range map; values on both sides of [0, 1] are present before the clamp in every case"""
    size, s, f32, signed, ld = case
    y, src = R.exit_case_inputs(case)
    ref, tol = R.exit_fp64(y, src, s, unit_in=signed, clamp=True, signed_out=signed)
    raw, _ = R.exit_fp64(y, src, s, unit_in=signed, clamp=False, signed_out=False)
    assert bool((raw > 1).any()) and bool((raw < 0).any()) and bool(((raw > 0) & (raw < 1)).any())
    assert not bool(((ref.float().double() - ref).abs() > tol).any())
    for mut in R.exit_mutants_of(case):
        wrong, _ = R.exit_fp64(y, src, s, unit_in=signed, clamp=True, signed_out=signed, mutant=mut)
        assert bool(((wrong - ref).abs() > tol).any()), mut


def test_every_mutant_is_exercised():
    for size in R.T.SIZES:
        assert {m for s, cfg in R.LAYER_CASES if s == size for m in R.layer_mutants_of(cfg)} == set(R.LAYER_MUTANTS)
    for size in R.EXIT_SIZES:
        seen = {m for c in R.EXIT_CASES if c[0] == size for m in R.exit_mutants_of(c)}
        assert seen == set(R.EXIT_MUTANTS) - ({"bilinear_base"} if size == (1, 1, 1) else set())


@pytest.mark.parametrize("num_conv,s", ((2, 2), (16, 4)))
def test_few_outputs_of_the_seeded_reference_saturate(num_conv, s):
    """the GPU test's end-to-end gate compares clamped outputs: a saturated output hides an error, so at most 10 % may be"""
    ref = R.seeded_reference(num_conv, s)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for shape in ((2, 3, 9, 17), (1, 3, 16, 32)):
            x = torch.rand(shape, generator=g)
            frac = R.saturated_fraction(ref, x)
            mid = ref.body[: -1]
            h = x
            for m in mid:
                h = m(h)
            assert 0 < frac <= 0.10, (shape, frac)
            assert 0.05 < float(h.pow(2).mean()) < 20, float(h.pow(2).mean())          # neither died nor blew up


# ------------------------------------------------------------------------------------------------------------- pipeline, driver
def _cpu_pipe():
    p = pkg()
    return p.I2VAdapterPipeline(unet=p.UNetMotionCrossFrameAttnModel(**SMALL_UNET))


def test_pipeline_enable_disable_and_the_latent_refusal(monkeypatch):
    pipe = _cpu_pipe()
    S = pkg().SRVGGNetCompact
    assert pipe.upscaler_enabled is False
    with pytest.raises(ValueError, match="enable_upscaler"):
        pipe.upscale_frames(torch.zeros(1, 2, 3, 8, 8))
    model = S(num_conv=1, upscale=2)
    pipe.enable_upscaler(model, frames_per_batch=3)
    assert pipe.upscaler_enabled and pipe._upscaler == (model, 3)
    state = R.seeded_reference(1, 2).state_dict()
    pipe.enable_upscaler(state)
    assert pipe._upscaler[0].num_conv == 1 and pipe._upscaler[0].upscale == 2 and pipe._upscaler[1] is None
    bare = {k: v for k, v in state.items() if v.dim() != 1 or k.endswith("bias")}
    pipe.enable_upscaler(bare, act_type="leakyrelu")
    assert pipe._upscaler[0].act_type == "leakyrelu"
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="frames_per_batch"):
            pipe.enable_upscaler(model, frames_per_batch=bad)
    with pytest.raises(ValueError, match="act_type"):
        pipe.enable_upscaler(model, act_type="relu")
    with pytest.raises(ValueError, match=r"\[B, F, 3, H, W\]"):
        pipe.upscale_frames(torch.zeros(2, 4, 8, 8))
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        pipe.upscale_frames(torch.zeros(1, 2, 3, 8, 8))
    # output_type="latent" is refused in phase 1: before anything is encoded
    def no_encode(*a, **kw):
        raise AssertionError("the refusal must come before anything is encoded")
    monkeypatch.setattr(pipe, "_encode_contexts", no_encode)
    monkeypatch.setattr(pipe, "encode_condition_image", no_encode)
    call = dict(condition_image_latents=torch.zeros(1, 4, 8, 8), num_frames=3, num_inference_steps=4,
                prompt_embeds=torch.zeros(1, 7, 64), negative_prompt_embeds=torch.zeros(1, 7, 64))
    with pytest.raises(ValueError, match="output_type='latent' with the upscaler enabled"):
        pipe(output_type="latent", **call)
    with pytest.raises(ValueError, match="output_type='latent' with the upscaler enabled"):
        pipe(**call)                                      # (no VAE: the default output is the latents)
    pipe.disable_upscaler()
    assert pipe.upscaler_enabled is False and pipe._upscaler is None
    with pytest.raises(AssertionError, match="before anything is encoded"):
        pipe(output_type="latent", **call)                # disabled: the call goes on to phase 2 as before


def test_driver_flags_parse():
    parser = pkg().pipeline_i2v_adapter.build_parser()
    a = parser.parse_args(["--task_name", "t"])
    assert a.upscaler is None and a.upscaler_act is None
    a = parser.parse_args(["--task_name", "t", "--upscaler", "/models/realesr-animevideov3.pth", "--upscaler_act", "leakyrelu"])
    assert a.upscaler == "/models/realesr-animevideov3.pth" and a.upscaler_act == "leakyrelu"
    with pytest.raises(SystemExit):
        parser.parse_args(["--task_name", "t", "--upscaler_act", "gelu"])
