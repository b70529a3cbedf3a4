"""AutoencoderTiny (TAESD) without a GPU: state-dict keys against the plain-torch restatement and the committed key list, the config
refusals, the ABI of the two new entry points and their host-side argument checks, the latent scaling, the driver's flag, the weight
packing of the 64 -> 64 kernel, and the two things the GPU gates rely on -- the per-element bound REJECTS five wrong evaluations of
every kernel case, and the fp16-storage yardstick is stable against the accumulation order."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import gemm_bounds as B
from tests import taesd_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def test_state_dict_keys_are_the_restatements_and_the_committed_list():
    ref = R.TaesdReference()
    keys = list(pkg().AutoencoderTiny().state_dict().keys())
    golden = open(os.path.join(ROOT, "tests", "golden", "taesd_keys.txt")).read().split()
    assert keys == list(ref.state_dict().keys()) == golden and len(keys) == 134
    shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert shapes["encoder.layers.0.weight"] == (64, 3, 3, 3) and shapes["encoder.layers.14.weight"] == (4, 64, 3, 3)
    assert shapes["decoder.layers.0.weight"] == (64, 4, 3, 3) and shapes["decoder.layers.18.weight"] == (3, 64, 3, 3)
    for i in (2, 6, 10):
        assert f"encoder.layers.{i}.weight" in shapes and f"encoder.layers.{i}.bias" not in shapes
    for i in (6, 11, 16):
        assert f"decoder.layers.{i}.weight" in shapes and f"decoder.layers.{i}.bias" not in shapes
    for i in (1, 3, 4, 5, 7, 8, 9, 11, 12, 13):
        assert all(f"encoder.layers.{i}.conv.{j}.{p}" in shapes for j in (0, 2, 4) for p in ("weight", "bias"))
    for i in (2, 3, 4, 7, 8, 9, 12, 13, 14, 17):
        assert all(f"decoder.layers.{i}.conv.{j}.{p}" in shapes for j in (0, 2, 4) for p in ("weight", "bias"))


def test_a_checkpoint_saved_by_the_restatement_loads_by_key(tmp_path):
    import json
    from safetensors.torch import save_file
    ref = R.seeded_reference(3)
    save_file({k: v.contiguous() for k, v in ref.state_dict().items()}, str(tmp_path / "diffusion_pytorch_model.safetensors"))
    cfg = dict(_class_name="AutoencoderTiny", _diffusers_version="0.24.0", in_channels=3, out_channels=3, act_fn="relu", latent_channels=4,
               encoder_block_out_channels=[64] * 4, decoder_block_out_channels=[64] * 4, upsampling_scaling_factor=2,
               num_encoder_blocks=[1, 3, 3, 3], num_decoder_blocks=[3, 3, 3, 1], latent_magnitude=3, latent_shift=0.5, force_upcast=False,
               scaling_factor=1.0, block_out_channels=[64] * 4)
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    m = pkg().AutoencoderTiny.from_pretrained(str(tmp_path))
    for k, v in ref.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    assert m.config["scaling_factor"] == 1.0 and m.config["block_out_channels"] == (64,) * 4 and m.dtype == torch.float32
    m.save_pretrained(str(tmp_path / "again"))
    again = pkg().AutoencoderTiny.from_pretrained(str(tmp_path / "again"))
    assert all(torch.equal(again.state_dict()[k], v) for k, v in ref.state_dict().items())


def test_config_defaults_and_refusals():
    T = pkg().AutoencoderTiny
    with torch.device("meta"):
        m = T()
        assert dict(m.config) == dict(in_channels=3, out_channels=3, encoder_block_out_channels=(64,) * 4, decoder_block_out_channels=(64,) * 4,
                                      act_fn="relu", latent_channels=4, upsampling_scaling_factor=2, num_encoder_blocks=(1, 3, 3, 3),
                                      num_decoder_blocks=(3, 3, 3, 1), latent_magnitude=3, latent_shift=0.5, force_upcast=False,
                                      scaling_factor=1.0, block_out_channels=(64,) * 4)
        for kw, key in ((dict(encoder_block_out_channels=(32, 64, 64, 64)), "encoder_block_out_channels"),
                        (dict(decoder_block_out_channels=(64, 64, 64, 128)), "decoder_block_out_channels"),
                        (dict(act_fn="silu"), "act_fn"), (dict(upsampling_scaling_factor=4), "upsampling_scaling_factor"),
                        (dict(shift_factor=0.1), "shift_factor")):
            with pytest.raises(NotImplementedError, match=key):
                T(**kw)
        with pytest.raises(NotImplementedError, match="tiled"):
            m.enable_tiling()
    assert pkg().autoencoder_tiny.AutoencoderTiny is T


def test_tiling_refusal_reaches_the_pipeline():
    """enable_vae_tiling with an AutoencoderTiny propagates its NotImplementedError"""
    P = pkg().pipeline_i2v_adapter.I2VAdapterPipeline
    with torch.device("meta"):
        vae = pkg().AutoencoderTiny()
    pipe = P.__new__(P)
    pipe.vae = vae
    with pytest.raises(NotImplementedError, match="tiled"):
        pipe.enable_vae_tiling()


def test_scale_and_unscale_latents_are_the_closed_form():
    with torch.device("meta"):
        m = pkg().AutoencoderTiny()
    z = torch.linspace(-5, 5, 41).reshape(1, 1, 1, 41)
    assert torch.equal(m.scale_latents(z), (z / 6 + 0.5).clamp(0, 1))
    u = torch.linspace(0, 1, 33)
    assert torch.equal(m.unscale_latents(u), (u - 0.5) * 6)
    inside = z[z.abs() < 3]
    assert torch.allclose(m.unscale_latents(m.scale_latents(inside)), inside, atol=1e-6)


def test_abi_declares_exports_and_binds_the_two_entry_points():
    lib = pkg()._lib
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 23
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for name in ("i2v_conv3x3_c64_f16", "i2v_taesd_prep_f16"):
        assert re.search(rf"\bint {name}\(", src) and name in lib.SIGNATURES and hasattr(h, name)
    from i2v_adapter_unofficial_amd import handle as H
    assert "i2v_conv3x3_c64_f16" not in H.ENTRY_IDS and "i2v_taesd_prep_f16" not in H.ENTRY_IDS      # the VAE is in no recorded plan


def test_ctypes_struct_matches_the_header(tmp_path):
    import subprocess
    lib = pkg()._lib
    prog = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "i2v_hip.h")}"', "int main(void){",
            'printf("size %zu\\n", sizeof(i2v_conv_c64_params));']
    prog += [f'printf("{f} %zu\\n", offsetof(i2v_conv_c64_params, {f}));' for f, _ in lib.ConvC64Params._fields_]
    prog.append("return 0;}")
    (tmp_path / "t.c").write_text("\n".join(prog))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "t"), str(tmp_path / "t.c")], check=True)
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(lib.ConvC64Params)
    for f, _ in lib.ConvC64Params._fields_:
        assert int(got[f]) == getattr(lib.ConvC64Params, f).offset, f


def test_bad_arguments_are_refused_on_the_host():
    """null / misaligned / aliased / C != 64 operands return I2V_ERR_INVALID_ARG before anything is launched: callable without a GPU"""
    lib = pkg()._lib
    h = lib.load()
    assert h.i2v_conv3x3_c64_f16(None, None) == -1 and b"null params" in h.i2v_last_error()

    def params(**kw):
        p = lib.ConvC64Params()
        p.x, p.w, p.out, p.ldx, p.ldo = 1 << 40, 1 << 41, 1 << 42, 64, 64
        p.n_img, p.height, p.width, p.cin, p.cout = 2, 9, 17, 64, 64
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    for kw, msg in ((dict(x=None), b"null pointer"), (dict(cin=32), b"64 -> 64"), (dict(cout=128), b"64 -> 64"), (dict(height=0), b"h 0"),
                    (dict(ldx=60), b"pixel strides"), (dict(ldo=68), b"pixel strides"), (dict(x=(1 << 40) + 8), b"16-byte"),
                    (dict(out=(1 << 42) + 2), b"16-byte"), (dict(bias=(1 << 43) + 4), b"16-byte"), (dict(out=1 << 40), b"out overlaps x"),
                    (dict(out=(1 << 40) + 64 * 2 * 16), b"out overlaps x"), (dict(residual=1 << 44, ldr=63), b"residual pixel stride"),
                    (dict(residual=(1 << 42) + 128, ldr=64), b"without being it"), (dict(residual=1 << 42, ldr=72), b"without being it"),
                    (dict(max_workgroups=-1), b"max_workgroups")):
        assert h.i2v_conv3x3_c64_f16(C.byref(params(**kw)), None) == -1, kw
        assert msg in h.i2v_last_error(), (kw, h.i2v_last_error())
    A, D = 1 << 40, 1 << 42
    for args, msg in (((None, 1, D, 64, 1, 3, 16, 0), b"null"), ((A, 1, D, 64, 1, 65, 16, 0), b"c 65"), ((A, 1, D, 64, 1, 3, 16, 3), b"mode 3"),
                      ((A, 1, D, 60, 1, 3, 16, 0), b"pixel stride"), ((A, 1, D + 8, 64, 1, 3, 16, 0), b"pixel stride"),
                      ((A, 1, A, 64, 1, 3, 16, 1), b"overlaps")):
        assert h.i2v_taesd_prep_f16(*args, None) == -1 and msg in h.i2v_last_error(), (args, h.i2v_last_error())


def test_driver_flag_parses():
    parser = pkg().pipeline_i2v_adapter.build_parser()
    assert parser.parse_args(["--task_name", "t"]).vae_tiny is None
    assert parser.parse_args(["--task_name", "t", "--vae_tiny", "/models/taesd", "--scheduler", "lcm"]).vae_tiny == "/models/taesd"


def test_pack_conv_c64_is_the_documented_fragment_order():
    K = pkg().kernels
    w = torch.randn(64, 64, 3, 3).half()
    pk = K.pack_conv_c64(w).view(9, 2, 4, 4, 16, 8)           # [tap, s, b, g, l, j]
    tap, s, b, g, l, j = torch.meshgrid(*[torch.arange(n) for n in pk.shape], indexing="ij")
    assert torch.equal(pk, w[32 * (b >> 1) + 8 * (l >> 2) + 4 * (b & 1) + (l & 3), 32 * s + 8 * g + j, tap // 3, tap % 3])
    narrow = torch.randn(64, 3, 3, 3).half()
    wide = torch.zeros(64, 64, 3, 3).half()
    wide[:, :3] = narrow
    assert torch.equal(K.pack_conv_c64(narrow), K.pack_conv_c64(wide))
    with pytest.raises(ValueError):
        K.pack_conv_c64(torch.zeros(32, 64, 3, 3))


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_bound_rejects_wrong_evaluations(case):
    """the per-element bound of tests/gemm_bounds.py (K = 576, the residual's term, through the 1-Lipschitz ReLU) accepts the layer
    rounded to fp16 and rejects each of the wrong evaluations that can differ for the configuration: a tap shifted by one pixel, the
    neighbouring image's row for the zero halo, the bias missing, ReLU before instead of after the residual, the two 32-channel halves
    of the contraction swapped"""
    _, (name, bias, relu_mid, relu_out, residual, _, _) = case
    x, w, b, r = R.case_inputs(case)
    ref, tol = R.layer_fp64(x, w, b, r, relu_mid, relu_out)
    assert not bool((B.excess(ref.half(), ref, tol) > 0).any())
    assert not bool((B.excess(ref.float().half(), ref, tol) > 0).any())
    muts = R.mutants_of(case[1])
    assert set(muts) <= set(R.MUTANTS) and len(muts) >= 3
    for mut in muts:
        wrong, _ = R.layer_fp64(x, w, b, r, relu_mid, relu_out, mutant=mut)
        assert bool((B.excess(wrong.half(), ref, tol) > 0).any()), mut


def test_every_mutant_is_exercised_at_every_size():
    for size in R.SIZES:
        seen = set()
        for s, cfg in R.CASES:
            if s == size:
                seen |= set(R.mutants_of(cfg))
        assert seen == set(R.MUTANTS)


def test_fp16_storage_yardstick_is_stable_against_the_accumulation():
    """the end-to-end gate of the GPU test allows twice the fp16-storage variant's own error against the fp32 restatement; before
    relying on it: the variant evaluated with ANOTHER accumulation (fp64 instead of fp32) stays within that gate on the same inputs,
    and the yardstick is far below what a lost ReLU does"""
    ref = R.seeded_reference(0)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for which, t in (("encode", torch.rand((1, 3, 32, 32), generator=g) * 2 - 1), ("decode", torch.randn((1, 4, 4, 4), generator=g))):
            exact = getattr(ref, which)(t)
            yard = float((R.run_fp16_storage(ref, t, which) - exact).abs().max())
            other = float((R.run_fp16_storage(ref, t, which, accumulate=torch.float64) - exact).abs().max())
            assert 0 < yard < 2e-2 * float(exact.abs().max()) + 1e-3 and other <= 2 * yard, (which, yard, other)
