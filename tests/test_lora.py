"""LoRA on the host: every accepted key spelling parses to one normalised dict, the kohya name table is unambiguous for the reduced and
the SD-1.5-width module tree, text-encoder keys are skipped and reported, unknown keys and wrong shapes raise, the state methods only
mark state, and the new struct of the C ABI matches its ctypes mirror.  No kernel is launched."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch

from tests.lora_reference import attention_paths, merge_reference, random_lora, target_shapes, to_state_dict
from tests.parity import ROOT, SD15, SMALL_UNET

HEADER = os.path.join(ROOT, "include", "i2v_hip.h")


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _product_unet(cfg=SMALL_UNET):
    with torch.device("meta"):
        return pkg().UNetMotionCrossFrameAttnModel(**cfg)


@pytest.fixture(scope="module")
def shapes():
    return pkg().lora.lora_target_shapes(_product_unet())


def _same(a, b):
    assert set(a) == set(b)
    for path in a:
        (d0, u0, al0), (d1, u1, al1) = a[path], b[path]
        assert d0.shape == d1.shape and u0.shape == u1.shape and d0.dim() == u0.dim() == 2, path
        assert torch.equal(d0, d1) and torch.equal(u0, u1) and al0 == al1, path


def test_targets_are_every_linear_and_conv_and_match_the_oracle(shapes):
    from tests.parity import oracle_small_unet
    assert shapes == target_shapes(oracle_small_unet())
    kinds = ("attn1.to_q", "attn2.to_k", "i2v_adapter.to_q", "i2v_adapter.to_out.0", "motion_modules.0.transformer_blocks.0.attn1.to_v",
             "ff.net.0.proj", "ff.net.2", "proj_in", "proj_out", "resnets.0.conv1", "resnets.0.conv2", "time_emb_proj",
             "downsamplers.0.conv", "upsamplers.0.conv", "conv_shortcut", "conv_in", "conv_out", "time_embedding.linear_1")
    for k in kinds:
        assert any(p.endswith(k) for p in shapes), k


@pytest.mark.parametrize("spelling,prefix", [("diffusers", ""), ("diffusers", "unet."), ("peft", ""), ("peft", "unet."), ("processor", ""),
                                             ("processor", "unet."), ("kohya", "")])      # (kohya keys carry their own lora_unet_ prefix)
def test_every_spelling_parses_to_the_same_dict(shapes, spelling, prefix):
    L = pkg().lora
    paths = attention_paths(shapes) if spelling == "processor" else None
    alpha = 2.0 if spelling == "kohya" else None
    lora = random_lora(shapes, rank=4, seed=3, paths=paths, alpha=alpha)
    sd = to_state_dict(lora, shapes, spelling, prefix=prefix)
    assert len(sd) == len(lora) * (3 if alpha is not None else 2)
    got, report = L.parse_lora_state_dict(sd, shapes)
    _same(got, lora)
    assert report == {"text_encoder_keys": 0, "unet_keys": len(sd)}
    if spelling == "kohya":          # conv factors arrive 4-D and come out [rank, Cin kh kw] / [Cout, rank]
        conv = next(p for p in lora if len(shapes[p]) == 4 and shapes[p][2] == 3)
        assert sd["lora_unet_" + conv.replace(".", "_") + ".lora_down.weight"].dim() == 4
    # the reference agrees on what the normalised factors mean
    path = next(iter(lora))
    d, u, al = got[path]
    base = torch.zeros(shapes[path])
    assert torch.equal(merge_reference(base, [(d, u, 1.0)]).reshape(shapes[path][0], -1), u.double() @ d.double())


def test_to_out_means_to_out_0_and_peft_adapter_names_and_alpha(shapes):
    L = pkg().lora
    path = next(p for p in shapes if p.endswith("attn1.to_out.0"))
    lora = random_lora(shapes, rank=2, seed=1, paths=[path])
    d, u, _ = lora[path]
    stem = path[: -len(".0")]
    got, _ = L.parse_lora_state_dict({f"{stem}.lora_A.default.weight": d, f"{stem}.lora_B.default.weight": u,
                                      f"{stem}.alpha": torch.tensor(8.0)}, shapes)
    assert list(got) == [path] and got[path][2] == 8.0 and torch.equal(got[path][0], d)
    flat = "lora_unet_" + stem.replace(".", "_")
    got, _ = L.parse_lora_state_dict({flat + ".lora_down.weight": d, flat + ".lora_up.weight": u}, shapes)
    assert list(got) == [path] and got[path][2] is None


@pytest.mark.parametrize("cfg", [SMALL_UNET, SD15], ids=["small", "sd15"])
def test_kohya_name_table_is_unambiguous(cfg):
    L = pkg().lora
    sh = L.lora_target_shapes(_product_unet(cfg))
    table = L.kohya_name_table(sh)
    assert len(table) == len(sh) and sorted(table.values()) == sorted(sh)
    assert "down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q" in table
    with pytest.raises(AssertionError, match="ambiguous"):
        L.kohya_name_table(["a.b_c", "a_b.c"])


def test_text_encoder_keys_are_skipped_and_reported(shapes):
    L = pkg().lora
    lora = random_lora(shapes, rank=2, seed=5, paths=attention_paths(shapes)[:3])
    sd = to_state_dict(lora, shapes, "kohya")
    sd["lora_te_text_model_encoder_layers_0_self_attn_q_proj.lora_down.weight"] = torch.zeros(2, 8)
    sd["lora_te_text_model_encoder_layers_0_self_attn_q_proj.lora_up.weight"] = torch.zeros(8, 2)
    sd["text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora.down.weight"] = torch.zeros(2, 8)
    got, report = L.parse_lora_state_dict(sd, shapes)
    _same(got, lora)
    assert report["text_encoder_keys"] == 3 and report["unet_keys"] == 6


def test_unknown_keys_and_wrong_shapes_raise_naming_the_key(shapes):
    L = pkg().lora
    path = attention_paths(shapes)[0]
    n_out, n_in = shapes[path]
    d, u = torch.zeros(4, n_in), torch.zeros(n_out, 4)
    bad = "down_blocks.9.attentions.0.to_q.lora.down.weight"
    with pytest.raises(ValueError, match=re.escape(bad)):
        L.parse_lora_state_dict({bad: d}, shapes)
    with pytest.raises(ValueError, match="lora_unet_nope_to_q"):
        L.parse_lora_state_dict({"lora_unet_nope_to_q.lora_down.weight": d}, shapes)
    with pytest.raises(ValueError, match="no known spelling"):
        L.parse_lora_state_dict({f"{path}.weight": d}, shapes)
    with pytest.raises(ValueError, match=re.escape(f"{path}.lora.down.weight")):
        L.parse_lora_state_dict({f"{path}.lora.down.weight": torch.zeros(4, n_in + 1), f"{path}.lora.up.weight": u}, shapes)
    with pytest.raises(ValueError, match=re.escape(f"{path}.lora.up.weight")):
        L.parse_lora_state_dict({f"{path}.lora.down.weight": d, f"{path}.lora.up.weight": torch.zeros(n_out, 5)}, shapes)
    with pytest.raises(ValueError, match="no up factor"):
        L.parse_lora_state_dict({f"{path}.lora.down.weight": d}, shapes)
    with pytest.raises(ValueError, match="repeats"):
        L.parse_lora_state_dict({f"{path}.lora.down.weight": d, f"{path}.lora_A.weight": d, f"{path}.lora.up.weight": u}, shapes)


def test_reading_files(tmp_path, shapes):
    from safetensors.torch import save_file
    L = pkg().lora
    lora = random_lora(shapes, rank=2, seed=9, paths=attention_paths(shapes)[:2])
    sd = to_state_dict(lora, shapes, "diffusers", prefix="unet.")
    os.makedirs(tmp_path / "sub")
    save_file(sd, str(tmp_path / "sub" / "a.safetensors"))
    torch.save(sd, str(tmp_path / "b.bin"))
    for got in (L.read_lora_file(str(tmp_path), weight_name="a.safetensors", subfolder="sub"), L.read_lora_file(str(tmp_path / "b.bin")),
                L.read_lora_file(sd)):
        _same(L.parse_lora_state_dict(got, shapes)[0], lora)
    with pytest.raises(EnvironmentError, match="not found"):
        L.read_lora_file(str(tmp_path), weight_name="missing.safetensors")


def test_state_methods_without_a_gpu():
    """no LoRA: no state, `_sync_lora` is a no-op, the pipeline delegates; loading needs the model on the device"""
    p = pkg()
    u = _product_unet()
    assert not u.has_lora() and u.get_active_adapters() == [] and u.lora_parameter_names() == []
    u._sync_lora()
    assert u.set_lora_scale(0.5) == 1.0 and u.set_lora_scale(1.0) == 0.5
    with pytest.raises(ValueError, match="not loaded"):
        u.set_adapters(["a"])
    with pytest.raises(ValueError, match="not loaded"):
        u.delete_adapters("a")
    with pytest.raises(ValueError, match="no LoRA"):
        u.fuse_lora()
    with pytest.raises(ValueError, match="no fused"):
        u.unfuse_lora()
    with pytest.raises(p.HipLibraryError, match="no CPU path"):
        u.load_lora({})
    pipe = p.I2VAdapterPipeline(unet=u)
    assert pipe.get_active_adapters() == []
    pipe.unload_lora_weights()
    assert set(u.state_dict()) == set(_product_unet().state_dict()), "LoRA state must not add state-dict keys"


def test_struct_matches_the_header_and_the_limits():
    lib = pkg()._lib
    src = open(HEADER).read()
    assert int(re.search(r"#define I2V_LORA_MAX_ADAPTERS (\d+)", src).group(1)) == lib.I2V_LORA_MAX_ADAPTERS == 8
    assert int(re.search(r"#define I2V_LORA_MAX_RANK (\d+)", src).group(1)) == lib.I2V_LORA_MAX_RANK == 256
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 13
    cls = lib.LoraAdapter
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("size %zu\\n", sizeof(i2v_lora_adapter));']
    for fname, _ in cls._fields_:
        prog.append(f'printf("{fname} %zu\\n", offsetof(i2v_lora_adapter, {fname}));')
    prog.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write("\n".join(prog))
        subprocess.run(["gcc", "-std=c99", "-o", exe, c], check=True)
        got = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(got["size"]) == C.sizeof(cls) == 24
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname


@pytest.fixture(scope="module")
def lib():
    p = pkg()
    if not os.path.exists(p._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return p._lib


def test_bad_arguments_return_error_codes_without_a_gpu(lib):
    """argument validation happens on the host before any launch"""
    h = lib.load()
    buf, other = (C.c_uint16 * 64)(), (C.c_uint16 * 64)()
    fac = (C.c_uint16 * 4096)()
    a, b = C.addressof(buf), C.addressof(other)
    one = (lib.LoraAdapter * 1)(lib.LoraAdapter(C.addressof(fac), C.addressof(fac) + 4096, 4, 1.0))
    assert h.i2v_lora_merge(None, b, 0, 8, 8, one, 1, None) == -1 and b"null pointer" in h.i2v_last_error()
    assert h.i2v_lora_merge(a, b, 0, 0, 8, one, 1, None) == -1
    assert h.i2v_lora_merge(a, a, 0, 8, 8, one, 1, None) == -1 and b"alias" in h.i2v_last_error()
    assert h.i2v_lora_merge(a, a + 16, 0, 8, 4, one, 1, None) == -1 and b"alias" in h.i2v_last_error()      # (overlapping ranges)
    assert h.i2v_lora_merge(a, b, 0, 8, 8, one, 9, None) == -1 and b"at most 8" in h.i2v_last_error()
    assert h.i2v_lora_merge(a, b, 0, 8, 8, None, 1, None) == -1
    big = (lib.LoraAdapter * 1)(lib.LoraAdapter(C.addressof(fac), C.addressof(fac) + 4096, 257, 1.0))
    assert h.i2v_lora_merge(a, b, 0, 8, 8, big, 1, None) == -1 and b"rank 257" in h.i2v_last_error()
    nul = (lib.LoraAdapter * 1)(lib.LoraAdapter(None, C.addressof(fac), 4, 1.0))
    assert h.i2v_lora_merge(a, b, 0, 8, 8, nul, 1, None) == -1 and b"adapter 0: null pointer" in h.i2v_last_error()
    onto = (lib.LoraAdapter * 1)(lib.LoraAdapter(a, C.addressof(fac), 4, 1.0))
    assert h.i2v_lora_merge(a, b, 0, 8, 8, onto, 1, None) == -1 and b"alias a factor" in h.i2v_last_error()
