"""The CLIP text encoder without a GPU: tests/clip_text_reference.py pinned against transformers' CLIPTextModel and against the
committed fixture, the module's state-dict keys, checkpoint round trips, the ABI, the constructor's refusals, the driver's command
line and `encode_prompt`'s host-side errors."""
import os
import re
import sys

import pytest
import torch

from tests.clip_text_reference import (PREFIX, ClipTextReference, StubTokenizer, prompt_like_ids, seeded_state, state_dict_keys,
                                       strip_prefix)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SMALL = dict(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
             max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=255)
# the pins compare two fp32 evaluations of the same sums.  Observed here: 0.0 (bit-identical -- the restatement issues the same torch
# ops in the same order as transformers' eager path) on every tensor.  The bound is fp32 round-off for a machine whose BLAS blocks the
# sums differently: 2^-24 times the ~100 rounded operations between an input and an output, i.e. the observed figure plus a decade
# above the format's own 6e-8.
PIN_REL = 1e-5


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _rel(got, ref):
    return (got.double() - ref.double()).abs().max().item() / ref.double().abs().max().item()


@pytest.mark.parametrize("prefixed", [True, False])
@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_reference_against_transformers(prefixed, act):
    pytest.importorskip("transformers")
    sys.path.insert(0, ROOT)
    from tools.make_clip_text_fixture import transformers_model
    cfg = dict(SMALL, hidden_act=act)
    state = seeded_state(cfg, seed=3, qk_gain=3.0)
    ids = prompt_like_ids(3, 77, cfg["vocab_size"], seed=1)
    with torch.no_grad():
        out = transformers_model(cfg, state)(input_ids=ids, output_hidden_states=True)
    ref = ClipTextReference(state if prefixed else strip_prefix(state), cfg)
    last, hidden = ref(ids, output_hidden_states=True)
    assert len(hidden) == len(out.hidden_states) == cfg["num_hidden_layers"] + 1
    for name, got, want in [("last", last, out.last_hidden_state)] + [(f"hidden {i}", g, w) for i, (g, w) in
                                                                      enumerate(zip(hidden, out.hidden_states))]:
        r = _rel(got, want)
        print(f"{act} {name}: rel {r:.2e}")
        assert r <= PIN_REL, (name, r)
    # ModelOutput's integer indexing skips None fields: the two forms encode_prompt reads
    assert out[0] is out.last_hidden_state and out[-1] is out.hidden_states
    assert _rel(ref.encode(ids, clip_skip=1), ref.final_layer_norm(hidden[-2])) == 0.0
    assert _rel(ref.encode(ids), last) == 0.0


def _fixture():
    from safetensors.torch import load_file
    blob = load_file(os.path.join(GOLDEN, "clip_text_small.safetensors"))
    state = {k: v for k, v in blob.items() if k.startswith(PREFIX)}
    return blob, state


def test_reference_against_the_committed_fixture():
    assert os.path.getsize(os.path.join(GOLDEN, "clip_text_small.safetensors")) < 1_000_000
    blob, state = _fixture()
    assert all(v.dtype == torch.float16 for v in state.values()) and sorted(state) == sorted(state_dict_keys(2))
    ref = ClipTextReference({k: v.float() for k, v in state.items()}, SMALL)
    ids = blob["input_ids"].long()
    assert ids.shape == (2, 77) and int(ids.max()) == 255 and int(ids[0, 0]) == 254
    last, hidden = ref(ids, output_hidden_states=True)
    assert len(hidden) == 3
    pairs = [("last", last, blob["last_hidden_state"])] + [(f"hidden {i}", hidden[i], blob[f"hidden_states.{i}"]) for i in range(3)]
    for name, got, want in pairs:
        r = _rel(got, want)
        print(f"fixture {name}: rel {r:.2e}")
        assert r <= PIN_REL, (name, r)
    # fp64 agrees with the fp32 run to fp32 round-off as well: the fixture is not pinned to one summation order
    assert _rel(ref.double()(ids)[0], blob["last_hidden_state"]) <= PIN_REL
    # causality of the restatement itself: ids changed at positions >= 40 leave positions < 40 alone
    ids2 = ids.clone()
    ids2[:, 40:] = (ids2[:, 40:] + 7) % 254
    assert torch.equal(ref(ids2)[0][:, :40], last[:, :40]) and not torch.equal(ref(ids2)[0][:, 40:], last[:, 40:])


def test_state_dict_keys_are_the_checkpoints():
    keys = open(os.path.join(GOLDEN, "clip_text_keys.txt")).read().split()
    assert len(keys) == 197 and PREFIX + "embeddings.position_ids" in keys
    with torch.device("meta"):
        m = pkg().CLIPTextModel()
    assert m.config.hidden_size == 768 and m.config.num_hidden_layers == 12 and m.config.eos_token_id == 2
    assert sorted(m.state_dict()) == sorted(k for k in keys if not k.endswith("position_ids"))
    assert sorted(state_dict_keys(12)) == sorted(m.state_dict())
    sd = m.state_dict()
    assert sd[PREFIX + "embeddings.token_embedding.weight"].shape == (49408, 768)
    assert sd[PREFIX + "encoder.layers.11.mlp.fc1.weight"].shape == (3072, 768)
    assert set(m.config) == {"vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                             "max_position_embeddings", "hidden_act", "layer_norm_eps", "eos_token_id"}


@pytest.mark.parametrize("layout", ["own", "bare", "position_ids"])
def test_save_and_from_pretrained_round_trip(tmp_path, layout):
    """own: save_pretrained's files; bare: a model.safetensors without the `text_model.` prefix and a transformers-style config.json
    (extra keys); position_ids: the prefixed file of older releases, with the buffer"""
    import json

    from safetensors.torch import save_file
    P = pkg()
    _, state = _fixture()
    m = P.CLIPTextModel(**SMALL)
    m.load_state_dict(state)
    d = str(tmp_path / "text_encoder")
    m.half().save_pretrained(d)
    assert sorted(os.listdir(d)) == ["config.json", "model.safetensors"]
    if layout != "own":
        st = strip_prefix(state) if layout == "bare" else dict(state, **{PREFIX + "embeddings.position_ids": torch.arange(77)[None]})
        save_file({k: v.contiguous() for k, v in st.items()}, os.path.join(d, "model.safetensors"))
        json.dump(dict(SMALL, architectures=["CLIPTextModel"], model_type="clip_text_model", projection_dim=768, dropout=0.0),
                  open(os.path.join(d, "config.json"), "w"))
    back = P.CLIPTextModel.from_pretrained(d)
    assert dict(back.config) == dict(m.config) and not back.training
    for k, v in m.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    save_file({"nonsense.weight": torch.zeros(1)}, os.path.join(d, "model.safetensors"))
    with pytest.raises(RuntimeError, match="missing keys"):
        P.CLIPTextModel.from_pretrained(d)
    assert P.CLIPTextModel.from_config(dict(SMALL, unknown=1)).config.hidden_size == 128


def test_constructor_refusals_and_no_cpu_path():
    P = pkg()
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        P.CLIPTextModel(**dict(SMALL, hidden_size=64, num_attention_heads=2))                  # head_dim 32
    with pytest.raises(NotImplementedError, match="128 positions"):
        P.CLIPTextModel(**dict(SMALL, max_position_embeddings=129))
    with pytest.raises(NotImplementedError, match="use_attention_mask"):
        P.CLIPTextModel(**SMALL, use_attention_mask=True)
    with pytest.raises(NotImplementedError, match="hidden_act"):
        P.CLIPTextModel(**dict(SMALL, hidden_act="relu"))
    P.CLIPTextModel(**dict(SMALL, max_position_embeddings=128))
    m = P.CLIPTextModel(**SMALL)
    ids = prompt_like_ids(1, 77, 256)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        m(ids, attention_mask=torch.ones_like(ids))
    with pytest.raises(P.HipLibraryError, match="no CPU fallback"):
        m(ids)
    with pytest.raises(P.HipLibraryError, match="no CPU fallback"):
        m.text_model.final_layer_norm(torch.zeros(1, 77, 128))
    out = P.clip_text.CLIPTextModelOutput("last", None, ("h0", "h1"))
    assert out[0] == "last" and out[-1] == ("h0", "h1") and len(out) == 2 and out.pooler_output is None
    assert P.clip_text.CLIPTextModelOutput("last")[-1] == "last"


@pytest.fixture(scope="module")
def lib():
    p = pkg()
    if not os.path.exists(p._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return p._lib


def test_abi_version_and_symbols(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 17
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for name in ("i2v_clip_embed_f16", "i2v_clip_attention_f16", "i2v_quick_gelu_f16"):
        assert hasattr(h, name) and name in lib.SIGNATURES and name in src
    K = pkg().kernels
    assert callable(K.clip_embed) and callable(K.clip_attention) and callable(K.quick_gelu)


def test_the_driver_command_line(capsys):
    drv = pkg().pipeline_i2v_adapter
    parser = drv.build_parser()
    args = parser.parse_args([])
    assert args.embeds is None and args.negative_prompt == ""
    args = parser.parse_args(["--negative_prompt", "blurry, low quality", "--task_name", "t"])
    assert args.embeds is None and args.negative_prompt == "blurry, low quality"
    old = parser.parse_args(["--embeds", "e.safetensors", "--scheduler", "dpmsolver++", "--num_inference_steps", "20"])
    assert old.embeds == "e.safetensors" and old.negative_prompt == "" and old.scheduler == "dpmsolver++" and old.guidance_scale == 7.5
    assert drv.main(["--embeds", "e.safetensors"]) == -1 and drv.main([]) == -1           # parsed; stops at the missing --task_name
    capsys.readouterr()


def _cpu_pipe(text_encoder=True):
    P = pkg()
    from tests.parity import SMALL_UNET
    with torch.device("meta"):
        unet = P.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    te = P.CLIPTextModel(**dict(SMALL, hidden_size=64, num_attention_heads=1)) if text_encoder else None
    return P.I2VAdapterPipeline(unet=unet, text_encoder=te, tokenizer=StubTokenizer(77, 256) if text_encoder else None)


def test_encode_prompt_host_side_errors():
    pipe = _cpu_pipe()
    pe = torch.zeros(1, 77, 64)
    with pytest.raises(TypeError, match="`negative_prompt` should be the same type to `prompt`, but got <class 'list'> != <class 'str'>."):
        pipe.encode_prompt("a", "cpu", 1, True, negative_prompt=["b"], prompt_embeds=pe)
    with pytest.raises(ValueError, match="has batch size 3, but `prompt`: \\['a', 'b'\\] has batch size 2. Please make sure that passed "
                                         "`negative_prompt` matches the batch size of `prompt`."):
        pipe.encode_prompt(["a", "b"], "cpu", 1, True, negative_prompt=["c", "d", "e"], prompt_embeds=torch.zeros(2, 77, 64))
    # given embeddings pass through: repeated per prompt in the reference's order (b0, b0, b1, b1), no tokenizer call
    a, b = torch.randn(2, 77, 64), torch.randn(2, 77, 64)
    p2, n2 = pipe.encode_prompt(None, "cpu", 2, True, prompt_embeds=a, negative_prompt_embeds=b)
    assert torch.equal(p2, a.repeat_interleave(2, 0)) and torch.equal(n2, b.repeat_interleave(2, 0)) and not pipe.tokenizer.calls
    p1, n1 = pipe.encode_prompt(None, "cpu", 1, False, prompt_embeds=a)
    assert torch.equal(p1, a) and n1 is None
    # no CPU path: a prompt reaches the encoder and raises there, after the reference's two tokenizer calls
    with pytest.raises(pkg().HipLibraryError):
        pipe.encode_prompt("a cute pig", "cpu", 1, True)
    assert [c[1:] for c in pipe.tokenizer.calls] == [("max_length", 77), ("longest", None)]


def test_a_prompt_needs_text_encoder_and_tokenizer():
    pipe = _cpu_pipe(text_encoder=False)
    with pytest.raises(ValueError, match="`text_encoder` and a `tokenizer`"):
        pipe(prompt="a", condition_image_latents=torch.zeros(1, 4, 16, 16))
    with pytest.raises(ValueError, match="`text_encoder` and a `tokenizer`"):
        pipe.encode_prompt("a", "cpu", 1, False)
    with pytest.raises(NotImplementedError, match="image encoder"):
        pipe(prompt_embeds=torch.zeros(1, 77, 64), ip_adapter_image=object())
    with pytest.raises(ValueError, match="Provide either `prompt` or `prompt_embeds`"):
        pipe(condition_image_latents=torch.zeros(1, 4, 16, 16))


def test_stub_tokenizer_truncates_like_clip():
    tok = StubTokenizer(8, 256)
    ids = tok("abcdefghij", padding="max_length", max_length=8, truncation=True).input_ids
    assert ids.tolist() == [[254, 97, 98, 99, 100, 101, 102, 255]]
    assert tok(["a", "abc"], padding="longest").input_ids.tolist() == [[254, 97, 255, 255, 255], [254, 97, 98, 99, 255]]
