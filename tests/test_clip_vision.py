"""The CLIP image encoder without a GPU: tests/clip_vision_reference.py pinned against transformers' CLIPVisionModelWithProjection and
against the committed fixture, the module's state-dict keys, checkpoint round trips, the ABI, the constructor's refusals,
`encode_image` on a stub encoder, `load_ip_adapter`'s image-encoder folder and `__call__`'s host-side errors."""
import json
import os
import re
import sys

import pytest
import torch

from tests.clip_vision_reference import (GOLDEN, POS, PREFIX, SMALL, VIT_H, ClipVisionReference, StubFeatureExtractor, fixture_state,
                                         load_fixture, pattern_pixels, pixel_like, seeded_state, state_dict_keys)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the pins compare two fp32 evaluations of the same sums: the bound is fp32 round-off for a machine whose BLAS blocks the sums
# differently -- 2^-24 times the ~100 rounded operations between an input and an output (tests/test_clip_text.py's bound; the patch
# convolution adds one 588-term sum)
PIN_REL = 1e-5
TINY = dict(hidden_size=64, intermediate_size=64, projection_dim=48, num_hidden_layers=1, num_attention_heads=1, num_channels=3,
            image_size=28, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5)


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _rel(got, ref):
    return (got.double() - ref.double()).abs().max().item() / ref.double().abs().max().item()


@pytest.mark.parametrize("act,size", [("gelu", 56), ("quick_gelu", 56), ("gelu", 224)])
def test_reference_against_transformers(act, size):
    pytest.importorskip("transformers")
    sys.path.insert(0, ROOT)
    from tools.make_clip_vision_fixture import transformers_model
    cfg = dict(SMALL, hidden_act=act, image_size=size)
    state = seeded_state(cfg, seed=3, qk_gain=3.0)
    px = pixel_like(2, size, seed=1)
    with torch.no_grad():
        out = transformers_model(cfg, state)(pixel_values=px, output_hidden_states=True)
    embeds, last, hidden = ClipVisionReference(state, cfg)(px, output_hidden_states=True)
    assert len(hidden) == len(out.hidden_states) == cfg["num_hidden_layers"] + 1 and last.shape == (2, (size // 14) ** 2 + 1, 160)
    pairs = [("image_embeds", embeds, out.image_embeds), ("last", last, out.last_hidden_state)]
    for name, got, want in pairs + [(f"hidden {i}", g, w) for i, (g, w) in enumerate(zip(hidden, out.hidden_states))]:
        r = _rel(got, want)
        print(f"{act} {size} {name}: rel {r:.2e}")
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=PIN_REL * want.abs().max().item()), (name, r)
    # what encode_image reads: attribute access, hidden_states[0] AFTER pre_layrnorm
    assert out.image_embeds.shape == (2, 64) and torch.equal(out.hidden_states[-1], out.last_hidden_state)


@pytest.mark.parametrize("size", [56, 224])
def test_reference_against_the_committed_fixture(size):
    for n in ("clip_vision_small.safetensors", "clip_vision_small_224.safetensors"):
        assert os.path.getsize(os.path.join(GOLDEN, n)) < 1024 * 1024
    blob, raw = load_fixture()
    assert all(v.dtype == torch.float16 for v in raw.values()) and sorted(raw) == state_dict_keys(2)
    assert blob["position_embedding_56.weight"].shape == (17, 160) and raw[POS].shape == (257, 160)
    _, state = fixture_state(size)
    cfg = dict(SMALL, image_size=size)
    px = pattern_pixels(2, size)
    assert torch.equal(px.half().float(), px) and px.abs().max() <= 2.0
    ref = ClipVisionReference(state, cfg)
    embeds, last, hidden = ref(px, output_hidden_states=True)
    assert len(hidden) == 3 and last.shape == (2, (size // 14) ** 2 + 1, 160)
    pairs = [("image_embeds", embeds, blob[f"out{size}.image_embeds"])]
    pairs += [(f"hidden {i}", hidden[i], blob[f"out{size}.hidden_states.{i}"]) for i in range(3)]
    for name, got, want in pairs:
        r = _rel(got, want)
        print(f"fixture {size} {name}: rel {r:.2e}")
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=PIN_REL * want.abs().max().item()), (name, r)
    # fp64 agrees with the fp32 run to fp32 round-off as well: the fixture is not pinned to one summation order
    assert _rel(ref.double()(px)[0], blob[f"out{size}.image_embeds"]) <= PIN_REL
    # the restatement is NOT causal: the last patch alone changes the class token's row
    px2 = px.clone()
    px2[:, :, -14:, -14:] += 0.5
    assert not torch.equal(ref(px2)[1][:, 0], last[:, 0])


def test_state_dict_keys_are_the_checkpoints():
    keys = open(os.path.join(GOLDEN, "clip_vision_keys.txt")).read().split()
    assert len(keys) == 521 and PREFIX + "embeddings.position_ids" in keys and PREFIX + "pre_layrnorm.weight" in keys
    with torch.device("meta"):
        m = pkg().CLIPVisionModelWithProjection()
    assert dict(m.config) == VIT_H
    assert sorted(m.state_dict()) == sorted(k for k in keys if not k.endswith("position_ids")) == state_dict_keys(32)
    sd = m.state_dict()
    assert sd[PREFIX + "embeddings.class_embedding"].shape == (1280,)
    assert sd[PREFIX + "embeddings.patch_embedding.weight"].shape == (1280, 3, 14, 14)
    assert sd[POS].shape == (257, 1280) and sd["visual_projection.weight"].shape == (1024, 1280)
    assert sd[PREFIX + "encoder.layers.31.mlp.fc1.weight"].shape == (5120, 1280)


@pytest.mark.parametrize("layout", ["own", "position_ids", "bin"])
def test_save_and_from_pretrained_round_trip(tmp_path, layout):
    """own: save_pretrained's files; position_ids: the file of older releases, with the buffer, beside a transformers-style config.json
    (extra keys); bin: pytorch_model.bin"""
    from safetensors.torch import save_file
    P = pkg()
    _, state = load_fixture()
    m = P.CLIPVisionModelWithProjection(**SMALL)
    m.load_state_dict(state)
    d = str(tmp_path / "image_encoder")
    m.half().save_pretrained(d, safe_serialization=layout != "bin")
    assert sorted(os.listdir(d)) == ["config.json", "pytorch_model.bin" if layout == "bin" else "model.safetensors"]
    if layout == "position_ids":
        st = dict(state, **{PREFIX + "embeddings.position_ids": torch.arange(257)[None]})
        save_file({k: v.contiguous() for k, v in st.items()}, os.path.join(d, "model.safetensors"))
        json.dump(dict(SMALL, architectures=["CLIPVisionModelWithProjection"], model_type="clip_vision_model", dropout=0.0,
                       attention_dropout=0.0, initializer_factor=1.0, torch_dtype="float16"), open(os.path.join(d, "config.json"), "w"))
    back = P.CLIPVisionModelWithProjection.from_pretrained(d)
    assert dict(back.config) == dict(m.config) and not back.training
    for k, v in m.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    if layout != "bin":
        save_file({"nonsense.weight": torch.zeros(1)}, os.path.join(d, "model.safetensors"))
        with pytest.raises(RuntimeError, match="missing keys"):
            P.CLIPVisionModelWithProjection.from_pretrained(d)
    assert P.CLIPVisionModelWithProjection.from_config(dict(TINY, unknown=1)).config.hidden_size == 64


def test_constructor_refusals_and_no_cpu_path():
    P = pkg()
    V = P.CLIPVisionModelWithProjection
    with pytest.raises(NotImplementedError, match="i2v_clip_vision_attention_f16.*head_dim 64 and 80"):
        V(**dict(TINY, hidden_size=80, num_attention_heads=2))                                # head_dim 40
    with pytest.raises(NotImplementedError, match="577 tokens.*i2v_clip_vision_attention_f16.*at most 288"):
        V(**dict(TINY, image_size=336))
    with pytest.raises(NotImplementedError, match="i2v_clip_patchify_f16"):
        V(**dict(TINY, image_size=30))
    with pytest.raises(NotImplementedError, match="hidden_act"):
        V(**dict(TINY, hidden_act="relu"))
    assert P.clip_vision.MAX_TOKENS == 288 and P.clip_vision.HEAD_DIMS == (64, 80)
    V(**dict(TINY, image_size=224, patch_size=14, hidden_act="quick_gelu"))                     # 257 tokens, OpenAI's activation
    with pytest.raises(NotImplementedError, match="290 tokens"):
        V(**dict(TINY, image_size=238))                                                        # 17 x 17 + 1 = 290 > 288
    m = V(**TINY)
    with pytest.raises(ValueError, match="expected \\[batch, 3, 28, 28\\]"):
        m(torch.zeros(1, 3, 56, 56))
    with pytest.raises(P.HipLibraryError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 28, 28))
    out = P.clip_vision.CLIPVisionModelOutput("embeds", "last", ("h0", "h1"))
    assert out[0] == "embeds" and out[1] == "last" and out[-1] == ("h0", "h1") and len(out) == 3 and out.image_embeds == "embeds"
    assert P.clip_vision.CLIPVisionModelOutput("embeds", "last")[-1] == "last"
    assert callable(P.clip_vision.init_clip_vision_weights_)
    # the layer modules and helpers are the text tower's, not copies
    assert P.clip_vision.CLIPEncoder is P.clip_text.CLIPEncoder and P.clip_vision.encoder_layer is P.clip_text.encoder_layer


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
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 18
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for name in ("i2v_clip_patchify_f16", "i2v_clip_vision_embed_f16", "i2v_clip_vision_attention_f16"):
        assert hasattr(h, name) and name in lib.SIGNATURES and name in src
    assert lib.SIGNATURES["i2v_clip_vision_attention_f16"] == lib.SIGNATURES["i2v_clip_attention_f16"]
    P = pkg()
    K = P.kernels
    assert callable(K.clip_patchify) and callable(K.clip_vision_embed) and callable(K.clip_vision_attention)
    for k in ("clip_patchify", "clip_vision_embed", "clip_vision_attention"):
        assert k in P.profiling._WRAPPED


# ------------------------------------------------------------------------------------------------------------ the pipeline, on stubs
class StubImageEncoder(torch.nn.Module):
    """the call interface of CLIPVisionModelWithProjection on the CPU: embeds = per-image channel means through a fixed matrix"""

    def __init__(self, dim=48):
        super().__init__()
        self.w = torch.nn.Parameter(torch.arange(3 * dim, dtype=torch.float32).view(dim, 3) / dim)
        self.calls = []

    @torch.no_grad()
    def forward(self, pixel_values, output_hidden_states=False):
        self.calls.append((tuple(pixel_values.shape), bool(output_hidden_states), bool((pixel_values == 0).all())))
        mean = pixel_values.float().mean(dim=(2, 3))
        embeds = mean @ self.w.t()
        hs = tuple((embeds[:, None, :] + i).expand(-1, 5, -1) for i in range(3))
        from i2v_adapter_unofficial_amd.clip_vision import CLIPVisionModelOutput
        return CLIPVisionModelOutput(embeds, hs[-1], hs if output_hidden_states else None)


def _cpu_pipe(image_encoder=None, feature_extractor=None, ip=False):
    P = pkg()
    from tests.parity import SMALL_UNET, sd15_ip_state_dict
    if ip:
        unet = P.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
        unet._load_ip_adapter_weights(sd15_ip_state_dict(unet, clip_dim=48))
    else:
        with torch.device("meta"):
            unet = P.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    return P.I2VAdapterPipeline(unet=unet, image_encoder=image_encoder, feature_extractor=feature_extractor)


def test_encode_image_on_a_stub_encoder():
    import PIL.Image
    enc, fe = StubImageEncoder(), StubFeatureExtractor(28)
    pipe = _cpu_pipe(enc, fe)
    px = pixel_like(2, 28, seed=2)
    # plain branch: embeds repeated per prompt in the reference's order (a, a, a, b, b, b), zero negatives, one encoder call
    e, n = pipe.encode_image(px, "cpu", 3)
    want = enc(px).image_embeds
    assert e.shape == (6, 48) and torch.equal(e, want.repeat_interleave(3, dim=0)) and torch.equal(n, torch.zeros_like(e))
    assert not torch.equal(e[0], e[3]) and fe.calls == 0
    enc.calls.clear()
    pipe.encode_image(px, "cpu", 1)
    assert enc.calls == [((2, 3, 28, 28), False, False)]
    # hidden-states branch: the penultimate states of the image and of a ZERO image
    enc.calls.clear()
    h, hn = pipe.encode_image(px, "cpu", 2, output_hidden_states=True)
    assert enc.calls == [((2, 3, 28, 28), True, False), ((2, 3, 28, 28), True, True)]
    assert h.shape == hn.shape == (4, 5, 48) and torch.equal(h, (want[:, None, :] + 1).expand(-1, 5, -1).repeat_interleave(2, dim=0))
    assert torch.equal(hn, torch.ones(4, 5, 48))
    # anything but a tensor goes through the feature extractor
    img = PIL.Image.fromarray((torch.rand(40, 50, 3, generator=torch.Generator().manual_seed(0)) * 255).to(torch.uint8).numpy())
    e1, _ = pipe.encode_image(img, "cpu", 1)
    e2, _ = pipe.encode_image([img, img], "cpu", 1)
    assert fe.calls == 2 and e1.shape == (1, 48) and e2.shape == (2, 48) and torch.allclose(e2[0], e1[0], rtol=1e-6, atol=0)
    assert torch.equal(e1, enc(fe(img).pixel_values).image_embeds)
    with pytest.raises(ValueError, match="feature_extractor"):
        _cpu_pipe(StubImageEncoder(), None).encode_image(img, "cpu", 1)
    with pytest.raises(ValueError, match="image_encoder"):
        _cpu_pipe(None, fe).encode_image(px, "cpu", 1)


def test_call_errors_for_ip_adapter_image():
    px = torch.zeros(1, 3, 28, 28)
    lat = torch.zeros(1, 4, 16, 16)
    pe = torch.zeros(1, 77, 64)
    # no image encoder: NotImplementedError that says how to get one (tests/test_clip_text.py pins the words `image encoder`)
    with pytest.raises(NotImplementedError, match="image encoder.*load_ip_adapter.*image_encoder"):
        _cpu_pipe()(prompt_embeds=pe, ip_adapter_image=px, condition_image_latents=lat)
    with pytest.raises(NotImplementedError, match="image encoder"):
        _cpu_pipe(ip=True)(prompt_embeds=pe, ip_adapter_image=px, condition_image_latents=lat)
    # both forms of the image prompt
    with pytest.raises(ValueError, match="both `ip_adapter_image` and `image_embeds`"):
        _cpu_pipe(StubImageEncoder(), ip=True)(prompt_embeds=pe, ip_adapter_image=px, image_embeds=torch.zeros(1, 48),
                                               condition_image_latents=lat)
    # an encoder but no IP-Adapter in the UNet: the reference would encode and ignore it
    enc = StubImageEncoder()
    with pytest.raises(ValueError, match="load_ip_adapter"):
        _cpu_pipe(enc)(prompt_embeds=pe, ip_adapter_image=px, condition_image_latents=lat)
    assert enc.calls == []


def _write_ip_folder(root, unet, with_encoder):
    from tests.parity import sd15_ip_state_dict
    os.makedirs(os.path.join(root, "models"))
    torch.save(sd15_ip_state_dict(unet, clip_dim=48), os.path.join(root, "models", "ip-adapter_sd15.bin"))
    if with_encoder:
        m = pkg().CLIPVisionModelWithProjection(**TINY)
        m.load_state_dict(seeded_state(TINY, seed=4))
        m.half().save_pretrained(os.path.join(root, "models", "image_encoder"))
        return m


@pytest.mark.parametrize("with_encoder", [True, False])
def test_load_ip_adapter_loads_the_image_encoder_folder(tmp_path, with_encoder):
    P = pkg()
    pipe = _cpu_pipe()
    pipe.unet = P.UNetMotionCrossFrameAttnModel(**__import__("tests.parity", fromlist=["SMALL_UNET"]).SMALL_UNET)
    saved = _write_ip_folder(str(tmp_path), pipe.unet, with_encoder)
    assert pipe.image_encoder is None and pipe.feature_extractor is None and pipe.unet.encoder_hid_proj is None
    pipe.load_ip_adapter(str(tmp_path), subfolder="models", weight_name="ip-adapter_sd15.bin")
    assert pipe.unet.encoder_hid_proj is not None
    if with_encoder:
        assert isinstance(pipe.image_encoder, P.CLIPVisionModelWithProjection) and dict(pipe.image_encoder.config) == TINY
        assert pipe.image_encoder.dtype == pipe.unet.dtype
        for k, v in saved.state_dict().items():
            assert torch.equal(pipe.image_encoder.state_dict()[k].float(), v.float()), k
    else:
        assert pipe.image_encoder is None                                                       # today's behaviour
    try:
        from transformers import CLIPImageProcessor
        assert isinstance(pipe.feature_extractor, CLIPImageProcessor)
    except ImportError:
        assert pipe.feature_extractor is None
    # an encoder and a feature extractor the pipeline already holds are kept; a state dict has no folder to look into
    enc, fe = StubImageEncoder(), StubFeatureExtractor(28)
    pipe2 = _cpu_pipe(enc, fe)
    pipe2.unet = pipe.unet
    pipe2.load_ip_adapter(str(tmp_path), subfolder="models", weight_name="ip-adapter_sd15.bin")
    assert pipe2.image_encoder is enc and pipe2.feature_extractor is fe
    pipe3 = _cpu_pipe()
    pipe3.unet = pipe.unet
    pipe3.load_ip_adapter(torch.load(os.path.join(str(tmp_path), "models", "ip-adapter_sd15.bin"), weights_only=True))
    assert pipe3.image_encoder is None
    # to() moves the image encoder with the rest
    if with_encoder:
        pipe.to("cpu", torch.float32)
        assert pipe.image_encoder.dtype == torch.float32


def test_the_driver_command_line():
    drv = pkg().pipeline_i2v_adapter
    parser = drv.build_parser()
    assert parser.parse_args([]).ip_adapter is False
    args = parser.parse_args(["--ip_adapter", "--ip_adapter_path", "x"])
    assert args.ip_adapter is True and args.ip_adapter_path == "x" and args.embeds is None


def test_stub_feature_extractor_normalises_like_clip():
    fe = StubFeatureExtractor(28)
    pv = fe(torch.full((3, 10, 12), 0.5)).pixel_values
    assert pv.shape == (1, 3, 28, 28)
    want = (0.5 - torch.tensor(fe.mean)) / torch.tensor(fe.std)
    assert torch.allclose(pv[0, :, 0, 0], want)
