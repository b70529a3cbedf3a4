"""IP-Adapter Plus on the host side (no GPU): the loader's Plus branch and its converter, the error cases, the file round trip, the
pipeline's scale setter and shape checks, the ABI.  The kernels and the numbers are tests/test_ip_adapter_plus_gpu.py's."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.ip_adapter_plus_reference import converted_image_proj, plus_state_dict  # noqa: E402
from tests.parity import SMALL_UNET, sd15_ip_state_dict  # noqa: E402


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


@pytest.fixture(scope="module")
def unet():
    return pkg().UNetMotionCrossFrameAttnModel(**SMALL_UNET)


def _snapshot(unet):
    return (type(unet.encoder_hid_proj).__name__, unet.config.get("encoder_hid_dim_type"), sorted(unet.state_dict().keys()),
            [(a.ip_num_tokens, a.ip_scale) for a in unet._cross_attention_layers()])


def test_plus_state_dict_loads(unet):
    """fails on the parent commit: NotImplementedError("only the plain IP-Adapter ...")"""
    P = pkg()
    sd = plus_state_dict(unet, embed_dims=48, hidden=128, heads=2, depth=2, num_queries=8)
    unet._load_ip_adapter_weights(sd)
    proj = unet.encoder_hid_proj
    assert isinstance(proj, P.blocks.Resampler) and unet.config.encoder_hid_dim_type == "ip_image_proj"
    assert (proj.embed_dims, proj.output_dims, proj.hidden_dims, proj.depth, proj.dim_head, proj.heads, proj.num_queries, proj.ffn_ratio) == \
        (48, SMALL_UNET["cross_attention_dim"], 128, 2, 64, 2, 8, 4)
    layers = unet._cross_attention_layers()
    assert len(layers) == 16 and all(a.ip_num_tokens == 8 and a.ip_scale == 1.0 for a in layers)
    for i, a in enumerate(layers):
        assert torch.equal(a.to_k_ip.weight, sd["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"])
        assert torch.equal(a.to_v_ip.weight, sd["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"])
    # motion modules and every other attention are untouched; the Resampler's attention is not an attention processor
    for name, proc in unet.attn_processors.items():
        assert proc.num_tokens == (8 if name.endswith("attn2.processor") and "motion_modules" not in name else 0), name
        assert not name.startswith("encoder_hid_proj")
    assert not any("_ip" in k for k in unet.state_dict() if "motion_modules" in k)
    # the Resampler holds the file's values, both halves of to_kv in place
    got, ip = proj.state_dict(), sd["image_proj"]
    assert torch.equal(got["layers.1.2.to_k.weight"], ip["layers.1.0.to_kv.weight"][:128])
    assert torch.equal(got["layers.1.2.to_v.weight"], ip["layers.1.0.to_kv.weight"][128:])
    assert torch.equal(got["layers.0.3.1.net.0.proj.weight"], ip["layers.0.1.1.weight"]) and torch.equal(got["latents"], ip["latents"])
    # loading the plain adapter afterwards restores 4 tokens and the plain branch
    unet._load_ip_adapter_weights(sd15_ip_state_dict(unet, clip_dim=48))
    assert isinstance(unet.encoder_hid_proj, P.blocks.ImageProjection) and all(a.ip_num_tokens == 4 for a in unet._cross_attention_layers())


def test_converted_keys_match_the_golden_list():
    """the SD-1.5 Plus geometry (1280 -> 768, 12 heads, depth 4, 16 queries) against a hand-written key + shape list"""
    P = pkg()
    with torch.device("meta"):
        big = P.UNetMotionCrossFrameAttnModel(**{**SMALL_UNET, "cross_attention_dim": 768})
        sd = plus_state_dict(big, embed_dims=1280, hidden=768, heads=12, depth=4, num_queries=16)
    kwargs, conv = P.unet_motion_cross_frame_attn.convert_ip_adapter_plus_image_proj(sd["image_proj"])
    assert kwargs == dict(embed_dims=1280, output_dims=768, hidden_dims=768, depth=4, dim_head=64, heads=12, num_queries=16, ffn_ratio=4)
    want = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "ip_adapter_plus_keys.txt")):
        key, *shape = line.split()
        want[key] = tuple(int(s) for s in shape)
    assert {k: tuple(v.shape) for k, v in conv.items()} == want
    with torch.device("meta"):
        assert {k: tuple(v.shape) for k, v in P.blocks.Resampler(**kwargs).state_dict().items()} == want


def test_to_kv_halves_land_in_to_k_and_to_v(unet):
    sd = plus_state_dict(unet)
    conv = converted_image_proj(sd)
    kv = sd["image_proj"]["layers.0.0.to_kv.weight"]
    assert torch.equal(conv["layers.0.2.to_k.weight"], kv[: kv.shape[0] // 2]) and torch.equal(conv["layers.0.2.to_v.weight"], kv[kv.shape[0] // 2:])
    assert not torch.equal(conv["layers.0.2.to_k.weight"], conv["layers.0.2.to_v.weight"])


def test_error_cases_leave_the_model_unchanged(unet):
    unet._load_ip_adapter_weights(sd15_ip_state_dict(unet, clip_dim=48))
    before = _snapshot(unet)
    good = plus_state_dict(unet)

    def variant(**changes):
        ip = dict(good["image_proj"])
        for k, v in changes.items():
            if v is None:
                ip.pop(k)
            else:
                ip[k] = v
        return {"image_proj": ip, "ip_adapter": good["ip_adapter"]}

    with pytest.raises(NotImplementedError, match="Full Face"):
        unet._load_ip_adapter_weights(variant(**{"proj.3.weight": torch.zeros(4, 4)}))
    assert _snapshot(unet) == before
    with pytest.raises(ValueError, match=r"missing key layers\.1\.0\.to_kv\.weight"):
        unet._load_ip_adapter_weights(variant(**{"layers.1.0.to_kv.weight": None}))
    assert _snapshot(unet) == before
    with pytest.raises(ValueError, match=r"unexpected key layers\.0\.0\.to_k\.weight"):
        unet._load_ip_adapter_weights(variant(**{"layers.0.0.to_k.weight": torch.zeros(128, 128)}))
    assert _snapshot(unet) == before
    with pytest.raises(ValueError, match=r"layers\.0\.0\.to_q\.weight has 96 rows.*multiple of the head dimension 64"):
        unet._load_ip_adapter_weights(variant(**{"layers.0.0.to_q.weight": torch.zeros(96, 128)}))
    assert _snapshot(unet) == before
    # the kernel's envelope, at load: T + num_queries <= 288 when T is known, num_queries <= 64
    with pytest.raises(NotImplementedError, match=r"281 image tokens \+ 8 queries.*at most 288"):
        unet._load_ip_adapter_weights(good, num_image_tokens=281)
    assert _snapshot(unet) == before
    with pytest.raises(NotImplementedError, match=r"num_queries 65.*1 to 64"):
        unet._load_ip_adapter_weights(plus_state_dict(unet, num_queries=65))
    assert _snapshot(unet) == before
    missing = {"image_proj": good["image_proj"], "ip_adapter": {k: v for k, v in good["ip_adapter"].items() if k != "31.to_v_ip.weight"}}
    with pytest.raises(ValueError, match=r"missing key 31\.to_v_ip\.weight"):
        unet._load_ip_adapter_weights(missing)
    assert _snapshot(unet) == before
    unet._load_ip_adapter_weights(good, num_image_tokens=280)          # 280 + 8 = 288 itself loads
    assert unet.encoder_hid_proj.num_queries == 8


def test_plain_adapter_tree_and_keys_are_as_before():
    """the plain branch: the module tree and the keys the parent commit's loader made (ImageProjection's four tensors, to_k_ip /
    to_v_ip on the 16 attn2 layers, nothing else)"""
    P = pkg()
    base = P.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    keys0 = set(base.state_dict())
    base._load_ip_adapter_weights(sd15_ip_state_dict(base, clip_dim=48))
    added = set(base.state_dict()) - keys0
    assert {k for k in added if k.startswith("encoder_hid_proj.")} == {"encoder_hid_proj." + k for k in (
        "image_embeds.weight", "image_embeds.bias", "norm.weight", "norm.bias")}
    rest = sorted(k for k in added if not k.startswith("encoder_hid_proj."))
    assert len(rest) == 32 and all(k.endswith(("attn2.to_k_ip.weight", "attn2.to_v_ip.weight")) and "motion_modules" not in k for k in rest)
    assert isinstance(base.encoder_hid_proj, P.blocks.ImageProjection) and base.encoder_hid_proj.num_image_text_embeds == 4


def test_file_round_trip_bin_and_safetensors(unet, tmp_path):
    from safetensors.torch import save_file
    from i2v_adapter_unofficial_amd.checkpoint import load_ip_adapter_file
    sd = plus_state_dict(unet)
    torch.save(sd, tmp_path / "ip-adapter-plus_sd15.bin")
    save_file({f"{a}.{k}": v.contiguous() for a, d in sd.items() for k, v in d.items()}, str(tmp_path / "ip-adapter-plus_sd15.safetensors"))
    for back in (load_ip_adapter_file(str(tmp_path), weight_name="ip-adapter-plus_sd15.bin"),
                 load_ip_adapter_file(str(tmp_path / "ip-adapter-plus_sd15.safetensors"))):
        assert set(back) == {"image_proj", "ip_adapter"}
        for part in sd:
            assert set(back[part]) == set(sd[part]) and all(torch.equal(back[part][k], v) for k, v in sd[part].items())
        unet._load_ip_adapter_weights(back)
        assert unet.encoder_hid_proj.num_queries == 8


def _pipe(unet):
    return pkg().I2VAdapterPipeline(unet=unet)


def test_set_ip_adapter_scale_changes_the_graph_key(unet):
    unet._load_ip_adapter_weights(plus_state_dict(unet))
    pipe = _pipe(unet)
    st = dict(latents=torch.zeros(1, 2, 4, 8, 8), copies=2, num_frames=2, guidance=7.5, t_table=torch.zeros(3), ctx_text=torch.zeros(2, 7, 64),
              ctx_ip=torch.zeros(2, 8, 64), coef=torch.zeros(3, 4))
    k1 = pipe._graph_key(st)
    pipe.set_ip_adapter_scale(0.5)
    k2 = pipe._graph_key(st)
    assert k1 != k2 and all(a.ip_scale == 0.5 for a in unet._cross_attention_layers())
    scales = lambda k: [t for t in k if isinstance(t, tuple) and len(t) == 16 and all(isinstance(e, tuple) and len(e) == 2 for e in t)]
    assert scales(k1) == [tuple((8, 1.0) for _ in range(16))] and scales(k2) == [tuple((8, 0.5) for _ in range(16))]
    assert [a for a in k1 if a not in scales(k1)] == [a for a in k2 if a not in scales(k2)]
    # motion modules' attentions carry no image branch and keep their scale
    mods = dict(unet.named_modules())
    assert all(mods[n[: -len(".processor")]].ip_scale == 1.0 for n in unet.attn_processor_names() if "motion_modules" in n)


def test_image_embeds_shape_errors(unet):
    cond = torch.zeros(1, 4, 8, 8)
    kw = dict(prompt_embeds=torch.zeros(1, 7, 64), negative_prompt_embeds=torch.zeros(1, 7, 64), condition_image_latents=cond,
              num_inference_steps=1)
    unet._load_ip_adapter_weights(plus_state_dict(unet))
    with pytest.raises(ValueError, match=r"`image_embeds` has shape \(1, 48\): IP-Adapter Plus is loaded \(Resampler\).*\[batch, tokens, 48\]"):
        _pipe(unet)(image_embeds=torch.zeros(1, 48), **kw)
    with pytest.raises(ValueError, match=r"`negative_image_embeds` has shape \(1, 48\)"):
        _pipe(unet)(image_embeds=torch.zeros(1, 5, 48), negative_image_embeds=torch.zeros(1, 48), **kw)
    unet._load_ip_adapter_weights(sd15_ip_state_dict(unet, clip_dim=48))
    with pytest.raises(ValueError, match=r"`image_embeds` has shape \(1, 5, 48\): the plain IP-Adapter is loaded \(ImageProjection\).*\[batch, embed_dim\]"):
        _pipe(unet)(image_embeds=torch.zeros(1, 5, 48), **kw)


def test_resampler_envelope_and_inputs():
    R = pkg().blocks.Resampler
    with torch.device("meta"):
        with pytest.raises(NotImplementedError, match="dim_head 80.*head_dim 64 only"):
            R(dim_head=80)
        with pytest.raises(NotImplementedError, match="num_queries 65"):
            R(num_queries=65)
        r = R(embed_dims=48, output_dims=64, hidden_dims=128, depth=1, heads=2, num_queries=16)
    r.check_tokens(272)
    with pytest.raises(NotImplementedError, match=r"273 image tokens \+ 16 queries.*at most 288"):
        r.check_tokens(273)
    with pytest.raises(ValueError, match=r"\[batch, tokens, 48\]"):
        r(torch.zeros(2, 48))


def test_export_denoiser_refuses_a_resampler(unet):
    unet._load_ip_adapter_weights(plus_state_dict(unet))
    with pytest.raises(NotImplementedError, match="IP-Adapter Plus"):
        pkg().handle.export_denoiser(_pipe(unet), "/nonexistent", batch=1, num_frames=2, latent_height=8, latent_width=8, ctx_len=7, clip_dim=48)


def test_driver_flags():
    src = open(os.path.join(ROOT, "i2v-adapter-unofficial_amd", "pipeline_i2v_adapter.py")).read()
    assert '"--ip_adapter_weight_name", type=str, default="ip-adapter_sd15.bin"' in src and '"--ip_adapter_scale"' in src
    assert "weight_name=args.ip_adapter_weight_name" in src


@pytest.fixture(scope="module")
def lib():
    p = pkg()
    if not os.path.exists(p._lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return p._lib


def test_abi_version_and_symbol(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 21
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    name = "i2v_perceiver_attention_f16"
    assert hasattr(h, name) and name in lib.SIGNATURES and name in src and len(lib.SIGNATURES[name][1]) == 21
    assert callable(pkg().kernels.perceiver_attention) and "perceiver_attention" in pkg().profiling._WRAPPED
