"""The CLIP text encoder on the GPU, through the C ABI: the embedding, quick-GELU and causal-attention kernels against their exact or
float64 yardsticks, the attention kernel's exact properties (causality, no pad leakage, batch / head independence, the unsupported
envelope), the whole tower against tests/clip_text_reference.py, and `pipe(prompt=...)` on the reduced UNet.

The accuracy gates are relative to what fp16 torch itself loses on the same problem, computed in the test: the kernel's (the model's)
error over max|ref| may be at most TWICE that of torch's fp16 CPU evaluation against the same float64 (fp32) yardstick.  Every
measured pair goes to $I2V_CLIP_TEXT_LOG as JSON lines (profiles/clip_text_errors.jsonl is one such run)."""
import ctypes as C
import os

import pytest
import torch

from tests.clip_text_reference import PREFIX, ClipTextReference, StubTokenizer, causal_attention, prompt_like_ids, seeded_state
from tests.parity import SMALL_UNET, fp16_gate, hip_model_random

pytestmark = pytest.mark.gpu
f16 = torch.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 2.0
SMALL = dict(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
             max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=255)


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _gate(name, got, half, ref, **extra):
    fp16_gate(name, got, half, ref, FACTOR, "I2V_CLIP_TEXT_LOG", **extra)


# ------------------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("B,L", [(1, 1), (3, 5), (2, 77)])
def test_embed_kernel_is_exact(dev, B, L):
    K = pkg().kernels
    vocab, hidden, positions = 50, 72, 77
    g = torch.Generator().manual_seed(B * 100 + L)
    tok, pos = torch.randn(vocab, hidden, generator=g).half(), torch.randn(positions, hidden, generator=g).half()
    ids = torch.randint(0, vocab, (B, L), generator=g)
    ids.view(-1)[-1] = vocab - 1
    if ids.numel() > 1:
        ids.view(-1)[0] = 0
    want = (tok.float()[ids] + pos.float()[:L]).half().view(B * L, hidden)
    for given in (ids, ids.to(torch.int32).to(dev)):                     # host int64 / device int32 ids
        got = K.clip_embed(tok.to(dev), pos.to(dev), given)
        assert got.shape == (B * L, hidden) and torch.equal(got.cpu(), want)


def test_embed_rejects_on_the_host(dev):
    P = pkg()
    K, lib = P.kernels, P._lib.load()
    vocab, hidden = 50, 72
    tok, pos = torch.zeros(vocab, hidden, dtype=f16, device=dev), torch.zeros(77, hidden, dtype=f16, device=dev)
    ids = torch.tensor([[0, vocab, 1]])
    with pytest.raises(P.HipLibraryError, match="status -1.*token id 50 at \\(0, 1\\)"):
        K.clip_embed(tok, pos, ids)
    with pytest.raises(P.HipLibraryError, match="status -1"):
        K.clip_embed(tok, pos, torch.tensor([[-1]]))
    with pytest.raises(P.HipLibraryError, match="status -1.*78 tokens"):
        K.clip_embed(tok, pos, torch.zeros(1, 78, dtype=torch.int64))
    # nothing was launched: the raw entry point leaves a sentinel-filled output alone
    out = torch.full((3, hidden), 7.0, dtype=f16, device=dev)
    host = ids.to(torch.int32).contiguous()
    d = host.to(dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.i2v_clip_embed_f16(p(tok), p(pos), p(d), p(host), p(out), 1, 3, vocab, 77, hidden, st) == -1
    assert lib.i2v_clip_embed_f16(p(tok), p(pos), p(d), p(host), p(out), 1, 3, vocab + 1, 77, 36, st) == -1      # hidden % 8
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ quick-GELU
def _ulp16(v):
    """spacing of fp16 at |v| (subnormal spacing 2^-24 below 2^-14)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))).clamp(-14, 15)
    return torch.pow(2.0, e - 10)


@pytest.mark.parametrize("n", [1, 7, 8, 77 * 3072 + 3])
@pytest.mark.parametrize("in_place", [False, True])
def test_quick_gelu_within_one_ulp(dev, n, in_place):
    K = pkg().kernels
    g = torch.Generator().manual_seed(n)
    special = torch.tensor([65504.0, -65504.0, 0.0, -0.0, 6e-8, -6e-8, 3e-5, -3e-5, 1.0, -1.0, 10.0, -10.0, -60.0]).half()
    x = (torch.randn(n, generator=g) * 3).half()
    k = min(n, special.numel())
    x[:k] = special[:k]
    ref = x.float() * torch.sigmoid(1.702 * x.float())
    xd = x.to(dev)
    got = K.quick_gelu(xd, out=xd if in_place else None)
    assert (got.data_ptr() == xd.data_ptr()) == in_place
    if not in_place:
        assert torch.equal(xd.cpu(), x)
    diff = (got.float().cpu() - ref).abs()
    assert torch.isfinite(got).all() and bool((diff <= _ulp16(ref)).all()), (diff / _ulp16(ref)).max().item()


def test_quick_gelu_unaligned_and_overlapping(dev):
    P = pkg()
    K = P.kernels
    base = (torch.randn(4099, generator=torch.Generator().manual_seed(1)) * 3).half().to(dev)
    x = base[1:]                                                          # 2 bytes off a 16-byte boundary: the one-value-per-lane form
    assert x.data_ptr() % 16 == 2
    ref = x.float().cpu() * torch.sigmoid(1.702 * x.float().cpu())
    got = K.quick_gelu(x)
    assert bool(((got.float().cpu() - ref).abs() <= _ulp16(ref)).all())
    with pytest.raises(P.HipLibraryError, match="status -1"):
        K.quick_gelu(base[:4000], out=base[8:4008])


# ------------------------------------------------------------------------------------------------------------ attention
def _qkv(B, L, heads, gain, seed, extra_rows=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B * L + extra_rows, 3 * heads * 64, generator=g)
    t[:, : heads * 64] *= gain                      # q.k over d = 64 at unit variance has std 8; x 1/8: logits of std `gain`
    return t.half()


def _split(qkv, B, L, heads):
    hid = heads * 64
    return [qkv[: B * L, i * hid:(i + 1) * hid].reshape(B, L, heads, 64).transpose(1, 2) for i in range(3)]


def _attn(dev, qkv, B, L, heads):
    return pkg().kernels.clip_attention(qkv.to(dev), batch=B, length=L, heads=heads, head_dim=64)


@pytest.mark.parametrize("L", [1, 15, 16, 17, 77, 128])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("heads", [1, 2, 12])
def test_attention_against_float64(dev, heads, B, L):
    for gain in (2.0, 6.0):
        qkv = _qkv(B, L, heads, gain, seed=L * 10 + B)
        q, k, v = _split(qkv, B, L, heads)
        ref = causal_attention(q.double(), k.double(), v.double(), 0.125)
        half = causal_attention(q, k, v, 0.125)
        got = _attn(dev, qkv, B, L, heads).view(B, L, heads, 64).transpose(1, 2)
        _gate(f"clip_attention heads={heads} B={B} L={L} logit_std={gain}", got, half, ref)


@pytest.mark.parametrize("j", [1, 16, 17, 76])
def test_attention_is_causal_bit_for_bit(dev, j):
    B, L, heads = 2, 77, 2
    a = _qkv(B, L, heads, 2.0, seed=1)
    b = a.clone()
    other = _qkv(B, L, heads, 2.0, seed=2).view(B, L, -1)
    b.view(B, L, -1)[:, j:] = other[:, j:] * 3
    oa, ob = _attn(dev, a, B, L, heads).view(B, L, -1), _attn(dev, b, B, L, heads).view(B, L, -1)
    assert torch.equal(oa[:, :j], ob[:, :j]) and not torch.equal(oa[:, j:], ob[:, j:])


@pytest.mark.parametrize("B,L", [(1, 1), (1, 15), (2, 17), (1, 77), (2, 77)])
def test_attention_pad_rows_do_not_leak(dev, B, L):
    K = pkg().kernels
    heads, extra = 2, 64
    buf = _qkv(B, L, heads, 2.0, seed=L, extra_rows=extra).to(dev)
    outs = []
    for fill in (0.0, 1e4):
        buf[B * L:] = fill
        obuf = torch.full((B * L + extra, heads * 64), -77.0, dtype=f16, device=dev)
        K.clip_attention(buf[: B * L], batch=B, length=L, heads=heads, head_dim=64, out=obuf[: B * L])
        assert bool((obuf[B * L:] == -77.0).all())
        assert torch.isfinite(obuf[: B * L]).all() and not bool((obuf[: B * L] == -77.0).all(dim=1).any())
        outs.append(obuf[: B * L].clone())
    assert torch.equal(outs[0], outs[1])


def test_attention_batches_and_heads_are_independent(dev):
    B, L, heads = 3, 17, 12
    qkv = _qkv(B, L, heads, 2.0, seed=5)
    out = _attn(dev, qkv, B, L, heads).view(B, L, heads, 64)
    perm = [2, 0, 1]
    out_p = _attn(dev, qkv.view(B, L, -1)[perm].reshape(B * L, -1), B, L, heads).view(B, L, heads, 64)
    assert torch.equal(out_p, out[perm])
    hp = torch.randperm(heads, generator=torch.Generator().manual_seed(0))
    qh = qkv.view(B * L, 3, heads, 64)[:, :, hp].reshape(B * L, -1).contiguous()
    assert torch.equal(_attn(dev, qh, B, L, heads).view(B, L, heads, 64), out[:, :, hp.to(dev)])
    # one batch entry alone, and a strided view of a wider buffer (offsets and row stride are the caller's)
    assert torch.equal(_attn(dev, qkv[L: 2 * L], 1, L, heads).view(L, heads, 64), out[1])
    wide = torch.zeros(B * L, 3 * heads * 64 + 16, dtype=f16, device=dev)
    wide[:, 8: 8 + 3 * heads * 64] = qkv.to(dev)
    hid = heads * 64
    got = pkg().kernels.clip_attention(wide, batch=B, length=L, heads=heads, head_dim=64, q_off=8, k_off=8 + hid, v_off=8 + 2 * hid)
    assert torch.equal(got.view(B, L, heads, 64), out)


def test_attention_outside_the_envelope_is_unsupported(dev):
    P = pkg()
    lib = P._lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    qkv = torch.zeros(129, 3 * 64, dtype=f16, device=dev)
    out = torch.full((129, 64), 5.0, dtype=f16, device=dev)
    assert lib.i2v_clip_attention_f16(p(qkv), 192, 0, 64, 128, p(out), 64, 1, 129, 1, 64, 0.125, st) == -2
    assert b"129 positions" in lib.i2v_last_error()
    assert lib.i2v_clip_attention_f16(p(qkv), 192, 0, 64, 128, p(out), 64, 1, 64, 2, 32, 0.125, st) == -2
    assert b"head_dim 32" in lib.i2v_last_error()
    assert lib.i2v_clip_attention_f16(p(qkv), 192, 0, 60, 128, p(out), 64, 1, 64, 1, 64, 0.125, st) == -1         # offset % 8
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    with pytest.raises(P.HipLibraryError, match="status -2"):
        P.kernels.clip_attention(qkv, batch=1, length=129, heads=1, head_dim=64)


# ------------------------------------------------------------------------------------------------------------ the whole tower
_MODELS = {}


def _model(dev, cfg, seed):
    """(HIP model on the device, fp32 reference, fp16 reference) of one seeded state, built once per configuration"""
    key = (tuple(sorted(cfg.items())), seed)
    if key not in _MODELS:
        if cfg == SMALL and seed is None:
            from safetensors.torch import load_file
            blob = load_file(os.path.join(ROOT, "tests", "golden", "clip_text_small.safetensors"))
            state = {k: v.float() for k, v in blob.items() if k.startswith(PREFIX)}
        else:
            state = seeded_state(cfg, seed=seed, qk_gain=3.0)
        m = pkg().CLIPTextModel(**cfg)
        m.load_state_dict(state)
        ref = ClipTextReference(state, cfg)
        _MODELS[key] = (m.half().to(dev).eval(), ref, ref.half())
    return _MODELS[key]


def _check_model(dev, cfg, seed, ids, name):
    m, ref, ref16 = _model(dev, cfg, seed)
    out = m(ids, output_hidden_states=True)
    want, want_h = ref(ids, output_hidden_states=True)
    half, half_h = ref16(ids, output_hidden_states=True)
    n = cfg["num_hidden_layers"]
    assert out.pooler_output is None and len(out.hidden_states) == n + 1 and out[0] is out.last_hidden_state and out[-1] is out.hidden_states
    assert out.last_hidden_state.shape == want.shape and out.last_hidden_state.dtype == f16
    _gate(f"{name} last_hidden_state", out.last_hidden_state, half, want)
    for i in range(n + 1):
        _gate(f"{name} hidden_states[{i}]", out.hidden_states[i], half_h[i], want_h[i])
    plain = m(ids)
    assert plain.hidden_states is None and len(plain) == 1 and torch.equal(plain[0], out[0])
    return m, out


@pytest.mark.parametrize("B,L", [(2, 77), (1, 77), (3, 77), (2, 20)])
def test_model_small_fixture(dev, B, L):
    if (B, L) == (2, 77):
        from safetensors.torch import load_file
        ids = load_file(os.path.join(ROOT, "tests", "golden", "clip_text_small.safetensors"))["input_ids"].long()
    else:
        ids = prompt_like_ids(B, L, 256, seed=B + L)
    _check_model(dev, SMALL, None, ids, f"small B={B} L={L}")


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_model_width_768_two_layers(dev, act):
    cfg = dict(vocab_size=1000, hidden_size=768, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=12,
               max_position_embeddings=77, hidden_act=act, layer_norm_eps=1e-5, eos_token_id=999)
    _check_model(dev, cfg, 11, prompt_like_ids(2, 77, 1000, seed=3), f"768x2 {act}")
    if act == "gelu":
        _check_model(dev, dict(SMALL, hidden_act="gelu"), 12, prompt_like_ids(3, 77, 256, seed=4), "small gelu")


def test_model_full_sd15_config(dev):
    cfg = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
               max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2)
    _check_model(dev, cfg, 21, prompt_like_ids(2, 77, 49408, seed=5), "sd15 12 layers")
    _MODELS.clear()


def test_model_is_causal_bit_for_bit(dev):
    m, _, _ = _model(dev, SMALL, None)
    ids = prompt_like_ids(3, 77, 256, seed=9)
    ids2 = ids.clone()
    ids2[:, 40:] = (ids2[:, 40:] + 7) % 254
    a, b = m(ids, output_hidden_states=True), m(ids2, output_hidden_states=True)
    for x, y in zip(a.hidden_states + (a.last_hidden_state,), b.hidden_states + (b.last_hidden_state,)):
        assert torch.equal(x[:, :40], y[:, :40]) and not torch.equal(x[:, 40:], y[:, 40:])


# ------------------------------------------------------------------------------------------------------------ the pipeline
TEXT64 = dict(SMALL, hidden_size=64, num_attention_heads=1)


@pytest.fixture(scope="module")
def pipe_parts(dev):
    unet = hip_model_random(SMALL_UNET, dev)
    te = pkg().CLIPTextModel(**TEXT64)
    te.load_state_dict(seeded_state(TEXT64, seed=31, qk_gain=3.0))
    return unet, te


def _pipe(parts, dev, text=True):
    unet, te = parts
    pipe = pkg().I2VAdapterPipeline(unet=unet, text_encoder=te if text else None, tokenizer=StubTokenizer(77, 256) if text else None)
    return pipe.to(dev, f16)


def _gens(seed=5):
    return dict(generator=torch.Generator().manual_seed(seed), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _kw(samples=2):
    cond = torch.randn(samples, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    return dict(condition_image_latents=cond, num_frames=4, num_inference_steps=3, guidance_scale=2.0, output_type="latent")


def test_pipeline_takes_a_prompt(dev, pipe_parts):
    """the test that shows the feature exists: `pipe(prompt=...)` raised NotImplementedError before"""
    pipe = _pipe(pipe_parts, dev)
    assert pipe.text_encoder.device.type == "cuda" and pipe.text_encoder.dtype == f16            # to() moved it
    got = pipe(prompt=["a", "b"], negative_prompt=["c", "d"], **_kw(), **_gens()).frames
    assert got.shape == (2, 4, 4, 16, 16) and torch.isfinite(got).all()
    pe, ne = pipe.encode_prompt(["a", "b"], dev, 1, True, negative_prompt=["c", "d"])
    assert pe.shape == ne.shape == (2, 77, 64) and pe.dtype == f16 and not torch.equal(pe, ne) and not torch.equal(pe[0], pe[1])
    want = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, **_kw(), **_gens()).frames
    assert torch.equal(got, want)
    again = pipe(prompt=["a", "b"], negative_prompt=["c", "d"], **_kw(), **_gens()).frames
    assert torch.equal(again, got) and len(pipe._graph_cache) == 1                             # replayed, not re-captured
    # the embeddings are the tower's: the reference on the same ids
    ref = ClipTextReference(seeded_state(TEXT64, seed=31, qk_gain=3.0), TEXT64)
    ids = StubTokenizer(77, 256)(["a", "b"], padding="max_length", max_length=77, truncation=True).input_ids
    _gate("pipeline prompt_embeds", pe, ref.half()(ids)[0], ref(ids)[0])
    # default negative prompt: "" per prompt
    _, ne0 = pipe.encode_prompt(["a", "b"], dev, 1, True)
    _, ne1 = pipe.encode_prompt(["a", "b"], dev, 1, True, negative_prompt=["", ""])
    assert torch.equal(ne0, ne1) and torch.equal(ne0[0], ne0[1])


def test_pipeline_clip_skip_and_videos_per_prompt(dev, pipe_parts):
    pipe = _pipe(pipe_parts, dev)
    te = pipe.text_encoder
    ids = pipe.tokenizer("a cute pig", padding="max_length", max_length=77, truncation=True).input_ids
    out = te(ids, output_hidden_states=True)
    skip, _ = pipe.encode_prompt("a cute pig", dev, 1, False, clip_skip=1)
    plain, none = pipe.encode_prompt("a cute pig", dev, 1, False)
    assert none is None
    assert torch.equal(skip, te.text_model.final_layer_norm(out.hidden_states[-2])) and torch.equal(plain, out.last_hidden_state)
    assert not torch.equal(skip, plain)
    # two videos per prompt: (a, a, b, b), negatives alike
    pe1, ne1 = pipe.encode_prompt(["a", "b"], dev, 1, True, negative_prompt=["c", "d"])
    pe2, ne2 = pipe.encode_prompt(["a", "b"], dev, 2, True, negative_prompt=["c", "d"])
    assert torch.equal(pe2, pe1.repeat_interleave(2, 0)) and torch.equal(ne2, ne1.repeat_interleave(2, 0))
    got = pipe(prompt=["a"], negative_prompt=["c"], num_videos_per_prompt=2, **_kw(2), **_gens()).frames
    want = pipe(prompt_embeds=pe1[:1].repeat(2, 1, 1), negative_prompt_embeds=ne1[:1].repeat(2, 1, 1), **_kw(2), **_gens()).frames
    assert got.shape[0] == 2 and torch.equal(got, want)
    # clip_skip reaches the call
    a = pipe(prompt="a cute pig", clip_skip=1, **_kw(1), **_gens()).frames
    b = pipe(prompt_embeds=skip, negative_prompt_embeds=pipe.encode_prompt("", dev, 1, False)[0], **_kw(1), **_gens()).frames
    assert torch.equal(a, b)


def test_pipeline_without_guidance_skips_the_negative_prompt(dev, pipe_parts):
    pipe = _pipe(pipe_parts, dev)
    kw = dict(_kw(1), guidance_scale=1.0)
    got = pipe(prompt="a", negative_prompt="never read", **kw, **_gens()).frames
    assert [c[0] for c in pipe.tokenizer.calls] == [("a",), ("a",)]                             # the prompt's two calls only
    pe, ne = pipe.encode_prompt("a", dev, 1, False, negative_prompt="never read")
    assert ne is None and torch.equal(got, pipe(prompt_embeds=pe, **kw, **_gens()).frames)


def test_pipeline_prompt_errors(dev, pipe_parts):
    pipe = _pipe(pipe_parts, dev)
    with pytest.raises(TypeError, match="`negative_prompt` should be the same type to `prompt`, but got <class 'list'> != <class 'str'>."):
        pipe(prompt="a", negative_prompt=["b"], **_kw(1), **_gens())
    with pytest.raises(ValueError, match="has batch size 1, but `prompt`"):
        pipe(prompt=["a", "b"], negative_prompt=["c"], **_kw(2), **_gens())
    with pytest.raises(NotImplementedError, match="image encoder"):
        pipe(prompt="a", ip_adapter_image=object(), **_kw(1), **_gens())
    bare = _pipe(pipe_parts, dev, text=False)
    with pytest.raises(ValueError, match="`text_encoder` and a `tokenizer`"):
        bare(prompt="a", **_kw(1), **_gens())
    pe = torch.zeros(1, 77, 64, dtype=f16, device=dev)
    assert bare(prompt_embeds=pe, negative_prompt_embeds=pe, **_kw(1), **_gens()).frames.shape == (1, 4, 4, 16, 16)
