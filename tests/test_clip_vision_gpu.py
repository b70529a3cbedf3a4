"""The CLIP image encoder on the GPU, through the C ABI: the patch im2col and the class-token / position assembly against exact
yardsticks, the bidirectional attention kernel against float64 and its exact properties (not causal, batch / head independence, no
pad leakage, output bounds, the unsupported envelope), the whole tower against tests/clip_vision_reference.py, and
`pipe(ip_adapter_image=...)` on the reduced UNet with an IP-Adapter installed.

The accuracy gate is tests/test_clip_text_gpu.py's: the kernel's (the model's) error may be at most TWICE that of torch's fp16 CPU
evaluation of the same problem against the same float64 (whole models: fp32) yardstick.  Every measured pair goes to
$I2V_CLIP_VISION_LOG as JSON lines (profiles/clip_vision_errors.jsonl is one such run)."""
import ctypes as C

import pytest
import torch

from tests.clip_vision_reference import (SMALL, VIT_H, ClipVisionReference, StubFeatureExtractor, attention, fixture_state, pixel_like,
                                         seeded_state)
from tests.parity import SMALL_UNET, fp16_gate, hip_model_random, sd15_ip_state_dict

pytestmark = pytest.mark.gpu
f16 = torch.float16
FACTOR = 2.0
L_MAX = 288


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _gate(name, got, half, ref, **extra):
    fp16_gate(name, got, half, ref, FACTOR, "I2V_CLIP_VISION_LOG", **extra)


def _raw(dev):
    lib = pkg()._lib.load()
    return lib, C.c_void_p(torch.cuda.current_stream().cuda_stream), (lambda t: C.c_void_p(t.data_ptr()))


# ------------------------------------------------------------------------------------------------------------ patchify
def _unfold(px, p):
    """[B, C, S, S] -> [B * (S/p)^2, C p p]: row (b, py, px), columns (c, dy, dx)"""
    B, Cc, S, _ = px.shape
    n = S // p
    return px.view(B, Cc, n, p, n, p).permute(0, 2, 4, 1, 3, 5).reshape(B * n * n, Cc * p * p)


@pytest.mark.parametrize("B,S,p", [(1, 14, 14), (2, 28, 14), (1, 224, 14), (2, 32, 16)])
def test_patchify_is_exact(dev, B, S, p):
    K = pkg().kernels
    px = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(S + B)).half()
    want = _unfold(px, p)
    kk = 3 * p * p
    assert torch.equal(want, torch.nn.functional.unfold(px.float(), p, stride=p).transpose(1, 2).reshape(-1, kk).half())
    for ld in (K.pad8(kk), K.pad8(kk) + 24):                                   # the GEMM's K, and a wider row
        out = torch.full((want.shape[0], ld), 7.0, dtype=f16, device=dev)       # a sentinel the pad columns must replace with zeros
        got = K.clip_patchify(px.to(dev), p, ld=ld, out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(got[:, :kk].cpu(), want)
        assert bool((got[:, kk:] == 0).all()) and got[:, kk:].numel() == want.shape[0] * (ld - kk)
    assert K.clip_patchify(px.to(dev), p).shape == (want.shape[0], K.pad8(kk))


def test_patchify_rejects_on_the_host(dev):
    P = pkg()
    lib, st, p = _raw(dev)
    px = torch.zeros(1, 3, 30, 30, dtype=f16, device=dev)
    out = torch.full((4, 592), 7.0, dtype=f16, device=dev)
    assert lib.i2v_clip_patchify_f16(p(px), p(out), 592, 1, 3, 30, 14, st) == -1 and b"not a multiple of the patch size" in lib.i2v_last_error()
    assert lib.i2v_clip_patchify_f16(p(px), p(out), 588, 1, 3, 28, 14, st) == -1                     # ld % 8
    assert lib.i2v_clip_patchify_f16(p(px), p(out), 584, 1, 3, 28, 14, st) == -1                     # ld < C p p
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(P.HipLibraryError, match="status -1"):
        P.kernels.clip_patchify(px, 14, ld=592, out=torch.empty(4, 592, dtype=f16, device=dev))


# ------------------------------------------------------------------------------------------------------------ embed
@pytest.mark.parametrize("B,Pn,hidden", [(1, 1, 72), (3, 4, 160), (2, 256, 1280)])
def test_embed_kernel_is_exact(dev, B, Pn, hidden):
    K = pkg().kernels
    g = torch.Generator().manual_seed(B * 100 + Pn)
    cls, pos, patch = torch.randn(hidden, generator=g).half(), torch.randn(Pn + 1, hidden, generator=g).half(), \
        torch.randn(B * Pn, hidden, generator=g).half()
    want = (torch.cat([cls.float().expand(B, 1, hidden), patch.float().view(B, Pn, hidden)], dim=1) + pos.float()[None]).half()
    got = K.clip_vision_embed(cls.to(dev), patch.to(dev), pos.to(dev), batch=B)
    assert got.shape == (B * (Pn + 1), hidden) and torch.equal(got.cpu(), want.view(-1, hidden))
    wide = torch.full((B * Pn, hidden + 16), float("nan"), dtype=f16, device=dev)             # a strided patch matrix: the gap is not read
    wide[:, :hidden] = patch.to(dev)
    assert torch.equal(K.clip_vision_embed(cls.to(dev), wide[:, :hidden], pos.to(dev), batch=B), got)
    lib, st, p = _raw(dev)
    out = torch.full((B * (Pn + 1), hidden), 7.0, dtype=f16, device=dev)
    assert lib.i2v_clip_vision_embed_f16(p(cls.to(dev)), p(patch.to(dev)), hidden, p(pos.to(dev)), p(out), B, Pn, hidden - 4, st) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ attention
def _qkv(B, L, heads, d, gain, seed, extra_rows=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(B * L + extra_rows, 3 * heads * d, generator=g)
    t[:, : heads * d] *= gain                      # q.k over d at unit variance has std sqrt(d); x 1/sqrt(d): logits of std `gain`
    return t.half()


def _split(qkv, B, L, heads, d):
    hid = heads * d
    return [qkv[: B * L, i * hid:(i + 1) * hid].reshape(B, L, heads, d).transpose(1, 2) for i in range(3)]


def _attn(dev, qkv, B, L, heads, d):
    return pkg().kernels.clip_vision_attention(qkv.to(dev), batch=B, length=L, heads=heads, head_dim=d)


@pytest.mark.parametrize("B,L", [(1, 1), (2, 15), (1, 16), (2, 17), (1, 33), (2, 257), (1, L_MAX)])
@pytest.mark.parametrize("d", [64, 80])
def test_attention_against_float64(dev, d, B, L):
    heads = 2
    qkv = _qkv(B, L, heads, d, 2.0, seed=L * 10 + B + d)
    q, k, v = _split(qkv, B, L, heads, d)
    ref = attention(q.double(), k.double(), v.double(), d ** -0.5)
    half = attention(q, k, v, d ** -0.5)
    got = _attn(dev, qkv, B, L, heads, d).view(B, L, heads, d).transpose(1, 2)
    _gate(f"clip_vision_attention d={d} B={B} L={L} logit_std=2", got, half, ref)


@pytest.mark.parametrize("L", [17, 257])
def test_attention_is_not_causal(dev, L):
    """changing only the LAST token's v changes query 0's output (a reused causal kernel fails this), and nothing but v's heads"""
    B, heads, d = 2, 2, 80
    a = _qkv(B, L, heads, d, 2.0, seed=1)
    b = a.clone()
    b.view(B, L, 3, heads * d)[:, L - 1, 2] += 1.0
    oa, ob = _attn(dev, a, B, L, heads, d).view(B, L, heads, d), _attn(dev, b, B, L, heads, d).view(B, L, heads, d)
    for bi in range(B):
        for h in range(heads):
            assert not torch.equal(oa[bi, 0, h], ob[bi, 0, h])
    # ... and only the last token's k changes every query's output too
    c = a.clone()
    c.view(B, L, 3, heads * d)[:, L - 1, 1] *= -1.0
    if L > 1:
        assert not torch.equal(_attn(dev, c, B, L, heads, d).view(B, L, heads, d)[:, 0], oa[:, 0])


@pytest.mark.parametrize("L", [17, 257])
def test_attention_batches_and_heads_are_independent(dev, L):
    B, heads, d = 2, 2, 80
    a = _qkv(B, L, heads, d, 2.0, seed=5)
    oa = _attn(dev, a, B, L, heads, d).view(B, L, heads, d)
    other = _qkv(B, L, heads, d, 2.0, seed=6)
    b = a.clone()
    b.view(B, L, -1)[1] = other.view(B, L, -1)[1] * 3                                           # batch 1 changed
    ob = _attn(dev, b, B, L, heads, d).view(B, L, heads, d)
    assert torch.equal(ob[0], oa[0]) and not torch.equal(ob[1], oa[1])
    c = a.clone()
    c.view(B * L, 3, heads, d)[:, :, 1] = other.view(B * L, 3, heads, d)[:, :, 1] * 3           # head 1 changed
    oc = _attn(dev, c, B, L, heads, d).view(B, L, heads, d)
    assert torch.equal(oc[:, :, 0], oa[:, :, 0]) and not torch.equal(oc[:, :, 1], oa[:, :, 1])
    # one batch entry alone, and a strided view of a wider buffer (offsets and row stride are the caller's)
    assert torch.equal(_attn(dev, a[L:], 1, L, heads, d).view(L, heads, d), oa[1])
    hid = heads * d
    wide = torch.zeros(B * L, 3 * hid + 16, dtype=f16, device=dev)
    wide[:, 8: 8 + 3 * hid] = a.to(dev)
    got = pkg().kernels.clip_vision_attention(wide, batch=B, length=L, heads=heads, head_dim=d, q_off=8, k_off=8 + hid, v_off=8 + 2 * hid)
    assert torch.equal(got.view(B, L, heads, d), oa)


@pytest.mark.parametrize("B,L", [(2, 17), (1, 257)])
def test_attention_pad_keys_do_not_leak_and_output_stays_in_bounds(dev, B, L):
    K = pkg().kernels
    heads, d, extra = 2, 80, 32
    hid = heads * d
    buf = _qkv(B, L, heads, d, 2.0, seed=L, extra_rows=extra).to(dev)             # qkv is a view: 32 more rows follow it in memory
    outs = []
    for fill in (float("nan"), 0.0):
        buf[B * L:] = fill
        obuf = torch.full((B * L + extra, hid + 24), -77.0, dtype=f16, device=dev)             # ld_out > hidden, sentinel rows behind
        K.clip_vision_attention(buf[: B * L], batch=B, length=L, heads=heads, head_dim=d, out=obuf[: B * L, :hid])
        assert bool((obuf[B * L:] == -77.0).all()) and bool((obuf[:, hid:] == -77.0).all())
        assert torch.isfinite(obuf[: B * L, :hid]).all() and not bool((obuf[: B * L, :hid] == -77.0).all(dim=1).any())
        outs.append(obuf[: B * L, :hid].clone())
    assert torch.equal(outs[0], outs[1])
    q, k, v = _split(buf.cpu(), B, L, heads, d)
    _gate(f"clip_vision_attention view d={d} B={B} L={L}", outs[0].view(B, L, heads, d).transpose(1, 2), attention(q, k, v, d ** -0.5),
          attention(q.double(), k.double(), v.double(), d ** -0.5))


def test_attention_outside_the_envelope_is_unsupported(dev):
    P = pkg()
    lib, st, p = _raw(dev)
    qkv = torch.zeros(L_MAX + 1, 3 * 80, dtype=f16, device=dev)
    out = torch.full((L_MAX + 1, 80), 5.0, dtype=f16, device=dev)
    assert lib.i2v_clip_vision_attention_f16(p(qkv), 240, 0, 80, 160, p(out), 80, 1, L_MAX + 1, 1, 80, 0.1, st) == -2
    assert f"{L_MAX + 1} tokens".encode() in lib.i2v_last_error()
    assert lib.i2v_clip_vision_attention_f16(p(qkv), 240, 0, 80, 160, p(out), 80, 1, 64, 2, 40, 0.1, st) == -2
    assert b"head_dim 40" in lib.i2v_last_error()
    assert lib.i2v_clip_vision_attention_f16(p(qkv), 240, 0, 84, 160, p(out), 80, 1, 64, 1, 80, 0.1, st) == -1      # offset % 8
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    with pytest.raises(P.HipLibraryError, match="status -2"):
        P.kernels.clip_vision_attention(qkv, batch=1, length=L_MAX + 1, heads=1, head_dim=80)
    assert lib.i2v_clip_vision_attention_f16(p(qkv), 240, 0, 80, 160, p(out), 80, 1, L_MAX, 1, 80, 0.1, st) == 0     # L_max itself runs
    torch.cuda.synchronize()
    assert bool((out[:L_MAX] == 0).all()) and bool((out[L_MAX:] == 5.0).all())                # v = 0 everywhere


# ------------------------------------------------------------------------------------------------------------ the whole tower
def _check_model(dev, cfg, state, px, name):
    """HIP model vs the fp32 reference, gated by the fp16 reference, on image_embeds, last_hidden_state and hidden_states[-2]"""
    m = pkg().CLIPVisionModelWithProjection(**cfg)
    m.load_state_dict(state)
    m = m.half().to(dev).eval()
    ref = ClipVisionReference(state, cfg)
    out = m(px.to(dev), output_hidden_states=True)
    want = ref(px, output_hidden_states=True)
    half = ref.half()(px.half(), output_hidden_states=True)
    n = cfg["num_hidden_layers"]
    tokens = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    assert len(out.hidden_states) == n + 1 and out[0] is out.image_embeds and out[1] is out.last_hidden_state and out[-1] is out.hidden_states
    assert out.image_embeds.shape == (px.shape[0], cfg["projection_dim"]) and out.image_embeds.dtype == f16
    assert out.last_hidden_state.shape == (px.shape[0], tokens, cfg["hidden_size"]) and out.hidden_states[-1] is not None
    _gate(f"{name} image_embeds", out.image_embeds, half[0], want[0])
    _gate(f"{name} last_hidden_state", out.last_hidden_state, half[1], want[1])
    _gate(f"{name} hidden_states[-2]", out.hidden_states[-2], half[2][-2], want[2][-2])
    _gate(f"{name} hidden_states[0]", out.hidden_states[0], half[2][0], want[2][0])         # after pre_layrnorm
    plain = m(px.to(dev))
    assert plain.hidden_states is None and len(plain) == 2 and torch.equal(plain[0], out[0]) and torch.equal(plain[1], out[1])
    return m, out


@pytest.mark.parametrize("size", [56, 224])
def test_model_small_fixture(dev, size):
    _, state = fixture_state(size)
    _check_model(dev, dict(SMALL, image_size=size), state, pixel_like(2, size, seed=size), f"small {size}px")


def test_model_head_dim_64_quick_gelu(dev):
    cfg = dict(hidden_size=128, intermediate_size=256, projection_dim=64, num_hidden_layers=2, num_attention_heads=2, num_channels=3,
               image_size=56, patch_size=14, hidden_act="quick_gelu", layer_norm_eps=1e-5)
    _check_model(dev, cfg, seeded_state(cfg, seed=12, qk_gain=3.0), pixel_like(3, 56, seed=4), "d64 quick_gelu")


def test_model_width_1280_two_layers(dev):
    cfg = dict(VIT_H, num_hidden_layers=2)
    _check_model(dev, cfg, seeded_state(cfg, seed=11, qk_gain=3.0), pixel_like(2, 224, seed=3), "1280x2")


def test_model_full_vit_h_config(dev):
    """32 layers once, batch 1, seeded device weights: a CPU float64 pass of this is minutes, so for THIS test the yardsticks are torch's
    fp32 and fp16 evaluations of the reference on the device"""
    P = pkg()
    with torch.device("meta"):
        m = P.CLIPVisionModelWithProjection(**VIT_H)
    m = P.clip_vision.init_clip_vision_weights_(m.to_empty(device=dev).half(), seed=21, qk_gain=3.0).eval()
    state = {k: v.detach().float() for k, v in m.state_dict().items()}
    ref = ClipVisionReference(state, VIT_H)
    px = pixel_like(1, 224, seed=5).to(dev)
    out = m(px, output_hidden_states=True)
    want = ref(px, output_hidden_states=True)
    half = ref.half()(px.half(), output_hidden_states=True)
    assert len(out.hidden_states) == 33 and out.image_embeds.shape == (1, 1024) and out.last_hidden_state.shape == (1, 257, 1280)
    _gate("vit-h 32 layers image_embeds", out.image_embeds, half[0], want[0], yardstick="device fp32")
    _gate("vit-h 32 layers last_hidden_state", out.last_hidden_state, half[1], want[1], yardstick="device fp32")
    _gate("vit-h 32 layers hidden_states[-2]", out.hidden_states[-2], half[2][-2], want[2][-2], yardstick="device fp32")


def test_model_is_not_causal_and_images_are_independent(dev):
    _, state = fixture_state(56)
    cfg = dict(SMALL, image_size=56)
    m = pkg().CLIPVisionModelWithProjection(**cfg)
    m.load_state_dict(state)
    m = m.half().to(dev).eval()
    px = pixel_like(2, 56, seed=9).to(dev)
    px2 = px.clone()
    px2[1, :, -14:, -14:] += 0.5                                                 # the LAST patch of image 1
    a, b = m(px), m(px2)
    assert torch.equal(a.image_embeds[0], b.image_embeds[0]) and torch.equal(a.last_hidden_state[0], b.last_hidden_state[0])
    assert not torch.equal(a.image_embeds[1], b.image_embeds[1]) and not torch.equal(a.last_hidden_state[1, 0], b.last_hidden_state[1, 0])


# ------------------------------------------------------------------------------------------------------------ the pipeline
VIS = dict(hidden_size=64, intermediate_size=64, projection_dim=48, num_hidden_layers=1, num_attention_heads=1, num_channels=3,
           image_size=224, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5)


class _Counting:
    """the image encoder with its calls counted"""

    def __init__(self, enc):
        self.enc, self.calls = enc, []

    def __call__(self, pixel_values, **kw):
        self.calls.append(tuple(pixel_values.shape))
        return self.enc(pixel_values, **kw)

    def __getattr__(self, name):
        return getattr(self.enc, name)


@pytest.fixture(scope="module")
def pipe_parts(dev):
    unet = hip_model_random(SMALL_UNET, dev)
    unet._load_ip_adapter_weights(sd15_ip_state_dict(unet, clip_dim=48))
    enc = pkg().CLIPVisionModelWithProjection(**VIS)
    enc.load_state_dict(seeded_state(VIS, seed=31, qk_gain=3.0))
    return unet, enc


def _pipe(parts, dev, fe=None):
    unet, enc = parts
    return pkg().I2VAdapterPipeline(unet=unet, image_encoder=enc, feature_extractor=fe).to(dev, f16)


def _gens(seed=5):
    return dict(generator=torch.Generator().manual_seed(seed), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _kw(samples=1, guidance=2.0):
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(samples, 4, 16, 16, generator=g)
    pe, ne = torch.randn(samples, 7, 64, generator=g).half(), torch.randn(samples, 7, 64, generator=g).half()
    return dict(condition_image_latents=cond, num_frames=4, num_inference_steps=3, guidance_scale=guidance, output_type="latent",
                prompt_embeds=pe, negative_prompt_embeds=ne)


def test_pipeline_takes_an_image_prompt(dev, pipe_parts):
    """the test that shows the feature exists: `pipe(ip_adapter_image=...)` raised NotImplementedError before"""
    pipe = _pipe(pipe_parts, dev)
    assert pipe.image_encoder.device.type == "cuda" and pipe.image_encoder.dtype == f16            # to() moved it
    px, px2 = pixel_like(1, 224, seed=1), pixel_like(1, 224, seed=2)
    got = pipe(ip_adapter_image=px, **_kw(), **_gens()).frames
    assert got.shape == (1, 4, 4, 16, 16) and torch.isfinite(got).all()
    e, n = pipe.encode_image(px, dev, 1)
    assert e.shape == (1, 48) and e.dtype == f16 and e.is_cuda and torch.equal(n, torch.zeros_like(e))
    want = pipe(image_embeds=e, **_kw(), **_gens()).frames
    assert torch.equal(got, want)
    # the embeddings are the tower's: the reference on the same pixels
    ref = ClipVisionReference(seeded_state(VIS, seed=31, qk_gain=3.0), VIS)
    _gate("pipeline image_embeds", e, ref.half()(px.half())[0], ref(px)[0])
    # a second image: other frames, the step captured once
    got2 = pipe(ip_adapter_image=px2, **_kw(), **_gens()).frames
    assert not torch.equal(got2, got) and len(pipe._graph_cache) == 1
    assert torch.equal(pipe(ip_adapter_image=px, **_kw(), **_gens()).frames, got)


def test_pipeline_feature_extractors(dev, pipe_parts):
    import numpy as np
    import PIL.Image
    img = PIL.Image.fromarray((np.random.RandomState(0).rand(70, 90, 3) * 255).astype("uint8"))
    fes = [StubFeatureExtractor(224)]
    try:
        from transformers import CLIPImageProcessor
        fes.append(CLIPImageProcessor())
    except ImportError:
        pass
    for fe in fes:
        pipe = _pipe(pipe_parts, dev, fe)
        got = pipe(ip_adapter_image=img, **_kw(), **_gens()).frames
        px = fe(img, return_tensors="pt").pixel_values
        assert tuple(px.shape) == (1, 3, 224, 224)
        e, _ = pipe.encode_image(px, dev, 1)
        assert torch.equal(pipe.encode_image(img, dev, 1)[0], e)
        assert torch.equal(got, pipe(image_embeds=e, **_kw(), **_gens()).frames), type(fe).__name__


def test_pipeline_without_guidance_encodes_no_negative_half(dev, pipe_parts):
    pipe = _pipe(pipe_parts, dev)
    pipe.image_encoder = _Counting(pipe.image_encoder)
    px = pixel_like(1, 224, seed=1)
    kw = _kw(guidance=1.0)
    kw.pop("negative_prompt_embeds")
    got = pipe(ip_adapter_image=px, **kw, **_gens()).frames
    assert pipe.image_encoder.calls == [(1, 3, 224, 224)]
    e, _ = pipe.encode_image(px, dev, 1)
    assert torch.equal(got, pipe(image_embeds=e, **kw, **_gens()).frames)
    # with guidance the negative half is zeros, not a second encode
    pipe.image_encoder.calls.clear()
    pipe(ip_adapter_image=px, **_kw(), **_gens())
    assert pipe.image_encoder.calls == [(1, 3, 224, 224)]


def test_pipeline_videos_per_prompt(dev, pipe_parts):
    pipe = _pipe(pipe_parts, dev)
    px = torch.cat([pixel_like(1, 224, seed=1), pixel_like(1, 224, seed=2)])
    e1, _ = pipe.encode_image(px, dev, 1)
    e2, n2 = pipe.encode_image(px, dev, 2)
    assert e2.shape == (4, 48) and torch.equal(e2, e1.repeat_interleave(2, dim=0)) and not torch.equal(e1[0], e1[1])      # (a, a, b, b)
    assert torch.equal(n2, torch.zeros_like(e2))
    got = pipe(ip_adapter_image=px, num_videos_per_prompt=2, **_kw(4), **_gens()).frames
    want = pipe(image_embeds=e1.repeat_interleave(2, dim=0), **_kw(4), **_gens()).frames
    assert got.shape[0] == 4 and torch.equal(got, want)
    h, hn = pipe.encode_image(px, dev, 2, output_hidden_states=True)                                # the hidden-states branch
    out = pipe.image_encoder(px.to(dev, f16), output_hidden_states=True)
    zero = pipe.image_encoder(torch.zeros_like(px).to(dev, f16), output_hidden_states=True)
    assert h.shape == (4, 257, 64) and torch.equal(h, out.hidden_states[-2].repeat_interleave(2, dim=0))
    assert torch.equal(hn, zero.hidden_states[-2].repeat_interleave(2, dim=0)) and not torch.equal(h, hn)


def test_pipeline_image_prompt_errors(dev, pipe_parts):
    pipe = _pipe(pipe_parts, dev)
    px = pixel_like(1, 224, seed=1)
    with pytest.raises(ValueError, match="both `ip_adapter_image` and `image_embeds`"):
        pipe(ip_adapter_image=px, image_embeds=torch.zeros(1, 48), **_kw(), **_gens())
    bare = pkg().I2VAdapterPipeline(unet=pipe_parts[0])
    with pytest.raises(NotImplementedError, match="image encoder"):
        bare(ip_adapter_image=px, **_kw(), **_gens())
    with pytest.raises(ValueError, match="feature_extractor"):
        pipe(ip_adapter_image=object(), **_kw(), **_gens())
    plain = pkg().I2VAdapterPipeline(unet=hip_model_random(SMALL_UNET, dev), image_encoder=pipe.image_encoder)
    with pytest.raises(ValueError, match="load_ip_adapter"):
        plain(ip_adapter_image=px, **_kw(), **_gens())
