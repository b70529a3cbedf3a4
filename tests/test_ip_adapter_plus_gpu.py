"""IP-Adapter Plus on the GPU: i2v_perceiver_attention_f16 against float64 and its exact properties, blocks.Resampler against
tests/ip_adapter_plus_reference.py, the 16-image-token hot path (i2v_cross_attn_fused_f16 at ip_len 1 / 15 / 16, the fall-back at 17,
the reduced UNet against the oracle carrying the same adapter) and the pipeline with a Plus adapter.

The accuracy gate is the CLIP towers': the kernel's (the module's) max error against the float64 (whole models: fp32) yardstick may be
at most TWICE that of torch's fp16 CPU evaluation of the same fp16 operands.  Every measured pair goes to $I2V_IP_PLUS_LOG."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.clip_vision_reference import attention, pixel_like, seeded_state
from tests.ip_adapter_plus_reference import ResamplerReference, install_plus_on_oracle, plus_state_dict
from tests.parity import (REL_TOL_MODULE, REL_TOL_UNET, SMALL_UNET, compare, fp16_gate, hip_model_random, hip_unet_from_oracle, oracle_small_unet,
                          sd15_ip_state_dict, small_unet_inputs)

pytestmark = pytest.mark.gpu
f16 = torch.float16
FACTOR = 2.0
D = 64
NAN = float("nan")


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _gate(name, got, half, ref, **extra):
    fp16_gate(name, got, half, ref, FACTOR, "I2V_IP_PLUS_LOG", **extra)


def _raw(dev):
    lib = pkg()._lib.load()
    return lib, C.c_void_p(torch.cuda.current_stream().cuda_stream), (lambda t: C.c_void_p(t.data_ptr()))


# ------------------------------------------------------------------------------------------------------------ the kernel
def _operands(B, nq, la, lb, heads, gain, seed):
    """(q [B, nq, hid], keys [B, la + lb, hid], values [B, la + lb, hid]) in fp16; q x gain: logits of std `gain`"""
    g = torch.Generator().manual_seed(seed)
    hid = heads * D
    q = (torch.randn(B, nq, hid, generator=g) * gain).half()
    return q, torch.randn(B, la + lb, hid, generator=g).half(), torch.randn(B, la + lb, hid, generator=g).half()


def _pack(q, k, v, la, lb, dev, pad_rows=3, fill=NAN):
    """the kernel's buffers: B = the packed q | k | v buffer of the queries' rows (needs lb == nq, else its own k | v buffer with a
    separate q), A = a packed k | v buffer.  Unused columns and `pad_rows` rows behind each source hold `fill`."""
    B, nq, hid = q.shape
    a = torch.full((B * la + pad_rows, 2 * hid + 16), fill, dtype=f16)
    a[: B * la, 8: 8 + hid] = k[:, :la].reshape(B * la, hid)
    a[: B * la, 16 + hid:] = v[:, :la].reshape(B * la, hid)
    qb = torch.full((B * nq + pad_rows, hid + 8), fill, dtype=f16)
    qb[: B * nq, :hid] = q.reshape(B * nq, hid)
    b = None
    if lb:
        b = torch.full((B * lb + pad_rows, 2 * hid + 8), fill, dtype=f16)
        b[: B * lb, :hid] = k[:, la:].reshape(B * lb, hid)
        b[: B * lb, hid + 8:] = v[:, la:].reshape(B * lb, hid)
    return qb.to(dev), a.to(dev), None if b is None else b.to(dev)


def _run(dev, q, k, v, la, lb, out=None, fill=NAN):
    B, nq, hid = q.shape
    qb, a, b = _pack(q, k, v, la, lb, dev, fill=fill)
    return pkg().kernels.perceiver_attention(qb[: B * nq], a[: B * la], None if b is None else b[: B * lb], batch=B, n_q=nq, len_a=la,
                                             len_b=lb, heads=hid // D, q_off=0, ka_off=8, va_off=16 + hid, kb_off=0, vb_off=hid + 8, out=out)


def _heads(t):
    B, L, hid = t.shape
    return t.view(B, L, hid // D, D).transpose(1, 2)


SHAPES = [(1, 1, 1, 0), (2, 16, 15, 1), (1, 16, 16, 16), (2, 16, 17, 16), (1, 17, 33, 0), (1, 64, 40, 24), (2, 16, 257, 16),
          (1, 16, 272, 16)]


@pytest.mark.parametrize("gain", [2.0, 6.0])
@pytest.mark.parametrize("B,nq,la,lb", SHAPES)
def test_kernel_against_float64(dev, B, nq, la, lb, gain):
    q, k, v = _operands(B, nq, la, lb, 2, gain, seed=B * 1000 + nq * 7 + la + lb)
    ref = attention(_heads(q).double(), _heads(k).double(), _heads(v).double(), D ** -0.5)
    half = attention(_heads(q), _heads(k), _heads(v), D ** -0.5)
    got = _heads(_run(dev, q, k, v, la, lb).view(B, nq, -1))
    _gate(f"perceiver_attention B={B} n_q={nq} len_a={la} len_b={lb} logit_std={gain:g}", got, half, ref)


def test_kernel_split_of_the_keys_does_not_matter(dev):
    """the same 33 concatenated keys split (20, 13), (33, 0) and (1, 32): bit-equal; and repeats are bit-equal"""
    q, k, v = _operands(2, 16, 33, 0, 2, 2.0, seed=5)
    outs = [_run(dev, q, k, v, la, 33 - la) for la in (20, 33, 1, 20)]
    assert all(torch.equal(outs[0], o) for o in outs[1:]) and torch.isfinite(outs[0]).all()
    # ... and the pad rows / columns of the packed buffers are not read: NaN there, zeros there, one result
    assert torch.equal(outs[0], _run(dev, q, k, v, 20, 13, fill=0.0))


def test_kernel_q_and_source_b_in_one_buffer(dev):
    """the Resampler's call: B is the latents' own packed q | k | v buffer, the memory q is read from"""
    B, nq, la, heads = 2, 16, 17, 2
    hid = heads * D
    q, k, v = _operands(B, nq, la, nq, heads, 2.0, seed=6)
    qkv = torch.cat([q.view(B * nq, hid), k[:, la:].reshape(B * nq, hid), v[:, la:].reshape(B * nq, hid)], dim=1).to(dev)
    kv = torch.cat([k[:, :la].reshape(B * la, hid), v[:, :la].reshape(B * la, hid)], dim=1).to(dev)
    got = pkg().kernels.perceiver_attention(qkv, kv, qkv, batch=B, n_q=nq, len_a=la, len_b=nq, heads=heads)
    assert torch.equal(got, _run(dev, q, k, v, la, nq))


def test_kernel_batches_and_heads_are_independent(dev):
    B, nq, la, lb, heads = 3, 16, 17, 16, 2
    q, k, v = _operands(B, nq, la, lb, heads, 2.0, seed=7)
    base = _run(dev, q, k, v, la, lb).view(B, nq, heads, D)
    k2, v2 = k.clone(), v.clone()
    k2[1, 3, :D] += 1.0                                                    # batch 1, head 0: one key of source A ...
    v2[1, la + 2, :D] += 1.0                                               # ... and one value of source B
    got = _run(dev, q, k2, v2, la, lb).view(B, nq, heads, D)
    assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2]) and torch.equal(got[1, :, 1], base[1, :, 1])
    assert not torch.equal(got[1, :, 0], base[1, :, 0])


def test_kernel_writes_only_its_view_of_out(dev):
    B, nq, la, lb, heads = 2, 17, 20, 13, 2
    hid = heads * D
    q, k, v = _operands(B, nq, la, lb, heads, 2.0, seed=8)
    want = _run(dev, q, k, v, la, lb)
    buf = torch.full((B * nq + 2, hid + 16), 7.0, dtype=f16, device=dev)
    got = _run(dev, q, k, v, la, lb, out=buf[: B * nq, :hid])
    assert got.data_ptr() == buf.data_ptr() and torch.equal(buf[: B * nq, :hid], want)
    assert bool((buf[B * nq:] == 7.0).all()) and bool((buf[:, hid:] == 7.0).all())


def test_kernel_envelope(dev):
    P = pkg()
    lib, st, p = _raw(dev)
    hid = 2 * D
    q = torch.zeros(2 * 65, 3 * hid, dtype=f16, device=dev)
    kv = torch.zeros(300, 2 * hid, dtype=f16, device=dev)
    out = torch.full((2 * 65, hid), 7.0, dtype=f16, device=dev)
    fn = lib.i2v_perceiver_attention_f16

    def call(n_q=16, la=17, lb=16, head_dim=64, heads=2, ka_off=0, ldo=hid):
        return fn(p(q), 3 * hid, 0, p(kv), 2 * hid, ka_off, hid, la, p(q), 3 * hid, hid, 2 * hid, lb, p(out), ldo, 1, n_q, heads, head_dim, 0.125, st)

    assert call(n_q=65) == -2 and b"65 queries are not supported (at most 64)" in lib.i2v_last_error()
    assert call(la=273, lb=16) == -2 and b"273 + 16 keys are not supported (at most 288)" in lib.i2v_last_error()
    assert call(la=289, lb=0) == -2
    assert call(head_dim=80, heads=1) == -2 and b"head_dim 80 is not supported" in lib.i2v_last_error()
    assert call(la=0) == -1 and b"len_a 0" in lib.i2v_last_error()
    assert call(ka_off=4) == -1 and b"multiples of 8" in lib.i2v_last_error()
    assert call(ldo=hid - 8) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(P.HipLibraryError, match="status -2"):
        P.kernels.perceiver_attention(q[:65], kv[:17], q[:65], batch=1, n_q=65, len_a=17, len_b=65, heads=2)
    assert call(n_q=64, la=224, lb=64) == 0 and call(n_q=16, la=288, lb=0) == 0              # the last supported sizes themselves run
    torch.cuda.synchronize()
    assert torch.isfinite(out[:64]).all()


# ------------------------------------------------------------------------------------------------------------ the Resampler
class _Cfg(dict):
    __getattr__ = dict.__getitem__


def _fake_unet(cross):
    """what plus_state_dict reads of a UNet when only the image projection matters"""
    class U:
        config = _Cfg(cross_attention_dim=cross)

        def attn_processor_names(self):
            return []

        def named_modules(self):
            return []
    return U()


def _resampler(dev, geometry, cross, seed):
    P = pkg()
    state = plus_state_dict(_fake_unet(cross), seed=seed, qk_gain=1.5, **geometry)
    kwargs, conv = P.unet_motion_cross_frame_attn.convert_ip_adapter_plus_image_proj(state["image_proj"])
    m = P.blocks.Resampler(**kwargs)
    m.load_state_dict(conv)
    return m.half().to(dev).eval(), ResamplerReference(conv, torch.float32)


@pytest.mark.parametrize("name,geometry,cross,T", [
    ("reduced", dict(embed_dims=48, hidden=128, heads=2, depth=2, num_queries=8), 64, 17),
    ("sd15", dict(embed_dims=1280, hidden=768, heads=12, depth=4, num_queries=16), 768, 257)])
def test_resampler_against_the_reference(dev, name, geometry, cross, T):
    m, ref = _resampler(dev, geometry, cross, seed=3)
    B, nq = 2, geometry["num_queries"]
    x = torch.randn(B, T, geometry["embed_dims"], generator=torch.Generator().manual_seed(T)).half()
    got = m(x.to(dev))
    assert got.shape == (B, nq, cross) and got.dtype == f16
    _gate(f"Resampler {name} T={T}", got, ref.half()(x), ref(x.float()), yardstick="fp32")
    # repeats are bit-equal; a changed image changes only its own batch row
    assert torch.equal(got, m(x.to(dev)))
    x2 = x.clone()
    x2[1, T - 1] += 0.5
    got2 = m(x2.to(dev))
    assert torch.equal(got2[0], got[0]) and not torch.equal(got2[1], got[1])
    # the packs follow the weights' versions: a modified weight changes the result, the restored weight restores it bit for bit
    w = m.layers[0][2].to_k.weight
    keep = w.detach().clone()
    with torch.no_grad():
        w.mul_(0.5)
    assert not torch.equal(m(x.to(dev)), got)
    with torch.no_grad():
        w.copy_(keep)
    assert torch.equal(m(x.to(dev)), got)
    assert torch.equal(m(x[:1].to(dev)), got[:1])                                                  # another batch size, the same rows


# ------------------------------------------------------------------------------------------------------------ the 16-token hot path
def _attn_ref(q, k, v, heads):
    """q [n_ctx, rows, c], k / v [n_ctx, L, c] fp32 -> [n_ctx, rows, c]"""
    n, r, c = q.shape
    d = c // heads
    sp = lambda t: t.view(n, -1, heads, d).transpose(1, 2)
    return attention(sp(q), sp(k), sp(v), d ** -0.5).transpose(1, 2).reshape(n, r, c)


@pytest.fixture(scope="module")
def fused_case(dev):
    """channels 320, 8 heads of 40, rows 256, 2 contexts of 77: the operands every ip_len shares, and the text-only reference"""
    k = pkg().kernels
    c, heads, d, eps, rows, n_ctx, lt = 320, 8, 40, 1e-5, 256, 2, 77
    g = torch.Generator().manual_seed(333)
    h = lambda t: t.half().float()
    x = h(torch.randn(rows, c, generator=g) * 1.5 + 0.3)
    gamma, beta = h(1 + 0.2 * torch.randn(c, generator=g)), h(0.1 * torch.randn(c, generator=g))
    wq = h(torch.randn(c, c, generator=g) * c ** -0.5)
    kk, vv = h(torch.randn(n_ctx, lt, c, generator=g)), h(torch.randn(n_ctx, lt, c, generator=g))
    ki, vi = h(torch.randn(n_ctx, 17, c, generator=g)), h(torch.randn(n_ctx, 17, c, generator=g))
    q = h(h(F.layer_norm(x, (c,), gamma, beta, eps)) @ wq.T).view(n_ctx, rows // n_ctx, c)
    Dv = lambda t: t.half().to(dev)

    def vt_of(v, L):
        vt = torch.full((n_ctx, c, k.pad8(L)), NAN)
        vt[:, :, :L] = v[:, :L].permute(0, 2, 1)
        return Dv(vt)

    xd, kd, vtd = Dv(x), Dv(kk.reshape(-1, c)), vt_of(vv, lt)
    nl = k.layernorm(xd, Dv(gamma), Dv(beta), eps)
    qd = k.gemm(nl, Dv(wq))
    return dict(k=k, c=c, heads=heads, d=d, eps=eps, rows=rows, n_ctx=n_ctx, lt=lt, q=q, ki=ki, vi=vi, vt_of=vt_of, Dv=Dv, xd=xd, kd=kd,
                vtd=vtd, qd=qd, g32=Dv(gamma).float(), b32=Dv(beta).float(), w=k.pack_cross_q(Dv(wq), heads),
                frag=k.pack_ctx_fragments(kd, vtd, heads, lt), ref_text=_attn_ref(q, kk, vv, heads),
                old_text=k.attention(qd, kd, vtd, batch_q=n_ctx, lq=rows // n_ctx, lk=lt, heads=heads, head_dim=d))


def _close(got, ref, rel, name):
    got, ref = got.float().cpu(), ref.float().cpu()
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"{name}: err {err:.3e} bound {rel * scale:.3e}")
    assert torch.isfinite(got).all() and err <= rel * scale, f"{name}: err {err:.3e} > {rel:g} x max|ref| {scale:.3e}"


@pytest.mark.parametrize("li", [1, 15, 16])
def test_fused_cross_attention_with_up_to_16_image_tokens(dev, fused_case, li):
    """i2v_cross_attn_fused_f16 with ip_len 1, 15 and 16 (no test ran it above 4), NaN in V^T's pad columns, at the bounds the
    4-token test uses (amp = 1): 3e-3 against fp32 torch, 1.5e-3 against the un-fused kernels"""
    s = fused_case
    k, c, heads, d, n_ctx, rows = s["k"], s["c"], s["heads"], s["d"], s["n_ctx"], s["rows"]
    ip_scale = 0.7
    ki, vi = s["ki"][:, :li], s["vi"][:, :li]
    ref = (s["ref_text"] + ip_scale * _attn_ref(s["q"], ki, vi, heads)).reshape(rows, c)
    kid, vtid = s["Dv"](ki.reshape(-1, c)), s["vt_of"](s["vi"], li)
    frag_ip = k.pack_ctx_fragments(kid, vtid, heads, li)
    assert torch.isfinite(frag_ip.float()).all()
    kw = dict(heads=heads, head_dim=d, ctx_len=s["lt"], rows_per_ctx=rows // n_ctx, eps=s["eps"], ip_frag=frag_ip, ip_len=li, ip_scale=ip_scale)
    out = k.cross_attn_fused(s["xd"], s["g32"], s["b32"], s["w"], s["frag"], **kw)
    _close(out, ref, 3e-3, f"fused text + {li} image tokens vs fp32 torch")
    old = s["old_text"].clone()
    k.attention(s["qd"], kid, vtid, batch_q=n_ctx, lq=rows // n_ctx, lk=li, heads=heads, head_dim=d, out=old, accumulate=True, acc_scale=ip_scale)
    _close(out, old, 1.5e-3, f"fused text + {li} image tokens vs the un-fused kernels")
    assert torch.equal(out, k.cross_attn_fused(s["xd"], s["g32"], s["b32"], s["w"], s["frag"], **kw))


def test_fused_cross_attention_refuses_17_image_tokens(dev, fused_case):
    s = fused_case
    k, c, heads = s["k"], s["c"], s["heads"]
    frag_ip = k.pack_ctx_fragments(s["Dv"](s["ki"].reshape(-1, c)), s["vt_of"](s["vi"], 17), heads, 17)
    with pytest.raises(pkg().HipLibraryError):
        k.cross_attn_fused(s["xd"], s["g32"], s["b32"], s["w"], s["frag"], heads=heads, head_dim=s["d"], ctx_len=s["lt"],
                           rows_per_ctx=s["rows"] // s["n_ctx"], eps=s["eps"], ip_frag=frag_ip, ip_len=17, ip_scale=0.7)


@pytest.mark.parametrize("li", [16, 17])
def test_transformer_block_with_16_and_17_image_tokens(dev, li):
    """I2VAdapterTransformer2DModel at the fused kernel's width (320, 8 heads of 40) with `li` image tokens on attn2: 16 runs
    i2v_cross_attn_fused_f16, 17 falls back to the un-fused kernels (bit-equal to the module with the fused text attention switched
    off); both against the oracle's module carrying the same tokens, at tests.parity's module tolerance"""
    from oracle.i2v_adapter import I2VAdapterTransformer2DModel as O
    from tests.parity import oracle_from_hip
    from i2v_adapter_unofficial_amd import i2v_adapter as mod, kernels as K
    c, hw, frames, cross = 320, 16, 2, 768
    kw = dict(num_attention_heads=8, attention_head_dim=40, in_channels=c, num_layers=1, cross_attention_dim=cross, norm_num_groups=32)
    m = hip_model_random(kw, dev, seed=41, cls=pkg().I2VAdapterTransformer2DModel)
    o = oracle_from_hip(m, O, kw)
    g = torch.Generator().manual_seed(li)
    h = lambda t: t.half().float()
    wk, wv = h(torch.randn(c, cross, generator=g) * cross ** -0.5), h(torch.randn(c, cross, generator=g) * cross ** -0.5)
    for mm in (m, o):
        mm.transformer_blocks[0].attn2.install_ip_adapter(wk, wv, num_tokens=li, scale=0.8)
    x = h(torch.randn(2 * frames, c, hw, hw, generator=g))
    ctx = h(torch.randn(2 * frames, 77 + li, cross, generator=g))
    assert K.cross_attn_fused_supported(2 * frames * hw * hw, c, 8, 40, 77, hw * hw) and mod.FUSED_TEXT_ATTN
    run = lambda: m(x.half().to(dev), enable_cross_frame_attn=True, num_frames=frames, encoder_hidden_states=ctx.half().to(dev),
                    return_dict=False)[0]
    with torch.no_grad():
        ref = o(x, enable_cross_frame_attn=True, num_frames=frames, encoder_hidden_states=ctx, return_dict=False)[0]
        got = run()
        mod.FUSED_TEXT_ATTN = False
        try:
            plain = run()
        finally:
            mod.FUSED_TEXT_ATTN = True
    compare(got, ref, rel=REL_TOL_MODULE, name=f"T2D C=320 with {li} image tokens")
    compare(plain, ref, rel=REL_TOL_MODULE, name=f"T2D C=320 with {li} image tokens, un-fused text attention")
    compare(got, plain, rel=REL_TOL_MODULE, name=f"T2D C=320 with {li} image tokens, fused vs un-fused")
    assert torch.equal(got, plain) == (li == 17)


PLUS_SMALL = dict(embed_dims=48, hidden=128, heads=2, depth=2, num_queries=16)


def test_small_unet_with_a_plus_adapter_against_the_oracle(dev):
    """the reduced UNet with a reduced Plus adapter (16 image tokens) against the oracle UNet carrying the same adapter, hidden states in
    `added_cond_kwargs`, at the tolerance of tests/test_modules_gpu.py's IP-Adapter forward.  (At SMALL_UNET's widths no block has
    i2v_cross_attn_fused_f16's shape, so I2V_TEXT_FUSED changes nothing here: the fused path with 16 tokens is the two tests above.)"""
    ou = oracle_small_unet(ip=False)
    state = plus_state_dict(ou, **PLUS_SMALL)
    install_plus_on_oracle(ou, state)
    hu = hip_unet_from_oracle(ou, dev, ip_state_dict=state)
    assert isinstance(hu.encoder_hid_proj, pkg().blocks.Resampler) and all(a.ip_num_tokens == 16 for a in hu._cross_attention_layers())
    inp = small_unet_inputs()
    hs = torch.randn(2, 17, 48, generator=torch.Generator().manual_seed(2)).half().float()
    with torch.no_grad():
        ref = ou(inp["sample"], inp["timestep"], True, inp["ctx"], added_cond_kwargs={"image_embeds": hs}).sample
        got = hu(inp["sample"].to(dev), inp["timestep"].to(dev), True, inp["ctx"].to(dev), added_cond_kwargs={"image_embeds": hs.to(dev)}).sample
        off = ou(inp["sample"], inp["timestep"], True, inp["ctx"], added_cond_kwargs={"image_embeds": torch.zeros_like(hs)}).sample
    err, scale = compare(got, ref, rel=REL_TOL_UNET, name="small UNet + IP-Adapter Plus")
    print(f"small UNet + Plus: max abs err {err:.3e} (max|ref| {scale:.3e})")
    assert (off - ref).abs().max().item() > REL_TOL_UNET * scale                # the image tokens are visible at this tolerance
    # project_context / _project_image_embeds with 16 tokens: the projected context gives the forward's result
    ctx_ip = hu._project_image_embeds({"image_embeds": hs.to(dev)})
    assert ctx_ip.shape == (2, 16, 64)
    pc = hu.project_context(inp["ctx"].to(dev, f16).contiguous(), ctx_ip)
    assert all(kv[2].shape[0] == 2 * 16 for kv in pc.kv.values())


# ------------------------------------------------------------------------------------------------------------ the pipeline
VIS = dict(hidden_size=64, intermediate_size=64, projection_dim=48, num_hidden_layers=2, num_attention_heads=1, num_channels=3,
           image_size=224, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5)
PLUS_PIPE = dict(embed_dims=64, hidden=128, heads=2, depth=2, num_queries=16)


@pytest.fixture(scope="module")
def parts(dev):
    unet = hip_model_random(SMALL_UNET, dev)
    enc = pkg().CLIPVisionModelWithProjection(**VIS)
    enc.load_state_dict(seeded_state(VIS, seed=31, qk_gain=3.0))
    return unet, enc.half().to(dev).eval(), plus_state_dict(unet, **PLUS_PIPE)


def _pipe(parts, dev, plus=True):
    unet, enc, state = parts
    pipe = pkg().I2VAdapterPipeline(unet=unet, image_encoder=enc)
    if plus:
        pipe.load_ip_adapter(state)
    return pipe


def _gens(seed=5):
    return dict(generator=torch.Generator().manual_seed(seed), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _kw(samples=1, guidance=2.0):
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(samples, 4, 16, 16, generator=g)
    pe, ne = torch.randn(samples, 7, 64, generator=g).half(), torch.randn(samples, 7, 64, generator=g).half()
    kw = dict(condition_image_latents=cond, num_frames=4, num_inference_steps=3, guidance_scale=guidance, output_type="latent", prompt_embeds=pe)
    if guidance > 1:
        kw["negative_prompt_embeds"] = ne
    return kw


def test_pipeline_takes_an_image_prompt_with_a_plus_adapter(dev, parts):
    """fails on the parent commit: `load_ip_adapter` of a Plus file raised NotImplementedError"""
    pipe = _pipe(parts, dev)
    px, px2 = pixel_like(1, 224, seed=1), pixel_like(1, 224, seed=2)
    got = pipe(ip_adapter_image=px, **_kw(), **_gens()).frames
    assert got.shape == (1, 4, 4, 16, 16) and torch.isfinite(got).all()
    h, hn = pipe.encode_image(px, dev, 1, True)
    assert h.shape == hn.shape == (1, 257, 64) and not torch.equal(h, hn)
    assert torch.equal(got, pipe(image_embeds=h, negative_image_embeds=hn, **_kw(), **_gens()).frames)
    # a different image changes the frames; the step was captured once and is replayed
    got2 = pipe(ip_adapter_image=px2, **_kw(), **_gens()).frames
    assert not torch.equal(got2, got) and len(pipe._graph_cache) == 1
    assert torch.equal(pipe(ip_adapter_image=px, **_kw(), **_gens()).frames, got) and len(pipe._graph_cache) == 1
    # the graph route equals the callback route bit for bit
    assert torch.equal(pipe(ip_adapter_image=px, use_graph=False, **_kw(), **_gens()).frames, got)
    seen = []
    cb = pipe(ip_adapter_image=px, callback=lambda i, t, lat: seen.append(i), callback_steps=1, **_kw(), **_gens()).frames
    assert torch.equal(cb, got) and seen == [0, 1, 2]


def test_pipeline_scale_zero_is_no_image_prompt(dev, parts):
    """set_ip_adapter_scale(0.0): the image branch adds exactly 0 x finite numbers, so the frames are bit-equal to `ip_scale = 0` set by
    hand; against the same pipeline WITHOUT an adapter (other launches: no image branch at all) they agree within the UNet tolerance"""
    pipe = _pipe(parts, dev)
    px = pixel_like(1, 224, seed=1)
    on = pipe(ip_adapter_image=px, **_kw(), **_gens()).frames
    key_on = next(iter(pipe._graph_cache))
    pipe.set_ip_adapter_scale(0.0)
    assert all(a.ip_scale == 0.0 for a in pipe.unet._cross_attention_layers())
    zero = pipe(ip_adapter_image=px, **_kw(), **_gens()).frames
    # the scale is in the graph key: one re-capture (the cache keeps one graph at a time)
    assert list(pipe._graph_cache) != [key_on] and len(pipe._graph_cache) == 1 and not torch.equal(zero, on)
    pipe.set_ip_adapter_scale(1.0)
    for a in pipe.unet._cross_attention_layers():
        a.ip_scale = 0.0
    assert torch.equal(pipe(ip_adapter_image=px, **_kw(), **_gens()).frames, zero)
    pipe.set_ip_adapter_scale(1.0)
    procs = pipe.unet.attn_processors
    pipe.unet.set_attn_processor({k: type(p)(0, 1.0) for k, p in procs.items()})       # the branch switched off: no image tokens at all
    try:
        none = pipe(ip_adapter_image=px, **_kw(), **_gens()).frames
    finally:
        pipe.unet.set_attn_processor(procs)
    compare(zero, none, rel=REL_TOL_UNET, name="Plus adapter at scale 0 vs the branch switched off")


def test_pipeline_videos_per_prompt_and_no_guidance(dev, parts):
    pipe = _pipe(parts, dev)
    px = torch.cat([pixel_like(1, 224, seed=1), pixel_like(1, 224, seed=2)])
    h1, n1 = pipe.encode_image(px, dev, 1, True)
    got = pipe(ip_adapter_image=px, num_videos_per_prompt=2, **_kw(4), **_gens()).frames
    want = pipe(image_embeds=h1.repeat_interleave(2, dim=0), negative_image_embeds=n1.repeat_interleave(2, dim=0), **_kw(4), **_gens()).frames
    assert got.shape[0] == 4 and torch.equal(got, want) and not torch.equal(got[0], got[2])
    # guidance_scale = 1 runs one copy: only the positive half is projected (the zero image is still encoded, as the reference does)
    calls = []
    proj = pipe.unet.encoder_hid_proj
    hook = proj.register_forward_hook(lambda mod, args, out: calls.append(tuple(args[0].shape)))
    try:
        one = pipe(ip_adapter_image=px[:1], **_kw(guidance=1.0), **_gens()).frames
        assert calls == [(1, 257, 64)]
        calls.clear()
        pipe(ip_adapter_image=px[:1], **_kw(), **_gens())
        assert calls == [(2, 257, 64)]
    finally:
        hook.remove()
    assert one.shape == (1, 4, 4, 16, 16) and torch.isfinite(one).all()
    assert torch.equal(one, pipe(image_embeds=h1[:1], **_kw(guidance=1.0), **_gens()).frames)


def test_pipeline_plain_adapter_after_plus(dev, parts):
    pipe = _pipe(parts, dev)
    unet = pipe.unet
    pipe.load_ip_adapter(sd15_ip_state_dict(unet, clip_dim=48))
    assert isinstance(unet.encoder_hid_proj, pkg().blocks.ImageProjection) and all(a.ip_num_tokens == 4 for a in unet._cross_attention_layers())
    px = pixel_like(1, 224, seed=1)
    got = pipe(ip_adapter_image=px, **_kw(), **_gens()).frames
    e, _ = pipe.encode_image(px, dev, 1)
    assert e.shape == (1, 48) and torch.equal(got, pipe(image_embeds=e, **_kw(), **_gens()).frames)
    with pytest.raises(ValueError, match="plain IP-Adapter is loaded"):
        pipe(image_embeds=torch.zeros(1, 257, 64, device=dev), **_kw(), **_gens())
