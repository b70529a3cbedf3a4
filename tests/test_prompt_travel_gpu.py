"""Prompt travel on the GPU: i2v_interp_rows_f16 against fp64 at the bound of tests/prompt_travel_reference.py; the per-step kernels
with one context per tile (i2v_cross_attn_fused_f16, i2v_attention_f16 with kv_group = 1) bit-equal to a launch with each context alone;
the transformer block on its fused and un-fused routes and the reduced UNet with one context per frame against the oracle that takes one
context per frame (tolerances of tests/parity.py, unchanged); and the pipeline on the reduced UNet with a small CLIP text encoder:
`prompt={0: a, 3: b}` equals the call with `encode_prompt_travel`'s 4-D embeds, captured equals eager, a second sample replays the
captured step, a single-key dict is the str call -- all bit for bit -- under every scheduler, without guidance, with FreeNoise, FreeInit,
a ControlNet, a T2I-Adapter, IP-Adapter and IP-Adapter Plus."""
import numpy as np
import pytest
import torch

from tests import prompt_travel_reference as R
from tests.clip_text_reference import StubTokenizer, seeded_state
from tests.parity import (REL_TOL_MODULE, REL_TOL_TRAJECTORY, REL_TOL_UNET, SMALL_UNET, compare, hip_model_random, hip_unet_from_oracle, round_fp16_,
                          small_ip_state_dict, small_unet_inputs)

pytestmark = pytest.mark.gpu
f16 = torch.float16


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def K():
    return pkg().kernels


def h16(t):
    return t.half().float()


def bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------- the kernel
POISON = -12345.0
WEIGHTS = {"zeros": lambda n: [0.0] * n, "ones": lambda n: [1.0] * n, "halves": lambda n: [0.5] * n,
           "linspace": lambda n: np.linspace(0.0, 1.0, n + 2).astype(np.float32)[1:-1].tolist() if n > 1 else [1.0 / 3.0]}


@pytest.mark.parametrize("n_out", [1, 5])
@pytest.mark.parametrize("e", [8, 7 * 48, 77 * 768])          # one chunk; an odd number of chunks; a prompt's embedding (more than one block)
def test_interp_rows_against_fp64(dev, e, n_out):
    """every weight set on a strided `out` inside poisoned guard rows: the bound against fp64, bit-exact copies where w is 0 or 1, a
    NaN row that no output row reads, guards and pad columns intact, a repeat run bit-equal"""
    g = torch.Generator().manual_seed(e + n_out)
    src = (torch.randn(4, e, generator=g) * 3).half()
    src[0, :4] = torch.tensor([0.0, -0.0, 6e-8, 65504.0]).half()
    src[3] = float("nan")                                                     # never referenced below
    d_src = src.to(dev)
    lo = [i % 3 for i in range(n_out)]
    hi = [(i + 1) % 3 for i in range(n_out)]
    ld = e + 16
    for name, make in WEIGHTS.items():
        w = make(n_out)
        buf = torch.full((n_out + 2, ld), POISON, dtype=f16, device=dev)
        out = buf[1:1 + n_out, :e]
        # a row with w == 0 (w == 1) may name the NaN row as the one it does not read
        hi_n = [3 if ww == 0.0 else b for b, ww in zip(hi, w)]
        lo_n = [3 if ww == 1.0 else a for a, ww in zip(lo, w)]
        got = K().interp_rows(d_src, lo_n, hi_n, w, out=out)
        assert got is out
        res = out.cpu()
        worst, ok = R.check_interp_rows(res, src, lo_n, hi_n, w)
        print(f"i2v_interp_rows_f16 e={e} n_out={n_out} w={name}: worst error / bound {worst:.3f}")
        assert ok, (name, worst)
        for r, ww in enumerate(w):
            if ww == 0.0:
                assert torch.equal(bits(res[r]), bits(src[lo_n[r]])), "w == 0 is not a bit-exact copy"
            if ww == 1.0:
                assert torch.equal(bits(res[r]), bits(src[hi_n[r]])), "w == 1 is not a bit-exact copy"
        whole = buf.cpu()
        assert (whole[0] == POISON).all() and (whole[-1] == POISON).all() and (whole[:, e:] == POISON).all(), "wrote outside out"
        again = torch.full_like(buf, POISON)
        K().interp_rows(d_src, lo_n, hi_n, w, out=again[1:1 + n_out, :e])
        assert torch.equal(bits(again), bits(buf)), "a repeat run differs"
    # a new contiguous tensor by default, rows of any shape
    nd = K().interp_rows(d_src.view(4, -1, 8), lo, hi, WEIGHTS["halves"](n_out))
    assert nd.shape == (n_out, e // 8, 8) and nd.is_contiguous()


def test_interp_rows_strided_source_and_wrapper_refusals(dev):
    g = torch.Generator().manual_seed(1)
    wide = (torch.randn(3, 48, generator=g)).half().to(dev)
    src = wide[:, :40]                                                        # row stride 48, row length 40
    out = K().interp_rows(src, [0, 2], [1, 0], [0.25, 0.0])
    assert R.check_interp_rows(out.cpu(), src.cpu(), [0, 2], [1, 0], [0.25, 0.0])[1]
    for args, msg in ((([0], [3], [0.5]), "hi\\[0\\] = 3 is outside"), (([-1], [0], [0.5]), "lo\\[0\\] = -1"),
                      (([0], [1], [1.5]), "w\\[0\\] = 1.5"), (([0], [1], [float("nan")]), "w\\[0\\]"), (([0, 1], [1], [0.5]), "one length"),
                      (([], [], []), "one length")):
        with pytest.raises(ValueError, match=msg):
            K().interp_rows(src, *args)
    with pytest.raises(TypeError, match="integers"):
        K().interp_rows(src, [0.0], [1], [0.5])
    with pytest.raises(ValueError, match="overlap"):
        K().interp_rows(wide, [0], [1], [0.5], out=wide[1:2])
    with pytest.raises(ValueError, match="multiple of 8"):
        K().interp_rows(wide[:, :12], [0], [1], [0.5])
    with pytest.raises(ValueError, match="host tables"):
        K().interp_rows(src, torch.tensor([0], device=dev), [1], [0.5])


# ---------------------------------------------------------------------------------------------------------- one context per tile
@pytest.mark.parametrize("lt", [7, 77])
def test_cross_attn_fused_with_one_context_per_tile(dev, lt):
    """rows = 256, rows_per_ctx = 128: the two 128-row tiles read two different contexts (tile / tiles_per_ctx with tiles_per_ctx = 1,
    the form prompt travel launches when a frame is one tile).  With and without 4 image tokens, with and without the out-projection:
    each context's rows are bit-equal to a launch with that context alone."""
    k = K()
    c, heads, d, eps, rows, rpc, li = 320, 8, 40, 1e-5, 256, 128, 4
    assert k.cross_attn_fused_supported(rows, c, heads, d, lt, rpc)
    g = torch.Generator().manual_seed(lt)
    D = lambda t: t.half().to(dev)
    x = D(torch.randn(rows, c, generator=g) * 1.5 + 0.3)
    g32, b32 = D(1 + 0.2 * torch.randn(c, generator=g)).float(), D(0.1 * torch.randn(c, generator=g)).float()
    w = k.pack_cross_q(D(torch.randn(c, c, generator=g) * c ** -0.5), heads)
    op = k.pack_attn_out(D(torch.randn(c, c, generator=g) * c ** -0.5), D(0.1 * torch.randn(c, generator=g)), heads)

    def fragments(length):
        kk, vv = torch.randn(2, length, c, generator=g), torch.randn(2, length, c, generator=g)
        vt = torch.zeros(2, c, k.pad8(length))
        vt[:, :, :length] = vv.permute(0, 2, 1)
        return k.pack_ctx_fragments(D(kk.reshape(-1, c)), D(vt), heads, length)
    frag, frag_ip = fragments(lt), fragments(li)
    assert not torch.equal(frag[0], frag[1])
    for with_ip in (False, True):
        for out_proj in (None, op):
            def run(xs, fr, fi):
                kw = dict(ip_frag=fi, ip_len=li, ip_scale=0.7) if with_ip else {}
                return k.cross_attn_fused(xs, g32, b32, w, fr, heads=heads, head_dim=d, ctx_len=lt, rows_per_ctx=rpc, eps=eps,
                                          out_proj=out_proj, **kw)
            both = run(x, frag, frag_ip)
            assert torch.isfinite(both.float()).all()
            for i in range(2):
                alone = run(x[i * rpc:(i + 1) * rpc].contiguous(), frag[i:i + 1].contiguous(), frag_ip[i:i + 1].contiguous())
                assert torch.equal(bits(both[i * rpc:(i + 1) * rpc]), bits(alone)), (with_ip, out_proj is not None, i)
            swapped = run(x, frag.flip(0).contiguous(), frag_ip.flip(0).contiguous())
            assert not torch.equal(swapped, both), "the context index does not reach the kernel"


def test_attention_with_kv_group_one_and_two_contexts(dev):
    """i2v_attention_f16 as the un-fused cross-attention launches it with per-frame contexts: kv_group = 1, lk = 77"""
    k = K()
    heads, d, lq, lk = 4, 16, 64, 77
    c = heads * d
    g = torch.Generator().manual_seed(5)
    D = lambda t: t.half().to(dev)
    q, kk = D(torch.randn(2 * lq, c, generator=g)), D(torch.randn(2 * lk, c, generator=g))
    vt = torch.zeros(2, c, k.pad8(lk))
    vt[:, :, :lk] = torch.randn(2, c, lk, generator=g)
    vt = D(vt)
    both = k.attention(q, kk, vt, batch_q=2, lq=lq, lk=lk, heads=heads, head_dim=d, kv_group=1)
    def one(i):                               # fp32 on the host: softmax(q k^T / sqrt(d)) v per head
        qh = q[i * lq:(i + 1) * lq].float().cpu().view(lq, heads, d).transpose(0, 1)
        kh = kk[i * lk:(i + 1) * lk].float().cpu().view(lk, heads, d).transpose(0, 1)
        vh = vt[i, :, :lk].float().cpu().view(heads, d, lk).transpose(1, 2)
        return (torch.softmax(qh @ kh.transpose(1, 2) * d ** -0.5, dim=-1) @ vh).transpose(0, 1).reshape(lq, c)
    ref = torch.cat([one(0), one(1)])
    compare(both, ref, rel=REL_TOL_MODULE, name="attention kv_group = 1, two contexts")
    for i in range(2):
        alone = k.attention(q[i * lq:(i + 1) * lq], kk[i * lk:(i + 1) * lk], vt[i:i + 1].contiguous(), batch_q=1, lq=lq, lk=lk, heads=heads,
                            head_dim=d, kv_group=1)
        assert torch.equal(bits(both[i * lq:(i + 1) * lq]), bits(alone)), i


# ---------------------------------------------------------------------------------------------------------- the block
def _block_pair(dev, dim, heads, head_dim, ctx_dim, ip_tokens, seed):
    from oracle.i2v_adapter import I2VAdapterTransformerBlock as O
    torch.manual_seed(seed)
    o = round_fp16_(O(dim, heads, head_dim, dropout=0.0, cross_attention_dim=ctx_dim)).eval()
    m = pkg().I2VAdapterTransformerBlock(dim, heads, head_dim, dropout=0.0, cross_attention_dim=ctx_dim)
    m.load_state_dict(o.state_dict())
    m = m.to(device=dev, dtype=f16).eval()
    if ip_tokens:
        g = torch.Generator().manual_seed(seed + 1)
        wk, wv = h16(torch.randn(dim, ctx_dim, generator=g) * 0.1), h16(torch.randn(dim, ctx_dim, generator=g) * 0.1)
        o.attn2.install_ip_adapter(wk, wv, num_tokens=ip_tokens, scale=0.7)
        m.attn2.install_ip_adapter(wk.to(dev), wv.to(dev), num_tokens=ip_tokens, scale=0.7)
    return o, m


@pytest.mark.parametrize("ip_tokens", [0, 4])
@pytest.mark.parametrize("dim,heads,head_dim,hw", [(320, 8, 40, 16), (64, 4, 16, 8)], ids=["width-320-fused", "width-64-unfused"])
def test_transformer_block_with_one_context_per_frame(dev, dim, heads, head_dim, hw, ip_tokens):
    """frames alternate between two contexts (+ image tokens that stay the sample's): against the oracle's block, which takes one context
    row per frame as it stands, at the tolerance of the block's existing test.  Width 320 at 16 x 16 runs i2v_cross_attn_fused_f16 with
    one context per frame, width 64 the un-fused kernels; with the CFG-shared prefix the block gets one half of the batch and the
    contexts of both."""
    frames, ctx_dim, lt, L = 2, 64, 77, hw * hw
    o, m = _block_pair(dev, dim, heads, head_dim, ctx_dim, ip_tokens, seed=dim)
    fused = K().cross_attn_fused_supported(2 * frames * L, dim, heads, head_dim, lt, L)
    assert fused == (dim == 320), "the route this case is here for"
    g = torch.Generator().manual_seed(2)
    x = h16(torch.randn(frames, L, dim, generator=g))
    two = h16(torch.randn(2, lt, ctx_dim, generator=g))
    ip = h16(torch.randn(1, ip_tokens, ctx_dim, generator=g)) if ip_tokens else None

    def context(order):                       # [len(order), lt (+ ip), D]
        t = two[list(order)]
        return t if ip is None else torch.cat([t, ip.expand(len(order), -1, -1)], dim=1)
    kw = dict(enable_cross_frame_attn=True, num_frames=frames)
    with torch.no_grad():
        ref = o(x, encoder_hidden_states=context((0, 1)), **kw)
        same = o(x, encoder_hidden_states=context((0, 0)), **kw)
        got = m(x.half().to(dev), encoder_hidden_states=context((0, 1)).half().to(dev), **kw)
    assert (ref - same).abs().max().item() > 10 * REL_TOL_MODULE * ref.abs().max().item(), "the second context does not move the output"
    compare(got, ref, name=f"block width {dim}, one context per frame, {ip_tokens} image tokens")
    # the CFG-shared prefix: x is ONE half, the contexts are [negative half ; positive half], each one per frame
    order = (1, 0, 0, 1)
    with torch.no_grad():
        ref2 = o(torch.cat([x, x]), encoder_hidden_states=context(order), **kw)
        ctx = context(order).half().to(dev)
        ct, ci = (ctx[:, :lt].contiguous(), ctx[:, lt:].contiguous()) if ip_tokens else (ctx, None)
        got2 = m._fwd(x.half().to(dev).view(-1, dim), frames, L, True, frames, ct, ci, cfg_expand=True)
    compare(got2.view(2 * frames, L, dim), ref2, name=f"block width {dim}, one context per frame, CFG-shared prefix")


# ---------------------------------------------------------------------------------------------------------- the UNet
@pytest.fixture(scope="module", params=[False, True], ids=["text", "text+ip"])
def per_frame_unet(request, dev):
    """(HIP UNet, inputs, per-frame contexts, the per-frame oracle's output, the output with every frame on its sample's first context):
    a CFG-shaped batch of 2 x 2 frames whose frames alternate between two contexts"""
    ip = request.param
    ou, ipsd = R.oracle_small_unet_per_frame(ip=ip)
    hu = hip_unet_from_oracle(ou, dev, ip_state_dict=ipsd)
    inp = small_unet_inputs(b=2, f=2)
    one = inp["sample"][:1]
    inp["sample"], inp["timestep"] = torch.cat([one, one]), torch.tensor([481, 481])
    g = torch.Generator().manual_seed(17)
    ctx = h16(torch.randn(4, 7, 64, generator=g))                             # rows in the order (sample, frame)
    added = {"image_embeds": inp["image_embeds"]} if ip else None
    with torch.no_grad():
        want = ou(inp["sample"], inp["timestep"], True, ctx, added_cond_kwargs=added).sample
        flat = ou(inp["sample"], inp["timestep"], True, ctx[[0, 0, 2, 2]], added_cond_kwargs=added).sample
    return hu, inp, ctx, want, flat, ip


@pytest.mark.parametrize("cfg_shared", [False, True])
def test_unet_with_one_context_per_frame_against_the_oracle(dev, per_frame_unet, cfg_shared):
    hu, inp, ctx, want, flat, ip = per_frame_unet
    moved = (want - flat).abs().max().item()
    assert moved > 10 * REL_TOL_UNET * want.abs().max().item(), "the per-frame contexts move the output by less than 10 x the tolerance"
    added = {"image_embeds": inp["image_embeds"].to(dev)} if ip else None
    kw = dict(cross_attention_kwargs={"cfg_shared_prefix": True}) if cfg_shared else {}
    with torch.no_grad():
        got = hu(inp["sample"].to(dev), inp["timestep"].to(dev), True, ctx.to(dev), added_cond_kwargs=added, **kw).sample
    compare(got, want, rel=REL_TOL_UNET, name=f"small UNet, one context per frame, ip={ip}, cfg_shared={cfg_shared}")
    if not cfg_shared:
        # the projected form the pipeline's step reads: K / V^T of B * F contexts, the image tokens expanded once
        with torch.no_grad():
            ctx_ip = hu._expand_image_tokens(hu._project_image_embeds(added), 4)
            pc = hu.project_context(ctx.to(dev).half(), ctx_ip)
            again = hu(inp["sample"].to(dev), inp["timestep"].to(dev), True, pc, added_cond_kwargs=added).sample
        assert torch.equal(again, got)
        with pytest.raises(ValueError, match=r"\[B, L, D\] or \[B \* F, L, D\]"):
            hu(inp["sample"].to(dev), inp["timestep"].to(dev), True, ctx[:3].to(dev), added_cond_kwargs=added)


# ---------------------------------------------------------------------------------------------------------- the pipeline
TEXT64 = dict(vocab_size=256, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1,
              max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=255)
A, B, C3 = "a red fox", "snow falls", "night"


@pytest.fixture(scope="module")
def parts(dev):
    unet = hip_model_random(SMALL_UNET, dev)
    te = pkg().CLIPTextModel(**TEXT64)
    te.load_state_dict(seeded_state(TEXT64, seed=31, qk_gain=3.0))
    return unet, te.half().to(dev).eval()


def _pipe(parts, **kw):
    unet, te = parts
    return pkg().I2VAdapterPipeline(unet=unet, text_encoder=te, tokenizer=StubTokenizer(77, 256), **kw)


def _gens(seed=5):
    return dict(generator=torch.Generator().manual_seed(seed), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _kw(samples=1, frames=4, **over):
    cond = torch.randn(samples, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    return {**dict(condition_image_latents=cond, num_frames=frames, num_inference_steps=3, guidance_scale=2.0, output_type="latent"), **over}


def test_encode_prompt_travel_against_the_reference(dev, parts):
    """the 4-D embeddings: keyframe frames are the text encoder's rows bit for bit, the frames between meet the kernel's bound against
    the fp64 interpolation of those rows, the last prompt is held; a batch of two dicts with different keys, a str negative prompt,
    two videos per prompt, no guidance, the callback"""
    pipe = _pipe(parts)
    prompts = [{0: A, 3: B, 5: C3}, {0: B, 6: A}]
    pe, ne = pipe.encode_prompt_travel(prompts, 8, dev, 1, True, negative_prompt="blurry")
    assert pe.shape == ne.shape == (2, 8, 77, 64) and pe.dtype == f16 and pe.is_cuda
    # the source rows: the same texts in the same single call (another batch of texts may take other GEMM routes: the keyframe frames are
    # copies of THIS call's rows)
    texts = ["blurry", "blurry", A, B, C3, B, A]
    enc = pipe._encode_texts(texts).cpu()
    first_row = {0: 2, 1: 5}
    for i, d in enumerate(prompts):
        keys = sorted(d)
        src = enc[first_row[i]: first_row[i] + len(keys)]
        lo, hi, w = R.batch_frame_sources([keys], 8)
        worst, ok = R.check_interp_rows(pe[i].cpu(), src, lo, hi, w)
        assert ok, (i, worst)
        for j, k in enumerate(keys):
            assert torch.equal(bits(pe[i, k].cpu()), bits(src[j])), "a keyframe's frame is not its embedding"
        assert torch.equal(pe[i, 7], pe[i, keys[-1]])                         # held to the end
        assert not torch.equal(pe[i, 1], pe[i, 0])
    assert all(torch.equal(bits(ne[i, f].cpu()), bits(enc[i])) for i in range(2) for f in range(8))
    # the keyframe texts of the whole batch, negative ones included, went through the text encoder in one call
    pipe.tokenizer.calls.clear()
    pipe.encode_prompt_travel(prompts, 8, dev, 1, True, negative_prompt="blurry")
    assert [c[0] for c in pipe.tokenizer.calls] == [tuple(texts)]
    # two videos per prompt: every sample twice in a row, negatives alike (the same texts, so the same rows)
    pe2, ne2 = pipe.encode_prompt_travel(prompts, 8, dev, 2, True, negative_prompt=["blurry", "blurry"])
    assert pe2.shape == (4, 8, 77, 64) and torch.equal(pe2, pe.repeat_interleave(2, 0)) and torch.equal(ne2, ne.repeat_interleave(2, 0))
    # a negative prompt may travel on its own
    _, ne3 = pipe.encode_prompt_travel(prompts, 8, dev, 1, True, negative_prompt=["blurry", {0: "x", 7: "y"}])
    assert torch.equal(ne3[0, 0], ne3[0, 7]) and not torch.equal(ne3[1, 3], ne3[1, 0]) and not torch.equal(ne3[1, 7], ne3[1, 0])
    pe1, none = pipe.encode_prompt_travel(prompts[0], 8, dev, 1, False, negative_prompt="never read")
    assert none is None and pe1.shape == (1, 8, 77, 64)
    assert R.check_interp_rows(pe1[0].cpu(), pipe._encode_texts([A, B, C3]).cpu(), *R.batch_frame_sources([[0, 3, 5]], 8))[1]
    skip, _ = pipe.encode_prompt_travel(prompts[0], 8, dev, 1, False, clip_skip=1)
    assert torch.equal(bits(skip[0, 3]), bits(pipe._encode_texts([A, B, C3], clip_skip=1)[1])) and not torch.equal(skip, pe1)
    calls = []

    def cb(s, e, a, b):
        calls.append((s, e))
        return torch.stack([a if i < e - s else b for i in range(e - s + 1)])           # a step: hold the start, jump at the end
    pc, _ = pipe.encode_prompt_travel(prompts[0], 8, dev, 1, False, interpolation_callback=cb)
    want = R.interpolate(pipe._encode_texts([A, B, C3]).cpu(), [0, 3, 5], 8, callback=cb)
    assert calls[:2] == [(0, 3), (3, 5)] and torch.equal(pc[0].cpu().double(), want)
    with pytest.raises(ValueError, match="interpolation_callback"):
        pipe.encode_prompt_travel(prompts[0], 8, dev, 1, False, interpolation_callback=lambda s, e, a, b: a)


def test_pipeline_takes_keyframed_prompts(dev, parts):
    """fails on the parent commit, where a dict `prompt` raises ValueError.  The dict call equals the call with the 4-D embeds of
    encode_prompt_travel; captured equals eager; a second call with other prompts replays the captured step and equals a fresh
    pipeline's result -- all bit for bit"""
    pipe = _pipe(parts)
    travel, neg = {0: A, 3: B}, "blurry"
    got = pipe(prompt=travel, negative_prompt=neg, **_kw(), **_gens()).frames
    assert got.shape == (1, 4, 4, 16, 16) and torch.isfinite(got).all()
    pe, ne = pipe.encode_prompt_travel(travel, 4, dev, 1, True, negative_prompt=neg)
    assert torch.equal(got, pipe(prompt_embeds=pe, negative_prompt_embeds=ne, **_kw(), **_gens()).frames)
    # a 3-D negative next to 4-D positive embeds is repeated per frame
    assert torch.equal(got, pipe(prompt_embeds=pe, negative_prompt_embeds=ne[:, 0], **_kw(), **_gens()).frames)
    assert torch.equal(got, pipe(prompt=travel, negative_prompt=neg, use_graph=False, **_kw(), **_gens()).frames)
    plain = pipe(prompt=A, negative_prompt=neg, **_kw(), **_gens()).frames
    assert not torch.equal(got[:, 3], plain[:, 3]), "the second keyframe does not reach the last frame"
    # a second sample with the same shapes and other prompts: the cache is hit, the per-frame contexts are copied in
    first = pipe(prompt=travel, negative_prompt=neg, **_kw(), **_gens()).frames
    graph = pipe._graph
    other = {0: B, 2: C3}
    again = pipe(prompt=other, negative_prompt={0: neg, 3: A}, **_kw(), **_gens()).frames
    assert pipe._graph is graph and len(pipe._graph_cache) == 1, "a second sample of the same shape re-captured the step"
    fresh = _pipe(parts)(prompt=other, negative_prompt={0: neg, 3: A}, **_kw(), **_gens()).frames
    assert torch.equal(first, got) and torch.equal(again, fresh) and not torch.equal(again, got)
    # a callback runs the steps eagerly: the same bits
    seen = []
    cb = pipe(prompt=travel, negative_prompt=neg, callback=lambda i, t, lat: seen.append(i), **_kw(), **_gens()).frames
    assert seen == [0, 1, 2] and torch.equal(cb, got)


def test_single_key_dict_is_the_str_call(dev, parts):
    pipe = _pipe(parts)
    want = pipe(prompt=A, negative_prompt="blurry", **_kw(), **_gens()).frames
    pipe.tokenizer.calls.clear()
    got = pipe(prompt={0: A}, negative_prompt={0: "blurry"}, **_kw(), **_gens()).frames
    assert torch.equal(got, want) and len(pipe._graph_cache) == 1
    assert [c[0] for c in pipe.tokenizer.calls] == [(A,), (A,), ("blurry",)]      # encode_prompt's calls, not the travel path's one
    two = pipe(prompt=[{0: A}, B], negative_prompt=["blurry", {0: "x"}], **_kw(2), **_gens()).frames
    assert torch.equal(two, pipe(prompt=[A, B], negative_prompt=["blurry", "x"], **_kw(2), **_gens()).frames)


@pytest.mark.parametrize("kind", ["ddim", "dpmsolver++", "lcm"])
def test_pipeline_graph_equals_eager_under_every_scheduler(dev, parts, kind):
    p = pkg()
    sched = {"ddim": p.DDIMScheduler, "dpmsolver++": p.DPMSolverMultistepScheduler, "lcm": p.LCMScheduler}[kind]
    pipe = _pipe(parts, scheduler=sched())
    travel = {0: A, 2: B}
    graph = pipe(prompt=travel, **_kw(), **_gens()).frames
    eager = pipe(prompt=travel, use_graph=False, **_kw(), **_gens()).frames
    assert torch.isfinite(graph).all() and torch.equal(graph, eager) and len(pipe._graph_cache) == 1
    assert not torch.equal(graph, pipe(prompt=A, **_kw(), **_gens()).frames)


def test_pipeline_without_guidance_runs_one_copy(dev, parts):
    pipe = _pipe(parts)
    kw = _kw(guidance_scale=1.0)
    got = pipe(prompt={0: A, 3: B}, negative_prompt={0: "never", 1: "read"}, **kw, **_gens()).frames
    pe, none = pipe.encode_prompt_travel({0: A, 3: B}, 4, dev, 1, False)
    assert none is None and torch.equal(got, pipe(prompt_embeds=pe, **kw, **_gens()).frames)
    assert torch.equal(got, pipe(prompt={0: A, 3: B}, use_graph=False, **kw, **_gens()).frames)


def test_pipeline_two_samples_and_two_videos_per_prompt(dev, parts):
    pipe = _pipe(parts)
    prompts = [{0: A, 3: B}, C3]
    got = pipe(prompt=prompts, negative_prompt="blurry", **_kw(2), **_gens()).frames
    pe, ne = pipe.encode_prompt_travel(prompts, 4, dev, 1, True, negative_prompt="blurry")
    assert got.shape[0] == 2 and torch.equal(got, pipe(prompt_embeds=pe, negative_prompt_embeds=ne, **_kw(2), **_gens()).frames)
    twice = pipe(prompt={0: A, 3: B}, num_videos_per_prompt=2, **_kw(2), **_gens()).frames
    pe2, ne2 = pipe.encode_prompt_travel({0: A, 3: B}, 4, dev, 2, True)
    assert torch.equal(twice, pipe(prompt_embeds=pe2, negative_prompt_embeds=ne2, **_kw(2), **_gens()).frames)


def test_pipeline_with_free_noise(dev, parts):
    """8 frames in windows of 4: the clip FreeNoise is for, with a prompt that travels over it"""
    pipe = _pipe(parts)
    pipe.enable_free_noise(context_length=4, context_stride=2)
    try:
        travel = {0: A, 4: B, 7: C3}
        graph = pipe(prompt=travel, **_kw(frames=8), **_gens()).frames
        eager = pipe(prompt=travel, use_graph=False, **_kw(frames=8), **_gens()).frames
        plain = pipe(prompt=A, **_kw(frames=8), **_gens()).frames
    finally:
        pipe.disable_free_noise()
    assert graph.shape[1] == 8 and torch.isfinite(graph).all() and torch.equal(graph, eager) and not torch.equal(graph, plain)


def test_pipeline_with_free_init(dev, parts):
    pipe = _pipe(parts)
    pipe.enable_free_init(num_iters=2)
    travel = {0: A, 3: B}
    graph = pipe(prompt=travel, **_kw(), **_gens()).frames
    eager = pipe(prompt=travel, use_graph=False, **_kw(), **_gens()).frames
    pipe.disable_free_init()
    once = pipe(prompt=travel, **_kw(), **_gens()).frames
    assert torch.isfinite(graph).all() and torch.equal(graph, eager) and not torch.equal(graph, once)
    assert len(pipe._graph_cache) == 1                                        # the rounds and the plain call replay one captured step


def test_pipeline_with_a_controlnet(dev, parts):
    from tests import controlnet_reference as CR
    cn = pkg().ControlNetModel(**CR.small_config())
    cn.load_state_dict(CR.small_reference().state_dict())
    pipe = _pipe(parts, controlnet=cn.to(dev, f16).eval())
    frames = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(9))
    travel = {0: A, 3: B}
    graph = pipe(prompt=travel, control_image=frames, **_kw(), **_gens()).frames
    eager = pipe(prompt=travel, control_image=frames, use_graph=False, **_kw(), **_gens()).frames
    plain = pipe(prompt=A, control_image=frames, **_kw(), **_gens()).frames
    off = pipe(prompt=travel, control_image=frames, controlnet_conditioning_scale=0.0, **_kw(), **_gens()).frames
    assert torch.isfinite(graph).all() and torch.equal(graph, eager) and not torch.equal(graph, plain)
    assert torch.equal(off, _pipe(parts)(prompt=travel, **_kw(), **_gens()).frames)     # scale 0: the pipeline without a ControlNet


def test_pipeline_with_a_t2i_adapter(dev, parts):
    from tests import t2i_adapter_reference as TR
    ad = pkg().T2IAdapter(**TR.small_config(3))
    ad.load_state_dict(TR.small_reference(3).state_dict())
    pipe = _pipe(parts, t2i_adapter=ad.to(dev, f16).eval())
    frames = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(9))
    travel = {0: A, 3: B}
    graph = pipe(prompt=travel, adapter_image=frames, **_kw(), **_gens()).frames
    eager = pipe(prompt=travel, adapter_image=frames, use_graph=False, **_kw(), **_gens()).frames
    off = pipe(prompt=travel, adapter_image=frames, adapter_conditioning_scale=0.0, **_kw(), **_gens()).frames
    assert torch.isfinite(graph).all() and torch.equal(graph, eager) and not torch.equal(graph, off)
    assert torch.equal(off, _pipe(parts)(prompt=travel, **_kw(), **_gens()).frames)


@pytest.mark.parametrize("plus", [False, True], ids=["ip-adapter", "ip-adapter-plus"])
def test_pipeline_with_an_ip_adapter(dev, parts, plus):
    """the image tokens (4, or 16 from the Resampler) are one set per sample and get one set per frame next to per-frame text contexts"""
    unet = hip_model_random(SMALL_UNET, dev)                                  # its own UNet: loading an adapter changes the model
    pipe = _pipe((unet, parts[1]))
    g = torch.Generator().manual_seed(4)
    if plus:
        from tests.ip_adapter_plus_reference import plus_state_dict
        pipe.load_ip_adapter(plus_state_dict(unet, embed_dims=64, hidden=128, heads=2, depth=2, num_queries=16))
        image, image2 = (torch.randn(1, 257, 64, generator=g).half() for _ in range(2))
    else:
        unet._load_ip_adapter_weights(small_ip_state_dict(unet))
        image, image2 = (torch.randn(1, 48, generator=g).half() for _ in range(2))
    assert {a.ip_num_tokens for a in unet._cross_attention_layers()} == {16 if plus else 4}
    travel = {0: A, 3: B}
    graph = pipe(prompt=travel, image_embeds=image, **_kw(), **_gens()).frames
    eager = pipe(prompt=travel, image_embeds=image, use_graph=False, **_kw(), **_gens()).frames
    assert torch.isfinite(graph).all() and torch.equal(graph, eager)
    pe, ne = pipe.encode_prompt_travel(travel, 4, dev, 1, True)
    assert torch.equal(graph, pipe(prompt_embeds=pe, negative_prompt_embeds=ne, image_embeds=image, **_kw(), **_gens()).frames)
    other = pipe(prompt=travel, image_embeds=image2, **_kw(), **_gens()).frames
    assert len(pipe._graph_cache) == 1 and not torch.equal(other, graph), "the image tokens do not reach the replayed graph"
    assert not torch.equal(graph, pipe(prompt=A, image_embeds=image, **_kw(), **_gens()).frames)
    # every frame on one context, given per frame: the image branch reads the sample's tokens on every frame, as the plain call does
    flat, _ = pipe.encode_prompt(A, dev, 1, False)
    neg, _ = pipe.encode_prompt("", dev, 1, False)
    want = pipe(prompt_embeds=flat, negative_prompt_embeds=neg, image_embeds=image, **_kw(), **_gens()).frames
    per_frame = pipe(prompt_embeds=flat[:, None].expand(-1, 4, -1, -1), negative_prompt_embeds=neg, image_embeds=image, **_kw(), **_gens()).frames
    # (two evaluations of one trajectory by other launch forms -- kv_group 1 against kv_group F: each is within the trajectory tolerance
    # of the exact result, so they are within twice that of each other)
    compare(per_frame, want, rel=2 * REL_TOL_TRAJECTORY, name=f"pipeline, per-frame copies of one context, plus={plus}")


def test_the_handle_and_the_trainer_refuse_per_frame_contexts(dev, parts):
    from i2v_adapter_unofficial_amd import handle, training
    pipe = _pipe(parts)
    pe, ne = pipe.encode_prompt_travel({0: A, 3: B}, 4, dev, 1, True)
    st = dict(latents=torch.zeros(1, 4, 4, 16, 16, device=dev), copies=2, ctx_text=torch.cat([ne, pe]).view(-1, 77, 64), ctx_ip=None)
    for fn in (handle.record_step_plan, handle.record_prepare_plan):
        with pytest.raises(NotImplementedError, match="per-frame text contexts"):
            fn(pipe, st)
    with pytest.raises(NotImplementedError, match="per-frame text contexts"):
        handle.export_denoiser(pipe, "unused", num_frames=4, latent_height=16, latent_width=16, per_frame_context=True)
    with pytest.raises(NotImplementedError, match="per-frame text contexts"):
        training.UNetAdapterTrainer(parts[0]).forward(torch.zeros(1, 4, 4, 16, 16, device=dev), 10, pe)
