"""Text contexts of 154 and 231 rows (two and three chunks of a long prompt) through every layer that reads a context, none of which
was tested beyond 77: the transformer block of width 320 at 16 x 16 -- where i2v_cross_attn_fused_f16 takes a 77-row context and
declines a longer one, which then goes through `attn2._cross` / i2v_attention_f16 -- with and without the IP-Adapter's image tokens,
with one context per frame and under the CFG-shared prefix; the reduced UNet (its levels are narrower than 320: every level un-fused)
with `project_context`, image tokens, per-frame contexts and `cfg_shared_prefix`; the ControlNet's context projection; and the
pipeline with long weighted prompts: graph equals eager, a second sample replays the captured step, and a 77-row call before and after
a 154-row call gives the same bits.  Against the oracle at the tolerances tests/parity.py applies to the same modules at 77 rows."""
import pytest
import torch

from tests import controlnet_reference as CR
from tests import prompt_travel_reference as PR
from tests.clip_text_reference import seeded_state
from tests.parity import (REL_TOL_MODULE, REL_TOL_UNET, SMALL_UNET, compare, hip_model_random, hip_unet_from_oracle, oracle_small_unet,
                          round_fp16_, small_unet_inputs)
from tests.textual_inversion_reference import WordTokenizer

pytestmark = pytest.mark.gpu
f16 = torch.float16
TEXT64 = dict(vocab_size=256, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1,
              max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=255)


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h16(t):
    return t.half().float()


# ---------------------------------------------------------------------------------------------------------- the block, width 320
@pytest.fixture(scope="module", params=[0, 4], ids=["text", "text+ip"])
def block320(request, dev):
    from oracle.i2v_adapter import I2VAdapterTransformerBlock as O
    dim, heads, head_dim, ctx_dim, ip_tokens = 320, 8, 40, 64, request.param
    torch.manual_seed(320)
    o = round_fp16_(O(dim, heads, head_dim, dropout=0.0, cross_attention_dim=ctx_dim)).eval()
    m = pkg().I2VAdapterTransformerBlock(dim, heads, head_dim, dropout=0.0, cross_attention_dim=ctx_dim)
    m.load_state_dict(o.state_dict())
    m = m.to(device=dev, dtype=f16).eval()
    if ip_tokens:
        g = torch.Generator().manual_seed(321)
        wk, wv = h16(torch.randn(dim, ctx_dim, generator=g) * 0.1), h16(torch.randn(dim, ctx_dim, generator=g) * 0.1)
        o.attn2.install_ip_adapter(wk, wv, num_tokens=ip_tokens, scale=0.7)
        m.attn2.install_ip_adapter(wk.to(dev), wv.to(dev), num_tokens=ip_tokens, scale=0.7)
    return o, m, ip_tokens


@pytest.mark.parametrize("lt", [154, 231])
def test_block_of_width_320_leaves_the_fused_kernel_for_a_long_context(dev, block320, lt):
    o, m, ip_tokens = block320
    dim, heads, head_dim, ctx_dim, frames, L = 320, 8, 40, 64, 2, 256
    sup = pkg().kernels.cross_attn_fused_supported
    # the launches below: frames * L rows with one context (rows_per_ctx = frames * L) or one per frame (L); 2 * frames * L under CFG
    for rows, rpc in ((frames * L, frames * L), (frames * L, L), (2 * frames * L, L)):
        assert sup(rows, dim, heads, head_dim, 77, rpc), "at 77 rows this launch takes the fused kernel"
        assert not sup(rows, dim, heads, head_dim, lt, rpc), "a long context must leave it"
    g = torch.Generator().manual_seed(lt)
    x = h16(torch.randn(frames, L, dim, generator=g))
    two = h16(torch.randn(2, lt, ctx_dim, generator=g))
    ip = h16(torch.randn(1, ip_tokens, ctx_dim, generator=g)) if ip_tokens else None

    def context(order):
        t = two[list(order)]
        return t if ip is None else torch.cat([t, ip.expand(len(order), -1, -1)], dim=1)
    kw = dict(enable_cross_frame_attn=True, num_frames=frames)
    with torch.no_grad():
        # one context for the sample (kv_group = frames), then one per frame (kv_group = 1)
        for order in ((0,), (0, 1)):
            ref = o(x, encoder_hidden_states=context(order) if len(order) == frames else context(order).expand(frames, -1, -1), **kw)
            got = m(x.half().to(dev), encoder_hidden_states=context(order).half().to(dev), **kw)
            compare(got, ref, rel=REL_TOL_MODULE, name=f"block 320, {lt}-row context, {ip_tokens} image tokens, {len(order)} context(s)")
        # a truncated context moves the output: the rows past 77 are read
        short = o(x, encoder_hidden_states=torch.cat([two[:1, :77]] + ([ip] if ip_tokens else []), dim=1).expand(frames, -1, -1), **kw)
        full = o(x, encoder_hidden_states=context((0,)).expand(frames, -1, -1), **kw)
        assert (short - full).abs().max().item() > 10 * REL_TOL_MODULE * full.abs().max().item()
        # the CFG-shared prefix: x is ONE half, the contexts are [negative half ; positive half], one per frame
        order = (1, 0, 0, 1)
        ref2 = o(torch.cat([x, x]), encoder_hidden_states=context(order), **kw)
        ctx = context(order).half().to(dev)
        ct, ci = (ctx[:, :lt].contiguous(), ctx[:, lt:].contiguous()) if ip_tokens else (ctx, None)
        got2 = m._fwd(x.half().to(dev).view(-1, dim), frames, L, True, frames, ct, ci, cfg_expand=True)
    compare(got2.view(2 * frames, L, dim), ref2, rel=REL_TOL_MODULE, name=f"block 320, {lt}-row context, CFG-shared prefix")


# ---------------------------------------------------------------------------------------------------------- the reduced UNet
@pytest.fixture(scope="module", params=[False, True], ids=["text", "text+ip"])
def small_unet(request, dev):
    ip = request.param
    ou, ipsd = PR.oracle_small_unet_per_frame(ip=ip)
    hu = hip_unet_from_oracle(ou, dev, ip_state_dict=ipsd)
    inp = small_unet_inputs(b=2, f=2)
    one = inp["sample"][:1]
    inp["sample"], inp["timestep"] = torch.cat([one, one]), torch.tensor([481, 481])          # CFG-shaped: cfg_shared_prefix applies
    return ou, hu, inp, ip


@pytest.mark.parametrize("lt", [154, 231])
def test_unet_with_a_long_context_against_the_oracle(dev, small_unet, lt):
    ou, hu, inp, ip = small_unet
    g = torch.Generator().manual_seed(lt)
    ctx = h16(torch.randn(4, lt, 64, generator=g))                                            # rows in the order (sample, frame)
    per_sample = ctx[[0, 0, 2, 2]]
    added = {"image_embeds": inp["image_embeds"]} if ip else None
    added_d = {"image_embeds": inp["image_embeds"].to(dev)} if ip else None
    sample, t = inp["sample"].to(dev), inp["timestep"].to(dev)
    with torch.no_grad():
        want = ou(inp["sample"], inp["timestep"], True, per_sample, added_cond_kwargs=added).sample
        want_pf = ou(inp["sample"], inp["timestep"], True, ctx, added_cond_kwargs=added).sample
        cut = ou(inp["sample"], inp["timestep"], True, per_sample[:, :77], added_cond_kwargs=added).sample
        assert (want - cut).abs().max().item() > 10 * REL_TOL_UNET * want.abs().max().item(), "the rows past 77 do not move the output"
        got = hu(sample, t, True, ctx[[0, 2]].to(dev), added_cond_kwargs=added_d).sample
        compare(got, want, rel=REL_TOL_UNET, name=f"small UNet, {lt}-row context, ip={ip}")
        shared = hu(sample, t, True, ctx[[0, 2]].to(dev), added_cond_kwargs=added_d, cross_attention_kwargs={"cfg_shared_prefix": True}).sample
        compare(shared, want, rel=REL_TOL_UNET, name=f"small UNet, {lt}-row context, ip={ip}, cfg_shared")
        # the projected form the pipeline's step reads: K and V^T (lk padded to 8: 154 -> 160, 231 -> 232) once per sample
        ctx_ip = hu._project_image_embeds(added_d) if ip else None
        pc = hu.project_context(ctx[[0, 2]].to(dev).half(), ctx_ip)
        assert torch.equal(hu(sample, t, True, pc, added_cond_kwargs=added_d).sample, got)
        # one context per frame (kv_group = 1), plain and under the CFG-shared prefix
        got_pf = hu(sample, t, True, ctx.to(dev), added_cond_kwargs=added_d).sample
        compare(got_pf, want_pf, rel=REL_TOL_UNET, name=f"small UNet, {lt}-row context per frame, ip={ip}")
        shared_pf = hu(sample, t, True, ctx.to(dev), added_cond_kwargs=added_d, cross_attention_kwargs={"cfg_shared_prefix": True}).sample
        compare(shared_pf, want_pf, rel=REL_TOL_UNET, name=f"small UNet, {lt}-row context per frame, ip={ip}, cfg_shared")


# ---------------------------------------------------------------------------------------------------------- the ControlNet
@pytest.mark.parametrize("lt", [154, 231])
def test_controlnet_with_a_long_context_against_the_reference(dev, lt):
    ref = CR.small_reference()
    cn = pkg().ControlNetModel(**CR.small_config())
    cn.load_state_dict(ref.state_dict())
    cn = cn.to(dev, f16).eval()
    inp = CR.small_inputs(batch=1)
    ctx = h16(torch.randn(inp["ctx"].shape[0], lt, inp["ctx"].shape[2], generator=torch.Generator().manual_seed(lt)))
    with torch.no_grad():
        down, mid = ref(inp["sample"], inp["timestep"], ctx, inp["cond"])
        out = cn(inp["sample"].to(dev).view(1, CR.SMALL_FRAMES, 4, CR.SMALL_LATENT, CR.SMALL_LATENT), inp["timestep"].to(dev), ctx.to(dev),
                 inp["cond"].to(dev))
    for i, (g, w) in enumerate(zip(out.down_block_res_samples + (out.mid_block_res_sample,), down + (mid,))):
        compare(g, w, rel=REL_TOL_UNET, name=f"ControlNet small, {lt}-row context, tensor {i}")


# ---------------------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def pipe(dev):
    unet = hip_model_random(SMALL_UNET, dev)
    te = pkg().CLIPTextModel(**TEXT64)
    te.load_state_dict(seeded_state(TEXT64, seed=31, qk_gain=3.0))
    return pkg().I2VAdapterPipeline(unet=unet, text_encoder=te.half().to(dev).eval(), tokenizer=WordTokenizer())


def _gens(seed=5):
    return dict(generator=torch.Generator().manual_seed(seed), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _kw():
    cond = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    return dict(condition_image_latents=cond, num_frames=4, num_inference_steps=2, guidance_scale=2.0, output_type="latent")


def _long(first, n, tail):
    return " ".join(f"w{i}" for i in range(first, first + n)) + " " + tail


def test_pipeline_with_long_prompts_graph_equals_eager_and_replays(dev, pipe):
    pipe.enable_prompt_weighting()
    try:
        a, na = _long(0, 80, "(red:1.3) fox"), "(blurry:1.2) ugly"                            # 154 rows; the negative is padded to them
        graph = pipe(prompt=a, negative_prompt=na, **_kw(), **_gens()).frames
        assert torch.isfinite(graph).all()
        pe, ne = pipe.encode_weighted_prompt(a, dev, 1, True, negative_prompt=na)
        assert pe.shape == ne.shape == (1, 154, 64)
        assert torch.equal(graph, pipe(prompt=a, negative_prompt=na, use_graph=False, **_kw(), **_gens()).frames)
        assert torch.equal(graph, pipe(prompt_embeds=pe, negative_prompt_embeds=ne, **_kw(), **_gens()).frames)
        first, cached = pipe._graph, len(pipe._graph_cache)
        b, nb = _long(40, 90, "[snow] falls"), _long(100, 78, "bad hands")                    # other long prompts, the same shapes
        again = pipe(prompt=b, negative_prompt=nb, **_kw(), **_gens()).frames
        assert pipe._graph is first and len(pipe._graph_cache) == cached, "a second sample of the same shape re-captured the step"
        assert torch.equal(again, pipe(prompt=b, negative_prompt=nb, use_graph=False, **_kw(), **_gens()).frames)
        assert not torch.equal(again, graph)
        # three chunks, and keyframes that are long and weighted
        c = _long(0, 160, "(night:0.8)")
        three = pipe(prompt=c, negative_prompt=na, **_kw(), **_gens()).frames
        assert pipe.encode_weighted_prompt(c, dev, 1, False)[0].shape == (1, 231, 64)
        assert torch.equal(three, pipe(prompt=c, negative_prompt=na, use_graph=False, **_kw(), **_gens()).frames)
        travel = {0: a, 3: b}
        tg = pipe(prompt=travel, negative_prompt=na, **_kw(), **_gens()).frames
        assert torch.equal(tg, pipe(prompt=travel, negative_prompt=na, use_graph=False, **_kw(), **_gens()).frames)
        assert not torch.equal(tg[:, 3], graph[:, 3])
    finally:
        pipe.disable_prompt_weighting()


def test_a_77_row_call_before_and_after_a_154_row_call_gives_the_same_bits(dev, pipe):
    short = dict(prompt="a red fox runs", negative_prompt="blurry")
    before = pipe(**short, **_kw(), **_gens()).frames
    pipe.enable_prompt_weighting()
    try:
        under = pipe(**short, **_kw(), **_gens()).frames                                        # unweighted and short: today's bits
        long_ = pipe(prompt=_long(0, 80, "fox"), negative_prompt="blurry", **_kw(), **_gens()).frames
        after = pipe(**short, **_kw(), **_gens()).frames
    finally:
        pipe.disable_prompt_weighting()
    assert torch.equal(before, under) and torch.equal(before, after) and not torch.equal(before, long_)
    assert torch.equal(before, pipe(**short, **_kw(), **_gens()).frames)
