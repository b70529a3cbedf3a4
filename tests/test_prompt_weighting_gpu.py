"""Weighted and long prompts on the GPU: i2v_weight_embeds_f16 against float64 under the bound of tests/prompt_weight_bounds.py (every
element of every case), its exact properties (all-ones weights are a copy, zero weights give zero rows, in place equals out of place,
strided rows inside poisoned buffers, repeats are bit-equal, a cancelling input reports a non-finite ratio and leaves x * w), and the
pipeline: `encode_weighted_prompt` against the restatement evaluated on the HIP encoder's own chunk outputs, the short-unweighted
invariant bit for bit, equal shapes for prompt and negative prompt, `num_videos_per_prompt`, `clip_skip`, and `pipe(prompt="(a:1.3) b")`
on the reduced UNet."""
import os

import pytest
import torch

from tests import prompt_weight_bounds as B
from tests import prompt_weight_reference as R
from tests.clip_text_reference import PREFIX, seeded_state
from tests.parity import ROOT, SMALL_UNET, hip_model_random
from tests.textual_inversion_reference import WordTokenizer

pytestmark = pytest.mark.gpu
f16 = torch.float16
POISON = -12345.0
SMALL = dict(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
             max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=255)
TEXT64 = dict(SMALL, hidden_size=64, num_attention_heads=1)


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def K():
    return pkg().kernels


def bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("p,t,d", B.CASES)
def test_weight_embeds_against_fp64(dev, p, t, d):
    x, w = B.case_inputs(p, t, d)
    for restore in (True, False):
        out, ratio = K().weight_embeds(x.to(dev), w.to(dev), restore_mean=restore)
        assert out.shape == x.shape and out.dtype == f16 and ratio.shape == (p,) and ratio.dtype == torch.float32
        worst, ok = B.check(out.cpu(), x, w, restore)
        print(f"i2v_weight_embeds_f16 P={p} T={t} D={d} restore_mean={restore}: worst error / bound {worst:.3f}")
        assert ok, worst
        want = R.weight_ref64(x, w, restore)[1]
        assert torch.allclose(ratio.cpu().double(), want, rtol=float(B.ratio_error(x, w, restore).max()) + 1e-12, atol=0)
        if not restore:
            assert bool((ratio == 1.0).all())
            assert torch.equal(out.cpu(), (x.float() * w[:, :, None]).half())       # one fp32 product, one rounding: exact


def test_weight_embeds_ill_conditioned_mean_meets_the_same_wider_bound(dev):
    x, w = B.case_inputs(1, 77, 768, offset=0.02)
    assert float(B.ratio_error(x, w)) > 5 * float(B.ratio_error(*B.case_inputs(1, 77, 768)))
    out, _ = K().weight_embeds(x.to(dev), w.to(dev))
    worst, ok = B.check(out.cpu(), x, w)
    print(f"i2v_weight_embeds_f16 ill-conditioned: worst error / bound {worst:.3f}")
    assert ok, worst


@pytest.mark.parametrize("p,t,d", [(1, 1, 8), (2, 231, 768), (5, 7, 24)])
def test_weight_embeds_exact_properties(dev, p, t, d):
    x, w = B.case_inputs(p, t, d)
    xd = x.to(dev)
    # all-ones weights: the two sums are one sequence of operations, r == 1, a copy -- also of -0, and also when the sums are 0 / 0
    xs = x.clone()
    xs.view(-1)[0] = -0.0
    for src in (xs, torch.zeros_like(x)):
        out, ratio = K().weight_embeds(src.to(dev), torch.ones(p, t, device=dev))
        assert torch.equal(bits(out.cpu()), bits(src))
        assert bool((ratio == 1.0).all()) or not src.any()
    # a zero weight gives zero rows, negative weights work, the bound holds for both
    wz = w.clone()
    wz[:, t // 2] = 0.0
    wz[:, -1] = -0.75
    out, _ = K().weight_embeds(xd, wz.to(dev))
    assert not out[:, t // 2].any() or t == 1
    assert B.check(out.cpu(), x, wz)[1]
    # in place equals out of place, repeats are bit-equal
    once, r1 = K().weight_embeds(xd, w.to(dev))
    again, r2 = K().weight_embeds(xd, w.to(dev))
    assert torch.equal(bits(once), bits(again)) and torch.equal(r1, r2)
    buf = xd.clone()
    same, r3 = K().weight_embeds(buf, w.to(dev), out=buf)
    assert same.data_ptr() == buf.data_ptr() and torch.equal(bits(buf), bits(once)) and torch.equal(r3, r1)
    assert torch.equal(xd.cpu(), x), "the out-of-place launch wrote its source"


@pytest.mark.parametrize("p,t,d", [(3, 154, 768), (2, 33, 1032), (5, 7, 24)])
def test_weight_embeds_strided_rows_inside_poisoned_buffers(dev, p, t, d):
    x, w = B.case_inputs(p, t, d)
    want, _ = K().weight_embeds(x.to(dev), w.to(dev))
    src = torch.full((p * t + 2, d + 16), POISON, dtype=f16, device=dev)
    out = torch.full((p * t + 2, d + 24), POISON, dtype=f16, device=dev)
    sv = src[1:1 + p * t].view(p, t, d + 16)[:, :, 8:8 + d]
    ov = out[1:1 + p * t].view(p, t, d + 24)[:, :, 16:16 + d]
    sv.copy_(x.to(dev))
    got, _ = K().weight_embeds(sv, w.to(dev), out=ov)
    assert got.data_ptr() == ov.data_ptr() and torch.equal(bits(ov), bits(want))
    margin = torch.ones_like(out, dtype=torch.bool)
    margin[1:1 + p * t, 16:16 + d] = False
    assert bool((out[margin] == POISON).all()), "the kernel wrote outside its rows"
    keep = torch.ones_like(src, dtype=torch.bool)
    keep[1:1 + p * t, 8:8 + d] = False
    assert bool((src[keep] == POISON).all()) and torch.equal(sv.cpu(), x)
    # refusals: a width that is no multiple of 8, rows that are not unit-stride, rows that do not start on 16 bytes
    with pytest.raises(ValueError, match="multiple of 8"):
        K().weight_embeds(x.to(dev)[:, :, :d - 4], w.to(dev))
    with pytest.raises(ValueError, match="unit-stride rows"):
        K().weight_embeds(torch.zeros(2, 8, 16, dtype=f16, device=dev)[:, :, ::2], torch.ones(2, 8, device=dev))
    with pytest.raises(pkg().HipLibraryError, match="16-byte"):
        K().weight_embeds(src[1:1 + p * t].view(p, t, d + 16)[:, :, 4:4 + d], w.to(dev))
    with pytest.raises(ValueError, match="weights must be"):
        K().weight_embeds(x.to(dev), w.to(dev)[:, :-1])
    with pytest.raises(pkg().HipLibraryError, match="overlaps src"):
        K().weight_embeds(src[0:p * t].view(p, t, d + 16)[:, :, :d], w.to(dev), out=src[1:1 + p * t].view(p, t, d + 16)[:, :, :d])


def test_weight_embeds_cancelling_weights_report_a_non_finite_ratio(dev):
    x = torch.ones(2, 4, 8).half()
    x[1] = torch.randn(4, 8, generator=torch.Generator().manual_seed(0)).half() + 0.5
    w = torch.tensor([[1.0, -1.0, 2.0, -2.0], [1.0, 1.2, 0.9, 1.0]])
    out, ratio = K().weight_embeds(x.to(dev), w.to(dev))
    assert not torch.isfinite(ratio[0]) and torch.isfinite(ratio[1])
    assert torch.equal(out[0].cpu(), (x[0].float() * w[0][:, None]).half())                     # r = 1 for the outputs
    assert B.check(out[1:].cpu(), x[1:], w[1:])[1]


# ---------------------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def unet(dev):
    return hip_model_random(SMALL_UNET, dev)


@pytest.fixture(scope="module")
def pipe128(dev, unet):
    """the committed small CLIP fixture (hidden 128) behind the word tokenizer: for the encode tests, which do not run the UNet"""
    from safetensors.torch import load_file
    blob = load_file(os.path.join(ROOT, "tests", "golden", "clip_text_small.safetensors"))
    te = pkg().CLIPTextModel(**SMALL)
    te.load_state_dict({k: v.float() for k, v in blob.items() if k.startswith(PREFIX)})
    return pkg().I2VAdapterPipeline(unet=unet, text_encoder=te.half().to(dev).eval(), tokenizer=WordTokenizer())


@pytest.fixture(scope="module")
def pipe64(dev, unet):
    te = pkg().CLIPTextModel(**TEXT64)
    te.load_state_dict(seeded_state(TEXT64, seed=31, qk_gain=3.0))
    return pkg().I2VAdapterPipeline(unet=unet, text_encoder=te.half().to(dev).eval(), tokenizer=WordTokenizer())


LONG = " ".join(f"w{i}" for i in range(80))                      # 80 tokens: two chunks
WEIGHTED = "a (red:1.4) fox [runs] on the ((beach)) at sunset"


def _reference(pipe, prompts, negatives, multiples, clip_skip=None):
    """(src [P, n * M, D] fp16 as the HIP encoder gives the chunks, weights [P, n * M]): negatives first"""
    tok, te = pipe.tokenizer, pipe.text_encoder
    ids, weights, n = R.prompt_rows(tok, negatives + prompts, multiples, tok.bos_id, tok.eos_id, tok.pad_id)
    src = {}
    for name, part in (("prompts", ids[len(negatives):]), ("negatives", ids[:len(negatives)])):    # the pipeline's two calls, in its order
        if part.shape[0]:
            flat = part.reshape(-1, 77)
            if clip_skip is None:
                e = te(flat)[0]
            else:
                e = te.text_model.final_layer_norm(te(flat, output_hidden_states=True)[-1][-(clip_skip + 1)])
            src[name] = e.reshape(part.shape[0], n * 77, -1)
    return torch.cat([src[k] for k in ("negatives", "prompts") if k in src]).cpu(), weights.float(), n


@pytest.mark.parametrize("restore", [True, False])
def test_encode_weighted_prompt_against_the_reference(dev, pipe128, restore):
    pipe = pipe128
    pipe.enable_prompt_weighting(max_embeddings_multiples=3, restore_mean=restore)
    try:
        prompts, negatives = [WEIGHTED, LONG + " (night:0.6)"], ["(blurry:1.3) ugly", ""]
        pe, ne = pipe.encode_weighted_prompt(prompts, dev, 1, True, negative_prompt=negatives)
        src, weights, n = _reference(pipe, prompts, negatives, 3)
        assert n == 2 and pe.shape == ne.shape == (2, 154, 128) and pe.dtype == f16 and pe.is_cuda
        got = torch.cat([ne, pe]).cpu()
        worst, ok = B.check(got, src, weights, restore)
        print(f"encode_weighted_prompt restore_mean={restore}: worst error / bound {worst:.3f}")
        assert ok, worst
        assert not torch.equal(got, src), "the weights do not reach the embeddings"
        # the empty negative prompt has only weights of 1: its rows are the encoder's, bit for bit, padding chunk included
        assert torch.equal(bits(ne[1].cpu()), bits(src[1]))
        # a text whose weights are all 1 does not depend on restore_mean; one whose weights differ does
        pipe.enable_prompt_weighting(3, restore_mean=not restore)
        pe2, ne2 = pipe.encode_weighted_prompt(prompts, dev, 1, True, negative_prompt=negatives)
        assert torch.equal(ne2[1], ne[1]) and not torch.equal(pe2[0], pe[0])
        # truncation to one chunk: both prompts and negatives are 77 rows
        pipe.enable_prompt_weighting(1, restore_mean=restore)
        pe1, ne1 = pipe.encode_weighted_prompt(prompts, dev, 1, True, negative_prompt=negatives)
        assert pe1.shape == ne1.shape == (2, 77, 128)
        src1, w1, _ = _reference(pipe, prompts, negatives, 1)
        assert B.check(torch.cat([ne1, pe1]).cpu(), src1, w1, restore)[1]
    finally:
        pipe.disable_prompt_weighting()


@pytest.mark.parametrize("multiples", [1, 3, 7])
def test_short_unweighted_prompt_is_encode_prompts_bits(dev, pipe128, multiples):
    pipe = pipe128
    prompts, negatives = ["a red fox runs", " ".join(f"w{i}" for i in range(75))], ["blurry", ""]
    pe0, ne0 = pipe.encode_prompt(prompts, dev, 1, True, negative_prompt=negatives)
    pipe.enable_prompt_weighting(multiples)
    try:
        pe, ne = pipe.encode_weighted_prompt(prompts, dev, 1, True, negative_prompt=negatives)
        assert pe.shape == (2, 77, 128) and torch.equal(bits(pe), bits(pe0)) and torch.equal(bits(ne), bits(ne0))
        one, none = pipe.encode_weighted_prompt(prompts[0], dev, 1, False, negative_prompt="never read")
        assert none is None and torch.equal(bits(one), bits(pipe.encode_prompt(prompts[0], dev, 1, False)[0]))
        skip, _ = pipe.encode_weighted_prompt(prompts[0], dev, 1, False, clip_skip=1)
        assert torch.equal(bits(skip), bits(pipe.encode_prompt(prompts[0], dev, 1, False, clip_skip=1)[0])) and not torch.equal(skip, one)
    finally:
        pipe.disable_prompt_weighting()


def test_shapes_videos_per_prompt_clip_skip_and_the_cancelling_error(dev, pipe128):
    pipe = pipe128
    # positive and negative have one shape when only one of them is long
    for prompt, negative in ((LONG, "blurry"), ("a fox", LONG)):
        pe, ne = pipe.encode_weighted_prompt(prompt, dev, 1, True, negative_prompt=negative)
        assert pe.shape == ne.shape == (1, 154, 128)
    # two videos per prompt: (a, a, b, b), negatives alike
    prompts, negatives = [WEIGHTED, "(night:1.2) snow"], ["blurry", "(ugly:1.5)"]
    pe1, ne1 = pipe.encode_weighted_prompt(prompts, dev, 1, True, negative_prompt=negatives)
    pe2, ne2 = pipe.encode_weighted_prompt(prompts, dev, 2, True, negative_prompt=negatives)
    assert pe2.shape == (4, 77, 128) and torch.equal(pe2, pe1.repeat_interleave(2, 0)) and torch.equal(ne2, ne1.repeat_interleave(2, 0))
    # a str negative prompt serves every prompt; None is ""
    _, nes = pipe.encode_weighted_prompt(prompts, dev, 1, True, negative_prompt="blurry")
    assert torch.equal(nes[0], nes[1])
    _, ne_none = pipe.encode_weighted_prompt(prompts, dev, 1, True)
    _, ne_empty = pipe.encode_weighted_prompt(prompts, dev, 1, True, negative_prompt=["", ""])
    assert torch.equal(ne_none, ne_empty)
    # clip_skip reaches the chunks
    skip, _ = pipe.encode_weighted_prompt(prompts, dev, 1, False, clip_skip=1)
    src, weights, _ = _reference(pipe, prompts, [], 3, clip_skip=1)
    assert B.check(skip.cpu(), src, weights)[1] and not torch.equal(skip, pe1)
    # a ratio that is not finite (a weight beyond fp32 makes the weighted sum inf - inf): the ValueError names the prompt
    with pytest.raises(ValueError, match=r"prompt 1 \('\(a:1e39\) fox'\).*not finite"):
        pipe.encode_weighted_prompt(["a fox", "(a:1e39) fox"], dev, 1, False)
    pipe.enable_prompt_weighting(restore_mean=False)
    try:
        pipe.encode_weighted_prompt(["a fox", "(a:1e39) fox"], dev, 1, False)                   # nothing to restore: no ratio to fail
    finally:
        pipe.disable_prompt_weighting()


def _gens(seed=5):
    return dict(generator=torch.Generator().manual_seed(seed), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _kw(samples=1, frames=4, **over):
    cond = torch.randn(samples, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    return {**dict(condition_image_latents=cond, num_frames=frames, num_inference_steps=2, guidance_scale=2.0, output_type="latent"), **over}


def test_pipeline_takes_weighted_prompts(dev, pipe64):
    """fails on the parent commit, which has no `enable_prompt_weighting`.  `(red:1.3)` moves the result; the call equals the call with
    `encode_weighted_prompt`'s embeddings bit for bit; with weighting disabled the same string gives today's bits (the brackets are
    literal characters, unknown words to the word tokenizer)"""
    pipe = pipe64
    plain_text, weighted_text, neg = "a red fox runs", "a (red:1.3) fox runs", "(blurry:1.2) ugly"
    before = pipe(prompt=weighted_text, negative_prompt=neg, **_kw(), **_gens()).frames
    pe0, ne0 = pipe.encode_prompt(weighted_text, dev, 1, True, negative_prompt=neg)
    assert torch.equal(before, pipe(prompt_embeds=pe0, negative_prompt_embeds=ne0, **_kw(), **_gens()).frames)
    pipe.enable_prompt_weighting()
    try:
        got = pipe(prompt=weighted_text, negative_prompt=neg, **_kw(), **_gens()).frames
        plain = pipe(prompt=plain_text, negative_prompt=neg, **_kw(), **_gens()).frames
        assert torch.isfinite(got).all() and not torch.equal(got, plain) and not torch.equal(got, before)
        pe, ne = pipe.encode_weighted_prompt(weighted_text, dev, 1, True, negative_prompt=neg)
        assert torch.equal(got, pipe(prompt_embeds=pe, negative_prompt_embeds=ne, **_kw(), **_gens()).frames)
        assert torch.equal(got, pipe(prompt=weighted_text, negative_prompt=neg, use_graph=False, **_kw(), **_gens()).frames)
        # the unweighted prompt under weighting is the plain call's bits (the short-unweighted invariant, through the whole pipeline)
        pipe.disable_prompt_weighting()
        assert torch.equal(before, pipe(prompt=weighted_text, negative_prompt=neg, **_kw(), **_gens()).frames)
        pipe.enable_prompt_weighting()
        a = pipe(prompt=plain_text, negative_prompt="blurry", **_kw(), **_gens()).frames
        pipe.disable_prompt_weighting()
        assert torch.equal(a, pipe(prompt=plain_text, negative_prompt="blurry", **_kw(), **_gens()).frames)
    finally:
        pipe.disable_prompt_weighting()


def test_prompt_travel_with_weighted_keyframes(dev, pipe64):
    """keyframes that are long and weighted: the source rows of the interpolation are the weighted embeddings, all padded to one chunk
    count; a keyframe's own frame is its weighted embedding bit for bit; the dict call equals the call with the 4-D embeddings"""
    pipe = pipe64
    travel, neg = {0: WEIGHTED, 3: LONG + " (night:1.3)"}, "(blurry:1.2)"
    pipe.enable_prompt_weighting()
    try:
        pe, ne = pipe.encode_prompt_travel(travel, 4, dev, 1, True, negative_prompt=neg)
        assert pe.shape == ne.shape == (1, 4, 154, 64)
        src = pipe._encode_weighted_texts([[neg, travel[0], travel[3]]])
        assert torch.equal(bits(pe[0, 0]), bits(src[1])) and torch.equal(bits(pe[0, 3]), bits(src[2]))
        assert all(torch.equal(bits(ne[0, f]), bits(src[0])) for f in range(4)) and not torch.equal(pe[0, 1], pe[0, 0])
        got = pipe(prompt=travel, negative_prompt=neg, **_kw(), **_gens()).frames
        assert torch.isfinite(got).all()
        assert torch.equal(got, pipe(prompt_embeds=pe, negative_prompt_embeds=ne, **_kw(), **_gens()).frames)
        # a one-key dict is still the str call
        one = pipe(prompt={0: WEIGHTED}, negative_prompt=neg, **_kw(), **_gens()).frames
        assert torch.equal(one, pipe(prompt=WEIGHTED, negative_prompt=neg, **_kw(), **_gens()).frames)
    finally:
        pipe.disable_prompt_weighting()
