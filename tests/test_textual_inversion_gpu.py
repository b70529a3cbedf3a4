"""Textual inversion on the GPU: with a two-vector inversion loaded, a prompt that uses the token encodes to what the encoder gives for
the expanded ids (against the CPU restatement tests/clip_text_reference.py over the grown token table, at the gate of
tests/test_clip_text_gpu.py), a prompt that does not use it keeps its bits, and after unloading everything is as before -- through
`encode_prompt`, `encode_weighted_prompt` and `pipe(prompt=...)` on the reduced UNet."""
import pytest
import torch

from tests.clip_text_reference import ClipTextReference, seeded_state
from tests.parity import SMALL_UNET, fp16_gate, hip_model_random
from tests.textual_inversion_reference import WordTokenizer

pytestmark = pytest.mark.gpu
f16 = torch.float16
FACTOR = 2.0                      # tests/test_clip_text_gpu.py's gate: at most twice the error of torch's own fp16 evaluation
TEXT64 = dict(vocab_size=256, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1,
              max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=255)


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def parts(dev):
    return hip_model_random(SMALL_UNET, dev), seeded_state(TEXT64, seed=31, qk_gain=3.0)


def _pipe(parts, dev):
    unet, state = parts
    te = pkg().CLIPTextModel(**TEXT64)
    te.load_state_dict(state)
    return pkg().I2VAdapterPipeline(unet=unet, text_encoder=te.half().to(dev).eval(), tokenizer=WordTokenizer())


def _gens(seed=5):
    return dict(generator=torch.Generator().manual_seed(seed), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _kw():
    cond = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    return dict(condition_image_latents=cond, num_frames=4, num_inference_steps=2, guidance_scale=2.0, output_type="latent")


def test_a_two_vector_inversion_through_the_encoder_and_the_pipeline(dev, parts):
    """fails on the parent commit, which has no `load_textual_inversion`"""
    pipe = _pipe(parts, dev)
    tok = pipe.tokenizer
    using, other = "a photo of <style> fox", "a red fox runs"
    pe_other, ne_other = pipe.encode_prompt(other, dev, 1, True, negative_prompt="blurry")
    frames_other = pipe(prompt=other, negative_prompt="blurry", **_kw(), **_gens()).frames
    table0 = pipe.text_encoder.text_model.embeddings.token_embedding.weight.clone()

    vec = (torch.randn(2, 64, generator=torch.Generator().manual_seed(9)) * 0.05).half()
    pipe.load_textual_inversion({"<style>": vec})
    assert pipe.text_encoder.config.vocab_size == 258 and pipe.text_encoder.device.type == "cuda"
    # the prompt that uses the token: the encoder's answer for the expanded ids, over the grown table
    pe, ne = pipe.encode_prompt(using, dev, 1, True, negative_prompt="<style>")
    ids = tok(["a photo of <style> <style>_1 fox", "<style> <style>_1"], padding="max_length", max_length=77, truncation=True,
              return_tensors="pt").input_ids
    assert ids[0, 4:6].tolist() == [256, 257] and ids[1, 1:3].tolist() == [256, 257]
    state = dict(parts[1])
    key = "text_model.embeddings.token_embedding.weight"
    state[key] = torch.cat([state[key], vec.float()])
    ref = ClipTextReference(state, dict(TEXT64, vocab_size=258))
    fp16_gate("textual inversion prompt_embeds", pe, ref.half()(ids[:1])[0], ref(ids[:1])[0], FACTOR, "I2V_CLIP_TEXT_LOG")
    fp16_gate("textual inversion negative_prompt_embeds", ne, ref.half()(ids[1:])[0], ref(ids[1:])[0], FACTOR, "I2V_CLIP_TEXT_LOG")
    assert torch.equal(bits(pe), bits(pipe.text_encoder(ids[:1])[0]))
    unknown = pipe.text_encoder(tok("a photo of <nope> fox", padding="max_length", max_length=77, truncation=True,
                                    return_tensors="pt").input_ids)[0]
    assert not torch.equal(pe, unknown)
    # the weighted path converts first, on the raw text: the bracket weighs both vectors (spaces: the word tokenizer, unlike CLIP's,
    # finds a token only as a word of its own)
    pw, _ = pipe.encode_weighted_prompt("a photo of ( <style> :1.2) fox", dev, 1, False)
    from tests import prompt_weight_bounds as B
    w = torch.ones(1, 77)
    w[0, 4:6] = 1.2
    assert B.check(pw.cpu(), pe.cpu(), w)[1]
    # the prompt that does not use it: the bits it had before loading, through the encoder and through the pipeline
    pe2, ne2 = pipe.encode_prompt(other, dev, 1, True, negative_prompt="blurry")
    assert torch.equal(bits(pe2), bits(pe_other)) and torch.equal(bits(ne2), bits(ne_other))
    assert torch.equal(pipe(prompt=other, negative_prompt="blurry", **_kw(), **_gens()).frames, frames_other)
    with_token = pipe(prompt=using, negative_prompt="blurry", **_kw(), **_gens()).frames
    assert torch.isfinite(with_token).all() and not torch.equal(with_token, frames_other)
    assert torch.equal(with_token, pipe(prompt_embeds=pe, negative_prompt_embeds=ne_other, **_kw(), **_gens()).frames)
    # prompt travel converts its keyframe texts too
    pt, _ = pipe.encode_prompt_travel({0: using, 3: other}, 4, dev, 1, False)
    both = pipe._encode_texts([using, other])
    assert torch.equal(bits(pt[0, 0]), bits(both[0])) and torch.equal(bits(pt[0, 3]), bits(both[1]))
    assert torch.equal(bits(both[0]), bits(pipe.text_encoder(torch.cat([ids[:1], tok(other, padding="max_length", max_length=77,
                                                                                     truncation=True, return_tensors="pt").input_ids]))[0][0]))

    # unloaded: the table's bits are back, the token is an unknown word again, the other prompt keeps its bits
    pipe.unload_textual_inversion()
    assert torch.equal(bits(pipe.text_encoder.text_model.embeddings.token_embedding.weight), bits(table0))
    assert pipe.text_encoder.config.vocab_size == 256 and len(tok) == 256
    pe3, _ = pipe.encode_prompt(using, dev, 1, False)
    assert torch.equal(bits(pe3), bits(pipe.encode_prompt("a photo of <nope> fox", dev, 1, False)[0]))
    pe4, ne4 = pipe.encode_prompt(other, dev, 1, True, negative_prompt="blurry")
    assert torch.equal(bits(pe4), bits(pe_other)) and torch.equal(bits(ne4), bits(ne_other))
    assert torch.equal(pipe(prompt=other, negative_prompt="blurry", **_kw(), **_gens()).frames, frames_other)


def test_reserved_ids_raise_after_unloading_with_a_tokenizer_that_cannot_remove(dev, parts):
    from tests.textual_inversion_reference import FixedWordTokenizer
    pipe = _pipe(parts, dev)
    pipe.tokenizer = FixedWordTokenizer()
    pipe.load_textual_inversion({"<style>": torch.zeros(2, 64)})
    pipe.encode_prompt("a <style> fox", dev, 1, False)
    pipe.unload_textual_inversion()
    with pytest.raises((ValueError, pkg().HipLibraryError)):                  # the reserved id 256 is past the table's 256 rows
        pipe.encode_prompt("a <style> fox", dev, 1, False)
    pipe.encode_prompt("a red fox", dev, 1, False)
