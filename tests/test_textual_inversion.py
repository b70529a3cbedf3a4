"""Textual inversion on the host: every source and format (written into tmp_path), lists, the token override, every ValueError with the
pipeline left as it was, `maybe_convert_prompt`, `CLIPTextModel.resize_token_embeddings`, the save / load round trip of a resized model,
unloading -- against tests/textual_inversion_reference.py -- and the same with transformers' CLIPTokenizer built from a tiny vocabulary.
No kernel is launched (the token table is a parameter on the host)."""
import json
import os

import pytest
import torch

from tests import textual_inversion_reference as R
from tests.parity import SMALL_UNET
from tests.textual_inversion_reference import FixedWordTokenizer, WordTokenizer

SMALL = dict(vocab_size=256, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1,
             max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=255)
D = SMALL["hidden_size"]


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _pipe(tokenizer=None, text=True):
    P = pkg()
    with torch.device("meta"):
        unet = P.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    te = P.CLIPTextModel(**SMALL).half() if text else None
    return P.I2VAdapterPipeline(unet=unet, text_encoder=te, tokenizer=(tokenizer or WordTokenizer()) if text else None)


def _table(pipe):
    return pipe.text_encoder.text_model.embeddings.token_embedding.weight


def _vec(n, seed):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------- sources and formats
@pytest.mark.parametrize("fmt", ["dict_1d", "dict_2d", "a1111_dict", "safetensors", "bin", "pt_a1111", "dir_weight_name", "subfolder"])
def test_every_source_and_format(tmp_path, fmt):
    from safetensors.torch import save_file
    pipe = _pipe()
    base = _table(pipe).clone()
    vec = torch.randn(3, D, generator=torch.Generator().manual_seed(1))
    kw, n = {}, 3
    if fmt == "dict_1d":
        src, n = {"<tok>": vec[0]}, 1
    elif fmt == "dict_2d":
        src = {"<tok>": vec}
    elif fmt == "a1111_dict":
        src = {"string_to_param": {"*": vec}, "name": "<tok>"}
    elif fmt == "safetensors":
        src = str(tmp_path / "tok.safetensors")
        save_file({"<tok>": vec}, src)
    elif fmt == "bin":
        src = str(tmp_path / "learned_embeds.bin")
        torch.save({"<tok>": vec}, src)
    elif fmt == "pt_a1111":
        src = str(tmp_path / "tok.pt")
        torch.save({"string_to_param": {"*": vec}, "name": "<tok>", "step": 100}, src)
    elif fmt == "dir_weight_name":
        torch.save({"<tok>": vec}, str(tmp_path / "w.bin"))
        src, kw = str(tmp_path), dict(weight_name="w.bin")
    else:
        os.makedirs(tmp_path / "sub")
        save_file({"<tok>": vec}, str(tmp_path / "sub" / "w.safetensors"))
        src, kw = str(tmp_path), dict(weight_name="w.safetensors", subfolder="sub")
    pipe.load_textual_inversion(src, **kw)
    tok = pipe.tokenizer
    assert len(tok) == 256 + n == pipe.text_encoder.config.vocab_size == _table(pipe).shape[0]
    assert tok.convert_tokens_to_ids(R.names("<tok>", n)) == list(range(256, 256 + n))
    want = R.expected_table(base, [vec[:n].half()])
    assert _table(pipe).dtype == torch.float16 and torch.equal(_bits(_table(pipe)), _bits(want))
    if fmt == "dir_weight_name":
        with pytest.raises(ValueError, match="weight_name"):
            _pipe().load_textual_inversion(str(tmp_path))
        with pytest.raises(EnvironmentError, match="not found"):
            _pipe().load_textual_inversion(str(tmp_path), weight_name="missing.bin")


def test_lists_of_sources_and_the_token_override(tmp_path):
    pipe = _pipe()
    base = _table(pipe).clone()
    a, b, c = _vec(2, 1), _vec(1, 2), _vec(3, 3)
    torch.save({"<file>": b}, str(tmp_path / "b.pt"))
    pipe.load_textual_inversion([{"<a>": a}, str(tmp_path / "b.pt"), {"string_to_param": {"*": c}, "name": "<c>"}],
                                token=["<a>", "<b>", "<cc>"])
    tok = pipe.tokenizer
    assert [r["token"] for r in pipe._textual_inversions] == ["<a>", "<b>", "<cc>"]
    assert tok.convert_tokens_to_ids(["<a>", "<a>_1", "<b>", "<cc>", "<cc>_1", "<cc>_2"]) == list(range(256, 262))
    assert tok.convert_tokens_to_ids("<file>") == tok.unk_id == tok.convert_tokens_to_ids("<c>")        # overridden names are not added
    assert torch.equal(_bits(_table(pipe)), _bits(R.expected_table(base, [a.half(), b.half(), c.half()])))
    # a second load appends; one token for one source overrides
    pipe.load_textual_inversion({"<x>": a[0]}, token="<y>")
    assert tok.convert_tokens_to_ids("<y>") == 262 and tok.convert_tokens_to_ids("<x>") == tok.unk_id
    # several keys: `token` names one
    pipe.load_textual_inversion({"<p>": a, "<q>": b}, token="<q>")
    assert torch.equal(_table(pipe)[263], b[0].half()) and len(tok) == 264


# ---------------------------------------------------------------------------------------------------------- errors
def test_every_value_error_leaves_the_pipeline_unmodified(tmp_path):
    pipe = _pipe()
    pipe.load_textual_inversion({"<a>": _vec(2, 1)})
    before, n_tok, n_rec = _table(pipe).clone(), len(pipe.tokenizer), len(pipe._textual_inversions)
    good = {"<new>": _vec(2, 5)}
    cases = [
        (dict(src={"<b>": torch.zeros(2, 32)}), r"dimension 32.*hidden size is 64"),
        (dict(src={"<a>": _vec(1, 2)}), "'<a>' is already in the tokenizer"),
        (dict(src={"fox": _vec(1, 2)}), "'fox' is already in the tokenizer"),                     # a word of the vocabulary
        (dict(src={"<z>": _vec(1, 2)}, token="<a>_1"), "already in the tokenizer"),
        (dict(src={"<a>_1": _vec(1, 2)}), "already in the tokenizer"),
        (dict(src=[good, {"<z>": _vec(3, 2)}], token=["<z>_2", "<z>"]), r"'<z>_2' \(multi-vector name of '<z>': 3 vectors\)"),
        (dict(src={"<p>": _vec(1, 1), "<q>": _vec(1, 2)}), "2 keys"),
        (dict(src={"<p>": _vec(1, 1), "<q>": _vec(1, 2)}, token="<r>"), "none of them"),
        (dict(src=[good, {"<b>": torch.zeros(3)}]), "dimension 3"),                               # the second of a list fails: the
        (dict(src=[good, good]), "'<new>' is already"),                                           # first is not loaded either
        (dict(src=[good, good], token="<t>"), "list of 2 tokens"),
        (dict(src=[good], token=["<s>", "<t>"]), "one length"),
        (dict(src={"<e>": torch.zeros(2, 3, 64)}), r"\[D\] or \[n, D\]"),
        (dict(src={"string_to_param": {}, "name": "<e>"}), "string_to_param"),
        (dict(src=7), "a path, a directory"),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            pipe.load_textual_inversion(kw["src"], token=kw.get("token"))
        assert torch.equal(_bits(_table(pipe)), _bits(before)) and len(pipe.tokenizer) == n_tok, kw
        assert len(pipe._textual_inversions) == n_rec and pipe.text_encoder.config.vocab_size == before.shape[0]
        assert pipe.tokenizer.convert_tokens_to_ids("<new>") == pipe.tokenizer.unk_id
    for kw in (dict(text=False),):
        with pytest.raises(ValueError, match="`text_encoder` and a `tokenizer`"):
            _pipe(**kw).load_textual_inversion(good)
    half = _pipe()
    half.tokenizer = None
    with pytest.raises(ValueError, match="`text_encoder` and a `tokenizer`"):
        half.load_textual_inversion(good)
    assert half.text_encoder.config.vocab_size == 256
    small = _pipe(WordTokenizer(77, 200))                     # ids 200.. would fall on rows the table already uses
    with pytest.raises(ValueError, match="200 tokens.*256 rows"):
        small.load_textual_inversion(good)


# ---------------------------------------------------------------------------------------------------------- conversion
def test_maybe_convert_prompt():
    pipe = _pipe()
    tok = pipe.tokenizer
    p = "a photo of <cat> on the beach"
    assert pipe.maybe_convert_prompt(p, tok) is p                                               # nothing loaded: the prompt itself
    lst = [p, "night"]
    assert pipe.maybe_convert_prompt(lst, tok) is lst
    pipe.load_textual_inversion([{"<cat>": _vec(3, 1)}, {"<one>": _vec(1, 2)}, {"<cat>x": _vec(2, 3)}])
    loaded = {"<cat>": 3, "<one>": 1, "<cat>x": 2}
    for prompt in (p, "<cat> <cat> and <one>", "<one> night", "night", "", "<cat>x <cat>", "a <cat>_1 alone"):
        got = pipe.maybe_convert_prompt(prompt, tok)
        assert tok.tokenize(got) == tok.tokenize(R.convert(prompt, loaded, tok)), prompt
    assert pipe.maybe_convert_prompt(p, tok) == "a photo of <cat> <cat>_1 <cat>_2 on the beach"
    assert pipe.maybe_convert_prompt("<one> night", tok) == "<one> night"
    assert pipe.maybe_convert_prompt([p, "night"], tok) == [R.convert(p, loaded, tok), "night"]
    ids = tok(pipe.maybe_convert_prompt("<cat> runs", tok)).input_ids
    assert ids == [tok.bos_id, 256, 257, 258, tok.vocab["runs"], tok.eos_id]


# ---------------------------------------------------------------------------------------------------------- the token table
def test_resize_token_embeddings_keeps_the_old_rows_and_drops_the_pack():
    m = pkg().CLIPTextModel(**SMALL).half()
    old = m.text_model.embeddings.token_embedding.weight.clone()
    m._packed, m._packed_key = {"stale": True}, ("key",)
    emb = m.resize_token_embeddings(260)
    assert emb is m.text_model.embeddings.token_embedding and emb.weight.shape == (260, 64) and emb.weight.dtype == torch.float16
    assert m.config.vocab_size == 260 and m._packed is None and m._packed_key is None
    assert torch.equal(_bits(emb.weight[:256]), _bits(old)) and not emb.weight[256:].any()
    assert "text_model.embeddings.token_embedding.weight" in m.state_dict()
    m.resize_token_embeddings(256)
    assert torch.equal(_bits(m.text_model.embeddings.token_embedding.weight), _bits(old)) and m.config.vocab_size == 256
    same = m.text_model.embeddings.token_embedding
    assert m.resize_token_embeddings(256) is same
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="new_num_tokens"):
            m.resize_token_embeddings(bad)


def test_save_and_from_pretrained_round_trip_of_a_resized_model(tmp_path):
    pipe = _pipe()
    pipe.load_textual_inversion({"<a>": _vec(2, 1)})
    d = str(tmp_path / "text_encoder")
    pipe.text_encoder.save_pretrained(d)
    assert json.load(open(os.path.join(d, "config.json")))["vocab_size"] == 258
    back = pkg().CLIPTextModel.from_pretrained(d)
    assert dict(back.config) == dict(pipe.text_encoder.config) and back.config.vocab_size == 258
    for k, v in pipe.text_encoder.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k


# ---------------------------------------------------------------------------------------------------------- unloading
@pytest.mark.parametrize("removable", [True, False])
def test_unload_restores_the_bits(removable):
    pipe = _pipe(WordTokenizer() if removable else FixedWordTokenizer())
    tok = pipe.tokenizer
    pipe.unload_textual_inversion()                                                             # nothing loaded: nothing happens
    base = _table(pipe).clone()
    a, b, c = _vec(2, 1), _vec(1, 2), _vec(2, 3)
    pipe.load_textual_inversion([{"<a>": a}, {"<b>": b}, {"<c>": c}])
    assert _table(pipe).shape[0] == 261
    with pytest.raises(ValueError, match="'<nope>'"):
        pipe.unload_textual_inversion(["<nope>"])
    pipe.unload_textual_inversion(tokens=["<b>"])
    assert [r["token"] for r in pipe._textual_inversions] == ["<a>", "<c>"]
    assert pipe.maybe_convert_prompt("<a> <c>", tok) == "<a> <a>_1 <c> <c>_1"
    for name, vec in (("<a>", a), ("<c>", c)):                                                  # the kept ones still find their rows
        ids = tok.convert_tokens_to_ids(R.names(name, 2))
        assert torch.equal(_table(pipe)[ids], vec.half())
    if removable:
        assert len(tok) == 260 == _table(pipe).shape[0] and tok.convert_tokens_to_ids("<b>") == tok.unk_id
    else:
        assert len(tok) == 261 == _table(pipe).shape[0] and tok.convert_tokens_to_ids("<b>") == 258      # reserved
    assert torch.equal(_bits(_table(pipe)[:256]), _bits(base))
    pipe.unload_textual_inversion()
    assert pipe._textual_inversions == [] and pipe.text_encoder.config.vocab_size == 256
    assert torch.equal(_bits(_table(pipe)), _bits(base))
    assert pipe.maybe_convert_prompt("<a> <c>", tok) == "<a> <c>"
    if removable:
        assert len(tok) == 256 and tok("<a>").input_ids[1] == tok.unk_id
        pipe.load_textual_inversion({"<a>": a})                                                 # and again
        assert tok.convert_tokens_to_ids("<a>") == 256
    else:
        assert len(tok) == 261 and tok("<a>").input_ids[1] == 256                               # past the table: encoding it raises
        with pytest.raises(ValueError, match="already in the tokenizer"):
            pipe.load_textual_inversion({"<a>": a})


# ---------------------------------------------------------------------------------------------------------- transformers' tokenizer
def test_with_transformers_clip_tokenizer(tmp_path):
    """CLIPTokenizer builds offline from a vocab.json + merges.txt written here (character tokens and their end-of-word forms, no
    merges), so the load / convert / unload case runs with it too.  It cannot remove tokens: the ids stay reserved."""
    transformers = pytest.importorskip("transformers")
    chars = "abcdefghijklmnopqrstuvwxyz<>_0123456789"
    vocab = {}
    for c in chars:
        vocab[c] = len(vocab)
        vocab[c + "</w>"] = len(vocab)
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    json.dump(vocab, open(tmp_path / "vocab.json", "w"))
    open(tmp_path / "merges.txt", "w").write("#version: 0.2\n")
    tok = transformers.CLIPTokenizer(str(tmp_path / "vocab.json"), str(tmp_path / "merges.txt"), model_max_length=77)
    n0 = len(tok)
    P = pkg()
    with torch.device("meta"):
        unet = P.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    pipe = P.I2VAdapterPipeline(unet=unet, text_encoder=P.CLIPTextModel(**dict(SMALL, vocab_size=n0)).half(), tokenizer=tok)
    base = _table(pipe).clone()
    assert pipe.maybe_convert_prompt("a <cat> b", tok) == "a <cat> b"
    vec = _vec(2, 4)
    pipe.load_textual_inversion({"<cat>": vec})
    assert len(tok) == n0 + 2 == _table(pipe).shape[0] and tok.convert_tokens_to_ids(["<cat>", "<cat>_1"]) == [n0, n0 + 1]
    assert torch.equal(_table(pipe)[n0:], vec.half()) and torch.equal(_bits(_table(pipe)[:n0]), _bits(base))
    conv = pipe.maybe_convert_prompt("a <cat> b", tok)
    assert conv == "a <cat> <cat>_1 b"
    ids = tok(conv, padding="max_length", max_length=77, truncation=True).input_ids
    assert ids[:6] == [vocab["<|startoftext|>"], vocab["a</w>"], n0, n0 + 1, vocab["b</w>"], vocab["<|endoftext|>"]]
    with pytest.raises(ValueError, match="already in the tokenizer"):
        pipe.load_textual_inversion({"<cat>": vec})
    pipe.unload_textual_inversion()
    assert torch.equal(_bits(_table(pipe)), _bits(base)) and pipe.text_encoder.config.vocab_size == n0
    assert len(tok) == n0 + 2 and pipe.maybe_convert_prompt("a <cat> b", tok) == "a <cat> b"
