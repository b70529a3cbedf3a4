"""Weighted and long prompts on the host: the parser against a table and against the character-by-character restatement
(tests/prompt_weight_reference.py), the chunker at its edges, truncation and its warning, equal chunk counts over a call's texts, the
settings' validation, the driver's flags, the ABI of i2v_weight_embeds_f16 with its host-side argument checks -- and the error bound
the GPU test holds the kernel to (tests/prompt_weight_bounds.py), shown here to pass a faithful fp32 evaluation and to reject five
wrong ones.  No kernel is launched."""
import logging
import os
import re

import pytest
import torch

from tests import prompt_weight_bounds as B
from tests import prompt_weight_reference as R
from tests.parity import ROOT, SMALL_UNET
from tests.textual_inversion_reference import WordTokenizer

f16 = torch.float16
SMALL = dict(vocab_size=256, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1,
             max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=255)


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def PW():
    from i2v_adapter_unofficial_amd import prompt_weighting
    return prompt_weighting


# ---------------------------------------------------------------------------------------------------------- the parser
X = 1.1
TABLE = [
    ("", [("", 1.0)]),
    ("a red fox", [("a red fox", 1.0)]),
    ("a (red) fox", [("a ", 1.0), ("red", X), (" fox", 1.0)]),
    ("a [red] fox", [("a ", 1.0), ("red", 1 / X), (" fox", 1.0)]),
    ("a (red:1.5) fox", [("a ", 1.0), ("red", 1.5), (" fox", 1.0)]),
    ("(a:.5)(b:2.)(c:1e0)(d: +0.25 )", [("a", 0.5), ("b", 2.0), ("c", 1.0), ("d", 0.25)]),
    ("(a:-1)", [("a", -1.0)]),
    ("((a))", [("a", X * X)]),
    ("([a])", [("a", 1 / X * X)]),
    ("(a (b:2) c:1.5)", [("a ", 1.5), ("b", 3.0), (" c", 1.5)]),
    ("(a [b] c)", [("a ", X), ("b", 1 / X * X), (" c", X)]),
    (r"\(a\) \[b\] \\", [("(a) [b] \\", 1.0)]),
    (r"(a \(b\):2)", [("a (b)", 2.0)]),                      # the `:2` directly in front of the `)` is plain text: it counts
    (r"(a\):2)", [("a)", 2.0)]),
    ("a (red fox", [("a ", 1.0), ("red fox", X)]),           # unclosed: closes at the end
    ("a (red:1.3", [("a ", 1.0), ("red", 1.3)]),
    ("a [red (fox", [("a ", 1.0), ("red ", 1 / X), ("fox", X / X)]),
    ("a) red] fox", [("a) red] fox", 1.0)]),                  # unmatched closing brackets are literals
    ("(a)) b", [("a", X), (") b", 1.0)]),
    ("(a)(b)", [("ab", X)]),                                  # equal neighbours merge
    ("(a:1.0) b", [("a b", 1.0)]),
    ("(a:b)", [("a:b", X)]),                                  # no number behind the colon
    ("(a:1.5:)", [("a:1.5:", X)]),
    ("(:2)", [("", 1.0)]),
    ("()", [("", 1.0)]),
    ("time 12:30 (x)", [("time 12:30 ", 1.0), ("x", X)]),
    ("a\\b (c)", [("a\\b ", 1.0), ("c", X)]),
]


@pytest.mark.parametrize("text,want", TABLE)
def test_parser_table(text, want):
    for fn in (PW().parse_prompt_attention, R.parse):
        got = fn(text)
        assert [s for s, _ in got] == [s for s, _ in want], (fn.__module__, got)
        assert [w for _, w in got] == pytest.approx([w for _, w in want], rel=1e-12), (fn.__module__, got)


def test_parser_agrees_with_the_restatement_on_generated_texts():
    g = torch.Generator().manual_seed(0)
    alphabet = ["a", "b ", " c", "(", ")", "[", "]", ":", "1.5", ":2", "\\", "\\(", "\\]", " "]
    for _ in range(3000):
        n = int(torch.randint(1, 12, (1,), generator=g))
        text = "".join(alphabet[int(i)] for i in torch.randint(0, len(alphabet), (n,), generator=g))
        assert PW().parse_prompt_attention(text) == R.parse(text), repr(text)
    with pytest.raises(TypeError):
        PW().parse_prompt_attention(["a"])


def test_a_text_without_syntax_is_tokenised_as_a_whole():
    tok = WordTokenizer()
    ids, w = PW().token_weights(tok, "a red fox runs")
    assert ids == tok("a red fox runs").input_ids[1:-1] and w == [1.0] * 4
    assert [c[0] for c in tok.calls[:1]] == [("a red fox runs",)]
    ids, w = PW().token_weights(tok, "a (red:1.5) [fox] runs")
    assert ids == tok("a red fox runs").input_ids[1:-1] and w == pytest.approx([1.0, 1.5, 1 / 1.1, 1.0])
    assert PW().token_weights(tok, "") == ([], []) == R.token_weights(tok, "")
    # a tokenizer that answers a str with a [1, L] batch (tests/clip_text_reference.StubTokenizer) is taken by its row
    from tests.clip_text_reference import StubTokenizer
    assert PW().token_weights(StubTokenizer(77, 256), "(ab:2)c") == ([97, 98, 99], [2.0, 2.0, 1.0])
    assert PW().special_ids(StubTokenizer(77, 256)) == (254, 255, 255) and PW().special_ids(tok) == (tok.bos_id, tok.eos_id, tok.pad_id)


# ---------------------------------------------------------------------------------------------------------- chunks
@pytest.mark.parametrize("n_ids,want_chunks", [(0, 1), (1, 1), (75, 1), (76, 2), (150, 2), (151, 3), (225, 3)])
def test_chunk_layout_at_the_edges(n_ids, want_chunks):
    tok = WordTokenizer()
    m = tok.model_max_length
    ids = [i % 200 for i in range(n_ids)]
    weights = [1.0 + 0.01 * i for i in range(n_ids)]
    assert PW().chunks_needed(n_ids, m) == R.chunk_count(n_ids, m) == want_chunks
    for n in (want_chunks, want_chunks + 1):
        rows, wrows = PW().chunk(ids, weights, m, tok.bos_id, tok.eos_id, tok.pad_id, n)
        assert (rows, wrows) == R.chunks(ids, weights, m, tok.bos_id, tok.eos_id, tok.pad_id, n)
        assert len(rows) == len(wrows) == n and all(len(r) == m for r in rows + wrows)
        assert [i for r in rows for i in r[1:-1] if i < 200] == ids or n_ids % 75 == 0       # (a full chunk's eos is its last id)
        for r, wr in zip(rows, wrows):
            assert r[0] == tok.bos_id and wr[0] == 1.0
            k = r.index(tok.eos_id)
            assert all(i == tok.pad_id for i in r[k + 1:]) and all(x == 1.0 for x in wr[k:])
        assert rows[-1] == [tok.bos_id, tok.eos_id] + [tok.pad_id] * (m - 2) or n == want_chunks
    with pytest.raises(ValueError, match="do not fit"):
        PW().chunk([1] * 76, [1.0] * 76, m, 0, 1, 2, 1)


def test_short_unweighted_ids_are_the_tokenizers_own_row():
    tok = WordTokenizer()
    for prompt in ("", "a red fox", " ".join(f"w{i}" for i in range(75))):
        ids, w = PW().token_weights(tok, prompt)
        rows, wrows = PW().chunk(ids, w, 77, *PW().special_ids(tok), 1)
        assert rows[0] == tok(prompt, padding="max_length", truncation=True).input_ids and wrows[0] == [1.0] * 77


def test_truncation_warns_with_the_removed_text(caplog):
    tok = WordTokenizer()
    words = [f"w{i}" for i in range(160)]
    ids, w = PW().token_weights(tok, " ".join(words))
    with caplog.at_level(logging.WARNING):
        kept, kw = PW().truncate(tok, ids, w, 77, 2)
    assert kept == ids[:150] and len(kw) == 150
    assert "truncated" in caplog.text and " ".join(words[150:]) in caplog.text and "w149" not in caplog.text
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        assert PW().truncate(tok, ids, w, 77, 3) == (ids, w)
    assert caplog.text == ""


def test_reference_pads_every_text_of_a_call_to_one_chunk_count():
    tok = WordTokenizer()
    long_ = " ".join(f"w{i}" for i in range(80))
    ids, weights, n = R.prompt_rows(tok, ["a (red:1.5) fox", long_, ""], 3, tok.bos_id, tok.eos_id, tok.pad_id)
    assert n == 2 and ids.shape == (3, 2, 77) and weights.shape == (3, 154)
    assert ids[0, 1].tolist() == ids[2, 0].tolist() == [tok.bos_id, tok.eos_id] + [tok.pad_id] * 75
    assert weights[0, :5].tolist() == [1.0, 1.0, 1.5, 1.0, 1.0]
    _, _, n1 = R.prompt_rows(tok, ["a (red:1.5) fox", long_, ""], 1, tok.bos_id, tok.eos_id, tok.pad_id)
    assert n1 == 1


# ---------------------------------------------------------------------------------------------------------- the pipeline's settings
def _cpu_pipe(text=True):
    P = pkg()
    with torch.device("meta"):
        unet = P.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    te = P.CLIPTextModel(**SMALL) if text else None
    return P.I2VAdapterPipeline(unet=unet, text_encoder=te, tokenizer=WordTokenizer() if text else None)


def test_enable_prompt_weighting_validates_its_arguments():
    pipe = _cpu_pipe()
    assert pipe.prompt_weighting_enabled is False
    for bad in (0, -1, 1.5, "3", True, None):
        with pytest.raises(ValueError, match="max_embeddings_multiples"):
            pipe.enable_prompt_weighting(max_embeddings_multiples=bad)
    with pytest.raises(ValueError, match="restore_mean"):
        pipe.enable_prompt_weighting(restore_mean=1)
    assert pipe.prompt_weighting_enabled is False
    pipe.enable_prompt_weighting()
    assert pipe.prompt_weighting_enabled and pipe._prompt_weighting == dict(max_embeddings_multiples=3, restore_mean=True)
    pipe.enable_prompt_weighting(1, restore_mean=False)
    assert pipe._prompt_weighting == dict(max_embeddings_multiples=1, restore_mean=False)
    # the longest context the cross-attention takes, from i2v_attention_f16's own check: (lk + 128) * k_row_stride * 2 < 2^30
    limit = PW().max_context_tokens(1280)
    assert (limit + 128) * 1280 * 2 < 2 ** 30 <= (limit + 1 + 128) * 1280 * 2 and limit == 419302
    widest = max(SMALL_UNET["block_out_channels"])
    over = PW().max_context_tokens(widest) // 77 + 1
    with pytest.raises(ValueError, match="exceeds"):
        pipe.enable_prompt_weighting(over)
    assert pipe._prompt_weighting == dict(max_embeddings_multiples=1, restore_mean=False)
    pipe.enable_prompt_weighting(over - 1)
    pipe.disable_prompt_weighting()
    assert pipe.prompt_weighting_enabled is False
    with pytest.raises(ValueError, match="text_encoder"):
        _cpu_pipe(text=False).encode_weighted_prompt("a", "cpu", 1, False)
    with pytest.raises(ValueError, match="`prompt` has to be"):
        pipe.encode_weighted_prompt(None, "cpu", 1, False)
    with pytest.raises(ValueError, match="batch size"):
        pipe.encode_weighted_prompt(["a", "b"], "cpu", 1, True, negative_prompt=["c"])
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        pipe.encode_weighted_prompt("a (red:1.2) fox", "cpu", 1, False)          # everything up to the encoder ran on the host


def test_call_signature_is_unchanged():
    import inspect
    params = inspect.signature(pkg().I2VAdapterPipeline.__call__).parameters
    assert "prompt_weighting" not in params and params["clip_skip"].default is None


# ---------------------------------------------------------------------------------------------------------- the driver
def test_driver_flags_and_their_conflicts(capsys, caplog):
    drv = pkg().pipeline_i2v_adapter
    parser = drv.build_parser()
    a = parser.parse_args(["--task_name", "t"])
    assert a.prompt_weighting is None and a.textual_inversion == []
    a = parser.parse_args(["--task_name", "t", "--prompt_weighting", "--textual_inversion", "neg.pt", "--textual_inversion", "s.bin:<s>"])
    assert a.prompt_weighting == 3 and a.textual_inversion == ["neg.pt", "s.bin:<s>"]
    a = parser.parse_args(["--task_name", "t", "--prompt_weighting", "2", "--prompt_travel_column", "travel"])
    assert a.prompt_weighting == 2 and a.prompt_travel_column == "travel"
    for flags, name in ((["--prompt_weighting"], "--prompt_weighting"), (["--textual_inversion", "x.pt"], "--textual_inversion")):
        caplog.clear()
        with caplog.at_level(logging.ERROR):
            assert drv.main(["--task_name", "t", "--embeds", "e.safetensors"] + flags) == -1
        assert name in caplog.text and "--embeds" in caplog.text
    caplog.clear()
    with caplog.at_level(logging.ERROR):
        assert drv.main(["--task_name", "t", "--prompt_weighting", "0"]) == -1
    assert "at least 1" in caplog.text
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------------------- ABI
def test_abi_27_declares_exports_and_binds_weight_embeds():
    lib = pkg()._lib
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 27
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    name = "i2v_weight_embeds_f16"
    assert re.search(rf"\bint {name}\(", src) and name in lib.SIGNATURES and hasattr(h, name)
    assert len(lib.SIGNATURES[name][1]) == 11
    assert callable(pkg().kernels.weight_embeds)
    comment = src[:src.index(f"int {name}(")].rsplit("/*", 1)[1]
    assert comment.lstrip().startswith("(ABI 27)") and comment.rstrip().endswith("*/")


def test_the_handles_tables_are_untouched():
    from i2v_adapter_unofficial_amd import handle as H
    name = "i2v_weight_embeds_f16"
    assert name not in H.ENTRY_IDS and name not in H.LATER_ENTRY_IDS and name not in H.ENTRY_NAMES.values()
    assert H.ENTRY_IDS["i2v_dpm_cfg_step"] == len(H.ENTRY_IDS) - 1 == 20 and sorted(H.ENTRY_NAMES) == list(range(22))
    hip = open(os.path.join(ROOT, "i2v-adapter-unofficial_amd", "csrc", "handle.hip")).read()
    assert "weight_embeds" not in hip


def test_weight_embeds_bad_arguments_are_refused_on_the_host():
    """I2V_ERR_INVALID_ARG before anything is launched: callable without a GPU (the pointers are never dereferenced)"""
    h = pkg()._lib.load()
    S, W, O, RT = 1 << 40, 1 << 41, 1 << 42, 1 << 43
    ok = dict(src=S, weights=W, out=O, ratio=RT, n=2, tokens=154, dim=768, ld_src=768, ld_out=776, restore=1)
    span = 2 * ((2 * 154 - 1) * 768 + 768)
    for kw, msg in ((dict(src=None), b"null"), (dict(weights=None), b"null"), (dict(out=None), b"null"), (dict(n=0), b"n_prompts 0"),
                    (dict(tokens=0), b"tokens 0"), (dict(dim=0), b"multiple of 8"), (dict(dim=764, ld_src=768), b"multiple of 8"),
                    (dict(ld_src=760), b"row strides"), (dict(ld_out=772), b"row strides"), (dict(ld_out=760), b"row strides"),
                    (dict(src=S + 8), b"16-byte"), (dict(out=O + 2), b"16-byte"), (dict(weights=W + 2), b"4-byte"),
                    (dict(ratio=RT + 1), b"4-byte"), (dict(tokens=1 << 22), b"too large"), (dict(ld_src=1 << 24), b"too large"),
                    (dict(out=S), b"overlaps src"),                                     # in place needs equal strides
                    (dict(out=S + 16, ld_out=768), b"overlaps src"), (dict(out=S + span - 16), b"overlaps src"),
                    (dict(weights=O + 64), b"overlaps weights"), (dict(ratio=O + 64), b"overlaps weights")):
        args = tuple({**ok, **kw}.values())
        assert h.i2v_weight_embeds_f16(*args, None) == -1, kw
        assert msg in h.i2v_last_error(), (kw, h.i2v_last_error())


def test_weight_embeds_wrapper_refuses_host_tensors():
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        pkg().kernels.weight_embeds(torch.zeros(1, 2, 8, dtype=f16), torch.ones(1, 2))


# ---------------------------------------------------------------------------------------------------------- the bound
CASES, case_inputs = B.CASES, B.case_inputs


def fp32_eval(x, w, restore_mean=True, how="right"):
    """the kernel's arithmetic in fp32 torch (the sums in torch's own order) -- and five ways of getting it slightly wrong"""
    xf = x.float()
    if how == "shifted":
        w = torch.roll(w, 1, dims=1)
    if how == "bos":
        w = w.clone()
        w[:, 0] = 1.1
    y = xf * w[:, :, None]
    if restore_mean:
        if how == "dim_only":
            r = (xf.sum(2) / y.sum(2))[:, :, None]
        else:
            r = (xf.sum((1, 2)) / y.sum((1, 2)))[:, None, None]
        if how == "inverted":
            r = 1 / r
    else:
        r = torch.ones(1, 1, 1)
    if how == "early_round":
        y = y.half().float()
    return (y * r).half()


@pytest.mark.parametrize("p,t,d", CASES)
def test_bound_passes_a_faithful_evaluation_and_rejects_wrong_ones(p, t, d):
    x, w = case_inputs(p, t, d)
    worst, ok = B.check(fp32_eval(x, w), x, w)
    assert ok and worst <= 1.0, worst
    assert B.check(fp32_eval(x, w, restore_mean=False), x, w, restore_mean=False)[1]
    rejected = {}
    for how in ("inverted", "dim_only", "shifted", "bos", "early_round"):
        worst, ok = B.check(fp32_eval(x, w, how=how), x, w)
        rejected[how] = not ok
    # a wrong way that IS the rule in a case cannot be told apart there: with one token the mean over dim is the mean, the shifted
    # weight is the weight and ANY single weight cancels against the restored mean; and rounding early moves a result by at most one
    # fp16 ulp, which shows among thousands of elements
    expect = {"inverted": True, "bos": t > 1, "dim_only": t > 1, "shifted": t > 1, "early_round": p * t * d >= 800}
    for how, want in expect.items():
        assert rejected[how] or not want, (how, rejected)
    assert sum(rejected.values()) >= (5 if t > 1 and p * t * d >= 800 else 1)


def test_bound_widens_for_an_ill_conditioned_mean_and_is_infinite_when_the_weights_cancel():
    x, w = case_inputs(1, 77, 768, offset=0.02)
    well = B.ratio_error(*case_inputs(1, 77, 768))
    ill = B.ratio_error(x, w)
    assert torch.isfinite(ill).all() and float(ill) > 5 * float(well)
    assert B.check(fp32_eval(x, w), x, w)[1]
    x = torch.ones(1, 2, 8).half()
    assert torch.isinf(B.ratio_error(x, torch.tensor([[1.0, -1.0]])))
    assert B.sum_depth(231, 768) == 8 * 22 + 6 + 16 and B.sum_depth(1, 8) == 8 + 6 + 16
