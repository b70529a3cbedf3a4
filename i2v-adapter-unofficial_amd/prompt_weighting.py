"""Weighted and long prompts on the host: the emphasis syntax SD-1.5 front ends share, and the chunking that carries a prompt past the
text encoder's 77 positions (`I2VAdapterPipeline.enable_prompt_weighting` / `encode_weighted_prompt`).

    parse_prompt_attention("a (red:1.3) [fox]") -> [("a ", 1.0), ("red", 1.3), (" ", 1.0), ("fox", 1 / 1.1)]
    token_weights(tokenizer, text)             -> (ids, weights): every segment tokenised on its own, each id with its segment's weight
    chunk(ids, weights, M, bos, eos, pad, n)   -> n rows of M ids / weights: [bos] + M - 2 ids + [eos], the tail [pad]; bos / eos / pad
                                                  weigh 1

The text encoder then sees every chunk as a prompt of its own ([P * n, M] ids in, [P, n * M, D] out, chunks in prompt-major order), and
ONE launch of `i2v_weight_embeds_f16` multiplies every token's embedding by its weight and restores each prompt's mean.  Pure Python:
nothing here touches the GPU.  Not implemented: `BREAK`, prompt editing / alternation (`[a:b:0.5]`, `[a|b]`), dropping the inner
bos / eos of middle chunks, Compel's `.and()` / `.blend()`."""
import logging
import re

logger = logging.getLogger(__name__)

ROUND, SQUARE = 1.1, 1 / 1.1
_TOKEN = re.compile(r"\\[()\[\]\\]|[()\[\]]|[^\\()\[\]]+|\\")
_NUMBER = re.compile(r"\s*[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?\s*\Z")


def parse_prompt_attention(text):
    """[(segment, weight), ...] of a prompt: `(x)` weighs x by 1.1, `[x]` by 1 / 1.1, `(x:1.5)` by 1.5 -- the number is a float literal
    after the LAST `:` of the text directly in front of the `)` --, brackets nest multiplicatively, `\\(` `\\)` `\\[` `\\]` `\\\\` are
    literal characters, an unclosed bracket closes at the end of the text (innermost first, round ones before square ones), a closing
    bracket without an open one is a literal.  Empty segments are dropped and neighbours of equal weight merged, so a text without the
    syntax is ONE segment of weight 1.0 (it is tokenised as a whole); the empty text is [("", 1.0)]."""
    if not isinstance(text, str):
        raise TypeError(f"a prompt is a str, got {type(text).__name__}")
    res, rounds, squares = [], [], []
    plain = False                      # the token in front is plain text: a `)` may find its `:number` there

    def close_round(start):
        mult = ROUND
        if plain and len(res) > start:
            seg = res[-1][0]
            colon = seg.rfind(":")
            if colon >= 0 and _NUMBER.match(seg[colon + 1:]):
                mult = float(seg[colon + 1:])
                res[-1][0] = seg[:colon]
        for r in res[start:]:
            r[1] *= mult

    for m in _TOKEN.finditer(text):
        tok = m.group(0)
        if tok == "(":
            rounds.append(len(res))
        elif tok == "[":
            squares.append(len(res))
        elif tok == ")" and rounds:
            close_round(rounds.pop())
        elif tok == "]" and squares:
            for r in res[squares.pop():]:
                r[1] *= SQUARE
        else:
            res.append([tok[1:] if len(tok) == 2 and tok[0] == "\\" else tok, 1.0])
            plain = tok[0] not in "\\()[]"
            continue
        plain = False
    while rounds:
        close_round(rounds.pop())
        plain = False
    while squares:
        for r in res[squares.pop():]:
            r[1] *= SQUARE
    out = []
    for seg, w in res:
        if not seg:
            continue
        if out and out[-1][1] == w:
            out[-1][0] += seg
        else:
            out.append([seg, w])
    return [(s, w) for s, w in out] or [("", 1.0)]


def _ids_of(tokenizer, text):
    """`tokenizer(text).input_ids[1:-1]`: the ids of a text without its bos / eos (a tokenizer that answers with a [1, L] batch is taken
    by its row)"""
    ids = tokenizer(text).input_ids
    if hasattr(ids, "tolist"):
        ids = ids.tolist()
    if ids and isinstance(ids[0], (list, tuple)):
        ids = ids[0]
    return [int(i) for i in ids[1:-1]]


def special_ids(tokenizer):
    """(bos, eos, pad) as the tokenizer itself lays a row out: the first three ids of the empty prompt padded to `model_max_length`"""
    m = tokenizer.model_max_length
    if m < 3:
        raise ValueError(f"tokenizer.model_max_length {m}: a chunk needs bos, eos and at least one token")
    row = tokenizer("", padding="max_length", max_length=m, truncation=True).input_ids
    if hasattr(row, "tolist"):
        row = row.tolist()
    if isinstance(row[0], (list, tuple)):
        row = row[0]
    return int(row[0]), int(row[1]), int(row[2])


def token_weights(tokenizer, text):
    """(ids, weights) of a prompt, without bos / eos: each segment of `parse_prompt_attention` tokenised on its own"""
    ids, weights = [], []
    for seg, w in parse_prompt_attention(text):
        part = _ids_of(tokenizer, seg)
        ids += part
        weights += [float(w)] * len(part)
    return ids, weights


def chunks_needed(n_ids, max_length):
    """how many chunks of `max_length - 2` ids a prompt of n_ids needs; the empty prompt is one chunk"""
    return max(1, -(-n_ids // (max_length - 2)))


def truncate(tokenizer, ids, weights, max_length, max_embeddings_multiples):
    """the ids `max_embeddings_multiples` chunks hold; what is beyond them is dropped with encode_prompt's warning"""
    keep = max_embeddings_multiples * (max_length - 2)
    if len(ids) > keep:
        removed = tokenizer.batch_decode([ids[keep:]])
        logger.warning("The following part of your input was truncated because prompt weighting is enabled with "
                       f"max_embeddings_multiples={max_embeddings_multiples} ({keep} tokens of CLIP's {max_length} - 2 per chunk): "
                       f"{removed}")
        ids, weights = ids[:keep], weights[:keep]
    return ids, weights


def chunk(ids, weights, max_length, bos, eos, pad, n_chunks):
    """(n_chunks rows of max_length ids, the same of weights): row i = [bos] + ids[i (M - 2): (i + 1)(M - 2)] + [eos] + [pad] * rest --
    the tokenizer's own layout under padding="max_length" --; rows past the prompt's last are [bos, eos, pad, ...]; bos, eos and pad
    weigh 1.0"""
    body = max_length - 2
    if len(ids) != len(weights):
        raise ValueError(f"{len(ids)} ids with {len(weights)} weights")
    if len(ids) > n_chunks * body:
        raise ValueError(f"{len(ids)} ids do not fit {n_chunks} chunks of {body}")
    id_rows, w_rows = [], []
    for i in range(n_chunks):
        part, wpart = ids[i * body: (i + 1) * body], weights[i * body: (i + 1) * body]
        rest = body - len(part)
        id_rows.append([bos] + list(part) + [eos] + [pad] * rest)
        w_rows.append([1.0] + list(wpart) + [1.0] * (1 + rest))
    return id_rows, w_rows


def check_settings(max_embeddings_multiples, restore_mean):
    if isinstance(max_embeddings_multiples, bool) or not isinstance(max_embeddings_multiples, int) or max_embeddings_multiples < 1:
        raise ValueError(f"`max_embeddings_multiples` must be an int >= 1, got {max_embeddings_multiples!r}")
    if not isinstance(restore_mean, bool):
        raise ValueError(f"`restore_mean` must be a bool, got {restore_mean!r}")


def max_context_tokens(k_row_stride=1280):
    """The longest context the cross-attention path takes, from its own argument checks: `i2v_attention_f16` addresses one
    (batch, head) slice of K with 32-bit byte offsets, (lk + 128) * k_row_stride * 2 < 2^30; `project_context` and the ControlNet's
    context projection are GEMMs over the context's rows and have no bound of their own below it.  At SD-1.5's widest K rows (1280
    values) that is 419 302 tokens -- 5445 chunks of 77."""
    return ((1 << 30) - 1) // (2 * k_row_stride) - 128
