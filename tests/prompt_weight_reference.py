"""Weighted and long prompts, restated: the specification `prompt_weighting.py`, `I2VAdapterPipeline.encode_weighted_prompt` and
`i2v_weight_embeds_f16` are tested against (tests/test_prompt_weighting.py, tests/test_prompt_weighting_gpu.py).  The parser is written
character by character (the package's works on regex tokens), the chunker row by row, the weighting rule in float64.  No product code
imports it.

    parse(text)                        [(segment, weight), ...]: (x) * 1.1, [x] / 1.1, (x:1.5), nesting multiplies, backslash escapes
    token_weights(tokenizer, text)     ids and weights, every segment tokenised on its own, without bos / eos
    chunks(ids, weights, M, ...)       rows [bos] + M - 2 ids + [eos], padded with [pad]; bos / eos / pad weigh 1
    weight_ref64(x, w, restore_mean)   out = x * w * (sum x / sum w x), the sums over each prompt's tokens * dim values
"""
import re

import torch

NUMBER = re.compile(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?")


def parse(text):
    chars = []                     # [character, weight, plain]: plain = an ordinary character (not escaped, not an unmatched bracket)
    rounds, squares = [], []
    edge = 0                       # len(chars) at the last bracket that was syntax: a `:number` does not reach across it

    def scale(start, mult):
        for c in chars[start:]:
            c[1] *= mult

    def close_round(start):
        lo = max(start, edge)
        j = len(chars)
        while j > lo and chars[j - 1][2]:
            j -= 1
        run = "".join(c[0] for c in chars[j:])
        colon = run.rfind(":")
        if colon >= 0 and NUMBER.fullmatch(run[colon + 1:].strip()):
            del chars[j + colon:]
            scale(start, float(run[colon + 1:]))
        else:
            scale(start, 1.1)

    i = 0
    while i < len(text):
        ch = text[i]
        if ch == "\\" and i + 1 < len(text) and text[i + 1] in "()[]\\":
            chars.append([text[i + 1], 1.0, False])
            i += 2
            continue
        i += 1
        if ch == "(":
            rounds.append(len(chars))
        elif ch == "[":
            squares.append(len(chars))
        elif ch == ")" and rounds:
            close_round(rounds.pop())
        elif ch == "]" and squares:
            scale(squares.pop(), 1 / 1.1)
        else:
            chars.append([ch, 1.0, ch not in "()[]\\"])
            continue
        edge = len(chars)
    while rounds:
        close_round(rounds.pop())
        edge = len(chars)
    while squares:
        scale(squares.pop(), 1 / 1.1)
    out = []
    for ch, w, _ in chars:
        if out and out[-1][1] == w:
            out[-1][0] += ch
        else:
            out.append([ch, w])
    return [(s, w) for s, w in out] or [("", 1.0)]


def token_weights(tokenizer, text):
    ids, weights = [], []
    for seg, w in parse(text):
        part = list(tokenizer(seg).input_ids)[1:-1]
        ids += part
        weights += [w] * len(part)
    return ids, weights


def chunk_count(n_ids, max_length):
    return max(1, (n_ids + max_length - 3) // (max_length - 2))


def chunks(ids, weights, max_length, bos, eos, pad, n_chunks):
    """(id rows, weight rows), n_chunks of each; ids beyond n_chunks * (max_length - 2) must have been dropped by the caller"""
    body = max_length - 2
    assert len(ids) == len(weights) <= n_chunks * body
    id_rows, w_rows = [], []
    for c in range(n_chunks):
        row, wrow = [bos], [1.0]
        for k in range(c * body, min(len(ids), (c + 1) * body)):
            row.append(ids[k])
            wrow.append(weights[k])
        row.append(eos)
        wrow.append(1.0)
        while len(row) < max_length:
            row.append(pad)
            wrow.append(1.0)
        id_rows.append(row)
        w_rows.append(wrow)
    return id_rows, w_rows


def prompt_rows(tokenizer, texts, max_multiples, bos, eos, pad):
    """(ids [P, n, M], weights [P, n * M], n) of the texts of one call: truncated to max_multiples chunks, all padded to the chunk
    count of the longest"""
    m = tokenizer.model_max_length
    pairs = []
    for t in texts:
        ids, w = token_weights(tokenizer, t)
        keep = max_multiples * (m - 2)
        pairs.append((ids[:keep], w[:keep]))
    n = max(chunk_count(len(ids), m) for ids, _ in pairs)
    rows = [chunks(ids, w, m, bos, eos, pad, n) for ids, w in pairs]
    return (torch.tensor([r[0] for r in rows], dtype=torch.int64),
            torch.tensor([[x for row in r[1] for x in row] for r in rows], dtype=torch.float64), n)


def weight_ref64(x, w, restore_mean=True):
    """x [P, T, D] (any dtype; taken as float64), w [P, T] -> (out float64 [P, T, D], ratio float64 [P])"""
    x, w = x.double(), w.double()
    y = x * w[:, :, None]
    ratio = x.sum((1, 2)) / y.sum((1, 2)) if restore_mean else torch.ones(x.shape[0], dtype=torch.float64)
    return y * ratio[:, None, None], ratio
