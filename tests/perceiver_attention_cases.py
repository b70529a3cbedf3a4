"""The cases of tests/golden/perceiver_attention_parent.json: inputs that any machine rebuilds from integers alone
(tests/clip_attention_cases.py: qkv_values -- no torch generator), the list of shapes, and the one function that runs a case through
`kernels.perceiver_attention` and returns the sha256 of the output's fp16 bytes.  tools/record_clip_attention.py --cases perceiver writes the
file with it, tests/test_perceiver_attention_parent_gpu.py compares against the file with it."""
import hashlib
import json
import os

import torch

from tests.clip_attention_cases import qkv_values

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perceiver_attention_parent.json")
GAINS = (2, 6)
HEADS, D = 2, 64
# (B, n_q, len_a, len_b): one tile and its edges, an odd tile count, a partial second query tile, all four waves, the Resampler's own
# 257 + 16, the envelope's last tile pair
SHAPES = [(1, 1, 1, 0), (2, 16, 15, 1), (1, 16, 16, 16), (2, 16, 17, 16), (1, 17, 33, 0), (1, 64, 40, 24), (2, 16, 257, 16),
          (1, 16, 272, 16)]
# "packed": q, A and B are three packed q | k | v matrices of their own (A's and B's q columns are not read)
# "strided": every operand at a column offset in a wider buffer, `out` a view of a wider poisoned buffer
# "shared": q and source B are ONE packed q | k | v buffer (the Resampler's call; needs len_b == n_q)
LAYOUTS = ("packed", "strided", "shared")


def cases():
    out = []
    for gain in GAINS:
        for B, nq, la, lb in SHAPES:
            out.append(dict(B=B, n_q=nq, len_a=la, len_b=lb, gain=gain, layout="packed"))
        out.append(dict(B=2, n_q=17, len_a=20, len_b=13, gain=gain, layout="strided"))
        out.append(dict(B=2, n_q=16, len_a=17, len_b=16, gain=gain, layout="shared"))
    for c in out:
        c["seed"] = 100000 * c["B"] + 1000 * c["len_a"] + 10 * c["len_b"] + c["n_q"]
    return out


def case_id(c):
    return f"B{c['B']}-q{c['n_q']}-a{c['len_a']}-b{c['len_b']}-gain{c['gain']}-{c['layout']}"


def _wide(t, left, right, fill, dev):
    """t at column `left` of a buffer `left + right` columns wider that holds `fill` elsewhere"""
    w = torch.full((t.shape[0], t.shape[1] + left + right), fill, dtype=torch.float16)
    w[:, left: left + t.shape[1]] = t
    return w.to(dev)


def run_case(kernels, dev, c):
    """sha256 of the entry point's output (fp16, contiguous, on the CPU)"""
    B, nq, la, lb, hidden = c["B"], c["n_q"], c["len_a"], c["len_b"], HEADS * D
    q = qkv_values(B * nq, HEADS, D, c["gain"], c["seed"])                   # the q columns carry the gain
    a = qkv_values(B * la, HEADS, D, 1, c["seed"] + 1)
    b = q if c["layout"] == "shared" else qkv_values(B * lb, HEADS, D, 1, c["seed"] + 2) if lb else None
    kw = dict(batch=B, n_q=nq, len_a=la, len_b=lb, heads=HEADS, head_dim=D)
    if c["layout"] == "strided":
        obuf = torch.full((B * nq + 2, hidden + 24), -77.0, dtype=torch.float16, device=dev)
        got = kernels.perceiver_attention(_wide(q, 8, 8, 5.0, dev), _wide(a, 16, 8, 5.0, dev), _wide(b, 24, 16, 5.0, dev), q_off=8,
                                          ka_off=16 + hidden, va_off=16 + 2 * hidden, kb_off=24 + hidden, vb_off=24 + 2 * hidden,
                                          out=obuf[: B * nq, 8: 8 + hidden], **kw)
        keep = torch.ones_like(obuf, dtype=torch.bool)
        keep[: B * nq, 8: 8 + hidden] = False
        assert bool((obuf[keep] == -77.0).all()), "the kernel wrote outside its view of out"
    else:
        qd = q.to(dev)
        bd = qd if c["layout"] == "shared" else None if b is None else b.to(dev)
        got = kernels.perceiver_attention(qd, a.to(dev), bd, ka_off=hidden, va_off=2 * hidden, **kw)
    assert got.shape == (B * nq, hidden) and got.dtype == torch.float16
    return hashlib.sha256(got.contiguous().cpu().numpy().tobytes()).hexdigest()


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
