"""The cases of tests/golden/clip_attention_parent.json: inputs that any machine rebuilds from integers alone (no torch generator), the
list of shapes, and the one function that runs a case through `kernels.clip_attention` / `kernels.clip_vision_attention` and returns
the sha256 of the output's fp16 bytes.  tools/record_clip_attention.py writes the file with it, tests/test_clip_attention_parent_gpu.py
compares against the file with it."""
import hashlib
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_attention_parent.json")
GAINS = (2, 6)
# causal, d = 64, (B, L, heads): one tile and its edges, an odd tile count, the 64-query block boundary, the prompt's 77, the envelope's end
CAUSAL = [(1, 1, 1), (2, 15, 2), (1, 16, 1), (2, 17, 2), (1, 33, 2), (1, 64, 1), (1, 65, 1), (2, 77, 2), (1, 128, 2)]
# bidirectional, d = 64 and 80, (B, L), 2 heads
BIDIRECTIONAL = [(1, 1), (2, 17), (1, 33), (1, 65), (2, 257), (1, 288)]


def qkv_values(rows, heads, d, gain, seed):
    """fp16 [rows, 3 * heads * d], uniform with unit variance, the q columns times `gain`:
    u[i] = ((i * 2654435761 + seed * 40503) mod 2^32) >> 8,  x = (u / 2^23 - 1) * sqrt(3) in float64"""
    hidden = heads * d
    i = np.arange(rows * 3 * hidden, dtype=np.uint64)
    u = ((i * np.uint64(2654435761) + np.uint64(seed * 40503)) % np.uint64(1 << 32)) >> np.uint64(8)
    x = ((u.astype(np.float64) / float(1 << 23) - 1.0) * np.sqrt(3.0)).reshape(rows, 3 * hidden)
    x[:, :hidden] *= gain
    return torch.from_numpy(x.astype(np.float16))


def cases():
    out = []
    for gain in GAINS:
        for B, L, heads in CAUSAL:
            out.append(dict(entry="clip_attention", B=B, L=L, heads=heads, d=64, gain=gain, strided=False))
        out.append(dict(entry="clip_attention", B=2, L=17, heads=2, d=64, gain=gain, strided=True))
        for d in (64, 80):
            for B, L in BIDIRECTIONAL:
                out.append(dict(entry="clip_vision_attention", B=B, L=L, heads=2, d=d, gain=gain, strided=False))
        out.append(dict(entry="clip_vision_attention", B=2, L=17, heads=2, d=80, gain=gain, strided=True))
    for c in out:
        c["seed"] = 1000 * c["L"] + 10 * c["d"] + c["B"] + c["heads"]
    return out


def case_id(c):
    return f"{c['entry']}-B{c['B']}-L{c['L']}-h{c['heads']}-d{c['d']}-gain{c['gain']}" + ("-strided" if c["strided"] else "")


def run_case(kernels, dev, c):
    """sha256 of the entry point's output (fp16, contiguous, on the CPU).  strided: qkv sits at column 8 of a buffer 16 columns wider
    (offsets 8, 8 + hidden, 8 + 2 hidden), `out` is the left part of a buffer 24 columns wider."""
    rows, hidden = c["B"] * c["L"], c["heads"] * c["d"]
    qkv = qkv_values(rows, c["heads"], c["d"], c["gain"], c["seed"]).to(dev)
    fn = getattr(kernels, c["entry"])
    kw = dict(batch=c["B"], length=c["L"], heads=c["heads"], head_dim=c["d"])
    if c["strided"]:
        wide = torch.zeros(rows, 3 * hidden + 16, dtype=torch.float16, device=dev)
        wide[:, 8: 8 + 3 * hidden] = qkv
        obuf = torch.full((rows, hidden + 24), -77.0, dtype=torch.float16, device=dev)
        got = fn(wide, q_off=8, k_off=8 + hidden, v_off=8 + 2 * hidden, out=obuf[:, :hidden], **kw)
        assert bool((obuf[:, hidden:] == -77.0).all())
    else:
        got = fn(qkv, **kw)
    assert got.shape == (rows, hidden) and got.dtype == torch.float16
    return hashlib.sha256(got.contiguous().cpu().numpy().tobytes()).hexdigest()


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
