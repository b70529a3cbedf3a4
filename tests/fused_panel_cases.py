"""The cases of tests/golden/fused_panel_parent.json: the three persistent kernels that LayerNorm a tile of rows into an LDS panel
(csrc/ln_qkv.hip, csrc/ff_fused.hip, csrc/motion_attn.hip) through `kernels.ln_qkv`, `kernels.ff_fused`, `kernels.motion_attn`,
`kernels.motion_attn_wide` and `kernels.cross_attn_fused`.  Inputs that any machine rebuilds from integers alone (`values`, the
generator of tests/clip_attention_cases.py: no torch generator), the list of cases, and the one function that runs a case and returns
the sha256 of its outputs' bytes.  tools/record_clip_attention.py --cases fused_panel writes the file with it,
tests/test_fused_panel_parent_gpu.py compares against the file with it.

Every kernel instantiation has a case of ONE tile and a case of MANY (771) tiles: above 512 tiles a workgroup of a 256-CU device
takes three (i2v_persistent_grid), so both panels are used again and the last workgroup runs short.  Every entry point has one
`strided` case of many tiles: x at a row stride of C + 64, `out` a view of a wider poisoned buffer that must keep its poison."""
import functools
import hashlib
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_panel_parent.json")
MANY = 771                    # tiles: 3 x 257, ceil(771 / 256) = 4 tiles per workgroup, the last workgroup one tile short
HEADS, EPS = 8, 1e-5
POISON = -77.0


def _unit(n, seed):
    """n float64 values, uniform with unit variance:
    u[i] = ((i * 2654435761 + seed * 40503) mod 2^32) >> 8,  x = (u / 2^23 - 1) * sqrt(3)"""
    i = np.arange(n, dtype=np.uint64)
    u = ((i * np.uint64(2654435761) + np.uint64(seed * 40503)) % np.uint64(1 << 32)) >> np.uint64(8)
    return (u.astype(np.float64) / float(1 << 23) - 1.0) * np.sqrt(3.0)


@functools.lru_cache(maxsize=6)
def _rows(n, seed):
    """n unit-variance values as fp16 (cached: the many-tile cases share their arrays of 771 x 128 x 320 values)"""
    return torch.from_numpy(_unit(n, seed).astype(np.float16))


def values(shape, seed, scale=1.0, offset=0.0):
    """fp32 tensor of `shape`: offset + scale * (unit-variance uniform values of `seed`)"""
    n = int(np.prod(shape))
    return torch.from_numpy((offset + scale * _unit(n, seed)).astype(np.float32)).view(*shape)


def cases():
    out = []
    for tiles in (1, MANY):
        for n_qk in (640, 960):
            out.append(dict(entry="ln_qkv", tiles=tiles, n_qk=n_qk, tiles_per_image=1 if tiles == 1 else 3, images=False, strided=False))
        # (the precise pair: in the rows' own order on one tile, through the permuting tail on many -- both row orders of that instantiation)
        for tail, perm, precise in ((False, False, False), (True, False, False), (True, True, False), (True, tiles != 1, True)):
            out.append(dict(entry="ff_fused", tiles=tiles, tail=tail, perm=perm, precise=precise, strided=False))
        for frames in (8, 16, 32):
            for outp in (False, True):
                out.append(dict(entry="motion_attn", tiles=tiles, frames=frames, outp=outp, strided=False))
        out.append(dict(entry="motion_attn_wide", tiles=tiles, frames=16, outp=True, strided=False))
        for outp in (False, True):
            out.append(dict(entry="cross_attn_fused", tiles=tiles, ctx_len=77, tiles_per_ctx=1 if tiles == 1 else 257, outp=outp,
                            ip_len=0, strided=False))
    # ln_qkv: 2 clips of 2 frames of 128 rows, the frame-0 rows of each clip read in place
    out.append(dict(entry="ln_qkv", tiles=2, n_qk=960, tiles_per_image=1, images=True, strided=False))
    # cross-attention: the context's lengths (one key tile, CLIP's 77 in the last tile, the envelope's end), 3 contexts of one tile
    for ctx_len in (5, 77, 80):
        for outp in (False, True):
            out.append(dict(entry="cross_attn_fused", tiles=3, ctx_len=ctx_len, tiles_per_ctx=1, outp=outp, ip_len=0, strided=False))
    out.append(dict(entry="cross_attn_fused", tiles=3, ctx_len=77, tiles_per_ctx=1, outp=False, ip_len=4, strided=False))
    out.append(dict(entry="cross_attn_fused", tiles=3, ctx_len=77, tiles_per_ctx=1, outp=True, ip_len=16, strided=False))
    # every entry point on many tiles with x at a row stride of C + 64 and `out` inside a wider poisoned buffer
    out.append(dict(entry="ln_qkv", tiles=MANY, n_qk=960, tiles_per_image=257, images=False, strided=True))
    out.append(dict(entry="ff_fused", tiles=MANY, tail=True, perm=True, precise=False, strided=True))
    out.append(dict(entry="motion_attn", tiles=MANY, frames=16, outp=True, strided=True))
    out.append(dict(entry="motion_attn_wide", tiles=MANY, frames=16, outp=True, strided=True))
    out.append(dict(entry="cross_attn_fused", tiles=MANY, ctx_len=77, tiles_per_ctx=3, outp=True, ip_len=4, strided=True))
    return out


def case_id(c):
    keys = [k for k in c if k not in ("entry", "tiles", "strided", "sha256")]
    return f"{c['entry']}-t{c['tiles']}-" + "-".join(f"{k}{int(c[k])}" for k in keys) + ("-strided" if c["strided"] else "")


def _x(c, rows, ch, dev):
    """the input rows [rows, ch] on the device; strided: a view of a buffer 64 columns wider that holds 5.0 elsewhere"""
    x = _rows(MANY * 128 * 320 if c["tiles"] == MANY else rows * ch, 7)[: rows * ch].view(rows, ch).to(dev)
    if not c["strided"]:
        return x
    wide = torch.full((rows, ch + 64), 5.0, dtype=torch.float16, device=dev)
    wide[:, :ch] = x
    return wide[:, :ch]


class _Out:
    """`out` operands: dense ones, or (strided) views at row 1, column 8 of a poisoned buffer 2 rows and 24 columns larger"""

    def __init__(self, c, dev):
        self.strided, self.dev, self.held = c["strided"], dev, []

    def __call__(self, rows, cols):
        if not self.strided:
            return torch.empty(rows, cols, dtype=torch.float16, device=self.dev)
        buf = torch.full((rows + 2, cols + 24), POISON, dtype=torch.float16, device=self.dev)
        self.held.append((buf, rows, cols))
        return buf[1: 1 + rows, 8: 8 + cols]

    def check(self):
        for buf, rows, cols in self.held:
            keep = torch.ones_like(buf, dtype=torch.bool)
            keep[1: 1 + rows, 8: 8 + cols] = False
            assert bool((buf[keep] == POISON).all()), "the kernel wrote outside its view of out"


def _ln_tables(ch, dev):
    return values((ch,), 11, 0.1, 1.0).to(dev), values((ch,), 12, 0.1).to(dev)


def _linear(n, k, seed, dev):
    return values((n, k), seed, k ** -0.5).half().to(dev)


def _ln_qkv(kernels, dev, c, mk):
    ch, rpi = 320, 128 * c["tiles_per_image"]
    gamma, beta = _ln_tables(ch, dev)
    w = kernels.pack_ln_qkv(_linear(c["n_qk"], ch, 21, dev), _linear(ch, ch, 22, dev))
    if c["images"]:
        clips, frames = c["tiles"], 2
        x = _x(c, clips * frames * rpi, ch, dev)
        qk, vt = kernels.ln_qkv(x, gamma, beta, w, n_qk=c["n_qk"], rows_per_image=rpi, eps=EPS, images=clips,
                                x_image_stride=frames * rpi * x.stride(0))
        return [qk, vt]
    rows = 128 * c["tiles"]
    qk, vt = kernels.ln_qkv(_x(c, rows, ch, dev), gamma, beta, w, n_qk=c["n_qk"], rows_per_image=rpi, eps=EPS, qk=mk(rows, c["n_qk"]))
    return [qk, vt]


def _ff_fused(kernels, dev, c, mk):
    ch, inner, rows = 320, 1280, 128 * c["tiles"]
    gamma, beta = _ln_tables(ch, dev)
    packed = kernels.pack_ff_fused(_linear(2 * inner, ch, 31, dev), values((2 * inner,), 32, 0.1).to(dev), _linear(ch, inner, 33, dev),
                                   values((ch,), 34, 0.1).to(dev))
    x = _x(c, rows, ch, dev)
    if not c["tail"]:
        return [kernels.ff_fused(x, gamma, beta, packed, eps=EPS, out=mk(rows, ch))]
    ptail = kernels.pack_ff_tail(_linear(ch, ch, 35, dev), values((ch,), 36, 0.1).to(dev))
    res2 = _rows(rows * ch, 37).view(rows, ch).to(dev)
    frames, hw = (16, 8) if c["perm"] else (0, 0)
    if c["precise"]:                 # the residual stream as an fp16 pair: res2 carries a low half, the result's is written beside it
        res2._i2v_lo = (_rows(rows * ch, 38).view(rows, ch) * 2.0 ** -12).to(dev)
        out = kernels.ff_fused(x, gamma, beta, packed, eps=EPS, tail=(ptail, res2, frames, hw), precise=True)
        assert kernels.lo_of(out) is not None
        return [out, kernels.lo_of(out)]
    return [kernels.ff_fused(x, gamma, beta, packed, eps=EPS, out=mk(rows, ch), tail=(ptail, res2, frames, hw))]


def _motion_attn(kernels, dev, c, mk):
    wide = c["entry"] == "motion_attn_wide"
    ch, d, rows = (640, 80, 64 * c["tiles"]) if wide else (320, 40, 128 * c["tiles"])
    gamma, beta = _ln_tables(ch, dev)
    g32, s32 = kernels.motion_attn_tables(gamma, beta, values((32, ch), 41, 0.5).to(dev), c["frames"])
    w = kernels.pack_motion_qkv(_linear(ch, ch, 42, dev), _linear(ch, ch, 43, dev), _linear(ch, ch, 44, dev), HEADS)
    op = kernels.pack_attn_out(_linear(ch, ch, 45, dev), values((ch,), 46, 0.1).to(dev), HEADS) if c["outp"] else None
    fn = kernels.motion_attn_wide if wide else kernels.motion_attn
    return [fn(_x(c, rows, ch, dev), g32, s32, w, heads=HEADS, head_dim=d, frames=c["frames"], eps=EPS, out_proj=op, out=mk(rows, ch))]


def _ctx_fragments(kernels, dev, n_ctx, length, ch, seed):
    k = values((n_ctx * length, ch), seed).half().to(dev)
    vt = torch.zeros(n_ctx, ch, kernels.pad8(length), dtype=torch.float16, device=dev)
    vt[:, :, :length] = values((n_ctx, ch, length), seed + 1).half().to(dev)
    return kernels.pack_ctx_fragments(k, vt, HEADS, length)


def _cross_attn_fused(kernels, dev, c, mk):
    ch, d, rows = 320, 40, 128 * c["tiles"]
    gamma, beta = _ln_tables(ch, dev)
    n_ctx = c["tiles"] // c["tiles_per_ctx"]
    kw = {}
    if c["ip_len"]:
        kw = dict(ip_frag=_ctx_fragments(kernels, dev, n_ctx, c["ip_len"], ch, 55), ip_len=c["ip_len"], ip_scale=0.7)
    if c["outp"]:
        kw["out_proj"] = kernels.pack_attn_out(_linear(ch, ch, 53, dev), values((ch,), 54, 0.1).to(dev), HEADS)
    return [kernels.cross_attn_fused(_x(c, rows, ch, dev), gamma, beta, kernels.pack_cross_q(_linear(ch, ch, 51, dev), HEADS),
                                     _ctx_fragments(kernels, dev, n_ctx, c["ctx_len"], ch, 52), heads=HEADS, head_dim=d,
                                     ctx_len=c["ctx_len"], rows_per_ctx=128 * c["tiles_per_ctx"], eps=EPS, out=mk(rows, ch), **kw)]


_RUN = {"ln_qkv": _ln_qkv, "ff_fused": _ff_fused, "motion_attn": _motion_attn, "motion_attn_wide": _motion_attn,
        "cross_attn_fused": _cross_attn_fused}


def run_case(kernels, dev, c):
    """sha256 of the entry point's outputs (fp16, contiguous, on the CPU; several outputs one after the other)"""
    mk = _Out(c, dev)
    outs = _RUN[c["entry"]](kernels, dev, c, mk)
    mk.check()
    h = hashlib.sha256()
    for t in outs:
        assert t.dtype == torch.float16 and bool(torch.isfinite(t).all())
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
