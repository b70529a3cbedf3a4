"""Host-side reference of the flash-attention backward (csrc/attention_bwd.hip: i2v_attention_bwd_f16, i2v_attention_lse_f32), the
case tables of tests/test_attention_bwd_edges_gpu.py and a helper that asks the library which kernels a case takes
(i2v_attention_bwd_route: the launch choices live in the library alone).  No GPU import and nothing of the package at import time:
the CPU suite (tests/test_attention_bwd_reference.py) checks the reference against autograd, the tables against the coverage they
are meant to give, and the asserted bound against an emulation of the kernels' roundings on exactly the inputs the GPU tests use.

    P = softmax(s Q K^T)   dP = dO V^T   delta = rowsum(dO o O)   dS = P o (dP - delta)
    dQ = s dS K            dK = s sum_group dS^T Q                dV = sum_group P^T dO
"""
import collections
import ctypes as C
import functools

import torch

LOG2E = 1.4426950408889634

Ref = collections.namedtuple("Ref", "dq dk dv o lse2")     # [bq, lq, C], [bkv, lk, C] x 2, [bq, lq, C], [bq, heads, lq] (log2)

# ---------------------------------------------------------------------------------------------- case tables
# (d, lq, lk, group, need_dkv): heads = 2, bkv = 2, bq = bkv * group.  What each row is there for (the forms as route_id() below names them):
RAGGED = [
    (8, 70, 77, 1, True),       # class <= 32 (KS 1, DT 2), one-tile forms, attn_lse_kernel<1>; lq, lk not multiples of 8
    (16, 45, 515, 1, True),     # dkv2 (lk >= 512, lq < 64) with lq % 8 != 0: the zero-filled pad of Q^T / dO^T
    (24, 603, 40, 1, True),     # dq2 (lq >= 512, lk < 64), partial d, lq % 8 != 0, wholly masked second tile of the last wave
    (32, 40, 601, 2, True),     # dkv2 with 2 partitions, lk % 8 != 0
    (32, 600, 601, 1, True),    # dq2_lds, dkv2_lds64, attn_lse_lds_kernel<1>
    (48, 100, 523, 1, True),    # dkv2_lds32; lq, lk not multiples of 8
    (56, 517, 600, 1, True),    # lq not a multiple of 8 in the LDS forms
    (72, 130, 77, 2, True),     # class <= 80 partial d; partitions + ragged lk in dkv1
    (88, 96, 643, 4, True),     # class <= 96; dkv2_lds32 with 4 partitions and a ragged lk
    (96, 600, 600, 1, True),    # class <= 96 in every two-tile form, attn_lse_lds_kernel<3>
    (104, 70, 130, 1, True),    # class <= 128 partial d, attn_lse_kernel<4>
    (128, 517, 523, 2, True),   # class <= 128 at long lengths: one-tile forms, large grid, 2 partitions
    (136, 33, 65, 1, True),     # class <= 160 partial d
    (160, 600, 520, 1, True),   # class <= 160 long
    (40, 601, 77, 2, False),    # the text cross-attention through dq2_lds
    (40, 520, 4, 2, False),     # the IP-Adapter tokens through dq2
    (40, 260, 1000, 8, True),   # dkv2_lds64, 8 partitions, ragged lk
    # every two-tile form in every class that has it (and the one-tile forms of classes (2, 4), (3, 6) beside them), at the smallest
    # ragged lengths that reach the form: lq / lk just above 512, and below 64 | just above 64 | just above 128 on the other side
    (24, 67, 517, 1, True),     # class (1, 2): dkv2_lds32
    (40, 45, 517, 1, True),     # class (2, 3): dkv2
    (64, 517, 45, 1, True),     # class (2, 4): dq2, dkv1
    (56, 45, 517, 1, True),     # class (2, 4): dq1, dkv2
    (64, 67, 517, 1, True),     # class (2, 4): dkv2_lds32
    (80, 517, 45, 1, True),     # class (3, 5): dq2
    (72, 517, 67, 1, True),     # class (3, 5): dq2_lds, attn_lse_lds_kernel<3> with partial d
    (80, 45, 517, 1, True),     # class (3, 5): dkv2
    (72, 67, 517, 1, True),     # class (3, 5): dkv2_lds32
    (80, 131, 517, 1, True),    # class (3, 5): dkv2_lds64
    (96, 517, 45, 1, True),     # class (3, 6): dq2, dkv1
    (88, 45, 517, 1, True),     # class (3, 6): dkv2
]
RAGGED_HEADS, RAGGED_BKV = 2, 2

# (heads, d, frames): a motion module's backward, lq = lk = frames, group 1, batch = SHORT_PIXELS
SHORT = ([(8, 40, f) for f in (2, 3, 5, 8, 12, 16, 24, 32)] +
         [(hh, d, f) for hh, d in ((8, 80), (2, 160), (4, 16)) for f in (3, 16, 24)])
SHORT_PIXELS = 256
ONE_FRAME = (8, 40, 1)                                        # P = 1: dV = dO, dQ = dK = 0

STRIDED = [(48, 100, 523, 1, True), (24, 603, 40, 1, True), (56, 517, 600, 1, True)]      # one per dq_form; rows of RAGGED
SCALED = [(40, 256, 256, 1, True), (40, 260, 1000, 8, True)]
SCALE_EXPONENTS = (-6, 6)                                     # dO * 2^e: the range a loss scale moves it through
ENV_CASES = [(40, 600, 601, 1, True), (96, 517, 523, 2, True)]
ENV_SWITCHES = [("I2V_ATTN_BWD_LDS", "0"), ("I2V_ATTN_BWD_QB", "32")]


def case_id(case):
    return "-".join(str(int(x)) for x in case)


# ---------------------------------------------------------------------------------------------- inputs
def make_inputs(d, lq, lk, group, heads=RAGGED_HEADS, bkv=RAGGED_BKV, do_exp=0):
    """(q [bq, lq, C], k, v [bkv, lk, C], dO [bq, lq, C]) in fp16: unit normal q, k, v, dO = 0.5 normal * 2^do_exp, seeded from
    the case.  The draws do not depend on do_exp."""
    bq, C = bkv * group, heads * d
    g = torch.Generator().manual_seed(((d * 2003 + lq) * 2003 + lk) * 64 + group * 8 + heads)
    q = torch.randn(bq, lq, C, generator=g).half()
    k = torch.randn(bkv, lk, C, generator=g).half()
    v = torch.randn(bkv, lk, C, generator=g).half()
    do = (torch.randn(bq, lq, C, generator=g) * (0.5 * 2.0 ** do_exp)).half()
    return q, k, v, do


def _split(t, heads):
    b, l, c = t.shape
    return t.view(b, l, heads, c // heads).transpose(1, 2)      # [b, heads, l, d]


def _merge(t):
    b, hh, l, d = t.shape
    return t.transpose(1, 2).reshape(b, l, hh * d)


# ---------------------------------------------------------------------------------------------- float64 reference
def reference(q, k, v, do, heads, group):
    """dQ, dK, dV, O and the log2-sum-exp in float64 from the formulas above (no autograd); the operands are taken as they are
    (fp16-rounded values) and converted to float64."""
    q, k, v, do = (_split(t.double(), heads) for t in (q, k, v, do))
    bq, _, lq, d = q.shape
    bkv, lk = k.shape[0], k.shape[2]
    assert bq == bkv * group
    s = d ** -0.5
    kk, vv = k.repeat_interleave(group, dim=0), v.repeat_interleave(group, dim=0)
    logits = s * (q @ kk.transpose(-1, -2))
    lse = torch.logsumexp(logits, dim=-1, keepdim=True)
    p = torch.exp(logits - lse)
    o = p @ vv
    dp = do @ vv.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq = s * (ds @ kk)
    dk = s * (ds.transpose(-1, -2) @ q).view(bkv, group, heads, lk, d).sum(1)
    dv = (p.transpose(-1, -2) @ do).view(bkv, group, heads, lk, d).sum(1)
    return Ref(_merge(dq), _merge(dk), _merge(dv), _merge(o), lse.squeeze(-1) * LOG2E)


# ---------------------------------------------------------------------------------------------- the kernels' roundings
def _r16(t):
    return t.half().float()


def emulate(q, k, v, do, heads, group):
    """The same formulas with the kernels' documented roundings: fp16 operands, fp32 sums, O rounded to fp16 before delta, P and
    dS rounded to fp16 before their second product (P from the fp32 log2-sum-exp), fp16 results.  What a correct kernel gives on
    these inputs up to the order of its fp32 sums."""
    q, k, v, do = (_split(t.float(), heads) for t in (q, k, v, do))
    bq, _, lq, d = q.shape
    bkv, lk = k.shape[0], k.shape[2]
    s = d ** -0.5
    c = s * LOG2E
    kk, vv = k.repeat_interleave(group, dim=0), v.repeat_interleave(group, dim=0)
    sc = c * (q @ kk.transpose(-1, -2))
    m = sc.max(-1, keepdim=True).values
    lse2 = m + torch.log2(torch.exp2(sc - m).sum(-1, keepdim=True))
    p = torch.exp2(sc - lse2)
    o = _r16(p @ vv)
    dp = do @ vv.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    ds16 = _r16(p * (dp - delta))
    p16 = _r16(p)
    dq = _r16(s * (ds16 @ kk))
    dk = _r16(s * (ds16.transpose(-1, -2) @ q).view(bkv, group, heads, lk, d).sum(1))
    dv = _r16((p16.transpose(-1, -2) @ do).view(bkv, group, heads, lk, d).sum(1))
    return Ref(_merge(dq), _merge(dk), _merge(dv), _merge(o), lse2.squeeze(-1))


@functools.lru_cache(maxsize=None)
def case_data(d, lq, lk, group, heads=RAGGED_HEADS, bkv=RAGGED_BKV, do_exp=0):
    """((q, k, v, dO) fp16, float64 reference) of one case, computed once per process and shared: treat it as read-only."""
    inp = make_inputs(d, lq, lk, group, heads, bkv, do_exp)
    return inp, reference(*inp, heads, group)


def short_case(heads, d, frames):
    """the (d, lq, lk, group, heads, bkv) arguments of case_data for a short-sequence case"""
    return (d, frames, frames, 1, heads, SHORT_PIXELS)


# ---------------------------------------------------------------------------------------------- the library's route
DQ_FORMS = ("dq1", "dq2", "dq2_lds")                          # I2V_ATTN_BWD_DQ* of include/i2v_hip.h, by value
DKV_FORMS = ("dkv1", "dkv2", "dkv2_lds32", "dkv2_lds64")      # I2V_ATTN_BWD_DKV*
LSE_FORMS = ("lse", "lse_lds")                                # I2V_ATTN_LSE*
KIND_DQ, KIND_DKV, KIND_LSE = 0, 1, 2                         # I2V_ATTN_BWD_KIND_*


def ask_route(lib, d, lq, lk, group, bkv=RAGGED_BKV, need_dkv=True, heads=RAGGED_HEADS):
    """i2v_attention_bwd_route for a case, as a dict of the fields of i2v_attn_bwd_route.  lib: the package's _lib module (this
    module imports nothing of the package itself).  Host arithmetic only: no GPU."""
    r = lib.AttnBwdRoute()
    rc = lib.load().i2v_attention_bwd_route(bkv * group, group, heads, d, lq, lk, int(need_dkv), C.byref(r))
    assert rc == 0, lib.load().i2v_last_error()
    return r.as_dict()


def route_forms(route):
    """(ks, dt, dq_form, dkv_form, lse_form) of a route with the forms by name; dkv_form None without the dK / dV sweep, lse_form
    None before the first log-sum-exp launch (a last route)"""
    name = lambda names, v: names[v] if v >= 0 else None
    return (route["ks"], route["dt"], name(DQ_FORMS, route["dq_form"]), name(DKV_FORMS, route["dkv_form"]),
            name(LSE_FORMS, route["lse_form"]))


def route_id(route):
    """dq2_lds/dkv2_lds64/lse_lds"""
    return "/".join(str(f) for f in route_forms(route)[2:])


if __name__ == "__main__":
    # the routes the library answers for ENV_CASES under this process's environment, as JSON [[ks, dt, dq, dkv, lse], ...]: the
    # switches are read once per process, so tests/test_attention_bwd_reference.py asks each in a child that carries it.  No GPU.
    import json
    import os
    import sys
    if sys.argv[1:] != ["--routes"]:
        sys.exit("usage: python tests/attn_bwd_reference.py --routes")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import i2v_adapter_unofficial_amd as pkg
    print(json.dumps([route_forms(ask_route(pkg._lib, *c[:4])) for c in ENV_CASES]))
