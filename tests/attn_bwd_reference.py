"""Host-side reference of the flash-attention backward (csrc/backward.hip: i2v_attention_bwd_f16, i2v_attention_lse_f32), the case
tables of tests/test_attention_bwd_edges_gpu.py and a mirror of the kernels' launch choices.  No GPU import: the CPU suite
(tests/test_attention_bwd_reference.py) checks the reference against autograd, the tables against the coverage they are meant to
give, and the asserted bound against an emulation of the kernels' roundings on exactly the inputs the GPU tests use.

    P = softmax(s Q K^T)   dP = dO V^T   delta = rowsum(dO o O)   dS = P o (dP - delta)
    dQ = s dS K            dK = s sum_group dS^T Q                dV = sum_group P^T dO
"""
import collections
import functools

import torch

LOG2E = 1.4426950408889634

Ref = collections.namedtuple("Ref", "dq dk dv o lse2")     # [bq, lq, C], [bkv, lk, C] x 2, [bq, lq, C], [bq, heads, lq] (log2)

# ---------------------------------------------------------------------------------------------- case tables
# (d, lq, lk, group, need_dkv): heads = 2, bkv = 2, bq = bkv * group.  What each row is there for (forms() below names the kernels):
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


# ---------------------------------------------------------------------------------------------- launch mirror
def dkv_partitions(batch_q, kv_group, heads, head_dim, lq, lk):
    """kernels.dkv_partitions without its environment switch, so that this module stays free of the package
    (tests/test_attention_bwd_reference.py checks that the two agree on every case)."""
    if kv_group < 2 or lq < 32:
        return 1
    two_k = lk >= 512 and head_dim <= 96
    blocks = ((lk + 127) // 128 if two_k else (lk + 63) // 64) * heads * (batch_q // kv_group)
    parts = 1
    while parts * 2 <= min(kv_group, 8) and kv_group % (parts * 2) == 0 and blocks * parts < 1024:
        parts *= 2
    return parts


CLASSES = [(32, 1, 2), (48, 2, 3), (64, 2, 4), (80, 3, 5), (96, 3, 6), (128, 4, 8), (160, 5, 10)]     # (max d, KS, DT)


def forms(d, lq, lk, lds=True, qb64=True):
    """(ks, dt, dq_form, dkv_form, lse_form): the template class and kernel forms launch_bwd / i2v_attention_lse_f32 of
    csrc/backward.hip choose for (head_dim, lq, lk).  lds=False: I2V_ATTN_BWD_LDS=0; qb64=False: I2V_ATTN_BWD_QB=32."""
    if d <= 0 or d % 8 != 0 or d > 160:
        raise ValueError(f"head_dim {d}: a multiple of 8, <= 160")
    ks, dt = next((ks, dt) for dmax, ks, dt in CLASSES if d <= dmax)
    two_q, two_k = lq >= 512 and dt <= 6, lk >= 512 and dt <= 6
    if two_q and lds and lk >= 64:
        dq_form = "dq2_lds"
    else:
        dq_form = "dq2" if two_q else "dq1"
    if two_k and lds and lq >= 128 and qb64:
        dkv_form = "dkv2_lds64"
    elif two_k and lds and lq >= 64:
        dkv_form = "dkv2_lds32"
    else:
        dkv_form = "dkv2" if two_k else "dkv1"
    lse_form = "lse_lds" if lds and lq >= 512 and lk >= 64 and (d + 31) // 32 <= 3 else "lse"
    return ks, dt, dq_form, dkv_form, lse_form
