"""Reference, inputs and error bound of the temporal-attention route tests (tests/test_tattn_routes.py, tests/test_tattn_routes_gpu.py;
tests/test_kernels_gpu.py uses the bound as well).

Reference: softmax attention per (pixel, head) over the `frames` keys in fp64 on the CPU from the fp16-rounded inputs,
ref = sum_k p_k v_k, and beside it W = sum_k p_k |v_k| (what the rounding of the weights scales with).

Bound, per element (query row i, channel c of head h), derived and not tuned, with the factor 2 of tests/gemm_bounds.py on every term:

    |got - ref| <= 2^-10 |ref| + (2^-10 + 4 ln2 delta_i + F 2^-22 + SOFTMAX_ERR) W + F 2^-24 max_k |v_k| + 2^-24
    delta_i = max_k ( scale log2e d 2^-23 sum_d |q_id| |k_kd|  +  2^-22 |t_ik| ),      t_ik = scale log2e q_i . k_k  (log2 units)

The kernels (csrc/temporal_attention.hip, both forms alike) compute
    s_ik = q_i . k_k            fp16 x fp16 products are exact in fp32; the MFMA sums d of them (the padding to DQK adds zeros) in
                                fp32: |error| <= d 2^-24 sum_d |q||k|
    t_ik = s_ik * scale_log2    scale_log2 = fl(fl(scale) * fl(log2 e)) carries three roundings, the product a fourth:
                                4 * 2^-24 |t| = 2^-22 |t|
    x_ik = t_ik - max_k t_ik    the maximum is one number for the whole row, so ITS error is a common shift and cancels in the
                                softmax; the subtraction rounds by 2^-24 |x_ik| <= 2^-24 (|t_ik| + max_k |t_ik|)
    e_ik = exp2(x_ik), l_i = sum_k e_ik, p_ik = fp16(e_ik * (1 / l_i))
    o_ic = fp16( sum_k p_ik v_kc )      one 32-key MFMA, fp32 accumulation
 - a logit error of at most delta' (log2 units) on every key of a row changes each weight by the relative 2 ln2 delta' (ln2 delta'
   in the numerator and in the sum).  delta' = max_k (scale log2e d 2^-24 sum|q||k| + 2^-22 |t_ik| + 2^-24 (|t_ik| + max|t|)); the
   term of the bound, 4 ln2 delta_i with the doubled accumulation term, is 2 ln2 max_k (2 scale log2e d 2^-24 sum|q||k| + 2^-21 |t_ik|)
   and 2^-21 max_k|t_ik| >= (2^-22 + 2^-23) max_k|t_ik|: it holds the subtraction's rounding, too.
 - the hardware exp2 and the reciprocal: SOFTMAX_ERR (relative, measured: below).
 - l_i is an fp32 sum of <= F positive terms (F 2^-24 relative), the scaling e * (1 / l) rounds once more, the PV product is an fp32
   sum of F terms (F 2^-24 W): together below 2 F 2^-24 W + 2^-24 W, doubled F 2^-22 W (+ 2^-23 W, which the fp16 terms dwarf).
 - P is rounded to fp16: 2^-11 relative in the normal range (doubled: 2^-10 W); a weight below 2^-14 errs by at most 2^-25 absolute,
   F of them by F 2^-25 max_k|v_k| (doubled: F 2^-24 max|v|).
 - the result is rounded to fp16: 2^-11 |ref| (doubled: 2^-10), 2^-25 absolute below the normal range (doubled: 2^-24, the bound's
   last term).
 - masked keys (frames .. 31) carry weight exp2(-inf) = 0 and their V^T entries are replaced by 0 before the product: a NaN in the
   V^T tail must not reach the result.
It holds for any kernel that evaluates these steps in fp32 with P and the result rounded to fp16, whatever its key order.

Inputs, from a generator seeded by the case's name; every V^T tail (frames .. vt_ld) holds NaN.
  unit   standard normal q, k, v
  large  q and k times 5: |logit| (natural units) reaches 60 and more on some rows (asserted)
  spike  unit, and one key per pixel times 128: on the rows where q . k of that key is positive its logit exceeds every other logit
         of the row by more than 140 in log2 units (asserted in fp64): a row maximum taken over fewer than all 32 key slots lets
         exp2 overflow there, and is invisible below that gap since P is normalised in fp32 before it is rounded.  The spiked key
         cycles with the pixel over keys 1, 12, 22, 31 (one per lane group, as far as frames reach), frames - 1 and, frames = 9, key 8.
"""
import functools
import math
import zlib

import torch

from tests.tattn_route_cases import CASES, CLASSES, layout

U10, U22, U23, U24 = 2.0 ** -10, 2.0 ** -22, 2.0 ** -23, 2.0 ** -24
LOG2E, LN2 = 1.0 / math.log(2.0), math.log(2.0)
# Relative error of the hardware exp2 and reciprocal in a softmax weight: cannot be derived from here.  Measured as `softmax_excess`
# below: the largest excess over the bound with SOFTMAX_ERR = 0, per unit of W, over the table's cases; SOFTMAX_ERR = twice that, or 0
# when nothing exceeds.
# Measured 2026-10-19 on an MI355X with the parent commit's library (the one before the route queries; its routes are the table's, the
# two chunk-overflow cases apart, which were left out): largest excess 0.0 over the 50 cases of the default environment that write a
# tensor of their own (34 LDS-form, 5 one-tile and 11 two-tile register-form cases, all three input families): no element exceeds,
# SOFTMAX_ERR = 0.
SOFTMAX_ERR = 0.0
LARGE_AMP, SPIKE_AMP, SPIKE_GAP, LARGE_LOGIT = 5.0, 128.0, 140.0, 60.0
POISON = 0x7E37          # an fp16 NaN with a payload: what the output buffers hold outside the view


# ------------------------------------------------------------------------------------------------------------------- inputs
def spike_keys(frames):
    """the keys that take the spike, cycled over the pixels"""
    keys = [k for k in (1, 12, 22, 31) if k < frames] + [frames - 1] + ([8] if frames == 9 else [])
    return sorted(set(keys))


def inputs(c):
    """q, k, v of a case as fp16 CPU tensors [n_pixels, frames, C]"""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    n, F, Cc = c["n_pixels"], c["frames"], c["heads"] * c["head_dim"]
    q, k, v = (torch.randn((n, F, Cc), generator=g, dtype=torch.float64) for _ in range(3))
    if c["inputs"] == "large":
        q, k = q * LARGE_AMP, k * LARGE_AMP
    elif c["inputs"] == "spike":
        keys = spike_keys(F)
        assert n >= len(keys), "a spike case needs a pixel per spiked key"
        for pix in range(n):
            k[pix, keys[pix % len(keys)]] *= SPIKE_AMP
    t = dict(q=q.half(), k=k.half(), v=v.half())
    logits = _logits(t["q"].double(), t["k"].double(), c["heads"], c["head_dim"] ** -0.5 * LOG2E)          # log2 units
    if c["inputs"] == "large":
        assert float(logits.abs().max()) * LN2 >= LARGE_LOGIT, c["name"]
    elif c["inputs"] == "spike":
        top2 = logits.topk(min(2, F), dim=-1).values
        gap = top2[..., 0] - top2[..., 1]                                   # [n, heads, F]
        keys = spike_keys(F)
        for j, key in enumerate(keys):                                      # every spiked key wins some row by more than the gap
            rows = (gap[j::len(keys)] > SPIKE_GAP) & (logits[j::len(keys)].argmax(dim=-1) == key)
            assert bool(rows.any()), (c["name"], key)
    return t


# ------------------------------------------------------------------------------------------------------------------- the operation
def _heads(x, heads):
    n, F, Cc = x.shape
    return x.view(n, F, heads, Cc // heads).permute(0, 2, 1, 3)             # [n, heads, F, d]


def _logits(q, k, heads, c):
    return c * (_heads(q, heads) @ _heads(k, heads).transpose(-1, -2))      # [n, heads, Fq, Fk]


def evaluate(q, k, v, heads, scale=None):
    """(ref, W, tol0) of fp16 q, k, v [n, F, C] in fp64, each [n, F, C]: the reference, sum_k p_k |v_k| and the bound of this module's
    docstring without its SOFTMAX_ERR W term"""
    n, F, Cc = q.shape
    d = Cc // heads
    c = (d ** -0.5 if scale is None else scale) * LOG2E
    qh, kh, vh = (_heads(x.double(), heads) for x in (q, k, v))
    t = c * (qh @ kh.transpose(-1, -2))
    p = torch.softmax(t * LN2, dim=-1)
    ref, W = p @ vh, p @ vh.abs()
    delta = (c * d * U23 * (qh.abs() @ kh.abs().transpose(-1, -2)) + U22 * t.abs()).amax(dim=-1, keepdim=True)       # [n, heads, F, 1]
    vmax = vh.abs().amax(dim=-2, keepdim=True)                                                                   # [n, heads, 1, d]
    tol0 = U10 * ref.abs() + (U10 + 4 * LN2 * delta + F * U22) * W + F * U24 * vmax + U24
    back = lambda x: x.permute(0, 2, 1, 3).reshape(n, F, Cc)
    return back(ref), back(W), back(tol0)


def class_of(head_dim):
    return next(cl for cl in CLASSES if head_dim <= cl[1])


def emulate(q, k, v, heads, *, p_bf16=False, out_bf16=False, drop_last=False, extra_slot=False, scale_dqk=False, next_head_v=False):
    """the kernels' arithmetic in plain torch on the CPU: fp32 logits, fp32 base-2 softmax, P rounded to fp16, fp32 PV, the result
    rounded to fp16 -- [n, F, C] fp16.  The keywords are the mutants of tests/test_tattn_routes.py."""
    n, F, Cc = q.shape
    d = Cc // heads
    scale = torch.tensor((class_of(d)[0] if scale_dqk else d) ** -0.5, dtype=torch.float32)
    scale_log2 = scale * torch.tensor(1.4426950408889634, dtype=torch.float32)
    qh, kh, vh = (_heads(x.float(), heads) for x in (q, k, v))
    if next_head_v:
        vh = torch.roll(vh, -1, dims=1)
    if drop_last:
        kh, vh = kh[:, :, :-1], vh[:, :, :-1]
    t = (qh @ kh.transpose(-1, -2)) * scale_log2
    if extra_slot:          # key slot `frames`: a zero K row (logit 0) and V = 0
        t = torch.cat([t, torch.zeros_like(t[..., :1])], dim=-1)
        vh = torch.cat([vh, torch.zeros_like(vh[:, :, :1])], dim=-2)
    e = torch.exp2(t - t.amax(dim=-1, keepdim=True))
    p = e * (1.0 / e.sum(dim=-1, keepdim=True))
    p = p.bfloat16().float() if p_bf16 else p.half().float()
    o = p @ vh
    o = o.bfloat16().half() if out_bf16 else o.half()
    return o.permute(0, 2, 1, 3).reshape(n, F, Cc)


def sdpa_fp32(q, k, v, heads):
    """plain fp32 scaled-dot-product attention, rounded to fp16"""
    import torch.nn.functional as Fn
    n, F, Cc = q.shape
    o = Fn.scaled_dot_product_attention(*(_heads(x.float(), heads) for x in (q, k, v)))
    return o.permute(0, 2, 1, 3).reshape(n, F, Cc).half()


@functools.lru_cache(maxsize=2)
def _reference(name):
    c = next(k for k in CASES if k["name"] == name)
    t = inputs(c)
    return (t,) + evaluate(t["q"], t["k"], t["v"], c["heads"])


def reference(c):
    """(inputs, ref, W, tol0) of a case, computed once and shared; read-only"""
    return _reference(c["name"])


def excess(got, ref, W, tol0, softmax_err=None):
    """|got - ref| - bound per element, fp64: positive where the bound is missed"""
    se = SOFTMAX_ERR if softmax_err is None else softmax_err
    return (got.double() - ref).abs() - (tol0 + se * W)


def check_against(got, ref, W, tol0):
    """None if `got` [n, F, C] obeys the bound on every element, else a message"""
    got = got.detach().cpu()
    if tuple(got.shape) != tuple(ref.shape):
        return f"shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not bool(torch.isfinite(got.float()).all()):
        return f"non-finite output ({int((~torch.isfinite(got.float())).sum())} elements)"
    ex = excess(got, ref, W, tol0)
    bad = ex > 0
    if bool(bad.any()):
        i = tuple(int(x) for x in bad.nonzero()[0])
        err = float((got[i].double() - ref[i]).abs())
        return (f"{int(bad.sum())}/{bad.numel()} elements miss the bound, largest excess {float(ex.max()):.3e}; first at {i}: got "
                f"{float(got[i]):.6g}, ref {float(ref[i]):.6g}, error {err:.3e}, allowed {err - float(ex[i]):.3e}")
    return None


def check(c, got):
    """None if the result [n_pixels, frames, C] of a case obeys the bound, else a message"""
    _, ref, W, tol0 = reference(c)
    return check_against(got, ref, W, tol0)


def check_tensors(q, k, v, heads, got):
    """the same for any fp16 q, k, v [n, F, C] (tests/test_kernels_gpu.py)"""
    return check_against(got, *evaluate(q, k, v, heads))


def softmax_excess(c, got):
    """how SOFTMAX_ERR is measured: the largest excess of a case's result over the bound evaluated with SOFTMAX_ERR = 0, per unit of W
    (what the bound multiplies SOFTMAX_ERR by).  0.0 when nothing exceeds."""
    _, ref, W, tol0 = reference(c)
    ex = excess(got.detach().cpu(), ref, W, tol0, softmax_err=0.0)
    return float((ex / W.clamp_min(1e-30)).clamp_min(0).max())


# ------------------------------------------------------------------------------------------------------------------- through the wrapper
def run(kernels, dev, c, t, with_out=True):
    """the case through kernels.temporal_attention with real device pointers.  Returns a dict: out ([n_pixels, frames, C] fp16, on the
    CPU), route (kernels.last_tattn_route()), untouched (None for o = "own", else whether every element of the output's buffer
    outside the view still holds POISON bit for bit).  with_out=False: without the `out=` argument (o = "own" only)."""
    lay = layout(c)
    n, F, rows, Cc = c["n_pixels"], c["frames"], lay["rows"], lay["C"]
    q2, k2 = t["q"].reshape(rows, Cc), t["k"].reshape(rows, Cc)
    if lay["shared"]:
        qk = torch.zeros((rows, lay["q"][0]), dtype=torch.float16)
        qk[:, :Cc], qk[:, Cc:2 * Cc] = q2, k2
        qk = qk.to(dev)
        qd, kd = qk[:, :Cc], qk[:, Cc:2 * Cc]
    else:
        def first_columns(x, ld):
            wide = torch.zeros((rows, ld), dtype=torch.float16)
            wide[:, :Cc] = x
            return wide.to(dev)[:, :Cc]
        qd, kd = first_columns(q2, lay["q"][0]), first_columns(k2, lay["k"][0])
    vt = torch.full((n, Cc, c["vt_ld"]), float("nan"), dtype=torch.float16)
    vt[:, :, :F] = t["v"].permute(0, 2, 1)
    kw, buf = {}, None
    if c["o"] != "own":
        brows, bcols, col0 = lay["o"]
        buf = torch.full((brows, bcols), POISON, dtype=torch.int16, device=dev).view(torch.float16)
        kw["out"] = buf[:rows, col0: col0 + Cc]
    elif with_out:
        kw["out"] = torch.empty((rows, Cc), dtype=torch.float16, device=dev)
    out = kernels.temporal_attention(qd, kd, vt.to(dev), n_pixels=n, frames=F, heads=c["heads"], head_dim=c["head_dim"], **kw)
    res = dict(route=kernels.last_tattn_route() if hasattr(kernels, "last_tattn_route") else None, untouched=None)
    if buf is not None:
        assert out.data_ptr() == kw["out"].data_ptr()
        probe = buf.clone().view(torch.int16)
        probe[:rows, col0: col0 + Cc] = POISON
        res["untouched"] = bool((probe == POISON).all())
    res["out"] = out.cpu().reshape(n, F, Cc).clone()
    return res
