"""Reference, inputs and error bounds of the attention-forward route tests (tests/test_attn_routes.py, tests/test_attn_routes_gpu.py;
tests/test_kernels_gpu.py uses the bounds as well).

Reference: softmax attention per (query batch, head) in fp64 on the CPU from the fp16-rounded inputs: ref = sum_k p_k v_k, beside it
W = sum_k p_k |v_k| (what a relative error of the weights scales with) and max_k |v_k|.  Every result is checked twice:
  (a) against the reference whose logits are t_ik = q'_i . k_k with q' = fp16(fl32(float(q) * scale_log2)), scale_log2 =
      fl32(fl32(scale) * fl32(log2 e)): the kernel's own pre-scaled Q (csrc/attention.hip, load_q), one deterministic IEEE
      multiplication and one conversion, reproduced bit for bit in float32 on the CPU (`q_prime`; round-to-nearest-even both, fp16
      subnormals kept, as the GPU's default modes).  With it the kernel's dominant error, the rounding of Q, is not an error.
  (b) against the plain reference, t_ik = scale log2e q_i . k_k in fp64 without any rounding, with the rounding of Q as one more term:
      this pins what the operation means, not only how it is implemented.

The kernel, per query row i (all in fp32 unless said), with m the running reference (log2 units), a_ik = sum_d |q'_id| |k_kd| and
M_i = max(|max of the first tile's logits|, |max_k t_ik|) + 8 >= |m| (the reference never decreases, starts at the first tile's
maximum and ends at most 8 below the row's):
    s_ik  = -m + sum_d q'_id k_kd     fp16 x fp16 products are exact in fp32; the MFMA chain sums d of them (the padding to DQK adds
                                      zeros) onto the initial accumulator -m: d roundings of partial sums that are at most
                                      a_ik + |m|:                                              |error| <= d 2^-24 (a_ik + M_i)
    the reference moves at most once per key tile (first tile: to the tile's maximum; later: by max(tile maximum, 0), and only if
    some score of the wave's 16 rows exceeds 2^8 = DEFER_THR): m is rounded (2^-24 M_i, an error of every LATER logit against the
    earlier ones, ntiles times at most), and the tile's own scores are shifted (one rounding of a number <= |s| + M_i, and a score
    that carries weight has |s| <= M_i).  O and l are multiplied by exp2(-shift) (one rounding each per tile, the hardware exp2).
  => logit k is off by at most 2^-24 (d (a_ik + M_i) + (ntiles + 2) M_i); doubled (the factor 2 of tests/gemm_bounds.py, on this as on
     every term below): delta_ik = 2^-23 (d (a_ik + M_i) + (ntiles + 2) M_i).  The kernel's weights are p_k u_k / sum_j p_j u_j with
     u_k = 2^(error of logit k) in [1 / (1 + g_ik), 1 + g_ik], g_ik = 2^(delta_ik) - 1.  Since sum_k p_k (v_k - ref) = 0,
     out - ref = sum_k p_k (u_k - c)(v_k - ref) / sum_j p_j u_j for any c; with c = u_k*, k* the row's heaviest key, and
     G_ik = (1 + g_ik)(1 + g_ik*) - 1 >= |u_k / u_k* - 1|, E_i = sum_{k != k*} p_ik G_ik:
     L_i = (sum_{k != k*} p_ik G_ik |v_k| + E_i |ref|) / (1 - E_i).  The error of a key that carries the whole row (the spiked key
     where it wins) is a common factor and costs nothing, nor does a key whose logit is large and whose weight is not (where it loses).
     (In check (b) of the `large` family E_i can reach 1: there the bound is infinite and says nothing; (a) asserts E_i < 1/2.)
    P_ik  = fp16(exp2(s_ik))          the reference is at most 8 below the row's running maximum, so P <= 2^8 (no overflow: fp16
                                      holds 65504) and the key that set the reference has P = 1: l >= 1.
      not SPARE: round to nearest, 2^-11 relative in the normal range -> 2^-11 W, doubled 2^-10 W.  l is the fp32 sum of the
                 UNROUNDED exp2 values.
      SPARE:     round toward zero (v_cvt_pkrtz), relative eps_k in [0, 2^-10), and l = sum_k P~_k from the same rounded P~ (V^T row
                 `head_dim` holds ones).  out - ref = -sum_k P_k eps_k (v_k - ref) / sum_k P~_k, and since sum_k P_k (v_k - ref) = 0
                 any constant may be subtracted from eps_k: with 2^-11, |out - ref| <= 2^-11 (W + |ref|) / (1 - 2^-10); doubled
                 2^-10 (W + |ref|).  (The bias of the truncation cancels in the ratio; what does not cancel is its spread.)
      below the normal range (P < 2^-14) the absolute error is 2^-25 (nearest) or 2^-24 (toward zero), against l >= 1: lk of them
      give lk 2^-25 max|v| (lk 2^-24 max|v|); doubled lk 2^-24 max|v| (SPARE: lk 2^-23 max|v|).
    O    += P~ V, l += P              fp32 sums over lk terms (lk 2^-24 relative each), the rescales (ntiles roundings each), 1 / l and
                                      the final product (one each, and the hardware reciprocal): (2 lk + 2 ntiles + 2) 2^-24 W;
                                      doubled (lk + ntiles + 1) 2^-22 W.
    out   = fp16(O / l)               2^-11 |ref|, doubled 2^-10 |ref|; 2^-25 below the normal range, doubled 2^-24.
    accumulate: out = fp16(prev + acc_scale * O * (1 / l)): two more fp32 roundings, 2^-23 (|prev| + |acc_scale ref|), doubled
                2^-22 (...); the terms above times |acc_scale|; the fp16 rounding applies to prev + acc_scale ref.
    hardware exp2, reciprocal and log2: SOFTMAX_ERR (relative to a weight; measured: below).

  (a)  |out - ref| <= 2^-10 |ref| + 2^-24
                      + L_i + (2^-10 + (lk + ntiles + 1) 2^-22 + SOFTMAX_ERR) W  [+ 2^-10 |ref| if SPARE]
                      + lk 2^-24 max|v|  [2^-23 if SPARE]
  (b)  the same around the plain reference with delta_ik + eta_ik for delta_ik, where eta_ik bounds what separates q'.k from
       scale log2e q.k: the rounding of q' to fp16 (2^-11 scale_log2 sum_d |q||k| per logit, 2^-25 sum_d |k| where q' is
       subnormal), the fp32 product before it (2^-24 of the same sum) and the three roundings of scale_log2 (3 2^-24 |t|); doubled
       eta_ik = (2^-10 + 2^-23) scale_log2 sum_d |q_id||k_kd| + 2^-24 sum_d |k_kd| + 2^-22 |t_ik|, and a_ik taken from the plain
       operands times (1 + 2^-10).
  Both hold for any kernel that evaluates these steps in fp32 with P and the result rounded to fp16, whatever its key order.

Fused lse (fp32 [batch_q, heads, lq], against log2 sum_k 2^(t_ik) of the q' logits): lse = log2(l) + m.  The logit errors shift it
by delta_ik* - log2(1 - E_i) at most; l carries lk + ntiles fp32 roundings ((lk + ntiles) 2^-24 / ln2 in log2 units); a SPARE kernel's l is the sum of
the P rounded toward zero, low by the relative 2^-10 at most and by lk 2^-24 in absolute terms against l >= 1; log2(l) (<= 8 + log2 lk),
m and their sum are rounded (3 2^-24 (|lse| + 8 + log2 lk)); the hardware log2 and exp2 (SOFTMAX_ERR / ln2).  Doubled:
       |lse - ref| <= delta_ik* - log2(1 - E_i) + ((lk + ntiles) 2^-23 + [2^-9 + lk 2^-23 if SPARE] + 2 SOFTMAX_ERR) / ln2 + 3 2^-23 (|ref| + 8 + log2 lk)

Inputs, from a generator seeded by the case's name; every V^T tail (lk .. vt_ld) holds NaN.
  unit   standard normal q, k, v
  heavy  standard normal v, q and k times 2: logits of +-10 log2 units, so two or three heavy keys carry each row whatever lk is.  W is
         then close to |ref| on many elements and the bound a small multiple of the fp16 roundings of P and of the result, over any
         number of keys and key tiles: the family on which the checker is shown to reject bf16 roundings and a scale off by 2^-10 on
         multi-tile cases (tests/test_attn_routes.py); with `unit` inputs the roundings of a hundred keys average out below any bound
  large  q and k times 5: |logit| (natural units) reaches 60 and more on some rows (asserted in fp64)
  spike  unit, and one key per (K/V batch, head) times 128: on the rows where q . k of that key is positive its logit exceeds every
         other logit of the row by more than 140 log2 units (asserted).  The key lies in the second key tile or later and cycles
         with the (batch, head) over `spike_keys`: one key per lane group and `kt` parity of the kernel's key order, key = 32 (kt >> 1)
         + 8 g + 4 (kt & 1) + r, the first key of the last tile and key lk - 1.
  creep  the deferred maximum with P far above 1 and a real rescale after it (needs three key tiles; asserted in fp64 with the
         kernel's tiles and 16-row groups): channel 0 of every head carries q = 1 / scale_log2 (q' = 1 within fp16) and k = 0 except on
         two keys whose other channels are 0, key kvt + 14 with k_0 = 7.9 and key min(2 kvt + 5, lk - 1) with k_0 = 9.9; the other channels are
         standard normal (k times 1/4).  Tile 0 sets the reference near 1, tile 1's maximum exceeds it by between 6 and 8 on every row
         of a 16-row group (no move: P = 2^7 there), tile 2's by more than 8 (the move).
"""
import functools
import math
import zlib

import torch

from tests.attn_route_cases import ACC_SCALE, CASES, CLASSES, layout, pad8

U9, U10, U22, U23, U24 = 2.0 ** -9, 2.0 ** -10, 2.0 ** -22, 2.0 ** -23, 2.0 ** -24
LOG2E, LN2 = 1.0 / math.log(2.0), math.log(2.0)
DEFER_THR = 8.0
# Relative error of the hardware exp2 / reciprocal / log2 in a softmax weight: cannot be derived from here.  Measured as
# `softmax_excess` below: the largest excess over bound (a) with SOFTMAX_ERR = 0, per unit of W, over the table's default-environment
# cases; SOFTMAX_ERR = twice that, or 0 when nothing exceeds.  It may not exceed 2^-18 (these instructions err by an fp32 ulp or two):
# more would be a finding about the kernel.
# Measured 2026-10-21 on an MI355X with the parent commit's library (ABI 34, the one before the route queries; the kernels' assembly is
# unchanged since): largest excess 0.0 over the 99 cases of the default environment (all five input families, accumulate and fused
# lse included; largest error / bound 0.50 in (a) and (b), 0.26 in the lse): no element exceeds, SOFTMAX_ERR = 0.
SOFTMAX_ERR = 0.0
assert SOFTMAX_ERR <= 2.0 ** -18
LARGE_AMP, SPIKE_AMP, SPIKE_GAP, LARGE_LOGIT, HEAVY_AMP = 5.0, 128.0, 140.0, 60.0, 2.0
CREEP_K1, CREEP_K2 = 7.9, 9.9
POISON = 0x7E37          # an fp16 NaN with a payload: what the output buffers hold outside the view (tattn_bounds.POISON)
CHUNK = 1 << 23          # logits evaluated at once


# ------------------------------------------------------------------------------------------------------------------- inputs
def scale_log2_f32(scale):
    """fl32(fl32(scale) * fl32(log2 e)), as launch_q computes it"""
    return torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)


def q_prime(q, scale):
    """the kernel's Q fragments: fp16(float(q) * scale_log2), bit for bit"""
    return (q.float() * scale_log2_f32(scale)).half()


def spike_keys(lk, kvt):
    """the keys that take the spike, cycled over the (batch, head) pairs: offsets 1, 14, 19, 28, 36, 41, 54, 59 of the second key tile
    are (lane group g, kt parity) = (0, 0) (1, 1) (2, 0) (3, 1) (0, 1) (1, 0) (2, 1) (3, 0); the first key of the last tile; lk - 1"""
    keys = [kvt + o for o in (1, 14, 19, 28, 36, 41, 54, 59) if kvt + o < lk] + [(lk - 1) // kvt * kvt, lk - 1]
    return sorted(set(keys))


def lane_slot(key, kvt):
    """(g, kt & 1) of a key in the kernel's order"""
    o = key % kvt % 32
    return o // 8, o % 8 // 4


def creep_keys(kvt, lk):
    return kvt + 14, min(2 * kvt + 5, lk - 1)


def inputs(c):
    """q [bq, lq, C], k, v [bq / grp, lk, C] of a case as fp16 CPU tensors (prev [bq, lq, C] too for form "acc")"""
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    bq, bkv, lq, lk, H, d = c["bq"], c["bq"] // c["grp"], c["lq"], c["lk"], c["heads"], c["d"]
    kvt = c["route"]["kvt"]
    q = torch.randn((bq, lq, H, d), generator=g, dtype=torch.float32)
    k = torch.randn((bkv, lk, H, d), generator=g, dtype=torch.float32)
    v = torch.randn((bkv, lk, H, d), generator=g, dtype=torch.float32)
    if c["inputs"] == "large":
        q, k = q * LARGE_AMP, k * LARGE_AMP
    elif c["inputs"] == "heavy":
        q, k = q * HEAVY_AMP, k * HEAVY_AMP
    elif c["inputs"] == "spike":
        assert lk > kvt, "a spike case needs a second key tile"
        keys = spike_keys(lk, kvt)
        for pair in range(bkv * H):
            k[pair // H, keys[pair % len(keys)], pair % H] *= SPIKE_AMP
    elif c["inputs"] == "creep":
        assert lk > 2 * kvt, "a creep case needs three key tiles"
        k1, k2 = creep_keys(kvt, lk)
        k *= 0.25
        k[..., 0] = 0.0
        k[:, k1], k[:, k2] = 0.0, 0.0
        k[:, k1, :, 0], k[:, k2, :, 0] = CREEP_K1, CREEP_K2
        q[..., 0] = 1.0 / float(scale_log2_f32(d ** -0.5))
    Cc = H * d
    t = dict(q=q.reshape(bq, lq, Cc).half(), k=k.reshape(bkv, lk, Cc).half(), v=v.reshape(bkv, lk, Cc).half())
    if c["form"] == "acc":
        t["prev"] = torch.randn((bq, lq, Cc), generator=g, dtype=torch.float32).half()
    return t


def _heads(x, H):
    b, n, Cc = x.shape
    return x.view(b, n, H, Cc // H).permute(0, 2, 1, 3)             # [b, H, n, d]


def _back(x):
    b, H, n, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, n, H * d)


def _batches(c, per_batch):
    """ranges [b0, b1) of query batches whose work stays below CHUNK elements"""
    step = max(1, CHUNK // max(1, per_batch))
    return [(b0, min(c["bq"], b0 + step)) for b0 in range(0, c["bq"], step)]


def _kv_index(c, b0, b1, wrong_group=False):
    idx = torch.arange(b0, b1)
    return idx % (c["bq"] // c["grp"]) if wrong_group else idx // c["grp"]


# ------------------------------------------------------------------------------------------------------------------- the reference
def evaluate(c, t):
    """the fp64 references and bounds of a case: dict(a=(ref, W, tol0), b=(ref, W, tol0), lse=(ref, tol0)) with ref, W, tol0 [bq, lq, C]
    and the lse pair [bq, H, lq]; tol0 is the bound without its SOFTMAX_ERR term.  Also asserts what the input family promises."""
    H, d, lq, lk, kvt, spare = c["heads"], c["d"], c["lq"], c["lk"], c["route"]["kvt"], bool(c["route"]["spare"])
    nt = -(-lk // kvt)
    scale = d ** -0.5
    sl2 = float(scale_log2_f32(scale))
    acc = ACC_SCALE if c["form"] == "acc" else None
    out = {"a": [[], [], []], "b": [[], [], []], "lse": [[], []]}
    seen = dict(large=0.0, spike=set(), creep=0)
    for b0, b1 in _batches(c, H * lq * max(lk, d)):
        kv = _kv_index(c, b0, b1)
        q, qp = _heads(t["q"][b0:b1].double(), H), _heads(q_prime(t["q"][b0:b1], scale).double(), H)
        k, v = _heads(t["k"][kv].double(), H), _heads(t["v"][kv].double(), H)
        kT, vabs = k.transpose(-1, -2), v.abs()
        vmax = vabs.amax(dim=-2, keepdim=True)
        prev = _heads(t["prev"][b0:b1].double(), H) if acc is not None else None
        t_a = qp @ kT
        for which, tl, a, eta in (("a", t_a, qp.abs() @ kT.abs(), 0.0), ("b", (scale * LOG2E) * (q @ kT), None, None)):
            if which == "b":
                qk = q.abs() @ kT.abs()
                a = (1 + U10) * sl2 * qk
                eta = (U10 + U23) * sl2 * qk + U24 * k.abs().sum(dim=-1).unsqueeze(-2) + U22 * tl.abs()
            p = torch.softmax(tl * LN2, dim=-1)
            ref, W = p @ v, p @ vabs
            M = _reference_range(tl, kvt)
            g = torch.expm1(LN2 * (U23 * (d * (a + M) + (nt + 2) * M) + eta))          # per key: 2^(delta_ik) - 1
            star = p.argmax(dim=-1, keepdim=True)                                   # k*: the row's heaviest key
            gstar = g.gather(-1, star)
            pG = (p * ((1 + g) * (1 + gstar) - 1)).scatter(-1, star, 0.0)
            E = pG.sum(dim=-1, keepdim=True)
            assert which == "b" or float(E.max()) < 0.5, (c["name"], float(E.max()))
            logit_term = torch.where(E < 1, (pG @ vabs + E * ref.abs()) / (1 - E).clamp_min(1e-300), torch.full_like(E, math.inf))
            core = logit_term + (U10 + (lk + nt + 1) * U22) * W + lk * (U23 if spare else U24) * vmax
            if spare:
                core = core + U10 * ref.abs()
            if acc is None:
                tol = core + U10 * ref.abs() + U24
            else:
                tol = abs(acc) * core + U22 * (prev.abs() + abs(acc) * ref.abs()) + U10 * (prev + acc * ref).abs() + U24
                ref, W = prev + acc * ref, abs(acc) * W
            for lst, x in zip(out[which], (ref, W, tol)):
                lst.append(_back(x))
            if which == "a":
                lse = torch.logsumexp(tl * LN2, dim=-1) * LOG2E
                ltol = (torch.log2(1 + gstar) - torch.log2(1 - E)).squeeze(-1) + ((lk + nt) * U23 + ((U9 + lk * U23) if spare else 0.0)) / LN2 + \
                    3 * U23 * (lse.abs() + 8 + math.log2(lk))
                out["lse"][0].append(lse)
                out["lse"][1].append(ltol)
        _family_facts(c, t_a, seen, b0, kv)
    _assert_family(c, seen)
    cat = lambda xs: torch.cat(xs, dim=0)
    return dict(a=tuple(map(cat, out["a"])), b=tuple(map(cat, out["b"])), lse=tuple(map(cat, out["lse"])))


def _reference_range(t, kvt):
    """M_i [.., lq, 1]: what |m| of a row can reach.  The running reference never decreases, starts at the first tile's maximum and
    ends at most 8 below the row's, so |m| <= max(|max of tile 0|, |max of the row|) + 8"""
    return torch.maximum(t[..., :kvt].amax(dim=-1, keepdim=True).abs(), t.amax(dim=-1, keepdim=True).abs()) + DEFER_THR


def _family_facts(c, t_a, seen, b0, kv):
    """what the input family promises, collected from the q' logits t_a [b, H, lq, lk] (log2 units) of one chunk"""
    H, lq, lk, kvt = c["heads"], c["lq"], c["lk"], c["route"]["kvt"]
    if c["inputs"] == "large":
        seen["large"] = max(seen["large"], float(t_a.abs().max()) * LN2)
    elif c["inputs"] == "spike":
        keys = spike_keys(lk, kvt)
        top2 = t_a.topk(2, dim=-1).values
        won = (top2[..., 0] - top2[..., 1] > SPIKE_GAP)
        arg = t_a.argmax(dim=-1)
        for i in range(t_a.shape[0]):
            for h in range(H):
                key = keys[(int(kv[i]) * H + h) % len(keys)]
                if bool((won[i, h] & (arg[i, h] == key)).any()):
                    seen["spike"].add(key)
    elif c["inputs"] == "creep":
        nt = -(-lk // kvt)
        pad = nt * kvt - lk
        tt = torch.cat([t_a, t_a.new_full(t_a.shape[:-1] + (pad,), -math.inf)], dim=-1).view(*t_a.shape[:-1], nt, kvt).amax(dim=-1)
        ref0 = tt[..., 0]
        e1 = tt[..., 1] - ref0                                          # tile 1 against the reference tile 0 set
        rows = e1.shape[-1]
        gpad = -rows % 16
        grp_max = torch.cat([e1, e1.new_full(e1.shape[:-1] + (gpad,), -math.inf)], dim=-1).view(*e1.shape[:-1], -1, 16).amax(dim=-1)
        grp_max = grp_max.repeat_interleave(16, dim=-1)[..., :rows]
        deferred = (e1 > 6) & (e1 < DEFER_THR) & (grp_max <= DEFER_THR)   # no row of the wave's 16 moves the reference in tile 1
        moved = (tt[..., 2] - ref0) > DEFER_THR
        seen["creep"] += int((deferred & moved).sum())


def _assert_family(c, seen):
    if c["inputs"] == "large":
        assert seen["large"] >= LARGE_LOGIT, (c["name"], seen["large"])
    elif c["inputs"] == "spike":
        keys = spike_keys(c["lk"], c["route"]["kvt"])
        pairs = c["bq"] // c["grp"] * c["heads"]
        want = {keys[p % len(keys)] for p in range(pairs)}
        assert seen["spike"] == want, (c["name"], sorted(want - seen["spike"]))
    elif c["inputs"] == "creep":
        assert seen["creep"] >= max(1, c["bq"] * c["heads"] * c["lq"] // 2), (c["name"], seen["creep"])


def class_of(head_dim):
    return next(cl for cl in CLASSES if head_dim <= cl[1])


# ------------------------------------------------------------------------------------------------------------------- the kernel's arithmetic
def _rtz_half(x):
    """fp32 -> fp16 toward zero (v_cvt_pkrtz_f16_f32), returned as fp32"""
    h = x.half()
    hf = h.float()
    over = hf.abs() > x.abs()
    bits = h.view(torch.int16)
    return torch.where(over, (bits - 1).view(torch.float16).float(), hf)          # one ulp toward zero (sign-magnitude: bits - 1)


def emulate(c, t, *, p_bf16=False, out_bf16=False, drop_last=False, extra_slot=False, scale_off=False, l_not_rescaled=False,
            next_head_v=False, wrong_group=False, swap_blocks=False, plain=False):
    """the kernel's arithmetic in plain torch on the CPU, (out [bq, lq, C] fp16, lse [bq, H, lq] fp32): q' as the kernel rounds it, fp32
    logits, key tiles of kvt keys with the deferred maximum (the reference moves on the first tile and when a score of the 16-row
    group exceeds it by more than 2^8), P rounded to fp16 (toward zero and summed rounded in a SPARE kernel), fp32 sums, the fp16
    result.  The keywords are the mutants of tests/test_attn_routes.py; plain=True is fp32 softmax attention without any of it."""
    H, d, lq, lk, kvt, spare, qt = c["heads"], c["d"], c["lq"], c["lk"], c["route"]["kvt"], bool(c["route"]["spare"]), c["route"]["qt"]
    scale = d ** -0.5 * ((1 + U10) if scale_off else 1.0)
    outs, lses = [], []
    for b0, b1 in _batches(c, H * lq * max(lk, d)):
        kv = _kv_index(c, b0, b1, wrong_group)
        qp = _heads(q_prime(t["q"][b0:b1], scale).float(), H)
        k, v = _heads(t["k"][kv].float(), H), _heads(t["v"][kv].float(), H)
        if next_head_v:
            v = torch.roll(v, -1, dims=1)
        if plain:
            o = torch.nn.functional.scaled_dot_product_attention(_heads(t["q"][b0:b1].float(), H), k, v)
            lse = torch.zeros(o.shape[:-1])
        else:
            if drop_last:
                k, v = k[:, :, :-1], v[:, :, :-1]
            s = qp @ k.transpose(-1, -2)
            if extra_slot:          # key slot lk: a zero K row (logit 0) and V = 0
                s = torch.cat([s, torch.zeros_like(s[..., :1])], dim=-1)
                v = torch.cat([v, torch.zeros_like(v[:, :, :1])], dim=-2)
            n = s.shape[-1]
            m = torch.zeros(s.shape[:-1])
            l = torch.zeros(s.shape[:-1])
            o = torch.zeros(s.shape[:-1] + (d,))
            moves = 0
            for k0 in range(0, n, kvt):
                st = s[..., k0:k0 + kvt] - m.unsqueeze(-1)
                mx = st.amax(dim=-1)
                if k0 == 0:
                    dlt = mx
                else:
                    gpad = -lq % 16
                    grp = torch.cat([mx, mx.new_full(mx.shape[:-1] + (gpad,), -math.inf)], dim=-1).view(*mx.shape[:-1], -1, 16)
                    trig = (grp.amax(dim=-1) > DEFER_THR).repeat_interleave(16, dim=-1)[..., :lq]
                    dlt = torch.where(trig, mx.clamp_min(0.0), torch.zeros_like(mx))
                alpha = torch.exp2(-dlt) if k0 else torch.ones_like(dlt)
                m = m + dlt
                st = st - dlt.unsqueeze(-1)
                o = o * alpha.unsqueeze(-1)
                skip_l = l_not_rescaled and k0 and bool((dlt > 0).any()) and moves == 0
                if skip_l:
                    moves += 1
                else:
                    l = l * alpha
                e = torch.exp2(st)
                if p_bf16:
                    pr = e.bfloat16().float()
                else:
                    pr = _rtz_half(e) if spare else e.half().float()
                l = l + (pr if spare else e).sum(dim=-1)
                o = o + pr @ v[:, :, k0:k0 + kvt]
            o = o * (1.0 / l).unsqueeze(-1)
            lse = torch.log2(l) + m
        if c["form"] == "acc":
            o = _heads(t["prev"][b0:b1].float(), H) + torch.tensor(ACC_SCALE, dtype=torch.float32) * o
        o = _back(o)
        outs.append(o.bfloat16().half() if out_bf16 else o.half())
        lses.append(lse)
    out = torch.cat(outs, dim=0)
    if swap_blocks:          # the workgroups of query blocks 0 and 1 (64 qt rows each) write each other's rows
        rows = 64 * qt
        n1 = min(rows, lq - rows)
        out = out.clone()
        a, b = out[:, :n1].clone(), out[:, rows:rows + n1].clone()
        out[:, :n1], out[:, rows:rows + n1] = b, a
    return out, torch.cat(lses, dim=0)


# ------------------------------------------------------------------------------------------------------------------- the checks
@functools.lru_cache(maxsize=2)
def _reference(name):
    c = next(k for k in CASES if k["name"] == name)
    t = inputs(c)
    return t, evaluate(c, t)


def reference(c):
    """(inputs, evaluate(...)) of a case, computed once and shared; read-only"""
    return _reference(c["name"])


def excess(got, ref, W, tol0, softmax_err=None):
    """|got - ref| - bound per element, fp64: positive where the bound is missed"""
    se = SOFTMAX_ERR if softmax_err is None else softmax_err
    return (got.double() - ref).abs() - (tol0 + se * W)


def ratio(got, ref, W, tol0):
    """the largest |got - ref| / bound"""
    return float(((got.double() - ref).abs() / (tol0 + SOFTMAX_ERR * W)).max())


def check_against(got, ref, W, tol0, what=""):
    """None if `got` obeys the bound on every element, else a message"""
    got = got.detach().cpu()
    if tuple(got.shape) != tuple(ref.shape):
        return f"{what}shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not bool(torch.isfinite(got.float()).all()):
        return f"{what}non-finite output ({int((~torch.isfinite(got.float())).sum())} elements)"
    ex = excess(got, ref, W, tol0)
    bad = ex > 0
    if bool(bad.any()):
        i = tuple(int(x) for x in bad.nonzero()[0])
        err = float((got[i].double() - ref[i]).abs())
        return (f"{what}{int(bad.sum())}/{bad.numel()} elements miss the bound, largest excess {float(ex.max()):.3e}; first at {i}: got "
                f"{float(got[i]):.6g}, ref {float(ref[i]):.6g}, error {err:.3e}, allowed {err - float(ex[i]):.3e}")
    return None


def check(c, got, which=("a", "b")):
    """None if the result [bq, lq, C] of a case obeys checks (a) and (b), else the first message"""
    ev = reference(c)[1]
    for w in which:
        msg = check_against(got, *ev[w], what=f"check ({w}): ")
        if msg is not None:
            return msg
    return None


def check_lse(c, lse):
    ref, tol0 = reference(c)[1]["lse"]
    return check_against(lse, ref, torch.full_like(ref, 2.0 / LN2), tol0, what="fused lse: ")


def ratios(c, got, lse=None):
    """error / bound, the largest per check: dict(a=, b=[, lse=])"""
    ev = reference(c)[1]
    r = {w: ratio(got.detach().cpu(), *ev[w]) for w in ("a", "b")}
    if lse is not None:
        ref, tol0 = ev["lse"]
        r["lse"] = ratio(lse.detach().cpu(), ref, torch.full_like(ref, 2.0 / LN2), tol0)
    return r


def check_tensors(q, k, vt, got, *, batch_q, lq, lk, heads, head_dim, kv_group=1, kvt=64):
    """checks (a) and (b) for any fp16 q [batch_q * lq, C], k [batch_kv * lk, C], vt [batch_kv, C, >= lk] (tests/test_kernels_gpu.py);
    returns (message or None, tol (a), tol (b), the plain fp64 reference), the last three [batch_q * lq, C]"""
    Cc = heads * head_dim
    bkv = batch_q // kv_group
    c = dict(name="tensors", bq=batch_q, grp=kv_group, heads=heads, d=head_dim, lq=lq, lk=lk, form="plain", inputs="unit",
             route=dict(kvt=kvt, spare=int(head_dim < class_of(head_dim)[1]), qt=1))
    t = dict(q=q.detach().cpu().reshape(batch_q, lq, Cc), k=k.detach().cpu().reshape(bkv, lk, Cc),
             v=vt.detach().cpu()[:, :, :lk].transpose(1, 2).contiguous())
    ev = evaluate(c, t)
    got = got.detach().cpu().reshape(batch_q, lq, Cc)
    msg = None
    for w in ("a", "b"):
        msg = msg or check_against(got, *ev[w], what=f"check ({w}): ")
    flat = lambda x: x.reshape(batch_q * lq, Cc)
    return msg, flat(ev["a"][2] + SOFTMAX_ERR * ev["a"][1]), flat(ev["b"][2] + SOFTMAX_ERR * ev["b"][1]), flat(ev["b"][0])


def softmax_excess(c, got):
    """how SOFTMAX_ERR is measured: the largest excess of a case's result over bound (a) evaluated with SOFTMAX_ERR = 0, per unit of W
    (what the bound multiplies SOFTMAX_ERR by).  0.0 when nothing exceeds.  Driven on the GPU by a loop over
    cases_of("default"):  t = reference(c)[0]; softmax_excess(c, run(kernels, dev, c, t)["out"]), the maximum over the cases."""
    ref, W, tol0 = reference(c)[1]["a"]
    ex = excess(got.detach().cpu(), ref, W, tol0, softmax_err=0.0)
    return float((ex / W.clamp_min(1e-30)).clamp_min(0).max())


# ------------------------------------------------------------------------------------------------------------------- through the wrapper
def run(kernels, dev, c, t):
    """the case through kernels.attention with real device pointers.  Returns a dict: out ([bq, lq, C] fp16, on the CPU), lse (fp32
    [bq, H, lq] on the CPU for form "lse", else None), route (kernels.last_attn_route(), None where the library has none), untouched
    (None for o = "own", else whether every element of the output's buffer outside the view still holds POISON bit for bit)."""
    lay = layout(c)
    Cc, bq, bkv, lq, lk = lay["C"], c["bq"], c["bq"] // c["grp"], c["lq"], c["lk"]

    def slice_of(x, rows, col0):
        if c["qk"] == "own":
            return x.reshape(rows, Cc).to(dev)
        wide = torch.full((rows, lay["qk_ld"]), float("nan"), dtype=torch.float16)
        wide[:, col0:col0 + Cc] = x.reshape(rows, Cc)
        return wide.to(dev)[:, col0:col0 + Cc]
    qd, kd = slice_of(t["q"], lay["q_rows"], 0), slice_of(t["k"], lay["k_rows"], lay["k_col"])
    vt = torch.full((bkv, Cc, c["vt_ld"]), float("nan"), dtype=torch.float16)
    vt[:, :, :lk] = t["v"].permute(0, 2, 1)
    brows, bcols, col0 = lay["o"]
    buf = None
    if c["o"] == "own":
        out = torch.empty((lay["q_rows"], Cc), dtype=torch.float16, device=dev)
    else:
        buf = torch.full((brows, bcols), POISON, dtype=torch.int16, device=dev).view(torch.float16)
        out = buf[:lay["q_rows"], col0:col0 + Cc]
    kw = {}
    if c["form"] == "acc":
        out.copy_(t["prev"].reshape(lay["q_rows"], Cc).to(dev))
        kw = dict(accumulate=True, acc_scale=ACC_SCALE)
    elif c["form"] == "lse":
        kw = dict(return_lse="fused")
    res = kernels.attention(qd, kd, vt.to(dev), batch_q=bq, lq=lq, lk=lk, heads=c["heads"], head_dim=c["d"], kv_group=c["grp"], out=out, **kw)
    lse = None
    if c["form"] == "lse":
        res, lse = res
        lse = lse.cpu()
    assert res.data_ptr() == out.data_ptr()
    r = dict(route=kernels.last_attn_route() if hasattr(kernels, "last_attn_route") else None, untouched=None, lse=lse)
    if buf is not None:
        probe = buf.clone().view(torch.int16)
        probe[:lay["q_rows"], col0:col0 + Cc] = POISON
        r["untouched"] = bool((probe == POISON).all())
    r["out"] = out.cpu().reshape(bq, lq, Cc).clone()
    return r
