"""Reference and error bound of the GEMM / conv route tests (tests/test_gemm_routes.py, tests/test_gemm_routes_gpu.py).

Reference: the operation in fp64 on the CPU from the fp16-rounded inputs -- matmul or F.conv2d in double, then bias, row vector,
residual, epilogue, out_scale; results are compared in LOGICAL row order (the store's permutation is undone on the kernel's output).

Bound, per element, derived and not tuned:

    |got - ref| <= 2^-10 |ref| + K 2^-23 S |out_scale| + 2^-24,        S = |A| |W|^T + |bias| + |rowvec| + |residual|  (fp64)

It holds for ANY kernel that multiplies fp16 operands exactly and accumulates in fp32, whatever its summation order, split or not:
fp16 x fp16 products are exact in fp32; an fp32 sum of K terms (and the few epilogue adds) errs by at most K 2^-24 S; the final
rounding to fp16 is 2^-11 relative (2^-25 absolute below the normal range); each term carries a factor of 2.

Inputs: magnitudes are log-uniform, 2^u with u in [-3, 3) (weights: / 8), so that tails, single large terms and small terms all occur.
Problems with K < 1024 draw random signs (cancellation: S >> |ref|).  From K = 1024 on every operand is positive, S = |ref|: with
random signs the accumulation term K 2^-23 S ~ K^2 of a long K exceeds the 2^-9 |ref| ~ sqrt(K) by which a result rounded through
bf16 differs, and the checker could not tell the two roundings apart (tests/test_gemm_routes.py shows on every case that it can).
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from tests.gemm_route_cases import EPI, STORE, VIEW_PAD, canon

U10, U21, U23, U24 = 2.0 ** -10, 2.0 ** -21, 2.0 ** -23, 2.0 ** -24
GELU_SLOPE = 1.13          # max |gelu'(x)| = 1.1289 (at x = sqrt(2))
# Error of the kernels' own erf, as an absolute error of gelu(x): cannot be derived from here.  Measured as `gelu_excess` below: the
# largest excess over the bound with GELU_ERR = 0, per unit of what the bound multiplies GELU_ERR by, over the table's GELU / GEGLU
# cases; GELU_ERR = twice that, or 0 when nothing exceeds.
# Measured 2026-10-19 on an MI355X with the parent commit's library (the one before the route queries): largest excess 0.0 over the
# 11 cases (t256 / t128 / p256 / p128 x -geglu, -ln-geglu; g3-plain-gelu, g3-plain-geglu-v1, -v0): no element exceeds, GELU_ERR = 0.
GELU_ERR = 0.0
LN_EPS = 1e-5


# ------------------------------------------------------------------------------------------------------------------- inputs
def _values(g, shape, signed, shift=0.0):
    mag = torch.exp2(torch.rand(shape, generator=g, dtype=torch.float64) * 6.0 - 3.0 + shift)
    if signed:
        mag = mag * (torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1)
    return mag.to(torch.float16)


def is_signed(o):
    return o["K"] < 1024


def inputs(c):
    """the case's operands as fp16 CPU tensors, from a generator seeded by the case's name"""
    o = canon(c)
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    sg, M, N, K = is_signed(o), o["M"], o["N"], o["K"]
    t = {}
    cv = o["conv"]
    if cv:
        t["x"] = _values(g, (cv["n"], cv["cin"], cv["h"], cv["w"]), sg)                       # NCHW here; the kernel gets NHWC
        t["w4"] = _values(g, (N, cv["cin"], 3, 3), sg, -3.0)
    else:
        k1 = o["a2"] if o["a2"] else K
        t["a"] = _values(g, (M, k1), sg)
        if o["a2"]:
            t["a2"] = _values(g, (M, K - k1), sg)
        t["w"] = _values(g, ((M // o["wstack"], N, K) if o["wstack"] else (N, K)), sg, -3.0)
    if o["bias"]:
        t["bias"] = _values(g, (N,), sg)
    if o["res"]:
        t["res"] = _values(g, (M, o["n_out"]), sg)
        if o["lo"]:
            t["res_lo"] = (_values(g, (M, o["n_out"]), True).float() * t["res"].float().abs() * 2.0 ** -14).to(torch.float16)
    if o["rowvec"] == "block":
        t["rowvec"] = _values(g, (M // o["rpv"], N), sg)
    elif o["rowvec"]:
        t["rowvec"] = _values(g, (N, o["rowvec"]) if o.get("rv_transposed") else (o["rowvec"], N), sg)
    if o["ln"]:
        t["wsum"] = t["w"].float().sum(dim=-1).contiguous()                                   # fp32 row sums of the fp16-rounded W'
    return t


# ------------------------------------------------------------------------------------------------------------------- the operation
def unpack_conv(wp, cin, taps=9):
    """[Cout, taps * Cin] in the kernel's contraction order (include/i2v_hip.h, conv_kblock) -> [Cout, Cin, taps]"""
    co = wp.shape[0]
    if cin % 64 == 0:
        return wp.reshape(co, cin // 64, taps, 64).permute(0, 1, 3, 2).reshape(co, cin, taps)
    return wp.reshape(co, taps, cin).permute(0, 2, 1)


def pack_conv(w3, cin, taps=9):
    """the inverse of unpack_conv"""
    co = w3.shape[0]
    if cin % 64 == 0:
        return w3.reshape(co, cin // 64, 64, taps).permute(0, 1, 3, 2).reshape(co, taps * cin)
    return w3.permute(0, 2, 1).reshape(co, taps * cin)


def _conv(o, x, w_packed, absolute=False):
    """the convolution of a case as [M, N] (rows (image, y, x)) from the PACKED weights the kernel reads"""
    cv = o["conv"]
    cin, N = cv["cin"], o["N"]
    if absolute:
        x, w_packed = x.abs(), w_packed.abs()
    if cv["up"] == 2:
        # four 2x2 convolutions of the source image, one per output parity; tap t = 2 ty + tx of phase (py, px) reads source pixel
        # (i + py - 1 + ty, j + px - 1 + tx): pad one row / column on the side the window reaches over
        out = x.new_zeros((cv["n"], N, cv["oh"], cv["ow"]))
        for ph in range(4):
            py, px = ph // 2, ph % 2
            w2 = unpack_conv(w_packed[ph], cin, 4).reshape(N, cin, 2, 2)
            xp = F.pad(x, (1 - px, px, 1 - py, py))
            out[:, :, py::2, px::2] = F.conv2d(xp, w2)
    else:
        w4 = unpack_conv(w_packed, cin).reshape(N, cin, 3, 3)
        if cv["up"]:
            x = F.interpolate(x, size=(cv["oh"], cv["ow"]), mode="nearest")
        if cv["asym"]:
            out = F.conv2d(F.pad(x, (0, 1, 0, 1)), w4, stride=2)
        else:
            out = F.conv2d(x, w4, stride=cv["stride"], padding=1)
    return out.permute(0, 2, 3, 1).reshape(o["M"], N)


def packed_weights(o, t):
    """the weight matrix as the kernel reads it, fp16: [N, K], [S, N, K] (stacked) or [4, N, 4 cin] (folded up-sampling)"""
    cv = o["conv"]
    if not cv:
        return t["w"]
    if cv["up"] == 2:
        from i2v_adapter_unofficial_amd.blocks import pack_upconv_fold
        return pack_upconv_fold(t["w4"].float())
    return pack_conv(t["w4"].reshape(o["N"], cv["cin"], 9), cv["cin"]).contiguous()


def _logical_a(o, t, dtype):
    a = t["a"].to(dtype)
    if o["a2"]:
        a = torch.cat([a, t["a2"].to(dtype)], dim=1)
    if o["a_perm"]:
        f, hw = o["a_perm"]
        a = a.view(-1, f, hw, a.shape[1]).permute(0, 2, 1, 3).reshape(o["M"], -1)
    return a


def _matmul(o, a, w):
    if o["wstack"]:
        return torch.bmm(a.view(w.shape[0], o["wstack"], -1), w.transpose(1, 2)).reshape(o["M"], o["N"])
    return a @ w.T


def _row_out(o):
    """physical row of logical row m for the row-permuted store (the residual is read in stored order, too)"""
    M, f, hw = o["M"], o["frames"], o["hw"]
    m = torch.arange(M)
    b, rem = m // (f * hw), m % (f * hw)
    return (b * f + rem % f) * hw + rem // f


def accumulate(o, t, dtype, wp=None, absolute=False, drop=()):
    """sum_k A[m, k] W[n, k] as [M, N] in `dtype`; drop = packed-K indices left out of the sum (the mutants)"""
    wp = packed_weights(o, t) if wp is None else wp
    w = wp.to(dtype)
    if drop:
        w = w.clone()
        w[..., list(drop)] = 0
    if o["conv"]:
        return _conv(o, t["x"].to(dtype), w, absolute)
    a = _logical_a(o, t, dtype)
    return _matmul(o, a.abs(), w.abs()) if absolute else _matmul(o, a, w)


def _addends(o, t, dtype, bias_shift=False):
    """bias + row vector + residual (+ its low half) as [M, N] terms in logical row order"""
    M, N = o["M"], o["N"]
    out = []
    if o["bias"]:
        b = t["bias"].to(dtype)
        out.append((torch.roll(b, 1) if bias_shift else b)[None, :].expand(M, N))
    if o["rowvec"] == "block":
        out.append(t["rowvec"].to(dtype).repeat_interleave(o["rpv"], dim=0))
    elif o["rowvec"]:
        tab = t["rowvec"].to(dtype)
        tab = tab.T if o.get("rv_transposed") else tab
        out.append(tab[torch.arange(M) % o["rowvec"]])
    if o["res"]:
        r = t["res"].to(dtype) + (t["res_lo"].to(dtype) if "res_lo" in t else 0)
        out.append(r[_row_out(o)] if o["store"] == "perm" else r)
    return out


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def evaluate(c, t, dtype=torch.float64, drop=(), bias_shift=False, swap_rows=False, with_bound=False):
    """the case's result [M, n_out] in `dtype`, before the final rounding, in logical row order; with_bound: (result, tolerance)
    -- the bound of this module's docstring with the form-specific terms below, evaluated beside the fp64 result.

    LayerNorm fold.  The kernel evaluates v = rstd (x.w' - mean wsum) + bias' (+ rowvec) with mean = sum x / K and
    var = sum x^2 / K - mean^2 from fp32 sums over the row.  Propagating the same terms: the dot product errs by K 2^-24 |x|.|w'|; the mean
    by K 2^-24 mean|x|, which wsum multiplies; so the bracket errs by K 2^-24 (|x|.|w'| + mean|x| |wsum|), times rstd.  The raw second
    moment errs by K 2^-24 E[x^2] and mean^2 by 2 |mean| K 2^-24 mean|x| <= 2 K 2^-24 E[x^2], so var errs by 3 K 2^-24 E[x^2] and
    rstd = (var + eps)^-1/2 by the relative 1.5 K 2^-24 E[x^2] / (var + eps) (+ 2^-23 of the reciprocal square root itself), which
    multiplies |pre| = |rstd (x.w' - mean wsum)|:
        S = rstd (|x|.|w'| + mean|x| |wsum|) + |pre| (1.5 E[x^2] / (var + eps) + 1) + |bias'| + |rowvec|
    The cancellation of x.w' against mean wsum shows up in S, where it belongs.

    GELU / GEGLU.  With d(x) = K 2^-23 S(x) the bound of a pre-activation x and |gelu'| <= 1.13: gelu(x) errs by 1.13 d(x) + GELU_ERR,
    and the GEGLU product v gelu(g) by |gelu(g)| d(v) + |v| (1.13 d(g) + GELU_ERR) + d(v) (1.13 d(g) + GELU_ERR), all times |out_scale|.
    """
    o = canon(c)
    K = o["K"]
    acc = accumulate(o, t, dtype, drop=drop)
    if with_bound:
        S = accumulate(o, t, dtype, absolute=True)
    if o["ln"]:
        x = _logical_a(o, t, dtype)
        mean, var = x.mean(dim=1, keepdim=True), x.var(dim=1, unbiased=False, keepdim=True)
        rstd = (var + LN_EPS) ** -0.5
        wsum = t["wsum"].to(dtype)[None, :]
        acc = rstd * (acc - mean * wsum)
        if with_bound:
            ex2 = (x * x).mean(dim=1, keepdim=True)
            S = rstd * (S + x.abs().mean(dim=1, keepdim=True) * wsum.abs()) + acc.abs() * (1.5 * ex2 / (var + LN_EPS) + 1.0)
    pre = acc
    for term in _addends(o, t, dtype, bias_shift):
        pre = pre + term
    if with_bound:
        for term in _addends(o, t, dtype):
            S = S + term.abs()
        d = K * U23 * S
    sc = o["out_scale"]
    if o["epi"] == "geglu":
        v, g = pre[:, 0::2], pre[:, 1::2]
        out = v * _gelu(g) * sc
        if with_bound:
            dv, dg = d[:, 0::2], GELU_SLOPE * d[:, 1::2] + GELU_ERR
            tol = abs(sc) * (_gelu(g).abs() * dv + v.abs() * dg + dv * dg)
    elif o["epi"] == "gelu":
        out = _gelu(pre) * sc
        if with_bound:
            tol = abs(sc) * (GELU_SLOPE * d + GELU_ERR)
    else:
        out = pre * sc
        if with_bound:
            tol = abs(sc) * d
    if swap_rows:
        out = out.clone()
        out[[o["M"] - 2, o["M"] - 1]] = out[[o["M"] - 1, o["M"] - 2]]
    if with_bound:
        return out, tol
    return out


@functools.lru_cache(maxsize=2)
def _reference(name):
    from tests.gemm_route_cases import CASES
    c = next(k for k in CASES if k["name"] == name)
    t = inputs(c)
    ref, tol = evaluate(c, t, torch.float64, with_bound=True)
    return t, ref, tol


def reference(c):
    """(inputs, fp64 reference [M, n_out], accumulation term of the bound) of a case, computed once and shared; read-only"""
    return _reference(c["name"])


def excess(got, ref, tol, rel=U10):
    """|got - ref| - (rel |ref| + tol + 2^-24) per element, fp64: positive where the bound is missed"""
    return (got.double() - ref).abs() - (rel * ref.abs() + tol + U24)


def check(c, got, got_lo=None):
    """None if the result [M, n_out] (logical row order; got_lo: its low half, hi + lo cases) obeys the bound, else a message"""
    _, ref, tol = reference(c)
    if tuple(got.shape) != tuple(ref.shape):
        return f"shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not bool(torch.isfinite(got.float()).all()):
        return "non-finite output"
    what = [("result", excess(got, ref, tol))]
    if got_lo is not None:
        what.append(("hi + lo", excess(got.double() + got_lo.double(), ref, tol, rel=U21)))
    for name, ex in what:
        bad = ex > 0
        if bool(bad.any()):
            m, n = [int(v) for v in bad.nonzero()[0]]
            return (f"{name}: {int(bad.sum())}/{bad.numel()} elements miss the bound, largest excess {float(ex.max()):.3e}; first at "
                    f"({m}, {n}): got {float(got[m, n]):.6g}, ref {float(ref[m, n]):.6g}, allowed {float(-ex[m, n] + (got[m, n].double() - ref[m, n]).abs()):.3e}")
    return None


def gelu_excess(c, got):
    """how GELU_ERR is measured: the largest excess of a GELU / GEGLU case's result over the bound evaluated with GELU_ERR = 0, per unit
    of what the bound multiplies GELU_ERR by (|value| |out_scale|; GELU: |out_scale|).  0.0 when nothing exceeds."""
    assert GELU_ERR == 0.0, "measure against the bound without the term"
    o = canon(c)
    t, ref, tol = reference(c)
    ex = excess(got, ref, tol)
    if o["epi"] == "geglu":
        pre = accumulate(o, t, torch.float64)
        if o["ln"]:
            x = _logical_a(o, t, torch.float64)
            mean, var = x.mean(dim=1, keepdim=True), x.var(dim=1, unbiased=False, keepdim=True)
            pre = (var + LN_EPS) ** -0.5 * (pre - mean * t["wsum"].double()[None, :])
        for term in _addends(o, t, torch.float64):
            pre = pre + term
        unit = pre[:, 0::2].abs() * abs(o["out_scale"])
    else:
        unit = torch.full_like(ref, abs(o["out_scale"]))
    return float((ex / unit.clamp_min(1e-30)).clamp_min(0).max())


# ------------------------------------------------------------------------------------------------------------------- through the wrappers
def _to_logical(o, out):
    """the wrapper's output tensor -> [M, n_out] in logical row order"""
    M, N = o["M"], o["N"]
    if o["conv"]:
        return out.reshape(M, N)
    if o["store"] == "perm":
        return out[_row_out(o).to(out.device)]
    if o["store"] == "vt":           # element (m, n) at [n / L][m][n % L]
        L = o["vt_len"]
        return out[:, :, :L].permute(1, 0, 2).reshape(M, N)
    if o["store"] == "vt_t":         # element (m, n) at [m / L][n][m % L]
        L = o["vt_len"]
        return out[:, :, :L].permute(0, 2, 1).reshape(M, N)
    return out


def run(kernels, dev, c, t, attach_workspace=True):
    """the case through kernels.gemm / conv3x3 / project_vt with real device pointers.  Returns a dict: out (logical [M, n_out], on the
    CPU), lo (its low half or None), route (kernels.last_gemm_route()), untouched (None, or whether everything outside the output view
    is still NaN: row-major / row-permuted stores write into a column slice of a wider NaN-filled matrix with one more NaN row block
    below), stats (GroupNorm partials) and raw (the wrapper's own output, on the device)."""
    o = canon(c)
    D = lambda x: None if x is None else x.to(dev)
    M, N, n_out = o["M"], o["N"], o["n_out"]
    res = {"lo": None, "untouched": None, "stats": None}
    real_attach = kernels._attach_splitk_workspace
    if not attach_workspace:
        kernels._attach_splitk_workspace = lambda lib, p, device: None
    try:
        if c["op"] == "conv":
            cv = o["conv"]
            x = D(t["x"].permute(0, 2, 3, 1).contiguous())
            wp = D(packed_weights(o, t))
            kw = dict(stride=cv["stride"], upsample=bool(cv["up"]), out_scale=o["out_scale"], asym_pad=bool(cv["asym"]), out_f32=bool(o["f32"]))
            if cv["up"] == 1 and (cv["oh"], cv["ow"]) != (2 * cv["h"], 2 * cv["w"]):
                kw["output_size"] = (cv["oh"], cv["ow"])
            if cv["up"] == 2:
                kw = dict(upsample=True, w_folded=wp)
                wp = None
            if o["rowvec"]:
                kw.update(rowvec=D(t["rowvec"]), rows_per_vec=o["rpv"])
            if o["res"]:
                r = D(t["res"].view(cv["n"], cv["oh"], cv["ow"], N))
                if "res_lo" in t:
                    r._i2v_lo = D(t["res_lo"].view(cv["n"], cv["oh"], cv["ow"], N))
                kw["residual"] = r
            if o["lo"]:
                kw["precise"] = True
            if o["gn"]:
                kw["gn_stats_groups"] = o["gn"]
            out = kernels.conv3x3(x, wp, D(t.get("bias")), **kw)
            if o["gn"]:
                out, res["stats"] = out
            raw = out
        elif c["op"] == "vt":
            kw = {}
            if o["ln"]:
                kw["ln"] = (D(t["wsum"]), LN_EPS)
            if c.get("pe"):
                kw.update(pe_t=D(t["rowvec"]), pe_period=c["pe"])
            if o["natural"]:
                raw = out = kernels.project_vt(D(t["a"]), D(t["w"]), c["L"], bias=D(t.get("bias")), **kw)
            else:                      # (swapped operand order: the tokens are the GEMM's W)
                raw = out = kernels.project_vt(D(t["w"]), D(t["a"]), c["L"])
        else:
            pad, nan = VIEW_PAD, float("nan")

            def view(x):       # views = 1: the operand as a column slice of a matrix 2 VIEW_PAD columns wider
                if not o["views"]:
                    return D(x)
                wide = torch.zeros((x.shape[0], x.shape[1] + 2 * pad), dtype=x.dtype, device=dev)
                wide[:, pad: pad + x.shape[1]] = D(x)
                return wide[:, pad: pad + x.shape[1]]
            kw = dict(epilogue=EPI[o["epi"]], store=STORE[o["store"]], frames=o["frames"], hw=o["hw"], out_scale=o["out_scale"])
            a = view(t["a"])
            if o["a2"]:
                kw["a2"] = D(t["a2"])
            if o["res"]:
                r = view(t["res"])
                if "res_lo" in t:
                    r._i2v_lo = view(t["res_lo"])
                kw["residual"] = r
            if o["rowvec"]:
                kw["rowvec"] = D(t["rowvec"])
                kw.update(dict(rows_per_vec=o["rpv"]) if o["rowvec"] == "block" else dict(rowvec_period=o["rowvec"]))
            if o["ln"]:
                kw["ln"] = (D(t["wsum"]), LN_EPS)
            if o["wstack"]:
                kw["w_rows"] = o["wstack"]
            if o["a_perm"]:
                kw["a_perm"] = o["a_perm"]
            wide = None
            if o["store"] in ("vt", "vt_t"):
                L = o["vt_len"]
                ld = (L + 7) // 8 * 8
                tokens, chans = (N, M) if o["store"] == "vt" else (M, N)
                kw.update(vt_len=L, vt_ld=ld, out=torch.zeros((tokens // L, chans, ld), dtype=torch.float16, device=dev))
            elif not o["lo"]:
                # untouched memory: the output is a column slice of a wider NaN matrix, one more NaN row block (256 rows) below it
                wide = torch.full((M + 256, n_out + 2 * pad), nan, dtype=torch.float16, device=dev)
                kw["out"] = wide[:M, pad: pad + n_out]
            if o["lo"]:
                kw["precise"] = True
            raw = out = kernels.gemm(a, D(t["w"]), D(t.get("bias")), **kw)
            if wide is not None:
                probe = wide.clone()
                probe[:M, pad: pad + n_out] = nan
                res["untouched"] = bool(torch.isnan(probe).all())
        res["route"] = kernels.last_gemm_route()
    finally:
        kernels._attach_splitk_workspace = real_attach
    lo = kernels.lo_of(raw)
    res["raw"] = raw
    res["out"] = _to_logical(o, raw).cpu()
    if o["lo"]:
        assert lo is not None
        res["lo"] = _to_logical(o, lo).cpu()
    return res
