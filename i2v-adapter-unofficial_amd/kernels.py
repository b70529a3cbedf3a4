"""Tensor-level wrappers over the C ABI (include/i2v_hip.h).

PyTorch is used only for device memory and the stream: every function validates its operands on the host
(shape / dtype / contiguity, so a kernel never sees shapes its grid does not assume), allocates the output with
torch.empty and launches the HIP kernel on torch's current stream through ctypes.  Nothing here computes with
torch ops and nothing falls back to the CPU: a CPU tensor or a missing library raises.
"""
import ctypes as C
import functools
import os
from typing import Optional

import torch

from . import _lib
from ._lib import (I2V_A_CONV3X3, I2V_A_PLAIN, I2V_EPI_GEGLU, I2V_EPI_GELU, I2V_EPI_NONE, I2V_STORE_ROWMAJOR,
                   I2V_STORE_ROWPERM, I2V_STORE_VT, I2V_STORE_VT_T, AttnBwdParams, AttnParams, GemmParams, GnParams,
                   HipLibraryError, LnParams, TAttnParams)

f16 = torch.float16


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t: torch.Tensor, name: str, dtype=f16):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise HipLibraryError(f"{name} is on {t.device}: the I2V-Adapter HIP path has no CPU fallback "
                              "(move tensors to a ROCm device)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t


def _mat(t: torch.Tensor, name: str):
    """2-D fp16 matrix whose rows are unit-stride; returns (tensor, leading dimension)."""
    _req(t, name)
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{name} must have unit stride along its last dim")
    ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
    return t, ld


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------- the precise residual stream
# (i2v_gemm_params.residual_lo / c_lo)  The stream between the UNet's modules as an fp16 pair: the tensor every kernel
# reads as before (hi) carries its low half -- the bits its fp16 rounding dropped -- as an attribute.  A producer called with
# `precise=True` adds the residual's low half (when the residual has one) and attaches the result's.
def lo_of(t):
    """the low half that travels with a stream tensor, or None"""
    return None if t is None else getattr(t, "_i2v_lo", None)


def sview(t, *shape):
    """t.view(*shape) that keeps the low half attached"""
    v, lo = t.view(*shape), lo_of(t)
    if lo is not None:
        v._i2v_lo = lo.view(*shape)
    return v


def _attach_lo(p_res_lo_setter, residual, out):
    """(residual's low half or None after checking it is laid out like the residual, fresh low half for `out`)"""
    rl = lo_of(residual)
    if rl is not None and (rl.shape != residual.shape or rl.stride() != residual.stride() or rl.dtype != f16):
        raise ValueError("the low half of a stream tensor must be laid out like the tensor")
    cl = torch.empty_like(out)
    if cl.stride() != out.stride():
        raise ValueError("precise stream: `out` must be dense")
    p_res_lo_setter(rl, cl)
    out._i2v_lo = cl
    return rl, cl


# ---------------------------------------------------------------------------------------------- GEMM / conv
def gemm(a, w, bias=None, *, a2=None, residual=None, rowvec=None, rows_per_vec=0, epilogue=I2V_EPI_NONE,
         out=None, store=I2V_STORE_ROWMAJOR, frames=0, hw=0, vt_len=0, vt_ld=0, out_scale=1.0, ln=None,
         rowvec_period=0, query_ln_support=False, w_rows=0, a_perm=None, query_batch_support=False, precise=False):
    """C = epi(A W^T + bias + rowvec + residual) * out_scale   (see i2v_gemm_f16).

    precise: the result is a tensor of the precise residual stream -- its low half is written beside it (`lo_of(out)`), and the
    residual's low half, if it has one, is added with it (row-major / row-permuted plain stores only).

    w may be a stack [S, N, K] of weight matrices with w_rows = rows of A per matrix (GroupNorm folded into proj_in,
    groupnorm_fold).  a_perm = (frames, hw): A's rows are (batch, frame, pixel) and are read as (batch, pixel, frame).
    query_batch_support=True launches nothing and returns whether the library implements those two for this problem.

    ln = (wsum fp32 [N], eps): LayerNorm of A's rows folded into the GEMM (w = W o gamma, bias = W beta + b; the row
    statistics are computed inside the kernel; see i2v_gemm_params.ln_wsum).  rowvec_period > 0: rowvec row = m % period (with a VT_T store the
    table is passed transposed, [N, >= period]).  query_ln_support=True launches nothing and returns whether the library
    implements the fold for exactly this problem."""
    lib = _lib.load()
    a, lda = _mat(a, "a")
    w_stack = None
    if w.dim() == 3:
        _req(w, "w")
        if w_rows <= 0 or not w.is_contiguous() or a.shape[0] != w.shape[0] * w_rows:
            raise ValueError(f"stacked w {tuple(w.shape)} needs contiguous storage and w_rows with S * w_rows == M")
        w_stack, w = w, w[0]
    w, ldw = _mat(w, "w")
    M, K1 = a.shape
    N, K = w.shape
    p = GemmParams()
    if w_stack is not None:
        p.w_batch_stride, p.rows_per_w = w_stack.stride(0), w_rows
    if a_perm is not None:
        p.a_perm_frames, p.a_perm_hw = int(a_perm[0]), int(a_perm[1])
    p.a, p.lda = _p(a), lda
    if a2 is not None:
        a2, lda2 = _mat(a2, "a2")
        if a2.shape[0] != M or K1 + a2.shape[1] != K:
            raise ValueError(f"dual-source A shapes {tuple(a.shape)} + {tuple(a2.shape)} do not match W {tuple(w.shape)}")
        p.a2, p.lda2, p.k_split = _p(a2), lda2, K1
    elif K1 != K:
        raise ValueError(f"A is {tuple(a.shape)} but W is {tuple(w.shape)}")
    p.a_mode = I2V_A_PLAIN
    p.w, p.ldw = _p(w), ldw
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != N or not bias.is_contiguous():
            raise ValueError("bias must be a contiguous vector of N elements")
        p.bias = _p(bias)
    n_out = N // 2 if epilogue == I2V_EPI_GEGLU else N
    if store in (I2V_STORE_VT, I2V_STORE_VT_T):
        tokens, chans = (N, M) if store == I2V_STORE_VT else (M, N)
        if out is None or vt_len <= 0 or vt_ld < vt_len or tokens % vt_len != 0:
            raise ValueError("VT store needs an `out` buffer, vt_len > 0, vt_ld >= vt_len and tokens % vt_len == 0")
        _req(out, "out")
        if not out.is_contiguous() or out.numel() < (tokens // vt_len) * chans * vt_ld:
            raise ValueError("VT `out` must be contiguous with at least (tokens / vt_len) * channels * vt_ld elements")
        p.c, p.ldc = _p(out), vt_ld
        p.vt_len, p.vt_ld = vt_len, vt_ld
    else:
        if out is None:
            out = torch.empty((M, n_out), dtype=f16, device=a.device)
        out, ldc = _mat(out, "out")
        if out.shape != (M, n_out):
            raise ValueError(f"out must be {(M, n_out)}, got {tuple(out.shape)}")
        p.c, p.ldc = _p(out), ldc
    if residual is not None:
        residual, ldr = _mat(residual, "residual")
        if residual.shape != (M, n_out) or epilogue == I2V_EPI_GEGLU:
            raise ValueError(f"residual must be {(M, n_out)} (and is not supported with GEGLU)")
        p.residual, p.ldr = _p(residual), ldr
    if rowvec is not None:
        rowvec, ldv = _mat(rowvec, "rowvec")
        if rowvec_period > 0:
            want = (N, rowvec_period) if store == I2V_STORE_VT_T else (rowvec_period, N)
            if rowvec.shape[0] < want[0] or rowvec.shape[1] < want[1] or (store != I2V_STORE_VT_T and rowvec.shape[1] != N):
                raise ValueError(f"periodic rowvec must cover {want}, got {tuple(rowvec.shape)}")
            p.rowvec, p.ld_rowvec, p.rowvec_period = _p(rowvec), ldv, rowvec_period
        else:
            if rows_per_vec <= 0 or M % rows_per_vec != 0 or rowvec.shape != (M // rows_per_vec, N):
                raise ValueError(f"rowvec must be [M / rows_per_vec, N], got {tuple(rowvec.shape)}")
            p.rowvec, p.ld_rowvec, p.rows_per_vec = _p(rowvec), ldv, rows_per_vec
    if ln is not None:
        wsum, eps = ln
        _req(wsum, "ln wsum", dtype=torch.float32)
        if wsum.numel() != N or not wsum.is_contiguous() or a2 is not None:
            raise ValueError(f"ln = (wsum fp32 [N], eps) with a single-source A expected, got {tuple(wsum.shape)}")
        p.ln_wsum, p.ln_eps = _p(wsum), float(eps)
    p.M, p.N, p.K = M, N, K
    p.epilogue, p.store_mode = epilogue, store
    p.frames, p.hw = frames, hw
    p.out_scale = out_scale
    if query_ln_support:
        return bool(lib.i2v_gemm_ln_supported(C.byref(p)))
    if query_batch_support:
        return bool(lib.i2v_gemm_batch_supported(C.byref(p)))
    keep = None
    if precise:
        if epilogue != I2V_EPI_NONE or store not in (I2V_STORE_ROWMAJOR, I2V_STORE_ROWPERM) or ln is not None:
            raise ValueError("precise=True needs a plain row-major / row-permuted store")

        def set_lo(rl, cl):
            p.residual_lo, p.c_lo = _p(rl), _p(cl)
        keep = _attach_lo(set_lo, residual, out)
    ws = _attach_splitk_workspace(lib, p, a.device)
    _lib.check(lib.i2v_gemm_f16(C.byref(p), _stream()), "i2v_gemm_f16")
    del ws, keep
    return out


def _attach_splitk_workspace(lib, p, device):
    """Small-M / long-K problems split K over workgroups; the fp32 partial tiles live in a caller-owned scratch."""
    need = lib.i2v_gemm_workspace_bytes(C.byref(p))
    if need <= 0:
        return None
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=device)
    p.workspace, p.workspace_bytes = _p(ws), need
    return ws


def last_gemm_route() -> dict:
    """the kernel instantiation that this thread's most recent `gemm` / `conv3x3` / `project_vt` launch took, as the fields of
    i2v_gemm_route (family, a_mode, rows, cols, stages, splits, kps, extra, persistent, generic_tile, vec4, epilogue, store_mode)"""
    r = _lib.GemmRoute()
    _lib.check(_lib.load().i2v_gemm_last_route(C.byref(r)), "i2v_gemm_last_route")
    return r.as_dict()


def conv_k_block(cin: int) -> int:
    """contraction order of the 3x3 convolution for this (padded) channel count: 64 = channel-block-major (the 9 taps
    of a 64-channel block are consecutive, i2v_gemm_params.conv_kblock), 0 = tap-major.  `blocks.pack_conv3x3` lays the
    weights out by the same rule."""
    return 64 if cin % 64 == 0 and os.environ.get("I2V_CONV_KBLOCK", "1") != "0" else 0


def _upconv_fold_params(p, n, h, wd, cin, cout):
    """the fields of the folded up-sampling convolution (i2v_gemm_params.upsample = 2): four phase matrices [Cout, 4 Cin]"""
    p.a_mode, p.lda = I2V_A_CONV3X3, cin
    p.M, p.N, p.K, p.ldw, p.ldc = 4 * n * h * wd, cout, 4 * cin, 4 * cin, cout
    p.epilogue, p.store_mode, p.out_scale = I2V_EPI_NONE, I2V_STORE_ROWMAJOR, 1.0
    p.n_img, p.in_h, p.in_w, p.cin = n, h, wd, cin
    p.out_h, p.out_w, p.stride, p.upsample = 2 * h, 2 * wd, 1, 2
    p.conv_kblock = conv_k_block(cin)
    p.w_batch_stride, p.rows_per_w = cout * 4 * cin, n * h * wd


@functools.lru_cache(maxsize=None)
def _upconv_fold_query(n, h, wd, cin, cout, kblock):
    p = GemmParams()
    _upconv_fold_params(p, n, h, wd, cin, cout)
    p.a = p.w = p.c = p.bias = 1 << 40          # (a query tests pointers for null and alignment only)
    return bool(_lib.load().i2v_gemm_upconv_fold_supported(C.byref(p)))


def upconv_fold_supported(x_shape, cout):
    """whether the library runs the up-sampling convolution of a token-major image of shape x_shape = (N, H, W, Cin) to Cout
    channels in the folded form (`conv3x3(..., w_folded=)`: four taps per output parity instead of nine); launches nothing"""
    n, h, wd, cin = (int(v) for v in x_shape)
    return _upconv_fold_query(n, h, wd, cin, int(cout), conv_k_block(cin))


def conv3x3(x, w_packed, bias=None, *, stride=1, upsample=False, rowvec=None, rows_per_vec=0, residual=None,
            out_scale=1.0, asym_pad=False, out_f32=False, gn_stats_groups=0, precise=False, output_size=None, w_folded=None):
    """3x3 / pad 1 convolution of a token-major image x [N, H, W, Cin] with w_packed [Cout, 9 * Cin]
    (k ordered as `blocks.pack_conv3x3` lays it out: tap-major, or channel-block-major when Cin % 64 == 0, see
    conv_k_block); optional nearest-2x upsampling of the input first.  asym_pad (stride 2): no
    padding at the top / left, one zero row / column at the bottom / right (the VAE encoder's Downsample2D(padding=0)).
    out_f32: the result stays fp32 (narrow outputs only, Cout <= 64: the UNet's conv_out feeding the DDIM / CFG kernel).
    gn_stats_groups > 0: returns (out, stats) -- stats = the GroupNorm statistics of `out` over that many channel groups as
    partials written by the convolution's epilogue (i2v_gemm_params.gn_partial), to hand to `groupnorm(out, ..., stats=stats)`,
    or None where the epilogue form is not implemented for this problem (the norm then runs its own statistics pass).
    precise: as `gemm` (the result and the residual are tensors of the precise residual stream).
    output_size (upsample only): (2 H, 2 W) or one less in either dimension -- `F.interpolate(size=output_size, mode="nearest")`
    in front of the convolution, the reference's forward_upsample_size path for latent sizes that are not multiples of 8
    (unet:1304-1311, 1414-1415).
    w_folded (upsample only, exactly 2x, bias only): [4, Cout, 4 * Cin] from `blocks.pack_upconv_fold` -- the up-sampling folded
    into the weights, one 2x2 convolution of the source image per output parity (i2v_gemm_params.upsample = 2); w_packed is then
    not read.  Ask `upconv_fold_supported` first: a problem the library does not take in this form is an error."""
    lib = _lib.load()
    _req(x, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"x must be a contiguous [N, H, W, C] tensor, got {tuple(x.shape)}")
    n, h, wd, cin = x.shape
    if w_folded is not None:
        if (not upsample or stride != 1 or asym_pad or rowvec is not None or residual is not None or out_scale != 1.0 or out_f32
                or gn_stats_groups or precise):
            raise ValueError("w_folded belongs to a plain up-sampling convolution (bias only)")
        if output_size is not None and tuple(int(v) for v in output_size) != (2 * h, 2 * wd):
            raise ValueError(f"w_folded: the folded form up-samples to exactly {(2 * h, 2 * wd)}, not {tuple(output_size)}")
        _req(w_folded, "w_folded")
        cout = w_folded.shape[1] if w_folded.dim() == 3 else 0
        if tuple(w_folded.shape) != (4, cout, 4 * cin) or not w_folded.is_contiguous():
            raise ValueError(f"w_folded must be a contiguous [4, Cout, {4 * cin}] tensor, got {tuple(w_folded.shape)}")
        out = torch.empty((n, 2 * h, 2 * wd, cout), dtype=f16, device=x.device)
        p = GemmParams()
        _upconv_fold_params(p, n, h, wd, cin, cout)
        p.a, p.w, p.c = _p(x), _p(w_folded), _p(out)
        if bias is not None:
            _req(bias, "bias")
            if bias.numel() != cout or not bias.is_contiguous():
                raise ValueError("bias must be a contiguous vector of Cout elements")
            p.bias = _p(bias)
        _lib.check(lib.i2v_gemm_f16(C.byref(p), _stream()), "i2v_gemm_f16(conv3x3, folded up-sampling)")
        return out
    w_packed, ldw = _mat(w_packed, "w_packed")
    cout, K = w_packed.shape
    if K != 9 * cin:
        raise ValueError(f"w_packed is {tuple(w_packed.shape)} but x has {cin} channels")
    if asym_pad and (stride != 2 or upsample):
        raise ValueError("asym_pad needs stride 2 and no upsampling")
    if upsample:
        if stride != 1:
            raise ValueError("upsample conv must have stride 1")
        oh, ow = 2 * h, 2 * wd
        if output_size is not None:
            oh, ow = int(output_size[0]), int(output_size[1])
            if oh not in (2 * h, 2 * h - 1) or ow not in (2 * wd, 2 * wd - 1):
                raise NotImplementedError(f"upsample to {(oh, ow)} from {(h, wd)}: only 2x and 2x - 1 (a level that was odd before its "
                                          "stride-2 down-sampler) occur on the UNet's path")
    else:
        if output_size is not None:
            raise ValueError("output_size belongs to an upsampling convolution")
        padsum = 1 if asym_pad else 2
        oh, ow = (h + padsum - 3) // stride + 1, (wd + padsum - 3) // stride + 1
    M = n * oh * ow
    if out_f32 and (cout > 64 or residual is not None):
        raise ValueError("out_f32 is for narrow outputs (Cout <= 64) without a residual")
    out = torch.empty((n, oh, ow, cout), dtype=torch.float32 if out_f32 else f16, device=x.device)
    p = GemmParams()
    p.c_is_f32 = 1 if out_f32 else 0
    p.a, p.lda = _p(x), cin
    p.a_mode = I2V_A_CONV3X3
    p.w, p.ldw = _p(w_packed), ldw
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != cout or not bias.is_contiguous():
            raise ValueError("bias must be a contiguous vector of Cout elements")
        p.bias = _p(bias)
    if residual is not None:
        _req(residual, "residual")
        if tuple(residual.shape) != (n, oh, ow, cout) or not residual.is_contiguous():
            raise ValueError(f"residual must be contiguous {(n, oh, ow, cout)}")
        p.residual, p.ldr = _p(residual), cout
    if rowvec is not None:
        rowvec, ldv = _mat(rowvec, "rowvec")
        if rows_per_vec <= 0 or M % rows_per_vec != 0 or rowvec.shape != (M // rows_per_vec, cout):
            raise ValueError(f"rowvec must be [M / rows_per_vec, Cout], got {tuple(rowvec.shape)}")
        p.rowvec, p.ld_rowvec, p.rows_per_vec = _p(rowvec), ldv, rows_per_vec
    p.c, p.ldc = _p(out), cout
    p.M, p.N, p.K = M, cout, K
    p.epilogue, p.store_mode = I2V_EPI_NONE, I2V_STORE_ROWMAJOR
    p.out_scale = out_scale
    p.n_img, p.in_h, p.in_w, p.cin = n, h, wd, cin
    p.out_h, p.out_w, p.stride, p.upsample = oh, ow, stride, 1 if upsample else 0
    p.asym_pad = 1 if asym_pad else 0
    p.conv_kblock = conv_k_block(cin)
    keep = None
    if precise:
        if out_f32 or gn_stats_groups:
            raise ValueError("precise=True is an fp16 result without GroupNorm partials")

        def set_lo(rl, cl):
            p.residual_lo, p.c_lo = _p(rl), _p(cl)
        keep = _attach_lo(set_lo, residual, out)
    ws = _attach_splitk_workspace(lib, p, x.device)
    stats = None
    if gn_stats_groups:
        p.gn_groups = int(gn_stats_groups)
        # (asked with the split-K workspace attached: a problem that splits K keeps doing so -- its partial tiles have no epilogue
        #  of their own -- and the norm runs its statistics pass)
        rows = lib.i2v_gemm_gn_partial_rows(C.byref(p))
        if rows > 0:
            part = torch.empty((n, (oh * ow) // rows, int(gn_stats_groups), 2), dtype=torch.float32, device=x.device)
            p.gn_partial = _p(part)
            stats = (part, rows)
    _lib.check(lib.i2v_gemm_f16(C.byref(p), _stream()), "i2v_gemm_f16(conv3x3)")
    del ws, keep
    return (out, stats) if gn_stats_groups else out


def pack_conv_c64(weight: torch.Tensor) -> torch.Tensor:
    """[64, Cin <= 64, 3, 3] -> the 36864 fp16 of `conv3x3_c64`'s weight in the kernel's MFMA-fragment order (include/i2v_hip.h,
    i2v_conv_c64_params.w): Cin zero-padded to 64,
        packed[tap, s, b, 16 g + l, j] = W[32 (b >> 1) + 8 (l >> 2) + 4 (b & 1) + (l & 3), 32 s + 8 g + j, tap]."""
    co, ci = weight.shape[:2]
    if co != 64 or ci > 64 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"pack_conv_c64 takes a [64, <= 64, 3, 3] weight, got {tuple(weight.shape)}")
    w = torch.nn.functional.pad(weight.detach().reshape(64, ci, 9), (0, 0, 0, 64 - ci))       # [cout, cin, tap]
    # cout = 32 bh + 8 q + 4 bl + e, cin = 32 s + 8 g + j  ->  [tap, s, (bh, bl), (g, (q, e)), j]
    w = w.reshape(2, 4, 2, 4, 2, 4, 8, 9)                                                      # [bh, q, bl, e, s, g, j, tap]
    return w.permute(7, 4, 0, 2, 5, 1, 3, 6).reshape(-1).to(f16).contiguous()


def _pixel_stride(t, name):
    """pixel stride of a token-major fp16 image view [N, H, W, C] whose pixels are `ld` elements apart and otherwise dense"""
    _req(t, name)
    if t.dim() != 4:
        raise ValueError(f"{name} must be [N, H, W, C], got {tuple(t.shape)}")
    n, h, w, c = t.shape
    ld = t.stride(2) if w > 1 else (t.stride(1) if h > 1 else (t.stride(0) // (h * w) if n > 1 else max(c, t.stride(2))))
    if t.stride(3) != 1 or (w > 1 and t.stride(2) != ld) or (h > 1 and t.stride(1) != w * ld) or (n > 1 and t.stride(0) != h * w * ld):
        raise ValueError(f"{name} must be a token-major image with one pixel stride, got strides {t.stride()}")
    return ld


def conv3x3_c64(x, w_packed, bias=None, *, relu_mid=False, relu_out=False, residual=None, out=None, max_workgroups=None, slope=None):
    """out = act_out(act_mid(conv3x3(x) + bias) + residual): the 64 -> 64, stride 1, pad 1 convolution of AutoencoderTiny with its
    epilogue in one launch (i2v_conv3x3_c64_f16).  x, out, residual: token-major fp16 [N, H, W, 64] views with a pixel stride >= 64
    (a multiple of 8); w_packed from `pack_conv_c64`; bias fp16 [64].  `out` may be `residual`, never `x`.  max_workgroups caps the
    persistent grid (a dispatch override, like the library's other ones: the result does not depend on it).
    slope (fp32 [64]): act_mid is the per-channel PReLU v >= 0 ? v : slope[c] v instead (i2v_conv3x3_c64_prelu_f16, the layer of
    `upscaler.SRVGGNetCompact`); relu_mid must then be False."""
    lib = _lib.load()
    ldx = _pixel_stride(x, "x")
    n, h, wd, c = x.shape
    _req(w_packed, "w_packed")
    if w_packed.numel() != 9 * 64 * 64 or not w_packed.is_contiguous():
        raise ValueError(f"w_packed must be the {9 * 64 * 64} values of pack_conv_c64, got {tuple(w_packed.shape)}")
    if out is None:
        out = torch.empty((n, h, wd, c), dtype=f16, device=x.device)
    ldo = _pixel_stride(out, "out")
    if tuple(out.shape) != (n, h, wd, c):
        raise ValueError(f"out must be {(n, h, wd, c)}, got {tuple(out.shape)}")
    p = _lib.ConvC64Params()
    p.x, p.ldx, p.w, p.out, p.ldo = _p(x), ldx, _p(w_packed), _p(out), ldo
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != c or not bias.is_contiguous():
            raise ValueError("bias must be a contiguous vector of Cout elements")
        p.bias = _p(bias)
    if residual is not None:
        p.ldr = _pixel_stride(residual, "residual")
        if tuple(residual.shape) != (n, h, wd, c):
            raise ValueError(f"residual must be {(n, h, wd, c)}, got {tuple(residual.shape)}")
        p.residual = _p(residual)
    p.n_img, p.height, p.width, p.cin, p.cout = n, h, wd, c, c
    p.relu_mid, p.relu_out = int(bool(relu_mid)), int(bool(relu_out))
    p.max_workgroups = 0 if max_workgroups is None else int(max_workgroups)
    if max_workgroups is not None and p.max_workgroups < 1:
        raise ValueError(f"max_workgroups must be positive, got {max_workgroups}")
    if slope is not None:
        _req(slope, "slope", dtype=torch.float32)
        if slope.numel() != 64 or not slope.is_contiguous():
            raise ValueError("slope must be a contiguous fp32 vector of 64 elements")
        _lib.check(lib.i2v_conv3x3_c64_prelu_f16(C.byref(p), _p(slope), _stream()), "i2v_conv3x3_c64_prelu_f16")
        return out
    _lib.check(lib.i2v_conv3x3_c64_f16(C.byref(p), _stream()), "i2v_conv3x3_c64_f16")
    return out


def conv3x3_c64_up2(x, w_packed, bias, slope, *, out=None, max_workgroups=None):
    """out = prelu(conv3x3(nearest_2x(x)) + bias; slope) without the upsampled tensor (i2v_conv3x3_c64_up2_prelu_f16): the 64-channel
    kernel's halo fetch reads source pixel (y >> 1, x >> 1).  x: token-major fp16 [N, H, W, 64] view; out: [N, 2 H, 2 W, 64];
    w_packed from `pack_conv_c64`; bias fp16 [64] or None; slope fp32 [64]."""
    lib = _lib.load()
    ldx = _pixel_stride(x, "x")
    n, h, wd, c = x.shape
    _req(w_packed, "w_packed")
    if w_packed.numel() != 9 * 64 * 64 or not w_packed.is_contiguous():
        raise ValueError(f"w_packed must be the {9 * 64 * 64} values of pack_conv_c64, got {tuple(w_packed.shape)}")
    if out is None:
        out = torch.empty((n, 2 * h, 2 * wd, c), dtype=f16, device=x.device)
    ldo = _pixel_stride(out, "out")
    if tuple(out.shape) != (n, 2 * h, 2 * wd, c):
        raise ValueError(f"out must be {(n, 2 * h, 2 * wd, c)}, got {tuple(out.shape)}")
    p = _lib.ConvC64Params()
    p.x, p.ldx, p.w, p.out, p.ldo = _p(x), ldx, _p(w_packed), _p(out), ldo
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != c or not bias.is_contiguous():
            raise ValueError("bias must be a contiguous vector of Cout elements")
        p.bias = _p(bias)
    p.n_img, p.height, p.width, p.cin, p.cout = n, 2 * h, 2 * wd, c, c
    p.max_workgroups = 0 if max_workgroups is None else int(max_workgroups)
    if max_workgroups is not None and p.max_workgroups < 1:
        raise ValueError(f"max_workgroups must be positive, got {max_workgroups}")
    _req(slope, "slope", dtype=torch.float32)
    if slope.numel() != 64 or not slope.is_contiguous():
        raise ValueError("slope must be a contiguous fp32 vector of 64 elements")
    _lib.check(lib.i2v_conv3x3_c64_up2_prelu_f16(C.byref(p), _p(slope), _stream()), "i2v_conv3x3_c64_up2_prelu_f16")
    return out


DENSE_CIN = (64, 96, 128, 160, 192)
DENSE_TILE = (16, 16)          # the dense kernel's output tile (rows, columns): the tests' sizes are built on it


def pack_conv_dense(weight: torch.Tensor) -> torch.Tensor:
    """[Cout in (32, 64), Cin in DENSE_CIN, 3, 3] -> the 9 Cin Cout fp16 of `conv3x3_dense`'s weight in the kernel's MFMA-fragment
    order (include/i2v_hip.h, i2v_conv_dense_params.w), 32 output channels after 32:
        packed[half, chunk, tap, b, 16 g + l, j] = W[32 half + 8 (l >> 2) + 4 b + (l & 3), 32 chunk + 8 g + j, tap]."""
    co, ci = weight.shape[:2]
    if co not in (32, 64) or ci not in DENSE_CIN or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"pack_conv_dense takes a [32 | 64, {' | '.join(map(str, DENSE_CIN))}, 3, 3] weight, got {tuple(weight.shape)}")
    # cout = 32 half + 8 q + 4 b + e, cin = 32 chunk + 8 g + j  ->  [half, chunk, tap, b, (g, (q, e)), j]
    w = weight.detach().reshape(co // 32, 4, 2, 4, ci // 32, 4, 8, 9)                         # [half, q, b, e, chunk, g, j, tap]
    return w.permute(0, 4, 7, 2, 5, 1, 3, 6).reshape(-1).to(f16).contiguous()


def conv3x3_dense(buf, cin, w_packed, bias=None, *, out, slope=0.2, s1=1.0, r1=None, s2=1.0, r2=None, max_workgroups=None):
    """out = fp16(s2 (s1 lrelu(conv3x3(buf[..., :cin]) + bias; slope) + r1) + r2): a layer of an RRDBNet dense block in one launch
    (i2v_conv3x3_dense_f16).  buf: token-major fp16 [N, H, W, >= cin] view (pixel stride a multiple of 8) of which only channels
    < cin are read; cin in DENSE_CIN; w_packed from `pack_conv_dense` (Cout = numel / (9 cin): 32 or 64); bias fp16 [Cout];
    out, r1, r2: [N, H, W, Cout] views.  out may be other channels of buf's pixels (`buf[..., cin: cin + 32]`: the block's
    concatenation is never built) and may be r1 or r2; any other overlap is refused.  slope 1: no activation.  max_workgroups caps
    the persistent grid and never changes the result."""
    lib = _lib.load()
    ldx = _pixel_stride(buf, "buf")
    n, h, wd, c = buf.shape
    cin = int(cin)
    if cin not in DENSE_CIN:
        raise ValueError(f"cin must be one of {DENSE_CIN}, got {cin}")
    if c < cin:
        raise ValueError(f"buf has {c} channels, fewer than cin {cin}")
    _req(w_packed, "w_packed")
    cout = w_packed.numel() // (9 * cin)
    if cout not in (32, 64) or w_packed.numel() != 9 * cin * cout or not w_packed.is_contiguous():
        raise ValueError(f"w_packed must be the 9 x {cin} x (32 | 64) values of pack_conv_dense, got {tuple(w_packed.shape)}")
    p = _lib.ConvDenseParams()
    p.x, p.ldx, p.w = _p(buf), ldx, _p(w_packed)
    for name, t in (("out", out), ("r1", r1), ("r2", r2)):
        if t is None:
            continue
        ld = _pixel_stride(t, name)
        if tuple(t.shape) != (n, h, wd, cout) or t.device != buf.device:
            raise ValueError(f"{name} must be {(n, h, wd, cout)} on buf's device, got {tuple(t.shape)}")
        if name == "out":
            p.out, p.ldo = _p(t), ld
        elif name == "r1":
            p.r1, p.ldr1 = _p(t), ld
        else:
            p.r2, p.ldr2 = _p(t), ld
    if out is None:
        raise ValueError("out is required (a view of the block's buffer, or of the next block's)")
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != cout or not bias.is_contiguous():
            raise ValueError("bias must be a contiguous vector of Cout elements")
        p.bias = _p(bias)
    p.n_img, p.height, p.width, p.cin, p.cout = n, h, wd, cin, cout
    p.slope, p.s1, p.s2 = float(slope), float(s1), float(s2)
    p.max_workgroups = 0 if max_workgroups is None else int(max_workgroups)
    if max_workgroups is not None and p.max_workgroups < 1:
        raise ValueError(f"max_workgroups must be positive, got {max_workgroups}")
    _lib.check(lib.i2v_conv3x3_dense_f16(C.byref(p), _stream()), "i2v_conv3x3_dense_f16")
    return out


def rgb_exit(y, *, clamp=True, signed_out=False, out=None):
    """RRDBNet's exit (i2v_rgb_exit_f32): y token-major fp16 [N, H, W, >= 3] view -> fp32 NCHW [N, 3, H, W] of channels 0..2, clamped
    to [0, 1] (clamp), then 2 v - 1 (signed_out)."""
    lib = _lib.load()
    ld = _pixel_stride(y, "y")
    n, h, w, c = y.shape
    if c < 3:
        raise ValueError(f"y must have at least 3 channels, got {c}")
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=y.device)
    _req(out, "out", dtype=torch.float32)
    if tuple(out.shape) != (n, 3, h, w) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {(n, 3, h, w)}, got {tuple(out.shape)}")
    _lib.check(lib.i2v_rgb_exit_f32(_p(y), ld, _p(out), n, h, w, int(bool(clamp)), int(bool(signed_out)), _stream()), "i2v_rgb_exit_f32")
    return out


TAESD_PREP_MODES = {"identity": _lib.I2V_TAESD_PREP_IDENTITY, "unit": _lib.I2V_TAESD_PREP_UNIT, "clamp": _lib.I2V_TAESD_PREP_CLAMP,
                    "unit_clamp": _lib.I2V_TAESD_PREP_UNIT_CLAMP}


def taesd_prep(src, mode="identity", out=None):
    """AutoencoderTiny's entry mover (i2v_taesd_prep_f16): src [N, C <= 64, H, W] fp32 / fp16 through `mode` -- "identity",
    "unit" (v + 1) / 2, "clamp" 3 tanh(v / 3), "unit_clamp" min(max((v + 1) / 2, 0), 1) (the upscaler's) -- to token-major fp16
    [N, H, W, 64] with channels C.. zero."""
    lib = _lib.load()
    _req(src, "src", dtype=None)
    if src.dtype not in (torch.float32, f16) or src.dim() != 4:
        raise TypeError("src must be a 4-D fp32 / fp16 tensor")
    if mode not in TAESD_PREP_MODES:
        raise ValueError(f"mode must be one of {sorted(TAESD_PREP_MODES)}, got {mode!r}")
    src = src.contiguous()
    n, c, h, w = src.shape
    if out is None:
        out = torch.empty((n, h, w, 64), dtype=f16, device=src.device)
    ld = _pixel_stride(out, "out")
    if tuple(out.shape) != (n, h, w, 64):
        raise ValueError(f"out must be {(n, h, w, 64)}, got {tuple(out.shape)}")
    _lib.check(lib.i2v_taesd_prep_f16(_p(src), 1 if src.dtype == torch.float32 else 0, _p(out), ld, n, c, h * w, TAESD_PREP_MODES[mode],
                                      _stream()), "i2v_taesd_prep_f16")
    return out


def pixel_shuffle_add(y, src, s, *, unit_in=False, clamp=True, signed_out=False, out=None):
    """The upscaler's exit (i2v_pixel_shuffle_add_f32): out[n, col, s i + dy, s j + dx] = range(clamp(y[n, i, j, (col s + dy) s + dx] +
    entry(src[n, col, i, j]))), PixelShuffle(s) of the exit convolution's result plus the nearest-upsampled source.  y: token-major
    fp16 [N, H, W, 64] view (pixel stride >= 64, a multiple of 8) of which channels < 3 s^2 are read; src: contiguous NCHW [N, 3, H, W]
    fp32 / fp16 BEFORE the entry map, which is the identity or, with unit_in, `taesd_prep`'s "unit_clamp"; clamp: to [0, 1];
    signed_out: 2 v - 1 after it.  s in 1..4.  Returns fp32 [N, 3, s H, s W] (`out`: a contiguous tensor of that shape)."""
    lib = _lib.load()
    ld = _pixel_stride(y, "y")
    n, h, w, c = y.shape
    _req(src, "src", dtype=None)
    if src.dtype not in (torch.float32, f16) or tuple(src.shape) != (n, 3, h, w) or not src.is_contiguous() or src.device != y.device:
        raise ValueError(f"src must be a contiguous fp32 / fp16 {(n, 3, h, w)} on y's device, got {src.dtype} {tuple(src.shape)}")
    s = int(s)
    if c != 64:
        raise ValueError(f"y must have 64 channels, got {c}")
    if out is None:
        out = torch.empty((n, 3, s * h, s * w), dtype=torch.float32, device=y.device)
    _req(out, "out", dtype=torch.float32)
    if tuple(out.shape) != (n, 3, s * h, s * w) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {(n, 3, s * h, s * w)}, got {tuple(out.shape)}")
    mode = _lib.I2V_TAESD_PREP_UNIT_CLAMP if unit_in else _lib.I2V_TAESD_PREP_IDENTITY
    _lib.check(lib.i2v_pixel_shuffle_add_f32(_p(y), ld, _p(src), 1 if src.dtype == torch.float32 else 0, _p(out), n, h, w, s, mode,
                                             int(bool(clamp)), int(bool(signed_out)), _stream()), "i2v_pixel_shuffle_add_f32")
    return out


def project_vt(tokens, w_v, batch_len, out=None, bias=None, ln=None, pe_t=None, pe_period=0, query_ln_support=False):
    """V^T[batch][channel][key] = (tokens W_v^T)^T, emitted directly by the GEMM epilogue (I2V_STORE_VT).
    tokens [batches * batch_len, K]; w_v [C, K]; returns [batches, C, pad8(batch_len)] (tail keys unwritten).
    ln / bias / pe_t: LayerNorm(+positional table, transposed [C, >= pe_period]) folded into the projection (see gemm)."""
    tokens, _ = _mat(tokens, "tokens")
    T = tokens.shape[0]
    if T % batch_len != 0:
        raise ValueError(f"{T} tokens are not a multiple of batch_len {batch_len}")
    ld = pad8(batch_len)
    Cc = w_v.shape[0]
    natural = Cc % 320 == 0 and batch_len % 4 == 0 and T >= 8192
    if out is None:
        out = torch.empty((T // batch_len, Cc, ld), dtype=f16, device=tokens.device)
    if query_ln_support:
        return natural and gemm(tokens, w_v, bias, store=I2V_STORE_VT_T, vt_len=batch_len, vt_ld=ld, ln=ln, rowvec=pe_t,
                                rowvec_period=pe_period, out=out, query_ln_support=True)
    if natural:
        # natural operand order (A = tokens): eligible for the 256-row LDS-DMA tile kernel, which transposes in its
        # MFMA operand order (I2V_STORE_VT_T)
        gemm(tokens, w_v, bias, store=I2V_STORE_VT_T, vt_len=batch_len, vt_ld=ld, out=out, ln=ln, rowvec=pe_t,
             rowvec_period=pe_period)
    else:
        if ln is not None or pe_t is not None or bias is not None:
            raise ValueError("the LayerNorm-folded V^T projection needs the natural operand order "
                             "(C % 320 == 0, batch_len % 4 == 0, >= 8192 tokens)")
        gemm(w_v, tokens, store=I2V_STORE_VT, vt_len=batch_len, vt_ld=ld, out=out)
    return out



# ---------------------------------------------------------------------------------------------- attention
def attention(q, k, vt, *, batch_q, lq, lk, heads, head_dim, kv_group=1, scale=None, out=None, accumulate=False,
              acc_scale=1.0, return_lse=False):
    """Flash attention forward.  q [batch_q * lq, >= heads*head_dim] (row-strided view is fine),
    k [batch_kv * lk, ...], vt [batch_kv, heads*head_dim, >= pad8(lk)], returns [batch_q * lq, heads*head_dim]
    return_lse: the pair (out, fp32 [batch_q, heads, lq] log2-sum-exp of the scaled logits): what attention_bwd otherwise
    recomputes.  True: the statistic of the logits the backward recomputes (attention_lse, a second launch).  "fused": the one
    the forward kernel writes in the same pass; it belongs to the kernel's own logits (Q scaled and rounded to fp16 before
    Q K^T) and is off by up to ~1e-3 of max|lse|: a backward fed with it recomputes rows of P that sum to 2^(-error), not 1."""
    lib = _lib.load()
    q, ldq = _mat(q, "q")
    k, ldk = _mat(k, "k")
    _req(vt, "vt")
    Cc = heads * head_dim
    bkv = batch_q // kv_group
    if q.shape[0] != batch_q * lq or q.shape[1] < Cc:
        raise ValueError(f"q is {tuple(q.shape)}, expected [{batch_q * lq}, >={Cc}]")
    if k.shape[0] != bkv * lk or k.shape[1] < Cc:
        raise ValueError(f"k is {tuple(k.shape)}, expected [{bkv * lk}, >={Cc}]")
    if vt.dim() != 3 or not vt.is_contiguous() or vt.shape[0] != bkv or vt.shape[1] != Cc or vt.shape[2] < pad8(lk):
        raise ValueError(f"vt is {tuple(vt.shape)}, expected contiguous [{bkv}, {Cc}, >={pad8(lk)}]")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs the `out` tensor holding the previous result")
        out = torch.empty((batch_q * lq, Cc), dtype=f16, device=q.device)
    out, ldo = _mat(out, "out")
    if out.shape[0] != batch_q * lq or out.shape[1] < Cc:
        raise ValueError("bad `out` shape")
    p = AttnParams()
    p.q, p.q_row_stride, p.q_batch_stride = _p(q), ldq, lq * ldq
    p.k, p.k_row_stride, p.k_batch_stride = _p(k), ldk, lk * ldk
    p.vt, p.vt_row_stride, p.vt_batch_stride = _p(vt), vt.shape[2], Cc * vt.shape[2]
    p.o, p.o_row_stride, p.o_batch_stride = _p(out), ldo, lq * ldo
    p.batch_q, p.kv_group, p.heads, p.head_dim, p.lq, p.lk = batch_q, kv_group, heads, head_dim, lq, lk
    p.scale = float(head_dim) ** -0.5 if scale is None else scale
    p.accumulate, p.acc_scale = 1 if accumulate else 0, acc_scale
    lse = None
    if return_lse:
        if accumulate:
            raise ValueError("return_lse is not combined with accumulate")
        if return_lse == "fused":
            lse = torch.empty((batch_q, heads, lq), dtype=torch.float32, device=q.device)
            p.lse = _p(lse)
        elif return_lse is not True:
            raise ValueError(f"return_lse must be False, True or 'fused', got {return_lse!r}")
    _lib.check(lib.i2v_attention_f16(C.byref(p), _stream()), "i2v_attention_f16")
    if return_lse and lse is None:
        lse = attention_lse(q, k, batch_q=batch_q, lq=lq, lk=lk, heads=heads, head_dim=head_dim, kv_group=kv_group, scale=p.scale)
    return (out, lse) if return_lse else out


def attn_route(batch_q, kv_group, heads, head_dim, lq, lk) -> dict:
    """the kernel `attention` takes for these sizes and its launch, as the fields of i2v_attn_route (dqk, dpv, spare, qt, kvt, walk,
    qbw, grid_x, grid_y, grid_z, remap): host arithmetic, no GPU"""
    r = _lib.AttnRoute()
    _lib.check(_lib.load().i2v_attention_route(batch_q, kv_group, heads, head_dim, lq, lk, C.byref(r)), "i2v_attention_route")
    return r.as_dict()


def last_attn_route() -> dict:
    """the route of this thread's most recent `attention` launch"""
    r = _lib.AttnRoute()
    _lib.check(_lib.load().i2v_attention_last_route(C.byref(r)), "i2v_attention_last_route")
    return r.as_dict()


def temporal_attention(q, k, vt, *, n_pixels, frames, heads, head_dim, scale=None, out=None):
    """Motion-module attention over the frame axis; tokens in (b, pixel, frame) order.
    q, k [n_pixels * frames, >= C]; vt [n_pixels, C, >= pad8(frames)].
    out: optional 2-D fp16 view [n_pixels * frames, >= C] to write into (columns [0, C); row stride a multiple of 4, base 8-byte
    aligned); by default a new [n_pixels * frames, C] tensor."""
    lib = _lib.load()
    q, ldq = _mat(q, "q")
    k, ldk = _mat(k, "k")
    _req(vt, "vt")
    Cc = heads * head_dim
    if q.shape[0] != n_pixels * frames or k.shape[0] != n_pixels * frames or q.shape[1] < Cc or k.shape[1] < Cc:
        raise ValueError("q / k must be [n_pixels * frames, >= C]")
    if vt.dim() != 3 or not vt.is_contiguous() or vt.shape[0] != n_pixels or vt.shape[1] != Cc or \
            vt.shape[2] < pad8(frames):
        raise ValueError(f"vt is {tuple(vt.shape)}, expected contiguous [{n_pixels}, {Cc}, >={pad8(frames)}]")
    if out is None:
        out, ldo = torch.empty((n_pixels * frames, Cc), dtype=f16, device=q.device), Cc
    else:
        out, ldo = _mat(out, "out")
        if out.shape[0] != n_pixels * frames or out.shape[1] < Cc or ldo % 4 != 0 or out.device != q.device:
            raise ValueError(f"out is {tuple(out.shape)} with row stride {ldo}, expected [{n_pixels * frames}, >={Cc}] on {q.device} "
                             "with a row stride that is a multiple of 4")
    p = TAttnParams()
    p.q, p.q_row_stride = _p(q), ldq
    p.k, p.k_row_stride = _p(k), ldk
    p.vt, p.vt_ld = _p(vt), vt.shape[2]
    p.o, p.o_row_stride = _p(out), ldo
    p.n_pixels, p.frames, p.heads, p.head_dim = n_pixels, frames, heads, head_dim
    p.scale = float(head_dim) ** -0.5 if scale is None else scale
    _lib.check(lib.i2v_temporal_attention_f16(C.byref(p), _stream()), "i2v_temporal_attention_f16")
    return out


def last_tattn_route() -> dict:
    """the kernel instantiation that this thread's most recent `temporal_attention` launch took, as the fields of i2v_tattn_route
    (form, dqk, dpv, pf, nqt, blocks)"""
    r = _lib.TAttnRoute()
    _lib.check(_lib.load().i2v_temporal_attention_last_route(C.byref(r)), "i2v_temporal_attention_last_route")
    return r.as_dict()


def attn_bwd_route(batch_q, kv_group, heads, head_dim, lq, lk, need_dkv=True) -> dict:
    """the kernels `attention_bwd` / `attention_lse` take for these sizes, as the fields of i2v_attn_bwd_route (ks, dt, dq_form,
    dkv_form, lse_form, kv_partitions, dq_blocks, dkv_blocks): host arithmetic, no GPU"""
    r = _lib.AttnBwdRoute()
    _lib.check(_lib.load().i2v_attention_bwd_route(batch_q, kv_group, heads, head_dim, lq, lk, int(need_dkv), C.byref(r)),
               "i2v_attention_bwd_route")
    return r.as_dict()


def last_attn_bwd_route() -> dict:
    """the kernels that this thread's most recent `attention_bwd` launch took, with the kv_partitions it ran with and the lse_form
    of this thread's most recent `attention_lse` (-1 before one)"""
    r = _lib.AttnBwdRoute()
    _lib.check(_lib.load().i2v_attention_bwd_last_route(C.byref(r)), "i2v_attention_bwd_last_route")
    return r.as_dict()


def motion_attn_supported(rows, channels, heads, head_dim, frames):
    """is the fused LayerNorm + q / k / v + temporal attention kernel implemented for this shape?"""
    return bool(_lib.load().i2v_motion_attn_supported(rows, channels, heads, head_dim, frames))


def _pack_head_fragments(weights, heads):
    """per head the rows of each weight, zero-padded to a multiple of 16 rows, in MFMA-fragment order
    [heads][parts][C / 32][pad16(d) / 16][lane = 16 (k chunk) + row][8] (returned as [rows, C])."""
    c_out, c_in = weights[0].shape
    d = c_out // heads
    dp = (d + 15) // 16 * 16
    n = len(weights)
    w = torch.zeros((heads, n, dp, c_in), dtype=f16, device=weights[0].device)
    for i, t in enumerate(weights):
        w[:, i, :d] = t.detach().to(f16).view(heads, d, c_in)
    w = w.view(heads, n, dp // 16, 16, c_in // 32, 4, 8).permute(0, 1, 4, 2, 5, 3, 6)      # [h, part, s, t, g, l15, 8]
    return w.contiguous().view(heads * n * dp, c_in)


def pack_motion_qkv(wq, wk, wv, heads):
    """`w_qkv` of i2v_motion_attn_f16: per head its rows of Wq, Wk, Wv in fragment order (`_pack_head_fragments`)."""
    w = _pack_head_fragments((wq, wk, wv), heads)
    if w.shape[0] != _lib.load().i2v_motion_attn_pack_rows(heads, wq.shape[0] // heads):
        raise RuntimeError("pack_motion_qkv: row count differs from i2v_motion_attn_pack_rows")
    return w


def pack_cross_q(wq, heads):
    """`w_q` of i2v_cross_attn_fused_f16: per head its rows of to_q in fragment order."""
    w = _pack_head_fragments((wq,), heads)
    if w.shape[0] != _lib.load().i2v_cross_attn_fused_pack_rows(heads, wq.shape[0] // heads):
        raise RuntimeError("pack_cross_q: row count differs from i2v_cross_attn_fused_pack_rows")
    return w


def cross_attn_fused_supported(rows, channels, heads, head_dim, ctx_len, rows_per_ctx):
    """is the fused LayerNorm + to_q + cross-attention kernel implemented for this shape?"""
    return bool(_lib.load().i2v_cross_attn_fused_supported(rows, channels, heads, head_dim, ctx_len, rows_per_ctx))


def pack_ctx_fragments(k, vt, heads, ctx_len, out=None):
    """`ctx_frag` of i2v_cross_attn_fused_f16 from the projected context as the other kernels take it -- k [n_ctx * ctx_len, C],
    vt [n_ctx, C, >= ctx_len] (V^T) -- as MFMA operand fragments [n_ctx][heads][30][64][4], zero beyond the context's length
    and the head's width (i2v_pack_ctx_fragments_f16; once per prompt with a `ProjectedContext`, else once per forward).
    `out`: a previous result to overwrite in place (a captured hipGraph keeps reading that memory for the next prompt)."""
    lib = _lib.load()
    k, ldk = _mat(k, "k")
    _req(vt, "vt")
    if vt.dim() != 3 or vt.stride(2) != 1:
        raise ValueError(f"pack_ctx_fragments: vt must be [n_ctx, C, >= ctx_len] with unit stride along the keys, got {tuple(vt.shape)}")
    n_ctx, c = vt.shape[0], vt.shape[1]
    d = c // heads
    dt, kt_n = (d + 15) // 16, 5
    if ctx_len > 16 * kt_n or k.shape[0] != n_ctx * ctx_len or k.shape[1] < c or vt.shape[2] < ctx_len or c % heads:
        raise ValueError(f"pack_ctx_fragments: k {tuple(k.shape)} / vt {tuple(vt.shape)} / ctx_len {ctx_len}")
    shape = (n_ctx, heads, 2 * kt_n * dt, 64, 4)
    if n_ctx * heads * 2 * kt_n * dt * 256 != lib.i2v_cross_attn_fused_ctx_elems(n_ctx, heads, d):
        raise RuntimeError("pack_ctx_fragments: size differs from i2v_cross_attn_fused_ctx_elems")
    if out is None:
        out = torch.empty(shape, dtype=f16, device=k.device)
    elif tuple(out.shape) != shape or out.dtype != f16 or not out.is_contiguous():
        raise ValueError(f"pack_ctx_fragments: out is {tuple(out.shape)}, expected {shape}")
    _lib.check(lib.i2v_pack_ctx_fragments_f16(_p(k), ldk, _p(vt), vt.stride(1), vt.stride(0), _p(out), n_ctx, heads, d, ctx_len,
                                              _stream()), "i2v_pack_ctx_fragments_f16")
    return out


def pack_attn_out(w_o, b_o, heads):
    """(w_o fragments, b_o fp32) of the out-projection inside i2v_motion_attn_f16 / i2v_cross_attn_fused_f16: to_out[0].weight's
    rows per head-sized slice in fragment order (the layout of `pack_cross_q`), the bias in fp32."""
    return pack_cross_q(w_o, heads), b_o.detach().float().contiguous()


def _attn_out_operands(out_proj, c, heads, head_dim, what):
    w_o, b_o = out_proj
    _req(w_o, "w_o")
    _req(b_o, "b_o", dtype=torch.float32)
    if tuple(w_o.shape) != (_lib.load().i2v_cross_attn_fused_pack_rows(heads, head_dim), c) or not w_o.is_contiguous() or \
            b_o.numel() != c or not b_o.is_contiguous():
        raise ValueError(f"{what}: out_proj is {tuple(w_o.shape)} / {tuple(b_o.shape)} (pack_attn_out)")
    return _p(w_o), _p(b_o)


def cross_attn_fused(x, gamma32, beta32, w_q, ctx_frag, *, heads, head_dim, ctx_len, rows_per_ctx, eps, scale=None, out=None,
                     ip_frag=None, ip_len=0, ip_scale=1.0, out_proj=None):
    """o = softmax((LayerNorm(x) Wq^T) K^T) V against a short context (i2v_cross_attn_fused_f16): x [rows, C]; ctx_frag from
    `pack_ctx_fragments`; rows [i * rows_per_ctx, (i + 1) * rows_per_ctx) use context i.  ip_frag (+ ip_len <= 16, ip_scale):
    the IP-Adapter's image tokens packed the same way; their softmax is added with weight ip_scale."""
    lib = _lib.load()
    x, ldx = _mat(x, "x")
    rows, c = x.shape
    _req(w_q, "w_q")
    _req(ctx_frag, "ctx_frag")
    for name, t in (("gamma32", gamma32), ("beta32", beta32)):
        _req(t, name, dtype=torch.float32)
        if tuple(t.shape) != (c,):
            raise ValueError(f"cross_attn_fused: {name} is {tuple(t.shape)}, expected ({c},)")
    n_ctx = -(-rows // rows_per_ctx)
    if c != heads * head_dim or not ctx_frag.is_contiguous() or \
            ctx_frag.numel() != lib.i2v_cross_attn_fused_ctx_elems(n_ctx, heads, head_dim):
        raise ValueError(f"cross_attn_fused: ctx_frag is {tuple(ctx_frag.shape)} for {n_ctx} contexts (pack_ctx_fragments)")
    if tuple(w_q.shape) != (lib.i2v_cross_attn_fused_pack_rows(heads, head_dim), c) or not w_q.is_contiguous():
        raise ValueError(f"cross_attn_fused: w_q is {tuple(w_q.shape)} (pack_cross_q)")
    if out is None:
        out = torch.empty((rows, c), dtype=f16, device=x.device)
    out, ldo = _mat(out, "out")
    p = _lib.CrossAttnFusedParams()
    p.x, p.ldx = _p(x), ldx
    p.gamma, p.beta, p.w_q = _p(gamma32), _p(beta32), _p(w_q)
    p.ctx_frag = _p(ctx_frag)
    p.out, p.ldo = _p(out), ldo
    p.rows, p.rows_per_ctx = rows, rows_per_ctx
    p.channels, p.heads, p.head_dim, p.ctx_len = c, heads, head_dim, ctx_len
    p.eps, p.scale = float(eps), float(head_dim) ** -0.5 if scale is None else float(scale)
    if ip_frag is not None:
        _req(ip_frag, "ip_frag")
        if not ip_frag.is_contiguous() or ip_frag.numel() != ctx_frag.numel():
            raise ValueError(f"cross_attn_fused: ip_frag is {tuple(ip_frag.shape)} (pack_ctx_fragments of the image tokens)")
        p.ip_frag, p.ip_len, p.ip_scale = _p(ip_frag), int(ip_len), float(ip_scale)
    if out_proj is not None:      # out = x + o Wo^T + bo in the same launch (`pack_attn_out`)
        p.w_o, p.b_o = _attn_out_operands(out_proj, c, heads, head_dim, "cross_attn_fused")
    _lib.check(lib.i2v_cross_attn_fused_f16(C.byref(p), _stream()), "i2v_cross_attn_fused_f16")
    return out


def ln_qkv_supported(rows, channels, n_qk, rows_per_image):
    """is the one-launch LayerNorm + [q | k | q_adapter] + V^T projection implemented for this shape?"""
    return bool(_lib.load().i2v_ln_qkv_supported(rows, channels, n_qk, rows_per_image))


def pack_ln_qkv(w_qk, w_v):
    """`w` of i2v_ln_qkv_f16: the rows of [w_qk ; w_v] per 16-row tile in fragment order [tile][C / 32][lane][8]."""
    w = torch.cat([w_qk.detach().to(f16), w_v.detach().to(f16)], dim=0)
    n, c = w.shape
    if n % 160 or c % 32:
        raise ValueError(f"pack_ln_qkv: {n} rows x {c} columns is not whole waves of 160 rows / K steps of 32")
    return w.view(n // 16, 16, c // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(n, c)     # [tile, s, g, l15, j]


def ln_qkv(x, gamma32, beta32, w_packed, *, n_qk, rows_per_image, eps, qk=None, vt=None, images=None, x_image_stride=0):
    """(qk [rows, n_qk], vt [rows / rows_per_image, C, pad8(rows_per_image)]) = projections of LayerNorm(x) in one launch
    (i2v_ln_qkv_f16); w_packed = `pack_ln_qkv(w_qk, w_v)`.  images / x_image_stride: only `images` blocks of rows_per_image rows
    of x are taken, block i starting at row i * x_image_stride / ldx (the frame-0 rows of every clip, read in place)."""
    lib = _lib.load()
    x, ldx = _mat(x, "x")
    rows, c = x.shape
    if images is not None:
        if x_image_stride % ldx or (images - 1) * (x_image_stride // ldx) + rows_per_image > rows:
            raise ValueError(f"ln_qkv: {images} images of {rows_per_image} rows at stride {x_image_stride} do not fit x {tuple(x.shape)}")
        rows = images * rows_per_image
    _req(w_packed, "w")
    for name, t in (("gamma32", gamma32), ("beta32", beta32)):
        _req(t, name, dtype=torch.float32)
    if tuple(gamma32.shape) != (c,) or tuple(beta32.shape) != (c,) or tuple(w_packed.shape) != (n_qk + c, c) or \
            not w_packed.is_contiguous():
        raise ValueError(f"ln_qkv: gamma {tuple(gamma32.shape)}, beta {tuple(beta32.shape)}, w {tuple(w_packed.shape)} for C {c}, "
                         f"n_qk {n_qk} (pack_ln_qkv)")
    if rows % rows_per_image:
        raise ValueError(f"ln_qkv: {rows} rows are not whole images of {rows_per_image}")
    n_img, ld = rows // rows_per_image, pad8(rows_per_image)
    if qk is None:
        qk = torch.empty((rows, n_qk), dtype=f16, device=x.device)
    if vt is None:
        vt = torch.empty((n_img, c, ld), dtype=f16, device=x.device)
    qk, ld_qk = _mat(qk, "qk")
    _req(vt, "vt")
    if tuple(qk.shape) != (rows, n_qk) or tuple(vt.shape) != (n_img, c, ld) or not vt.is_contiguous():
        raise ValueError(f"ln_qkv: qk {tuple(qk.shape)}, vt {tuple(vt.shape)}")
    p = _lib.LnQkvParams()
    p.x, p.ldx = _p(x), ldx
    p.gamma, p.beta, p.w = _p(gamma32), _p(beta32), _p(w_packed)
    p.qk, p.ld_qk = _p(qk), ld_qk
    p.vt, p.vt_batch_stride, p.vt_row_stride = _p(vt), c * ld, ld
    p.rows, p.rows_per_image, p.channels, p.n_qk, p.eps = rows, rows_per_image, c, n_qk, float(eps)
    p.x_image_stride = int(x_image_stride) if images is not None else 0
    _lib.check(lib.i2v_ln_qkv_f16(C.byref(p), _stream()), "i2v_ln_qkv_f16")
    return qk, vt


def ff_fused_supported(rows, channels, inner):
    """is the one-launch GEGLU feed-forward implemented for this shape?"""
    return bool(_lib.load().i2v_ff_fused_supported(rows, channels, inner))


def pack_ff_fused(w1, b1, w2, b2):
    """(w1 fragments, b1 fp32, w2 fragments, b2 fp32) of i2v_ff_fused_f16 from diffusers' GEGLU.proj (w1 [2 inner, C], rows
    [values ; gates]) and the output Linear (w2 [C, inner]); layouts in include/i2v_hip.h."""
    inner, c = w2.shape[1], w2.shape[0]
    nch, heads, dn = inner // 128, 8, c // 8
    dt = (dn + 15) // 16
    dev = w1.device
    # W1 rows of tile (ch, w, u): m = 0 .. 15 -> (m & 1) * inner + 128 ch + 16 w + 8 u + (m >> 1)
    m = torch.arange(16, device=dev)
    idx = ((m & 1) * inner + (m >> 1))[None, None, None, :] + (128 * torch.arange(nch, device=dev))[:, None, None, None] + \
        (16 * torch.arange(8, device=dev))[None, :, None, None] + (8 * torch.arange(2, device=dev))[None, None, :, None]   # [nch, 8, 2, 16]
    t1 = w1.detach().to(f16)[idx.reshape(-1)].view(nch, 8, 2, 16, c // 32, 4, 8)                      # [ch, w, u, l15, s, g, j]
    w1f = t1.permute(0, 1, 2, 4, 5, 3, 6).contiguous().view(-1, 8)                                     # [ch, w, u, s, g, l15, j]
    b1f = b1.detach().float()[idx.reshape(-1)].view(nch, 8, 2, 16).contiguous()
    w2p = torch.zeros((heads, 16 * dt, inner), dtype=f16, device=dev)
    w2p[:, :dn] = w2.detach().to(f16).view(heads, dn, inner)
    t2 = w2p.view(heads, dt, 16, nch, 4, 4, 8)                                                         # [w, t, l15, ch, ks, g, j]
    w2f = t2.permute(0, 3, 4, 1, 5, 2, 6).contiguous().view(-1, 8)                                     # [w, ch, ks, t, g, l15, j]
    return w1f, b1f, w2f, b2.detach().float().contiguous()


def ff_fused_tail_supported(rows, channels, inner, perm_frames=0, perm_hw=0):
    """... and with the Linear that follows the block in the same launch (`tail=` of ff_fused)?"""
    return bool(_lib.load().i2v_ff_fused_tail_supported(rows, channels, inner, perm_frames, perm_hw))


def pack_ff_tail(w3, b3):
    """(w3 fragments, b3 fp32) of the tail of i2v_ff_fused_f16: the [C, C] Linear per 40-row slice in fragment order."""
    return pack_cross_q(w3, 8), b3.detach().float().contiguous()


def ff_fused(x, gamma32, beta32, packed, *, eps, out=None, tail=None, precise=False):
    """out = x + GEGLU-FF(LayerNorm(x)) in one launch (i2v_ff_fused_f16); packed = `pack_ff_fused(...)`.
    tail = (packed_tail, res2, perm_frames, perm_hw): the block's proj_out in the same launch --
    out[perm(r)] = res2[perm(r)] + (x + FF(LN(x)))[r] W3^T + b3, packed_tail = `pack_ff_tail(w3, b3)`; perm_frames > 0: rows are
    in (batch, pixel, frame) order and leave in (batch, frame, pixel) order (res2 is read in that order too).
    precise (with a tail whose res2 carries a low half, `lo_of`): res2 + its low half is added and the result's low half is written."""
    lib = _lib.load()
    x, ldx = _mat(x, "x")
    rows, c = x.shape
    w1f, b1f, w2f, b2f = packed
    inner = b1f.numel() // 2
    for name, t, dt_ in (("gamma32", gamma32, torch.float32), ("beta32", beta32, torch.float32), ("w1", w1f, f16),
                         ("b1", b1f, torch.float32), ("w2", w2f, f16), ("b2", b2f, torch.float32)):
        _req(t, name, dtype=dt_)
    if tuple(gamma32.shape) != (c,) or tuple(beta32.shape) != (c,) or b2f.numel() != c or w1f.numel() != 2 * inner * c or \
            w2f.numel() != 8 * ((c // 8 + 15) // 16 * 16) * inner:
        raise ValueError(f"ff_fused: operand sizes do not match C {c}, inner {inner} (pack_ff_fused)")
    if out is None:
        out = torch.empty((rows, c), dtype=f16, device=x.device)
    out, ldo = _mat(out, "out")
    if tuple(out.shape) != (rows, c):
        raise ValueError(f"ff_fused: out is {tuple(out.shape)}")
    p = _lib.FfFusedParams()
    p.x, p.ldx = _p(x), ldx
    p.gamma, p.beta = _p(gamma32), _p(beta32)
    p.w1, p.b1, p.w2, p.b2 = _p(w1f), _p(b1f), _p(w2f), _p(b2f)
    p.out, p.ldo = _p(out), ldo
    p.rows, p.channels, p.inner, p.eps = rows, c, inner, float(eps)
    keep = None
    if tail is not None:
        (w3f, b3f), res2, perm_frames, perm_hw = tail
        _req(w3f, "w3")
        _req(b3f, "b3", dtype=torch.float32)
        res2, ld2 = _mat(res2, "res2")
        if tuple(w3f.shape) != (8 * ((c // 8 + 15) // 16 * 16), c) or not w3f.is_contiguous() or b3f.numel() != c or \
                tuple(res2.shape) != (rows, c):
            raise ValueError(f"ff_fused: tail operands w3 {tuple(w3f.shape)}, b3 {tuple(b3f.shape)}, res2 {tuple(res2.shape)} "
                             f"do not match rows {rows}, C {c} (pack_ff_tail)")
        if perm_frames and out.data_ptr() == x.data_ptr():
            raise ValueError("ff_fused: out must not alias x when the tail permutes the rows")
        p.w3, p.b3, p.res2, p.ld_res2 = _p(w3f), _p(b3f), _p(res2), ld2
        p.perm_frames, p.perm_hw = int(perm_frames), int(perm_hw)
        if precise and lo_of(res2) is not None:
            def set_lo(rl, cl):
                p.res2_lo, p.out_lo = _p(rl), _p(cl)
            keep = _attach_lo(set_lo, res2, out)
    _lib.check(lib.i2v_ff_fused_f16(C.byref(p), _stream()), "i2v_ff_fused_f16")
    del keep
    return out


def motion_attn_tables(gamma, beta, pe, frames):
    """(gamma fp32 [C], shift fp32 [frames, C] = beta + pe[frame]): the LayerNorm constants of i2v_motion_attn_f16."""
    return (gamma.detach().float().contiguous(),
            (beta.detach().float()[None, :] + pe.detach().float()[:frames]).contiguous())


def motion_attn_wide_supported(rows, channels, heads, head_dim, frames):
    """is the 64-row-tile form of the fused motion attention sub-block (C = 640, to_out + residual inside) implemented for this shape?"""
    return bool(_lib.load().i2v_motion_attn_wide_supported(rows, channels, heads, head_dim, frames))


def motion_attn_wide(x, gamma32, shift32, w_qkv, *, heads, head_dim, frames, eps, out_proj, scale=None, out=None):
    """x + to_out(temporal attention of LayerNorm(x) + pe) at the 32^2 level (i2v_motion_attn_wide_f16): the arguments of
    `motion_attn`, `out_proj` (`pack_attn_out`) required.  (Goes through `motion_attn`, so a KernelProfile times and tags it like the
    64^2 launch -- `motion_attn 32768x640 F16 h8 d80 (...)` -- with the same FLOP and byte accounting.)"""
    if out_proj is None:
        raise ValueError("motion_attn_wide: out_proj is required (pack_attn_out)")
    return motion_attn(x, gamma32, shift32, w_qkv, heads=heads, head_dim=head_dim, frames=frames, eps=eps, scale=scale, out=out,
                       out_proj=out_proj, _entry="i2v_motion_attn_wide_f16")


def motion_attn(x, gamma32, shift32, w_qkv, *, heads, head_dim, frames, eps, scale=None, out=None, out_proj=None,
                _entry="i2v_motion_attn_f16"):
    """o = temporal attention over the `frames` rows of each pixel of LayerNorm(x) + pe, q / k / v projected inside
    (i2v_motion_attn_f16); x [rows, C] in (batch, pixel, frame) order, (gamma32, shift32) from `motion_attn_tables`,
    w_qkv from `pack_motion_qkv`."""
    lib = _lib.load()
    x, ldx = _mat(x, "x")
    rows, c = x.shape
    _req(w_qkv, "w_qkv")
    for name, t in (("gamma32", gamma32), ("shift32", shift32)):
        _req(t, name, dtype=torch.float32)
    if c != heads * head_dim or tuple(gamma32.shape) != (c,) or tuple(shift32.shape) != (frames, c) or not shift32.is_contiguous():
        raise ValueError(f"motion_attn: C {c} vs heads {heads} x head_dim {head_dim}, gamma {tuple(gamma32.shape)}, "
                         f"shift {tuple(shift32.shape)} (expected [{frames}, {c}])")
    if tuple(w_qkv.shape) != (lib.i2v_motion_attn_pack_rows(heads, head_dim), c) or not w_qkv.is_contiguous():
        raise ValueError(f"motion_attn: w_qkv is {tuple(w_qkv.shape)} (pack_motion_qkv)")
    if out is None:
        out = torch.empty((rows, c), dtype=f16, device=x.device)
    out, ldo = _mat(out, "out")
    if tuple(out.shape) != (rows, c):
        raise ValueError(f"motion_attn: out is {tuple(out.shape)}")
    p = _lib.MotionAttnParams()
    p.x, p.ldx = _p(x), ldx
    p.gamma = _p(gamma32)
    p.shift, p.ld_shift = _p(shift32), c
    p.w_qkv = _p(w_qkv)
    p.out, p.ldo = _p(out), ldo
    p.rows, p.channels, p.heads, p.head_dim, p.frames = rows, c, heads, head_dim, frames
    p.eps, p.scale = float(eps), float(head_dim) ** -0.5 if scale is None else float(scale)
    if out_proj is not None:      # out = x + o Wo^T + bo in the same launch (`pack_attn_out`)
        p.w_o, p.b_o = _attn_out_operands(out_proj, c, heads, head_dim, "motion_attn")
    _lib.check(getattr(lib, _entry)(C.byref(p), _stream()), _entry)
    return out


# ---------------------------------------------------------------------------------------------- norms
def groupnorm(x, gamma, beta, groups, eps, *, x2=None, silu=False, frames_per_stat=1, out_perm=False, frames=0, stats=None):
    """GroupNorm (+SiLU) of a token-major image batch x [N, H, W, C1] (optionally concatenated with x2 along C).
    Returns [N, H, W, C]; with out_perm the rows are written in (b, pixel, frame) order and the result is
    returned flat as [N * H * W, C]."""
    lib = _lib.load()
    _req(x, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"x must be contiguous [N, H, W, C], got {tuple(x.shape)}")
    n, h, w, c1 = x.shape
    c2 = 0
    if x2 is not None:
        _req(x2, "x2")
        if x2.dim() != 4 or not x2.is_contiguous() or x2.shape[:3] != x.shape[:3]:
            raise ValueError("x2 must be contiguous [N, H, W, C2] with the same N, H, W as x")
        c2 = x2.shape[3]
    Cc = c1 + c2
    _req(gamma, "gamma")
    _req(beta, "beta")
    if gamma.numel() != Cc or beta.numel() != Cc:
        raise ValueError(f"gamma / beta must have {Cc} elements")
    ws = torch.empty((lib.i2v_groupnorm_workspace_bytes(n, h * w, Cc) + 3) // 4, dtype=torch.float32, device=x.device)
    y = torch.empty((n * h * w, Cc) if out_perm else (n, h, w, Cc), dtype=f16, device=x.device)
    p = GnParams()
    p.x, p.c1, p.x2, p.c2 = _p(x), c1, _p(x2), c2
    p.gamma, p.beta, p.y = _p(gamma.contiguous()), _p(beta.contiguous()), _p(y)
    p.n_img, p.hw, p.groups, p.frames_per_stat = n, h * w, groups, frames_per_stat
    p.eps, p.silu = eps, 1 if silu else 0
    p.out_perm, p.frames = (1 if out_perm else 0), frames
    p.workspace = _p(ws)
    if stats is not None:       # (partials, rows per partial block) from `conv3x3(..., gn_stats_groups=groups)`: no statistics pass
        part, rows = stats
        _req(part, "stats", dtype=torch.float32)
        if x2 is not None or frames_per_stat != 1 or out_perm or tuple(part.shape) != (n, (h * w) // rows, groups, 2) or \
                not part.is_contiguous():
            raise ValueError(f"groupnorm: stats {tuple(part.shape)} / rows {rows} do not describe x {tuple(x.shape)} in {groups} groups")
        p.gpartial_in, p.gpartial_rows = _p(part), int(rows)
    _lib.check(lib.i2v_groupnorm_f16(C.byref(p), _stream()), "i2v_groupnorm_f16")
    return y


def groupnorm_fold(x, gamma, beta, groups, eps, w, bias, *, x2=None, frames_per_stat=1):
    """GroupNorm (no activation) of x [N, H, W, C1] (+ x2 along C) folded into the Linear (w [n_out, C], bias) that
    consumes it: returns (w_s [S, n_out, C], bias_s [S, n_out]) with S = N / frames_per_stat statistics groups, such that
    Linear(GroupNorm(x)) = x w_s[s]^T + bias_s[s] for the rows of group s (i2v_groupnorm_fold_f16)."""
    lib = _lib.load()
    _req(x, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"x must be contiguous [N, H, W, C], got {tuple(x.shape)}")
    n, h, wd, c1 = x.shape
    c2 = 0
    if x2 is not None:
        _req(x2, "x2")
        if x2.dim() != 4 or not x2.is_contiguous() or x2.shape[:3] != x.shape[:3]:
            raise ValueError("x2 must be contiguous [N, H, W, C2] with the same N, H, W as x")
        c2 = x2.shape[3]
    Cc = c1 + c2
    _req(gamma, "gamma")
    _req(beta, "beta")
    w2, ldw = _mat(w, "w")
    if gamma.numel() != Cc or beta.numel() != Cc or w2.shape[1] != Cc:
        raise ValueError(f"gamma / beta / w columns must have {Cc} elements")
    n_out = w2.shape[0]
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != n_out or not bias.is_contiguous():
            raise ValueError("bias must be a contiguous vector of n_out elements")
    if frames_per_stat <= 0 or n % frames_per_stat != 0:
        raise ValueError(f"batch {n} is not a multiple of frames_per_stat {frames_per_stat}")
    S = n // frames_per_stat
    ws = torch.empty((lib.i2v_groupnorm_workspace_bytes(n, h * wd, Cc) + 3) // 4, dtype=torch.float32, device=x.device)
    w_s = torch.empty((S, n_out, Cc), dtype=f16, device=x.device)
    b_s = torch.empty((S, n_out), dtype=f16, device=x.device)
    p = GnParams()
    p.x, p.c1, p.x2, p.c2 = _p(x), c1, _p(x2), c2
    p.gamma, p.beta = _p(gamma.contiguous()), _p(beta.contiguous())
    p.n_img, p.hw, p.groups, p.frames_per_stat = n, h * wd, groups, frames_per_stat
    p.eps = eps
    p.workspace = _p(ws)
    _lib.check(lib.i2v_groupnorm_fold_f16(C.byref(p), _p(w2), ldw, _p(bias), n_out, _p(w_s), _p(b_s), _stream()),
               "i2v_groupnorm_fold_f16")
    return w_s, b_s


def layernorm(x, gamma, beta, eps, *, pe=None, pe_period=0):
    """LayerNorm over the last dim of a 2-D token matrix (+ pe[row % pe_period]).  x may also be a 3-D view
    [batches, rows_per_batch, C] with arbitrary batch stride (e.g. the frame-0 rows of every clip, i2v:484): the rows are
    read in place and the result is the dense [batches * rows_per_batch, C] matrix."""
    lib = _lib.load()
    batched = None
    if x.dim() == 3:
        _req(x, "x")
        if x.stride(2) != 1 or x.stride(1) % 8 != 0 or x.stride(0) % 8 != 0 or x.stride(0) <= 0:
            raise ValueError("batched layernorm input needs unit last stride and row / batch strides that are multiples of 8")
        batched = (x.shape[1], x.stride(0))
        ldx = x.stride(1)
        rows, Cc = x.shape[0] * x.shape[1], x.shape[2]
    else:
        x, ldx = _mat(x, "x")
        rows, Cc = x.shape
    _req(gamma, "gamma")
    _req(beta, "beta")
    y = torch.empty((rows, Cc), dtype=f16, device=x.device)
    p = LnParams()
    p.x, p.ldx = _p(x), ldx
    p.gamma, p.beta = _p(gamma), _p(beta)
    if pe is not None:
        pe, ldpe = _mat(pe, "pe")
        if pe.shape[1] != Cc or pe.shape[0] < pe_period or pe_period <= 0:
            raise ValueError("pe must be [>= pe_period, C]")
        p.pe, p.ld_pe, p.pe_period = _p(pe), ldpe, pe_period
    p.y, p.ldy = _p(y), Cc
    p.rows, p.C, p.eps = rows, Cc, eps
    if batched is not None:
        p.x_rows_per_batch, p.x_batch_stride = batched
    _lib.check(lib.i2v_layernorm_f16(C.byref(p), _stream()), "i2v_layernorm_f16")
    return y


def softmax_rows(x, scale=1.0, out=None):
    """row-wise softmax(scale * x) of a 2-D fp16 matrix (in place when out is x)."""
    lib = _lib.load()
    x, ldx = _mat(x, "x")
    if out is None:                      # rows start on 16-byte boundaries: leading dimension rounded up to 8
        out = torch.empty((x.shape[0], pad8(x.shape[1])), dtype=f16, device=x.device)[:, : x.shape[1]]
    out, ldy = _mat(out, "out")
    if out.shape != x.shape:
        raise ValueError("softmax_rows: out must have x's shape")
    _lib.check(lib.i2v_softmax_rows_f16(_p(x), ldx, _p(out), ldy, x.shape[0], x.shape[1], float(scale), _stream()),
               "i2v_softmax_rows_f16")
    return out


# ---------------------------------------------------------------------------------------------- edges / misc
def nchw_to_tokens(src, c_pad=None):
    """[N, C, H, W] (fp32 or fp16) -> token-major fp16 [N, H, W, c_pad]."""
    lib = _lib.load()
    _req(src, "src", dtype=None)
    if src.dtype not in (torch.float32, f16) or src.dim() != 4:
        raise TypeError("src must be a 4-D fp32 / fp16 tensor")
    src = src.contiguous()
    n, c, h, w = src.shape
    c_pad = c if c_pad is None else c_pad
    dst = torch.empty((n, h, w, c_pad), dtype=f16, device=src.device)
    _lib.check(lib.i2v_nchw_to_tokens(_p(src), 1 if src.dtype == torch.float32 else 0, _p(dst), n, c, h * w, c_pad,
                                      _stream()), "i2v_nchw_to_tokens")
    return dst


def tokens_to_nchw(src, c=None, dtype=f16):
    """token-major fp16 / fp32 [N, H, W, ld] -> [N, c, H, W] in `dtype` (fp16 / fp32)."""
    lib = _lib.load()
    _req(src, "src", dtype=None)
    if src.dtype not in (torch.float32, f16):
        raise TypeError("src must be fp16 or fp32")
    if src.dim() != 4 or not src.is_contiguous():
        raise ValueError("src must be contiguous [N, H, W, C]")
    n, h, w, ld = src.shape
    c = ld if c is None else c
    if dtype not in (torch.float32, f16):
        raise TypeError("dtype must be fp32 or fp16")
    dst = torch.empty((n, c, h, w), dtype=dtype, device=src.device)
    _lib.check(lib.i2v_tokens_to_nchw(_p(src), 1 if src.dtype == torch.float32 else 0, ld, _p(dst),
                                      1 if dtype == torch.float32 else 0, n, c, h * w, _stream()), "i2v_tokens_to_nchw")
    return dst


def timestep_embedding(t, dim, t_index=None):
    """t fp32 [n] (or a table indexed by the device scalar `t_index`, with n = t_rows) -> [n, dim] fp16."""
    lib = _lib.load()
    _req(t, "t", dtype=torch.float32)
    n = 1 if t_index is not None else t.numel()
    if t_index is not None:
        _req(t_index, "t_index", dtype=torch.int32)
    out = torch.empty((n, dim), dtype=f16, device=t.device)
    _lib.check(lib.i2v_timestep_embedding(_p(t), _p(t_index), t.numel(), _p(out), n, dim, _stream()),
               "i2v_timestep_embedding")
    return out


def silu(x):
    lib = _lib.load()
    _req(x, "x")
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.check(lib.i2v_silu_f16(_p(x), _p(y), x.numel(), _stream()), "i2v_silu_f16")
    return y


# ---------------------------------------------------------------------------------------------- CLIP text tower (clip_text.py)
def clip_embed(token_embedding, position_embedding, input_ids):
    """token + position embedding lookup (i2v_clip_embed_f16): tables fp16 [vocab, hidden] / [max_positions, hidden] on the device,
    input_ids an integer [B, L] tensor on either side -> fp16 [B * L, hidden].  The ids are validated on the HOST (an id outside the
    vocabulary raises before anything is launched), so ids that live on the device are copied back once."""
    lib = _lib.load()
    tok, pos = _req(token_embedding, "token_embedding"), _req(position_embedding, "position_embedding")
    if tok.dim() != 2 or pos.dim() != 2 or tok.shape[1] != pos.shape[1] or not tok.is_contiguous() or not pos.is_contiguous():
        raise ValueError(f"embedding tables must be contiguous [rows, hidden] of one width, got {tuple(tok.shape)} / {tuple(pos.shape)}")
    if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2 or input_ids.dtype not in (torch.int32, torch.int64):
        raise TypeError("input_ids must be an int32 / int64 [B, L] tensor")
    host = input_ids.detach().to("cpu", torch.int32).contiguous()
    dev = host.to(tok.device)
    b, l = host.shape
    out = torch.empty((b * l, tok.shape[1]), dtype=f16, device=tok.device)
    _lib.check(lib.i2v_clip_embed_f16(_p(tok), _p(pos), _p(dev), C.c_void_p(host.data_ptr()), _p(out), b, l, tok.shape[0], pos.shape[0],
                                      tok.shape[1], _stream()), "i2v_clip_embed_f16")
    return out


def _attn_operand(t, name, rows, hidden, *offsets):
    """a packed operand of csrc/short_attention.hip's entries, fp16 [rows, >= offset + hidden] for each offset -> (tensor, row stride)"""
    t, ld = _mat(t, name)
    if t.shape[0] != rows or max(offsets) + hidden > t.shape[1]:
        raise ValueError(f"{name} is {tuple(t.shape)}: expected [{rows}, >= offset + {hidden}]")
    return t, ld


def _attn_out(out, rows, hidden, device):
    """their `out`: the caller's [rows, hidden] view or a new tensor -> (tensor, row stride)"""
    if out is None:
        out = torch.empty((rows, hidden), dtype=f16, device=device)
    out, ldo = _mat(out, "out")
    if out.shape != (rows, hidden):
        raise ValueError(f"out must be {(rows, hidden)}, got {tuple(out.shape)}")
    return out, ldo


def _clip_attention(entry_name, qkv, *, batch, length, heads, head_dim, q_off=None, k_off=None, v_off=None, scale=None, out=None):
    """what `clip_attention` and `clip_vision_attention` share (csrc/short_attention.hip: one kernel, one set of argument checks): qkv
    fp16 [batch * length, >= 3 * hidden], head h of q / k / v in columns q_off / k_off / v_off + h * head_dim (default 0, hidden,
    2 * hidden) -> fp16 [batch * length, hidden]; `entry_name` is the C entry point, which holds the envelope."""
    lib = _lib.load()
    hidden = heads * head_dim
    q_off = 0 if q_off is None else q_off
    k_off = hidden if k_off is None else k_off
    v_off = 2 * hidden if v_off is None else v_off
    qkv, ld = _attn_operand(qkv, "qkv", batch * length, hidden, q_off, k_off, v_off)
    out, ldo = _attn_out(out, batch * length, hidden, qkv.device)
    scale = float(head_dim) ** -0.5 if scale is None else float(scale)
    _lib.check(getattr(lib, entry_name)(_p(qkv), ld, q_off, k_off, v_off, _p(out), ldo, batch, length, heads, head_dim, scale, _stream()),
               entry_name)
    return out


def clip_attention(qkv, **kw):
    """causal self-attention of `batch` sequences of `length` tokens (i2v_clip_attention_f16), q / k / v read in place from the packed
    result of one QKV GEMM: qkv fp16 [batch * length, >= 3 * hidden], head h of q / k / v in columns q_off / k_off / v_off + h * head_dim
    (default 0, hidden, 2 * hidden) -> fp16 [batch * length, hidden].  head_dim 64 and length <= 128 only (anything else raises)."""
    return _clip_attention("i2v_clip_attention_f16", qkv, **kw)


def quick_gelu(x, out=None):
    """x * sigmoid(1.702 x) in fp32, rounded to fp16 (i2v_quick_gelu_f16); `out` may be x itself (in place)."""
    lib = _lib.load()
    _req(x, "x")
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")
    if out is None:
        out = torch.empty_like(x)
    _req(out, "out")
    if out.shape != x.shape or not out.is_contiguous():
        raise ValueError("out must be contiguous with x's shape")
    if x.numel() == 0:
        return out
    _lib.check(lib.i2v_quick_gelu_f16(_p(x), _p(out), x.numel(), _stream()), "i2v_quick_gelu_f16")
    return out


# ---------------------------------------------------------------------------------------------- CLIP vision tower (clip_vision.py)
def clip_patchify(pixel_values, patch, ld=None, out=None):
    """im2col of the patch embedding (i2v_clip_patchify_f16): pixel_values fp16 [B, C, S, S] contiguous -> fp16 [B * (S / patch)^2, ld],
    row b * P + py * (S / patch) + px = patch (py, px) in column order (c, dy, dx), columns C * patch^2 .. ld - 1 zero.  ld defaults to
    pad8(C * patch^2); S % patch != 0 raises (nothing is launched)."""
    lib = _lib.load()
    _req(pixel_values, "pixel_values")
    if pixel_values.dim() != 4 or pixel_values.shape[2] != pixel_values.shape[3] or not pixel_values.is_contiguous():
        raise ValueError(f"pixel_values must be contiguous [B, C, S, S], got {tuple(pixel_values.shape)}")
    b, c, s, _ = pixel_values.shape
    ld = pad8(c * patch * patch) if ld is None else ld
    rows = b * (s // patch) ** 2
    if out is None:
        out = torch.empty((rows, ld), dtype=f16, device=pixel_values.device)
    _req(out, "out")
    if out.shape != (rows, ld) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous {(rows, ld)}, got {tuple(out.shape)}")
    _lib.check(lib.i2v_clip_patchify_f16(_p(pixel_values), _p(out), ld, b, c, s, patch, _stream()), "i2v_clip_patchify_f16")
    return out


def clip_vision_embed(class_embedding, patch_embeds, position_embedding, *, batch):
    """class token + patch embeddings + positions (i2v_clip_vision_embed_f16): class_embedding fp16 [hidden], patch_embeds fp16
    [batch * P, hidden] (the patch GEMM's result), position_embedding fp16 [P + 1, hidden] -> fp16 [batch * (P + 1), hidden]."""
    lib = _lib.load()
    cls, pos = _req(class_embedding, "class_embedding"), _req(position_embedding, "position_embedding")
    patch_embeds, ldp = _mat(patch_embeds, "patch_embeds")
    hidden = patch_embeds.shape[1]
    if patch_embeds.shape[0] % batch != 0:
        raise ValueError(f"{patch_embeds.shape[0]} patch rows for a batch of {batch}")
    patches = patch_embeds.shape[0] // batch
    if cls.shape != (hidden,) or pos.shape != (patches + 1, hidden) or not cls.is_contiguous() or not pos.is_contiguous():
        raise ValueError(f"class_embedding must be [{hidden}] and position_embedding [{patches + 1}, {hidden}], contiguous; got "
                         f"{tuple(cls.shape)} / {tuple(pos.shape)}")
    out = torch.empty((batch * (patches + 1), hidden), dtype=f16, device=patch_embeds.device)
    _lib.check(lib.i2v_clip_vision_embed_f16(_p(cls), _p(patch_embeds), ldp, _p(pos), _p(out), batch, patches, hidden, _stream()),
               "i2v_clip_vision_embed_f16")
    return out


def clip_vision_attention(qkv, **kw):
    """NON-causal self-attention of `batch` sequences of `length` tokens (i2v_clip_vision_attention_f16), q / k / v read in place from the
    packed result of one QKV GEMM, as `clip_attention` takes them -> fp16 [batch * length, hidden].  head_dim 64 or 80 and length <= 288
    only (anything else raises)."""
    return _clip_attention("i2v_clip_vision_attention_f16", qkv, **kw)


def perceiver_attention(q, kv_a, kv_b=None, *, batch, n_q, len_a, len_b=0, heads, head_dim=64, q_off=0, ka_off=0, va_off=None, kb_off=None,
                        vb_off=None, scale=None, out=None):
    """attention of `n_q` queries per batch entry over the concatenation of two key / value row sources (i2v_perceiver_attention_f16,
    the Resampler's attention): q fp16 [batch * n_q, >= q_off + hidden]; kv_a fp16 [batch * len_a, ...] with head h of k / v in columns
    ka_off / va_off + h * head_dim (default 0, hidden); kv_b the same for len_b rows per entry (default offsets hidden, 2 * hidden: a
    packed q | k | v buffer, which may be `q` itself) -> fp16 [batch * n_q, hidden].  head_dim 64, n_q <= 64, len_a >= 1 and
    len_a + len_b <= 288 only (anything else raises)."""
    lib = _lib.load()
    hidden = heads * head_dim
    va_off = hidden if va_off is None else va_off
    kb_off = hidden if kb_off is None else kb_off
    vb_off = 2 * hidden if vb_off is None else vb_off
    q, ldq = _attn_operand(q, "q", batch * n_q, hidden, q_off)
    kv_a, lda = _attn_operand(kv_a, "kv_a", batch * len_a, hidden, ka_off, va_off)
    if len_b > 0:
        if kv_b is None:
            raise ValueError(f"len_b = {len_b} needs kv_b")
        kv_b, ldb = _attn_operand(kv_b, "kv_b", batch * len_b, hidden, kb_off, vb_off)
        pb = _p(kv_b)
    else:
        pb, ldb, kb_off, vb_off = None, 0, 0, 0
    out, ldo = _attn_out(out, batch * n_q, hidden, q.device)
    scale = float(head_dim) ** -0.5 if scale is None else float(scale)
    _lib.check(lib.i2v_perceiver_attention_f16(_p(q), ldq, q_off, _p(kv_a), lda, ka_off, va_off, len_a, pb, ldb, kb_off, vb_off, len_b,
                                               _p(out), ldo, batch, n_q, heads, head_dim, scale, _stream()),
               "i2v_perceiver_attention_f16")
    return out


def select_row(table, row_index, out=None):
    """[1, cols] = table[clamp(*row_index)] for a device int32 scalar `row_index` (a replayed step's row of a per-timestep
    table)."""
    lib = _lib.load()
    table, ld = _mat(table, "table")
    _req(row_index, "row_index", dtype=torch.int32)
    if out is None:
        out = torch.empty((1, table.shape[1]), dtype=f16, device=table.device)
    _lib.check(lib.i2v_select_row_f16(_p(table), ld, table.shape[0], _p(row_index), _p(out), table.shape[1], _stream()),
               "i2v_select_row_f16")
    return out


def repeat_rows(x, repeat):
    lib = _lib.load()
    x, _ = _mat(x, "x")
    x = x.contiguous()
    y = torch.empty((x.shape[0] * repeat, x.shape[1]), dtype=f16, device=x.device)
    _lib.check(lib.i2v_repeat_rows_f16(_p(x), _p(y), x.shape[0], x.shape[1], repeat, _stream()), "i2v_repeat_rows_f16")
    return y


def copy3d(src, dst):
    """dst[b, r, :] = src[b, r, :] for 3-D fp16 tensors whose last dim is unit-stride (views allowed)."""
    lib = _lib.load()
    _req(src, "src")
    _req(dst, "dst")
    if src.dim() != 3 or dst.shape != src.shape or src.stride(2) != 1 or dst.stride(2) != 1:
        raise ValueError("copy3d needs two 3-D tensors of equal shape with unit last stride")
    b, r, c = src.shape
    _lib.check(lib.i2v_copy3d_f16(_p(src), src.stride(0), src.stride(1), _p(dst), dst.stride(0), dst.stride(1), b, r, c,
                                  _stream()), "i2v_copy3d_f16")
    return dst


def duplicate_batch(x):
    """[x ; x] along the leading dimension (the second CFG half of a tensor computed once for both, unet._fwd_tokens)."""
    _req(x, "x")
    lo = lo_of(x)
    x = x.contiguous()
    rows = x.shape[0]
    y = torch.empty((2 * rows,) + tuple(x.shape[1:]), dtype=f16, device=x.device)
    c = x.shape[-1]
    copy3d(x.view(1, -1, c).expand(2, -1, c), y.view(2, -1, c))
    if lo is not None:                      # a tensor of the precise residual stream: its low half travels with it
        y._i2v_lo = duplicate_batch(lo)
    return y


def first_frame_prior(cond, mask_uniform, noise, sigma, strength, sqrt_alpha, sqrt_one_minus_alpha):
    """latents = sqrt_alpha * (mask * blur3x3_sigma(cond) + (1 - mask) * cond) + sqrt_one_minus_alpha * noise with
    mask = (mask_uniform < strength): the first-frame-similarity prior + add_noise of pipe:647-656 in one kernel.
    cond fp32 [B, C, H, W]; mask_uniform / noise fp32 [B, F, C, H, W]; returns fp32 [B, F, C, H, W]."""
    import math
    lib = _lib.load()
    for t, name in ((cond, "cond"), (mask_uniform, "mask_uniform"), (noise, "noise")):
        _req(t, name, dtype=torch.float32)
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if cond.dim() != 4 or noise.dim() != 5 or mask_uniform.shape != noise.shape or \
            (noise.shape[0], noise.shape[2], noise.shape[3], noise.shape[4]) != tuple(cond.shape):
        raise ValueError(f"cond {tuple(cond.shape)} / mask {tuple(mask_uniform.shape)} / noise {tuple(noise.shape)} mismatch")
    if not sigma > 0:
        raise ValueError("sigma must be positive")
    b, f, c, h, w = noise.shape
    e = math.exp(-0.5 / (sigma * sigma))                      # torchvision _get_gaussian_kernel1d, kernel_size 3
    kc, ke = 1.0 / (1.0 + 2.0 * e), e / (1.0 + 2.0 * e)
    out = torch.empty_like(noise)
    _lib.check(lib.i2v_first_frame_prior_f32(_p(cond), _p(mask_uniform), _p(noise), _p(out), b, f, c, h, w, kc, ke,
                                             float(strength), float(sqrt_alpha), float(sqrt_one_minus_alpha),
                                             _stream()), "i2v_first_frame_prior_f32")
    return out


def gaussian_sample(moments, eps):
    """mean + exp(0.5 clamp(logvar, -30, 20)) * eps for moments fp32 [N, 2C, H, W] = (mean | logvar), eps fp32 [N, C, H, W]."""
    lib = _lib.load()
    _req(moments, "moments", dtype=torch.float32)
    _req(eps, "eps", dtype=torch.float32)
    n, c2, h, w = moments.shape
    if c2 % 2 != 0 or tuple(eps.shape) != (n, c2 // 2, h, w) or not moments.is_contiguous() or not eps.is_contiguous():
        raise ValueError(f"moments {tuple(moments.shape)} / eps {tuple(eps.shape)} mismatch")
    out = torch.empty_like(eps)
    _lib.check(lib.i2v_gaussian_sample_f32(_p(moments), _p(eps), _p(out), n, c2 // 2, h * w, _stream()),
               "i2v_gaussian_sample_f32")
    return out


def ddim_prep(latents, cond, c_pad, cfg_copies):
    """latents fp32 [B, F, C, H, W] (frame 0 overwritten in place with cond [B, C, H, W]) ->
    model input tokens fp16 [cfg_copies * B * F, H, W, c_pad]."""
    lib = _lib.load()
    _req(latents, "latents", dtype=torch.float32)
    _req(cond, "cond", dtype=torch.float32)
    if latents.dim() != 5 or not latents.is_contiguous() or not cond.is_contiguous():
        raise ValueError("latents must be contiguous [B, F, C, H, W]; cond contiguous [B, C, H, W]")
    b, f, c, h, w = latents.shape
    if tuple(cond.shape) != (b, c, h, w):
        raise ValueError(f"cond must be {(b, c, h, w)}, got {tuple(cond.shape)}")
    out = torch.empty((cfg_copies * b * f, h, w, c_pad), dtype=f16, device=latents.device)
    _lib.check(lib.i2v_ddim_prep(_p(latents), _p(cond), _p(out), b, f, c, h * w, c_pad, cfg_copies, _stream()),
               "i2v_ddim_prep")
    return out


def ddim_cfg_step(latents, noise_pred, coef, step_index, guidance_scale, cfg_copies):
    """In-place DDIM update of latents fp32 [B, F, C, H, W] from noise_pred tokens (fp32, or fp16)
    [cfg_copies * B * F, H, W, ld]; coef fp32 [steps, 4]; step_index device int32 scalar (advanced by one, wrapping
    to 0 at the end of the table)."""
    lib = _lib.load()
    _req(latents, "latents", dtype=torch.float32)
    _req(noise_pred, "noise_pred", dtype=None)
    if noise_pred.dtype not in (torch.float32, f16):
        raise TypeError("noise_pred must be fp32 or fp16")
    _req(coef, "coef", dtype=torch.float32)
    _req(step_index, "step_index", dtype=torch.int32)
    b, f, c, h, w = latents.shape
    if noise_pred.dim() != 4 or not noise_pred.is_contiguous() or noise_pred.shape[0] != cfg_copies * b * f or \
            noise_pred.shape[1] != h or noise_pred.shape[2] != w or noise_pred.shape[3] < c:
        raise ValueError(f"noise_pred must be contiguous [{cfg_copies * b * f}, {h}, {w}, >={c}]")
    if coef.dim() != 2 or coef.shape[1] != 4 or not coef.is_contiguous():
        raise ValueError("coef must be contiguous [steps, 4]")
    _lib.check(lib.i2v_ddim_cfg_step(_p(latents), _p(noise_pred), 1 if noise_pred.dtype == torch.float32 else 0,
                                     noise_pred.shape[3], _p(coef), coef.shape[0],
                                     _p(step_index), float(guidance_scale), b, f, c, h * w, cfg_copies, _stream()),
               "i2v_ddim_cfg_step")
    return latents


def dpm_cfg_step(latents, x0_prev, noise_pred, coef, step_index, guidance_scale, cfg_copies):
    """In-place DPM-Solver++ (2M) update of latents fp32 [B, F, C, H, W] from noise_pred tokens (fp32, or fp16)
    [cfg_copies * B * F, H, W, ld]; x0_prev fp32 like the latents (the previous step's data prediction: read by second-order
    rows, written by every row); coef fp32 [steps, 6] (`DPMSolverMultistepScheduler.step_coefficients`); step_index device
    int32 scalar (advanced by one, wrapping to 0 at the end of the table)."""
    lib = _lib.load()
    _req(latents, "latents", dtype=torch.float32)
    _req(x0_prev, "x0_prev", dtype=torch.float32)
    _req(noise_pred, "noise_pred", dtype=None)
    if noise_pred.dtype not in (torch.float32, f16):
        raise TypeError("noise_pred must be fp32 or fp16")
    _req(coef, "coef", dtype=torch.float32)
    _req(step_index, "step_index", dtype=torch.int32)
    b, f, c, h, w = latents.shape
    if tuple(x0_prev.shape) != tuple(latents.shape) or not x0_prev.is_contiguous() or not latents.is_contiguous():
        raise ValueError(f"latents and x0_prev must be contiguous {tuple(latents.shape)}")
    if noise_pred.dim() != 4 or not noise_pred.is_contiguous() or noise_pred.shape[0] != cfg_copies * b * f or \
            noise_pred.shape[1] != h or noise_pred.shape[2] != w or noise_pred.shape[3] < c:
        raise ValueError(f"noise_pred must be contiguous [{cfg_copies * b * f}, {h}, {w}, >={c}]")
    if coef.dim() != 2 or coef.shape[1] != 6 or not coef.is_contiguous():
        raise ValueError("coef must be contiguous [steps, 6]")
    _lib.check(lib.i2v_dpm_cfg_step(_p(latents), _p(x0_prev), _p(noise_pred), 1 if noise_pred.dtype == torch.float32 else 0,
                                    noise_pred.shape[3], _p(coef), coef.shape[0],
                                    _p(step_index), float(guidance_scale), b, f, c, h * w, cfg_copies, _stream()),
               "i2v_dpm_cfg_step")
    return latents


def lcm_cfg_step(latents, noise, noise_pred, coef, step_index, guidance_scale, cfg_copies):
    """In-place latent-consistency (LCM) update of latents fp32 [B, F, C, H, W] from noise_pred tokens (fp32, or fp16)
    [cfg_copies * B * F, H, W, ld]; noise fp32 [n, B, F, C, H, W] (`LCMScheduler.step_noise`: row min(step, n - 1) re-noises every
    step but the last; None for a single-step schedule); coef fp32 [steps, 6] (`LCMScheduler.step_coefficients`); step_index device
    int32 scalar (advanced by one, wrapping to 0 at the end of the table)."""
    lib = _lib.load()
    _req(latents, "latents", dtype=torch.float32)
    _req(noise_pred, "noise_pred", dtype=None)
    if noise_pred.dtype not in (torch.float32, f16):
        raise TypeError("noise_pred must be fp32 or fp16")
    _req(coef, "coef", dtype=torch.float32)
    _req(step_index, "step_index", dtype=torch.int32)
    if latents.dim() != 5 or not latents.is_contiguous():
        raise ValueError("latents must be contiguous [B, F, C, H, W]")
    b, f, c, h, w = latents.shape
    if noise is not None:
        _req(noise, "noise", dtype=torch.float32)
        if noise.dim() != 6 or tuple(noise.shape[1:]) != tuple(latents.shape) or noise.shape[0] < 1 or not noise.is_contiguous():
            raise ValueError(f"noise must be contiguous [n >= 1, {', '.join(str(v) for v in latents.shape)}], got {tuple(noise.shape)}")
    if noise_pred.dim() != 4 or not noise_pred.is_contiguous() or noise_pred.shape[0] != cfg_copies * b * f or \
            noise_pred.shape[1] != h or noise_pred.shape[2] != w or noise_pred.shape[3] < c:
        raise ValueError(f"noise_pred must be contiguous [{cfg_copies * b * f}, {h}, {w}, >={c}]")
    if coef.dim() != 2 or coef.shape[1] != 6 or not coef.is_contiguous():
        raise ValueError("coef must be contiguous [steps, 6]")
    _lib.check(lib.i2v_lcm_cfg_step(_p(latents), _p(noise) if noise is not None else None, noise.shape[0] if noise is not None else 0,
                                    _p(noise_pred), 1 if noise_pred.dtype == torch.float32 else 0, noise_pred.shape[3], _p(coef),
                                    coef.shape[0], _p(step_index), float(guidance_scale), b, f, c, h * w, cfg_copies, _stream()),
               "i2v_lcm_cfg_step")
    return latents


def sigma_prep(latents, cond, coef, step_index, c_pad, cfg_copies):
    """`ddim_prep` with Euler's `scale_model_input`: latents fp32 [B, F, C, H, W] (frame 0 overwritten in place with cond [B, C, H, W],
    unscaled) -> model input tokens fp16 [cfg_copies * B * F, H, W, c_pad] = fp16(v * coef[step][1]); coef fp32 [steps, >= 2] (the
    samplers' `step_coefficients`: column 1 is 1 / sqrt(sigma^2 + 1)); step_index device int32 scalar, read and not advanced."""
    lib = _lib.load()
    _req(latents, "latents", dtype=torch.float32)
    _req(cond, "cond", dtype=torch.float32)
    _req(coef, "coef", dtype=torch.float32)
    _req(step_index, "step_index", dtype=torch.int32)
    if latents.dim() != 5 or not latents.is_contiguous() or not cond.is_contiguous():
        raise ValueError("latents must be contiguous [B, F, C, H, W]; cond contiguous [B, C, H, W]")
    b, f, c, h, w = latents.shape
    if tuple(cond.shape) != (b, c, h, w):
        raise ValueError(f"cond must be {(b, c, h, w)}, got {tuple(cond.shape)}")
    if coef.dim() != 2 or coef.shape[0] < 1 or coef.shape[1] < 2 or not coef.is_contiguous():
        raise ValueError("coef must be contiguous [steps >= 1, >= 2]")
    out = torch.empty((cfg_copies * b * f, h, w, c_pad), dtype=f16, device=latents.device)
    _lib.check(lib.i2v_sigma_prep(_p(latents), _p(cond), _p(out), _p(coef), coef.shape[1], coef.shape[0], _p(step_index), b, f, c, h * w,
                                  c_pad, cfg_copies, _stream()),
               "i2v_sigma_prep")
    return out


def euler_cfg_step(latents, noise, noise_pred, coef, step_index, guidance_scale, cfg_copies):
    """In-place Euler / Euler-ancestral update of latents fp32 [B, F, C, H, W] from noise_pred tokens (fp32, or fp16)
    [cfg_copies * B * F, H, W, ld]: x' = x + eps (sigma_to - sigma) + sigma_up z.  coef fp32 [steps, 4] rows {sigma,
    1 / sqrt(sigma^2 + 1), sigma_to, sigma_up} (`EulerDiscreteScheduler.step_coefficients` / `EulerAncestralDiscreteScheduler.
    step_coefficients`); noise fp32 [n >= steps, B, F, C, H, W] (`EulerAncestralDiscreteScheduler.step_noise`: row `step` is z), None for
    Euler, whose rows all have sigma_up = 0; step_index device int32 scalar (advanced by one, wrapping to 0 at the end of the table).
    noise=None with a table that has a non-zero sigma_up is refused here, where the table can be read: outside stream capture (a
    captured step has had its eager warm-up step)."""
    lib = _lib.load()
    _req(latents, "latents", dtype=torch.float32)
    _req(noise_pred, "noise_pred", dtype=None)
    if noise_pred.dtype not in (torch.float32, f16):
        raise TypeError("noise_pred must be fp32 or fp16")
    _req(coef, "coef", dtype=torch.float32)
    _req(step_index, "step_index", dtype=torch.int32)
    if latents.dim() != 5 or not latents.is_contiguous():
        raise ValueError("latents must be contiguous [B, F, C, H, W]")
    b, f, c, h, w = latents.shape
    if coef.dim() != 2 or coef.shape[1] != 4 or coef.shape[0] < 1 or not coef.is_contiguous():
        raise ValueError("coef must be contiguous [steps, 4]")
    if noise is not None:
        _req(noise, "noise", dtype=torch.float32)
        if noise.dim() != 6 or tuple(noise.shape[1:]) != tuple(latents.shape) or noise.shape[0] < coef.shape[0] or not noise.is_contiguous():
            raise ValueError(f"noise must be contiguous [n >= {coef.shape[0]}, {', '.join(str(v) for v in latents.shape)}], "
                             f"got {tuple(noise.shape)}")
    elif not torch.cuda.is_current_stream_capturing() and bool((coef[:, 3] != 0).any()):
        raise ValueError("noise is None and the coefficient table has a row with sigma_up != 0 (an ancestral table needs its noise table)")
    if noise_pred.dim() != 4 or not noise_pred.is_contiguous() or noise_pred.shape[0] != cfg_copies * b * f or \
            noise_pred.shape[1] != h or noise_pred.shape[2] != w or noise_pred.shape[3] < c:
        raise ValueError(f"noise_pred must be contiguous [{cfg_copies * b * f}, {h}, {w}, >={c}]")
    _lib.check(lib.i2v_euler_cfg_step(_p(latents), _p(noise) if noise is not None else None, noise.shape[0] if noise is not None else 0,
                                      _p(noise_pred), 1 if noise_pred.dtype == torch.float32 else 0, noise_pred.shape[3], _p(coef),
                                      coef.shape[0], _p(step_index), float(guidance_scale), b, f, c, h * w, cfg_copies, _stream()),
               "i2v_euler_cfg_step")
    return latents


def freeu(hidden, skip, b, s):
    """FreeU on the operands of an up block's skip concatenation (i2v_freeu_f16; diffusers apply_freeu, unet:453-478): hidden
    [N, H, W, C1], skip [N, H, W, C2] fp16 token-major -> (hidden', skip'), new tensors.  hidden'[..., :C1 // 2] = hidden * b, the
    other channels copied; skip' = skip with its four lowest spatial frequencies scaled by s.  A hidden tensor of the precise residual
    stream (`lo_of(hidden)`) is scaled as hi + lo and comes back with a fresh low half."""
    lib = _lib.load()
    _req(hidden, "hidden")
    _req(skip, "skip")
    if hidden.dim() != 4 or skip.dim() != 4 or tuple(hidden.shape[:3]) != tuple(skip.shape[:3]):
        raise ValueError(f"hidden {tuple(hidden.shape)} and skip {tuple(skip.shape)} must be [N, H, W, C1] and [N, H, W, C2]")
    if not hidden.is_contiguous() or not skip.is_contiguous():
        raise ValueError("hidden and skip must be contiguous")
    n, hh, ww, c1 = hidden.shape
    lo = lo_of(hidden)
    if lo is not None and (lo.shape != hidden.shape or lo.stride() != hidden.stride() or lo.dtype != f16):
        raise ValueError("the low half of a stream tensor must be laid out like the tensor")
    h_out, s_out = torch.empty_like(hidden), torch.empty_like(skip)
    lo_out = None if lo is None else torch.empty_like(hidden)
    _lib.check(lib.i2v_freeu_f16(_p(hidden), _p(lo), _p(h_out), _p(lo_out), _p(skip), _p(s_out), n, hh, ww, c1, skip.shape[3],
                                 float(b), float(s), _stream()), "i2v_freeu_f16")
    if lo_out is not None:
        h_out._i2v_lo = lo_out
    return h_out, s_out


def add_residuals(skips, residuals, scale=None, out=None):
    """ControlNet residuals into skip tensors (i2v_add_residuals_f16; unet:1379-1389, 1402-1403): out_i = skip_i + s * residual_i for
    a list of fp16 tensor pairs of any sizes (numel % 8 == 0), I2V_ADD_RES_MAX pairs per launch.  scale = None (s = 1) or
    (table fp32 [rows], step_idx int32 [1] or None): s = table[clamp(*step_idx)], read on the device.  out = None: new tensors;
    out = a list: written there (out[i] may be skips[i]: in place).  A skip of the precise residual stream (`lo_of`) is added as
    hi + lo and the result carries a fresh low half (in place: the skip's own is rewritten).  Returns the list of results."""
    lib = _lib.load()
    skips, residuals = list(skips), list(residuals)
    if len(skips) != len(residuals) or not skips:
        raise ValueError(f"add_residuals: {len(skips)} skip tensors and {len(residuals)} residuals")
    if out is not None and len(out) != len(skips):
        raise ValueError(f"add_residuals: {len(out)} outputs for {len(skips)} skip tensors")
    table = idx = None
    if scale is not None:
        table, idx = scale
        _req(table, "scale table", dtype=torch.float32)
        if table.dim() != 1 or table.numel() < 1 or not table.is_contiguous():
            raise ValueError("add_residuals: the scale table is a contiguous fp32 vector")
        if idx is not None:
            _req(idx, "step_idx", dtype=torch.int32)
    outs, los = [], []
    for i, (s, r) in enumerate(zip(skips, residuals)):
        _req(s, f"skips[{i}]")
        _req(r, f"residuals[{i}]")
        if s.shape != r.shape or not s.is_contiguous() or not r.is_contiguous():
            raise ValueError(f"add_residuals: pair {i}: skip {tuple(s.shape)} and residual {tuple(r.shape)} must be contiguous tensors "
                             "of one shape")
        if s.numel() == 0 or s.numel() % 8 != 0:
            raise ValueError(f"add_residuals: pair {i} has {s.numel()} values, not a positive multiple of 8")
        lo = lo_of(s)
        if lo is not None and (lo.shape != s.shape or lo.stride() != s.stride() or lo.dtype != f16):
            raise ValueError("the low half of a stream tensor must be laid out like the tensor")
        o = torch.empty_like(s) if out is None else _req(out[i], f"out[{i}]")
        if o.shape != s.shape or not o.is_contiguous():
            raise ValueError(f"add_residuals: out[{i}] must be contiguous {tuple(s.shape)}")
        outs.append(o)
        los.append(None if lo is None else (lo if o is s else torch.empty_like(s)))
    for first in range(0, len(skips), _lib.I2V_ADD_RES_MAX):
        p = _lib.AddResidualsParams()
        n = min(_lib.I2V_ADD_RES_MAX, len(skips) - first)
        for j in range(n):
            i, e = first + j, p.t[j]
            e.dst, e.dst_lo, e.skip, e.skip_lo, e.res = _p(outs[i]), _p(los[i]), _p(skips[i]), _p(lo_of(skips[i])), _p(residuals[i])
            e.numel = skips[i].numel()
        p.n = n
        if table is not None:
            p.scale_table, p.scale_rows, p.step_idx = _p(table), table.numel(), _p(idx)
        _lib.check(lib.i2v_add_residuals_f16(C.byref(p), _stream()), "i2v_add_residuals_f16")
    for o, lo in zip(outs, los):
        if lo is not None:
            o._i2v_lo = lo
    return outs


def add_multi_residuals(skips, residual_sets, scale=None, out=None):
    """The residuals of N ControlNets into skip tensors in one launch (i2v_add_multi_residuals_f16): out_i = skip_i + sum_k s_k *
    residual_sets[k][i], summed in fp32 in net order and rounded once.  residual_sets: a list of N (1 .. I2V_ADD_RES_NETS_MAX) lists
    shaped like `skips`.  scale = None (every s_k = 1) or (table fp32 [N, rows], step_idx int32 [1] or None):
    s_k = table[k, clamp(*step_idx)], read on the device.  `out`, the precise residual stream's low halves and the split over several
    launches beyond I2V_ADD_RES_MAX tensors are `add_residuals`'; with N = 1 so are the bits.  Returns the list of results."""
    lib = _lib.load()
    skips, sets = list(skips), [list(r) for r in residual_sets]
    if not 1 <= len(sets) <= _lib.I2V_ADD_RES_NETS_MAX:
        raise ValueError(f"add_multi_residuals: {len(sets)} residual sets, not 1 .. {_lib.I2V_ADD_RES_NETS_MAX}")
    for k, rs in enumerate(sets):
        if len(skips) != len(rs) or not skips:
            raise ValueError(f"add_multi_residuals: {len(skips)} skip tensors and {len(rs)} residuals in set {k}")
    if out is not None and len(out) != len(skips):
        raise ValueError(f"add_multi_residuals: {len(out)} outputs for {len(skips)} skip tensors")
    table = idx = None
    if scale is not None:
        table, idx = scale
        _req(table, "scale table", dtype=torch.float32)
        if table.dim() != 2 or table.shape[0] != len(sets) or table.shape[1] < 1 or not table.is_contiguous():
            raise ValueError(f"add_multi_residuals: the scale table is a contiguous fp32 [{len(sets)}, rows] matrix, one row per set")
        if idx is not None:
            _req(idx, "step_idx", dtype=torch.int32)
    outs, los = [], []
    for i, s in enumerate(skips):
        _req(s, f"skips[{i}]")
        for k, rs in enumerate(sets):
            r = _req(rs[i], f"residual_sets[{k}][{i}]")
            if s.shape != r.shape or not s.is_contiguous() or not r.is_contiguous():
                raise ValueError(f"add_multi_residuals: tensor {i}: skip {tuple(s.shape)} and residual {tuple(r.shape)} of set {k} must "
                                 "be contiguous tensors of one shape")
        if s.numel() == 0 or s.numel() % 8 != 0:
            raise ValueError(f"add_multi_residuals: tensor {i} has {s.numel()} values, not a positive multiple of 8")
        lo = lo_of(s)
        if lo is not None and (lo.shape != s.shape or lo.stride() != s.stride() or lo.dtype != f16):
            raise ValueError("the low half of a stream tensor must be laid out like the tensor")
        o = torch.empty_like(s) if out is None else _req(out[i], f"out[{i}]")
        if o.shape != s.shape or not o.is_contiguous():
            raise ValueError(f"add_multi_residuals: out[{i}] must be contiguous {tuple(s.shape)}")
        outs.append(o)
        los.append(None if lo is None else (lo if o is s else torch.empty_like(s)))
    for first in range(0, len(skips), _lib.I2V_ADD_RES_MAX):
        p = _lib.AddMultiResidualsParams()
        n = min(_lib.I2V_ADD_RES_MAX, len(skips) - first)
        for j in range(n):
            i, e = first + j, p.t[j]
            e.dst, e.dst_lo, e.skip, e.skip_lo = _p(outs[i]), _p(los[i]), _p(skips[i]), _p(lo_of(skips[i]))
            for k, rs in enumerate(sets):
                e.res[k] = _p(rs[i])
            e.numel = skips[i].numel()
        p.n, p.n_nets = n, len(sets)
        if table is not None:
            p.scale_table, p.scale_rows, p.step_idx = _p(table), table.shape[1], _p(idx)
        _lib.check(lib.i2v_add_multi_residuals_f16(C.byref(p), _stream()), "i2v_add_multi_residuals_f16")
    for o, lo in zip(outs, los):
        if lo is not None:
            o._i2v_lo = lo
    return outs


# ---------------------------------------------------------------------------------------------- T2I-Adapter (t2i_adapter.py)
def pixel_unshuffle8(src):
    """PixelUnshuffle(8) of [N, C, H, W] fp32 / fp16 images (C = 1 or 3; H, W multiples of 8) -> tokens fp16 [N, H / 8, W / 8, 64 C] in
    PyTorch's channel order c * 64 + dy * 8 + dx (i2v_pixel_unshuffle8_f16): one rounding."""
    lib = _lib.load()
    _req(src, "src", dtype=None)
    if src.dtype not in (torch.float32, f16) or src.dim() != 4:
        raise TypeError("src must be a 4-D fp32 / fp16 tensor")
    n, c, h, w = src.shape
    if c not in (1, 3) or n < 1 or h < 8 or w < 8 or h % 8 or w % 8:
        raise ValueError(f"pixel_unshuffle8: src {tuple(src.shape)} must be [N, 1 or 3, H, W] with H and W positive multiples of 8")
    src = src.contiguous()
    dst = torch.empty((n, h // 8, w // 8, 64 * c), dtype=f16, device=src.device)
    _lib.check(lib.i2v_pixel_unshuffle8_f16(_p(src), 1 if src.dtype == torch.float32 else 0, _p(dst), n, c, h, w, _stream()),
               "i2v_pixel_unshuffle8_f16")
    return dst


def avgpool2x(x):
    """AvgPool2d(2, stride 2, ceil_mode=True) of tokens [N, H, W, C] (C % 8 == 0) -> [N, ceil(H / 2), ceil(W / 2), C]: a window at the
    edge of an odd size averages its in-bounds taps (i2v_avgpool2x_f16)."""
    lib = _lib.load()
    _req(x, "x")
    if x.dim() != 4 or not x.is_contiguous() or x.numel() == 0 or x.shape[3] % 8:
        raise ValueError(f"avgpool2x: x must be a contiguous [N, H, W, C] tensor with C % 8 == 0, got {tuple(x.shape)}")
    n, h, w, c = x.shape
    out = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=f16, device=x.device)
    _lib.check(lib.i2v_avgpool2x_f16(_p(x), _p(out), n, h, w, c, _stream()), "i2v_avgpool2x_f16")
    return out


def relu(x, out=None):
    """max(x, 0) of a contiguous fp16 tensor (numel % 8 == 0); out = x: in place (i2v_relu_f16)."""
    lib = _lib.load()
    _req(x, "x")
    out = torch.empty_like(x) if out is None else _req(out, "out")
    if not x.is_contiguous() or not out.is_contiguous() or out.shape != x.shape or x.numel() == 0 or x.numel() % 8:
        raise ValueError(f"relu: x and out must be contiguous tensors of one shape with numel % 8 == 0, got {tuple(x.shape)}")
    _lib.check(lib.i2v_relu_f16(_p(x), _p(out), x.numel(), _stream()), "i2v_relu_f16")
    return out


def add_broadcast_residual(x, feat, scale=None, out=None):
    """A T2I-Adapter feature map into the UNet's down path (i2v_add_broadcast_residual_f16): out[i] = x[i] + s * feat[i mod feat.numel()]
    for contiguous fp16 tensors with x.numel() % feat.numel() == 0 and feat.numel() % 8 == 0 -- `feat` is [N, H, W, C] and `x`
    [k N, H, W, C]: one copy of the features serves every repetition of the batch.  scale = None (s = 1) or (table fp32 [rows],
    step_idx int32 [1] or None): s = table[clamp(*step_idx)], read on the device.  out = None: a new tensor; out may be x (in place).
    An x of the precise residual stream (`lo_of`) is added as hi + lo and the result carries a fresh low half (in place: x's own is
    rewritten).  Per element the arithmetic, and the bits, are `add_residuals`'."""
    lib = _lib.load()
    _req(x, "x")
    _req(feat, "feat")
    if not x.is_contiguous() or not feat.is_contiguous():
        raise ValueError("add_broadcast_residual: x and feat must be contiguous")
    if feat.numel() == 0 or feat.numel() % 8 != 0 or x.numel() == 0 or x.numel() % feat.numel() != 0:
        raise ValueError(f"add_broadcast_residual: x has {x.numel()} values and feat {feat.numel()}: feat must hold a positive multiple "
                         "of 8 values that divides x's")
    if tuple(x.shape[1:]) != tuple(feat.shape[1:]):
        raise ValueError(f"add_broadcast_residual: x {tuple(x.shape)} and feat {tuple(feat.shape)} differ behind the batch dimension")
    table = idx = None
    if scale is not None:
        table, idx = scale
        _req(table, "scale table", dtype=torch.float32)
        if table.dim() != 1 or table.numel() < 1 or not table.is_contiguous():
            raise ValueError("add_broadcast_residual: the scale table is a contiguous fp32 vector")
        if idx is not None:
            _req(idx, "step_idx", dtype=torch.int32)
    lo = lo_of(x)
    if lo is not None and (lo.shape != x.shape or lo.stride() != x.stride() or lo.dtype != f16):
        raise ValueError("the low half of a stream tensor must be laid out like the tensor")
    o = torch.empty_like(x) if out is None else _req(out, "out")
    if o.shape != x.shape or not o.is_contiguous():
        raise ValueError(f"add_broadcast_residual: out must be contiguous {tuple(x.shape)}")
    o_lo = None if lo is None else (lo if o is x else torch.empty_like(x))
    _lib.check(lib.i2v_add_broadcast_residual_f16(_p(x), _p(lo), _p(feat), _p(o), _p(o_lo), x.numel(), feat.numel(), _p(table),
                                                  0 if table is None else table.numel(), _p(idx), _stream()),
               "i2v_add_broadcast_residual_f16")
    if o_lo is not None:
        o._i2v_lo = o_lo
    return o


# ---------------------------------------------------------------------------------------------- prompt travel (pipeline)
def interp_rows(src, lo, hi, w, out=None):
    """out[r] = (1 - w[r]) * src[lo[r]] + w[r] * src[hi[r]] (i2v_interp_rows_f16): the per-frame text contexts of prompt travel from the
    keyframes' embeddings, and with w = 0 a row gather.  src fp16 [n_src, ...] (a row = everything behind the leading dimension,
    contiguous, a multiple of 8 values; the leading stride is free); lo, hi (ints) and w (floats) are HOST sequences of one length
    n_out: they are range-checked here -- 0 <= lo, hi < n_src, 0 <= w <= 1 -- and uploaded (the C entry cannot check device tables).
    out: fp16 [n_out, ...] of src's row shape (leading stride free), not overlapping src; None: a new contiguous tensor.
    fp32 arithmetic, one rounding; w == 0 / w == 1 copy a row bit for bit and never read the other one."""
    lib = _lib.load()
    _req(src, "src")
    if src.dim() < 2 or src.shape[0] < 1:
        raise ValueError(f"interp_rows: src must be [n_src, ...] with n_src >= 1, got {tuple(src.shape)}")
    row = tuple(src.shape[1:])
    e = 1
    for s in row:
        e *= s

    def rows_of(t, name):
        if tuple(t.shape[1:]) != row or not t[0].is_contiguous():
            raise ValueError(f"interp_rows: {name} must be [n, {', '.join(map(str, row))}] with contiguous rows, got {tuple(t.shape)} "
                             f"with strides {t.stride()}")
        ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), e)
        if ld < e or ld % 8:
            raise ValueError(f"interp_rows: the row stride {ld} of {name} must be a multiple of 8 and at least the row length {e}")
        return ld
    if e < 8 or e % 8:
        raise ValueError(f"interp_rows: a row holds {e} values, not a positive multiple of 8")
    ld_src = rows_of(src, "src")
    lo_t = torch.as_tensor(lo).reshape(-1)
    hi_t = torch.as_tensor(hi).reshape(-1)
    w_t = torch.as_tensor(w, dtype=torch.float32).reshape(-1)
    if lo_t.is_cuda or hi_t.is_cuda or w_t.is_cuda:
        raise ValueError("interp_rows: lo, hi and w are host tables (they are checked before the upload)")
    n_out = lo_t.numel()
    if n_out < 1 or hi_t.numel() != n_out or w_t.numel() != n_out:
        raise ValueError(f"interp_rows: lo, hi and w must have one length >= 1, got {lo_t.numel()}, {hi_t.numel()}, {w_t.numel()}")
    if lo_t.is_floating_point() or hi_t.is_floating_point() or lo_t.dtype == torch.bool or hi_t.dtype == torch.bool:
        raise TypeError("interp_rows: lo and hi must hold integers")
    n_src = src.shape[0]
    for name, t in (("lo", lo_t), ("hi", hi_t)):
        bad = ((t < 0) | (t >= n_src)).nonzero()
        if bad.numel():
            r = int(bad[0])
            raise ValueError(f"interp_rows: {name}[{r}] = {int(t[r])} is outside src's {n_src} rows")
    bad = (~((w_t >= 0) & (w_t <= 1))).nonzero()
    if bad.numel():
        r = int(bad[0])
        raise ValueError(f"interp_rows: w[{r}] = {float(w_t[r])} is outside [0, 1]")
    if out is None:
        out = torch.empty((n_out,) + row, dtype=f16, device=src.device)
    _req(out, "out")
    if out.dim() != src.dim() or out.shape[0] != n_out or out.device != src.device:
        raise ValueError(f"interp_rows: out must be [{n_out}, ...] on src's device, got {tuple(out.shape)}")
    ld_out = rows_of(out, "out")
    a0, a1 = src.data_ptr(), src.data_ptr() + ((n_src - 1) * ld_src + e) * 2
    b0, b1 = out.data_ptr(), out.data_ptr() + ((n_out - 1) * ld_out + e) * 2
    if a0 < b1 and b0 < a1:
        raise ValueError("interp_rows: out must not overlap src")
    dev = src.device
    lo_d, hi_d, w_d = lo_t.to(torch.int32).to(dev), hi_t.to(torch.int32).to(dev), w_t.to(dev)
    _lib.check(lib.i2v_interp_rows_f16(_p(src), ld_src, n_src, _p(lo_d), _p(hi_d), _p(w_d), _p(out), ld_out, n_out, e, _stream()),
               "i2v_interp_rows_f16")
    return out


# ---------------------------------------------------------------------------------------------- prompt weighting (pipeline)
def weight_embeds(src, weights, restore_mean=True, out=None):
    """out[p, t, :] = fp16((src[p, t, :] * weights[p, t]) * r[p]) with r[p] = sum(src[p]) / sum(weights[p] * src[p]) over the whole
    prompt in fp32, or exactly 1 without `restore_mean` (i2v_weight_embeds_f16).  src fp16 [P, T, D] with D a multiple of 8,
    unit-stride rows and prompts T rows apart (the row stride is free: a column slice of a wider buffer is taken); weights fp32
    [P, T] on src's device; out: as src, `src` itself for in place, None: a new contiguous tensor.  Returns (out, ratio) with ratio
    fp32 [P] on the device; a ratio that is not finite left its prompt at src * weights -- the caller reads it and decides."""
    lib = _lib.load()
    _req(src, "src")
    _req(weights, "weights", dtype=torch.float32)
    if src.dim() != 3 or src.numel() < 1:
        raise ValueError(f"weight_embeds: src must be a non-empty [P, T, D], got {tuple(src.shape)}")
    n, t, d = src.shape
    if d % 8:
        raise ValueError(f"weight_embeds: D = {d} is not a multiple of 8")
    if tuple(weights.shape) != (n, t) or weights.device != src.device:
        raise ValueError(f"weight_embeds: weights must be [{n}, {t}] on src's device, got {tuple(weights.shape)} on {weights.device}")
    weights = weights.contiguous()

    def ld_of(x, name):
        ld = x.stride(1) if t > 1 else max(x.stride(1), d)
        if x.stride(2) != 1 or ld < d or ld % 8 or (n > 1 and x.stride(0) != t * ld):
            raise ValueError(f"weight_embeds: {name} needs unit-stride rows, a row stride that is a multiple of 8 and at least {d}, and "
                             f"prompts {t} rows apart; got strides {x.stride()}")
        return ld
    ld_src = ld_of(src, "src")
    if out is None:
        out = torch.empty((n, t, d), dtype=f16, device=src.device)
    _req(out, "out")
    if tuple(out.shape) != (n, t, d) or out.device != src.device:
        raise ValueError(f"weight_embeds: out must be {(n, t, d)} on src's device, got {tuple(out.shape)}")
    ld_out = ld_of(out, "out")
    ratio = torch.empty(n, dtype=torch.float32, device=src.device)
    _lib.check(lib.i2v_weight_embeds_f16(_p(src), _p(weights), _p(out), _p(ratio), n, t, d, ld_src, ld_out, 1 if restore_mean else 0,
                                         _stream()), "i2v_weight_embeds_f16")
    return out, ratio


# ---------------------------------------------------------------------------------------------- video-to-video with a mask (pipeline)
def masked_renoise(latents, source, noise, mask, coef, step_index):
    """In place: latents = m * latents + (1 - m) * (coef[r][0] * source + coef[r][1] * noise) (i2v_masked_renoise_f32), diffusers'
    inpainting update for a 4-channel UNet.  latents, source, noise fp32 [B, F, C, H, W] contiguous; mask fp32 [B, F, 1, H, W]
    contiguous, one plane for all channels: 1 regenerates (the latent's bits are kept), 0 keeps the source, any float is taken;
    coef fp32 [rows, 2] contiguous; step_index device int32 scalar, READ and not advanced: r = clamp(step_index, 0, rows - 1).
    Table convention: the scheduler-step kernels have already advanced the counter, and they wrap it to 0 after the last row, so row 0
    is (1, 0) -- the clean source after the last step -- and row r >= 1 is (sqrt(abar), sqrt(1 - abar)) of timesteps[r]; a one-step
    schedule falls on row 0 (`I2VAdapterPipeline.renoise_table`).  m == 0 at the row (1, 0) gives the source's bits."""
    lib = _lib.load()
    for t, name in ((latents, "latents"), (source, "source"), (noise, "noise"), (mask, "mask"), (coef, "coef")):
        _req(t, name, dtype=torch.float32)
        if not t.is_contiguous():
            raise ValueError(f"masked_renoise: {name} must be contiguous")
    _req(step_index, "step_index", dtype=torch.int32)
    if latents.dim() != 5 or latents.numel() < 1:
        raise ValueError(f"masked_renoise: latents must be a non-empty [B, F, C, H, W], got {tuple(latents.shape)}")
    b, f, c, h, w = latents.shape
    if tuple(source.shape) != tuple(latents.shape) or tuple(noise.shape) != tuple(latents.shape):
        raise ValueError(f"masked_renoise: source {tuple(source.shape)} and noise {tuple(noise.shape)} must have the latents' shape "
                         f"{tuple(latents.shape)}")
    if tuple(mask.shape) != (b, f, 1, h, w):
        raise ValueError(f"masked_renoise: mask must be {(b, f, 1, h, w)}, got {tuple(mask.shape)}")
    if coef.dim() != 2 or coef.shape[1] != 2 or coef.shape[0] < 1:
        raise ValueError(f"masked_renoise: coef must be [rows >= 1, 2], got {tuple(coef.shape)}")
    if step_index.numel() != 1:
        raise ValueError("masked_renoise: step_index must hold one int32")
    for t in (source, noise, mask, coef, step_index):
        if t.device != latents.device:
            raise ValueError("masked_renoise: all operands must be on the latents' device")
    _lib.check(lib.i2v_masked_renoise_f32(_p(latents), _p(source), _p(noise), _p(mask), _p(coef), coef.shape[0], _p(step_index), b * f, c,
                                          h * w, _stream()), "i2v_masked_renoise_f32")
    return latents


# ---------------------------------------------------------------------------------------------- hires fix: latent upscale + re-noise
def resize_renoise(src, tables, noise=None, a=1.0, b=0.0):
    """out[..., Y, X] = a * sum_ky sum_kx wy[Y, ky] wx[X, kx] src[..., iy[Y, ky], ix[X, kx]] + b * noise[..., Y, X]
    (i2v_resize_renoise_f32): the hires fix's latent upscale with the second pass's re-noise fused in.  src fp32 [..., h, w] contiguous
    (at least 2-D; the leading axes are planes); tables = (iy, wy, ix, wx) from `hires_fix.device_tables`: int32 / fp32 [H, 4] and
    [W, 4] on src's device, H >= h and W >= w (upscaling only); noise None (then `b` is ignored) or fp32 [..., H, W] contiguous.  Returns
    a new fp32 [..., H, W].  All fp32, a fixed-order 16-term sum, then a * r (+ b * noise): the operations of `axpby`, so the fused call
    gives the bits of resize_renoise(src, tables) followed by axpby(out, noise, a, b)."""
    lib = _lib.load()
    iy, wy, ix, wx = tables
    _req(src, "src", dtype=torch.float32)
    for t, name, dt in ((iy, "iy", torch.int32), (wy, "wy", torch.float32), (ix, "ix", torch.int32), (wx, "wx", torch.float32)):
        _req(t, name, dtype=dt)
        if t.dim() != 2 or t.shape[1] != 4 or not t.is_contiguous() or t.device != src.device:
            raise ValueError(f"resize_renoise: {name} must be a contiguous [n_out, 4] table on src's device, got {tuple(t.shape)}")
    if src.dim() < 2 or src.numel() < 1 or not src.is_contiguous():
        raise ValueError(f"resize_renoise: src must be a non-empty contiguous [..., h, w], got {tuple(src.shape)}")
    if iy.shape != wy.shape or ix.shape != wx.shape:
        raise ValueError("resize_renoise: the index and weight tables of an axis must have the same shape")
    h, w = src.shape[-2:]
    height, width = iy.shape[0], ix.shape[0]
    if height < h or width < w:
        raise ValueError(f"resize_renoise: {h} x {w} -> {height} x {width} is a downscale: upscaling only")
    shape = tuple(src.shape[:-2]) + (height, width)
    if noise is not None:
        _req(noise, "noise", dtype=torch.float32)
        if tuple(noise.shape) != shape or not noise.is_contiguous() or noise.device != src.device:
            raise ValueError(f"resize_renoise: noise must be a contiguous {shape} on src's device, got {tuple(noise.shape)}")
    out = torch.empty(shape, dtype=torch.float32, device=src.device)
    planes = src.numel() // (h * w)
    _lib.check(lib.i2v_resize_renoise_f32(_p(src), _p(out), _p(noise) if noise is not None else None, _p(iy), _p(wy), _p(ix), _p(wx),
                                          float(a), float(b), planes, h, w, height, width, _stream()), "i2v_resize_renoise_f32")
    return out


_freeinit_ws = {}


def _freenoise_rows(t, name, rows):
    t, ld = _mat(t, name)
    if t.shape[0] != rows or t.shape[1] % 8 != 0:
        raise ValueError(f"{name} is {tuple(t.shape)}, expected [{rows}, C] with C a multiple of 8")
    return t, ld


def freenoise_gather(t, starts, *, n_pixels, frames, length):
    """FreeNoise's window expansion (i2v_freenoise_gather_f16): t [n_pixels * frames, C] fp16 rows in (b, pixel, frame) order (any row
    stride) -> [n_pixels * windows * length, C], row (p, w, j) = row (p, starts[w] + j) bit for bit.  starts: device int32 [windows]
    (`free_noise.tables`)."""
    lib = _lib.load()
    t, ld = _freenoise_rows(t, "t", n_pixels * frames)
    _req(starts, "starts", dtype=torch.int32)
    if starts.dim() != 1 or not starts.is_contiguous() or starts.numel() < 1:
        raise ValueError("starts must be a contiguous int32 vector")
    windows, c = starts.numel(), t.shape[1]
    out = torch.empty((n_pixels * windows * length, c), dtype=f16, device=t.device)
    _lib.check(lib.i2v_freenoise_gather_f16(_p(t), ld, _p(out), c, _p(starts), n_pixels, frames, windows, length, c, _stream()),
               "i2v_freenoise_gather_f16")
    return out


def freenoise_blend(tw, idx, coef, *, n_pixels, windows, length):
    """FreeNoise's weighted mean of the windows (i2v_freenoise_blend_f16): tw [n_pixels * windows * length, C] fp16 ->
    [n_pixels * frames, C], row (p, f) = sum_k coef[f, k] * row (p, idx[f, k]) in fp32, rounded once.  idx int32 / coef fp32 device
    tables [frames, pairs] (`free_noise.tables`); pairs with coefficient 0 behind the first are padding."""
    lib = _lib.load()
    tw, ld = _freenoise_rows(tw, "tw", n_pixels * windows * length)
    _req(idx, "idx", dtype=torch.int32)
    _req(coef, "coef", dtype=torch.float32)
    if idx.dim() != 2 or idx.shape != coef.shape or not idx.is_contiguous() or not coef.is_contiguous():
        raise ValueError("idx / coef must be contiguous [frames, pairs] tables of one shape")
    frames, pairs = idx.shape
    c = tw.shape[1]
    out = torch.empty((n_pixels * frames, c), dtype=f16, device=tw.device)
    _lib.check(lib.i2v_freenoise_blend_f16(_p(tw), ld, _p(out), c, _p(idx), _p(coef), n_pixels, frames, windows, length, pairs, c,
                                           _stream()), "i2v_freenoise_blend_f16")
    return out


def freeinit_mix(latents, init_noise, z_rand, lpf, sqrt_alpha, sqrt_one_minus_alpha):
    """FreeInit's re-initialisation (i2v_freeinit_mix; diffusers FreeInitMixin._apply_free_init): latents / init_noise / z_rand fp32
    contiguous [B, F, C, H, W], lpf fp32 contiguous [F, H, W] (the centred low-pass table, `free_init.free_init_filter`) -> a new
    tensor: the low frequencies over (F, H, W) of sqrt_alpha * latents + sqrt_one_minus_alpha * init_noise and the high ones of
    z_rand.  F <= 32, H, W <= 128, any length.  The complex workspace (8 bytes per value) is kept per (device, shape): the launches
    are stream-ordered, so consecutive calls share it."""
    lib = _lib.load()
    for t, name in ((latents, "latents"), (init_noise, "init_noise"), (z_rand, "z_rand"), (lpf, "lpf")):
        _req(t, name, dtype=torch.float32)
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if latents.dim() != 5 or init_noise.shape != latents.shape or z_rand.shape != latents.shape:
        raise ValueError(f"latents {tuple(latents.shape)} / init_noise {tuple(init_noise.shape)} / z_rand {tuple(z_rand.shape)} must be "
                         "one shape [B, F, C, H, W]")
    b, f, c, h, w = latents.shape
    if tuple(lpf.shape) != (f, h, w):
        raise ValueError(f"lpf must be {(f, h, w)}, got {tuple(lpf.shape)}")
    if len({t.device for t in (latents, init_noise, z_rand, lpf)}) != 1:
        raise ValueError("latents, init_noise, z_rand and lpf must be on one device")
    need = lib.i2v_freeinit_workspace_bytes(b, f, c, h, w)
    if need < 0:
        _lib.check(int(need), "i2v_freeinit_workspace_bytes")
    key = (str(latents.device), b, f, c, h, w)
    ws = _freeinit_ws.get(key)
    if ws is None or ws.numel() < need:
        _freeinit_ws.clear()                  # one shape at a time, like the pipeline's captured step
        ws = _freeinit_ws[key] = torch.empty(need, dtype=torch.uint8, device=latents.device)
    out = torch.empty_like(latents)
    _lib.check(lib.i2v_freeinit_mix(_p(latents), _p(init_noise), _p(z_rand), _p(lpf), _p(out), _p(ws), ws.numel(), b, f, c, h, w,
                                    float(sqrt_alpha), float(sqrt_one_minus_alpha), _stream()), "i2v_freeinit_mix")
    return out


def vae_tile_blend(tile, out, oy, ox, blend_extent, limit, up=None, left=None, upleft=None, c=None):
    """One tile of the tiled VAE into the stitched image (i2v_vae_tile_blend; diffusers tiled_decode / tiled_encode): tile
    [N, th, tw, ld] token-major, fp32 (the decoder's conv_out) or fp16 (quant_conv), is blended over its first `blend_extent` rows
    with the last rows of `up` [N, up_h, tw, ld] and over its first columns with the last columns of `left` [N, th, left_w, ld]
    (`upleft` [N, up_h, left_w, ld] enters their common corner), cropped to limit x limit and written to
    out[:, :, oy : oy + min(th, limit), ox : ox + min(tw, limit)] of the fp32 NCHW image `out` [N, c, H, W].  The neighbours are the
    RAW tiles (the closed form of diffusers' in-place blends, include/i2v_hip.h); nothing else of `out` is written."""
    lib = _lib.load()
    _req(tile, "tile", dtype=None)
    if tile.dtype not in (torch.float32, f16):
        raise TypeError("tile must be fp16 or fp32")
    if tile.dim() != 4 or not tile.is_contiguous():
        raise ValueError("tile must be contiguous [N, th, tw, ld]")
    n, th, tw, ld = tile.shape
    c = ld if c is None else c
    _req(out, "out", dtype=torch.float32)
    if out.dim() != 4 or not out.is_contiguous() or out.shape[0] != n or out.shape[1] != c:
        raise ValueError(f"out must be contiguous fp32 [{n}, {c}, H, W], got {tuple(out.shape)}")
    up_h = left_w = 0
    if up is not None:
        up_h = up.shape[1] if up.dim() == 4 else 0
        want = (n, up_h, tw, ld)
        if up.dtype != tile.dtype or tuple(up.shape) != want or not up.is_contiguous() or not up.is_cuda:
            raise ValueError(f"up must be a contiguous {tile.dtype} device tensor [{n}, up_h, {tw}, {ld}], got {tuple(up.shape)}")
    if left is not None:
        left_w = left.shape[2] if left.dim() == 4 else 0
        want = (n, th, left_w, ld)
        if left.dtype != tile.dtype or tuple(left.shape) != want or not left.is_contiguous() or not left.is_cuda:
            raise ValueError(f"left must be a contiguous {tile.dtype} device tensor [{n}, {th}, left_w, {ld}], got {tuple(left.shape)}")
    if upleft is not None and up is not None and left is not None:
        if upleft.dtype != tile.dtype or tuple(upleft.shape) != (n, up_h, left_w, ld) or not upleft.is_contiguous() or \
                not upleft.is_cuda:
            raise ValueError(f"upleft must be a contiguous {tile.dtype} device tensor [{n}, {up_h}, {left_w}, {ld}], got "
                             f"{tuple(upleft.shape)}")
    _lib.check(lib.i2v_vae_tile_blend(_p(tile), _p(up), _p(left), _p(upleft), 1 if tile.dtype == torch.float32 else 0, n, th, tw, ld,
                                      c, up_h, left_w, int(blend_extent), int(limit), _p(out), out.shape[2], out.shape[3], int(oy),
                                      int(ox), _stream()), "i2v_vae_tile_blend")
    return out


def lora_merge(dst, base, adapters):
    """dst = round(base + sum_j scale_j * up_j @ down_j) for one weight (i2v_lora_merge): base / dst contiguous, both fp16 or both
    fp32, [out, in] or a conv weight [Cout, Cin, kh, kw] (in = Cin kh kw), not overlapping; `adapters` = [(down, up, scale), ...], at
    most 8, down fp16 [rank, in] (or [rank, Cin, kh, kw]), up fp16 [out, rank] (or [out, rank, 1, 1]), contiguous, rank <= 256.  The
    products are fp32 (MFMA), the scales multiply them in fp32 and the sum is rounded once; `base` is not modified.  `dst` may be a
    Parameter: its version counter is bumped after the launch -- a write through a raw pointer does not do that, and the kernel-layout
    packs (`HipModule.packed`) and the pipeline's graph key are keyed on it."""
    lib = _lib.load()
    _req(base, "base", dtype=None)
    _req(dst, "dst", dtype=None)
    if base.dtype not in (torch.float32, f16) or dst.dtype != base.dtype:
        raise TypeError(f"base and dst must both be fp16 or both fp32, got {base.dtype} and {dst.dtype}")
    if base.dim() < 2 or dst.shape != base.shape or not base.is_contiguous() or not dst.is_contiguous():
        raise ValueError(f"base {tuple(base.shape)} and dst {tuple(dst.shape)} must be contiguous weights of one shape, [out, in, ...]")
    out_f, in_f = base.shape[0], base.numel() // max(base.shape[0], 1)
    if out_f < 1 or in_f < 1:
        raise ValueError(f"empty weight {tuple(base.shape)}")
    arr = (_lib.LoraAdapter * max(len(adapters), 1))()
    for j, (down, up, scale) in enumerate(adapters):
        _req(down, f"adapters[{j}].down")
        _req(up, f"adapters[{j}].up")
        if not down.is_contiguous() or not up.is_contiguous():
            raise ValueError(f"adapters[{j}]: the factors must be contiguous")
        rank = down.shape[0] if down.dim() >= 2 else 0
        if rank < 1 or down.numel() != rank * in_f or up.dim() < 2 or up.shape[0] != out_f or up.numel() != out_f * rank:
            raise ValueError(f"adapters[{j}]: down {tuple(down.shape)} / up {tuple(up.shape)} do not fit a weight [{out_f}, {in_f}] "
                             "(down [rank, in], up [out, rank])")
        arr[j] = _lib.LoraAdapter(down.data_ptr(), up.data_ptr(), rank, float(scale))
    _lib.check(lib.i2v_lora_merge(_p(dst), _p(base), 1 if base.dtype == torch.float32 else 0, out_f, in_f, arr, len(adapters), _stream()),
               "i2v_lora_merge")
    torch.autograd.graph.increment_version(dst)
    return dst


# ---------------------------------------------------------------------------------------------- backward
def transpose_tokens(x, batch_len, out=None):
    """[B * L, C] token-major -> [B, C, pad8(L)] channel-major (zero-filled pad): the K^T / Q^T / dO^T operands of the
    attention backward and the operands of a weight gradient (i2v_transpose_f16).  x may be a column slice."""
    lib = _lib.load()
    x, ldx = _mat(x, "x")
    rows, c = x.shape
    if rows % batch_len != 0:
        raise ValueError(f"{rows} rows do not split into batches of {batch_len}")
    b, lp = rows // batch_len, pad8(batch_len)
    if out is None:
        out = torch.empty((b, c, lp), dtype=f16, device=x.device)
    _req(out, "out")
    if tuple(out.shape) != (b, c, lp) or not out.is_contiguous():
        raise ValueError(f"out must be contiguous [{b}, {c}, {lp}]")
    _lib.check(lib.i2v_transpose_f16(_p(x), batch_len * ldx, ldx, _p(out), c * lp, lp, b, batch_len, c, _stream()),
               "i2v_transpose_f16")
    return out


def attention_lse(q, k, *, batch_q, lq, lk, heads, head_dim, kv_group=1, scale=None):
    """fp32 [batch_q, heads, lq] log2-sum-exp of the forward attention over (q, k) (i2v_attention_lse_f32)."""
    lib = _lib.load()
    q, ldq = _mat(q, "q")
    k, ldk = _mat(k, "k")
    Cc, bkv = heads * head_dim, batch_q // kv_group
    if q.shape[0] != batch_q * lq or q.shape[1] < Cc or k.shape[0] != bkv * lk or k.shape[1] < Cc:
        raise ValueError(f"q {tuple(q.shape)} / k {tuple(k.shape)} do not match batch_q {batch_q}, lq {lq}, lk {lk}")
    lse = torch.empty((batch_q, heads, lq), dtype=torch.float32, device=q.device)
    p = AttnParams()
    p.q, p.q_row_stride, p.q_batch_stride = _p(q), ldq, lq * ldq
    p.k, p.k_row_stride, p.k_batch_stride = _p(k), ldk, lk * ldk
    p.batch_q, p.kv_group, p.heads, p.head_dim, p.lq, p.lk = batch_q, kv_group, heads, head_dim, lq, lk
    p.scale = float(head_dim) ** -0.5 if scale is None else scale
    _lib.check(lib.i2v_attention_lse_f32(C.byref(p), _p(lse), _stream()), "i2v_attention_lse_f32")
    return lse


def rowdot_heads(a, b, *, rows_per_batch, heads, head_dim):
    """fp32 [batches, heads, rows_per_batch]: sum over each head's channels of a * b (delta = rowsum(dO o O))."""
    lib = _lib.load()
    a, lda = _mat(a, "a")
    b, ldb = _mat(b, "b")
    rows = a.shape[0]
    if b.shape[0] != rows or rows % rows_per_batch != 0 or min(a.shape[1], b.shape[1]) < heads * head_dim:
        raise ValueError("rowdot_heads: shape mismatch")
    out = torch.empty((rows // rows_per_batch, heads, rows_per_batch), dtype=torch.float32, device=a.device)
    _lib.check(lib.i2v_rowdot_heads_f32(_p(a), lda, _p(b), ldb, _p(out), rows, rows_per_batch, heads, head_dim, _stream()),
               "i2v_rowdot_heads_f32")
    return out


def attention_bwd(q, k, v, o, dout, *, batch_q, lq, lk, heads, head_dim, kv_group=1, scale=None, need_dkv=True, lse=None):
    """Gradients of softmax(scale q k^T) v with respect to q (and k, v when need_dkv): token-major fp16 matrices in, the
    channel-major operand copies, the log-sum-exp (unless `lse` from the forward pass is given) and delta are made here.  Returns (dq, dk, dv); dk / dv [batch_kv * lk, C]
    are summed over the kv_group batch entries that share k / v (the frames of a clip for the cross-frame attention)."""
    lib = _lib.load()
    q, ldq = _mat(q, "q")
    k, ldk = _mat(k, "k")
    v, ldv = _mat(v, "v")
    o, _ = _mat(o, "o")
    dout, ldo = _mat(dout, "dout")
    Cc, bkv = heads * head_dim, batch_q // kv_group
    sc = float(head_dim) ** -0.5 if scale is None else scale
    if lse is None:   # (the forward pass can hand it over: attention(..., return_lse=True))
        lse = attention_lse(q, k, batch_q=batch_q, lq=lq, lk=lk, heads=heads, head_dim=head_dim, kv_group=kv_group, scale=sc)
    elif lse.dtype != torch.float32 or tuple(lse.shape) != (batch_q, heads, lq) or not lse.is_contiguous():
        raise ValueError(f"lse must be contiguous fp32 [{batch_q}, {heads}, {lq}]")
    delta = rowdot_heads(dout, o, rows_per_batch=lq, heads=heads, head_dim=head_dim)
    kt = transpose_tokens(k[:, :Cc], lk)
    dq = torch.empty((batch_q * lq, Cc), dtype=f16, device=q.device)
    p = AttnBwdParams()
    p.q, p.q_row_stride, p.q_batch_stride = _p(q), ldq, lq * ldq
    p.k, p.k_row_stride, p.k_batch_stride = _p(k), ldk, lk * ldk
    p.v, p.v_row_stride, p.v_batch_stride = _p(v), ldv, lk * ldv
    p.kt, p.kt_row_stride, p.kt_batch_stride = _p(kt), kt.shape[2], Cc * kt.shape[2]
    p.dout, p.do_row_stride, p.do_batch_stride = _p(dout), ldo, lq * ldo
    p.lse, p.delta = _p(lse), _p(delta)
    p.dq, p.dq_row_stride, p.dq_batch_stride = _p(dq), Cc, lq * Cc
    dk = dv = qt = dot = None
    if need_dkv:
        qt, dot = transpose_tokens(q[:, :Cc], lq), transpose_tokens(dout[:, :Cc], lq)
        dk = torch.empty((bkv * lk, Cc), dtype=f16, device=q.device)
        dv = torch.empty((bkv * lk, Cc), dtype=f16, device=q.device)
        p.qt, p.qt_row_stride, p.qt_batch_stride = _p(qt), qt.shape[2], Cc * qt.shape[2]
        p.doutt, p.dot_row_stride, p.dot_batch_stride = _p(dot), dot.shape[2], Cc * dot.shape[2]
        p.dk, p.dk_row_stride, p.dk_batch_stride = _p(dk), Cc, lk * Cc
        p.dv, p.dv_row_stride, p.dv_batch_stride = _p(dv), Cc, lk * Cc
    p.batch_q, p.kv_group, p.heads, p.head_dim, p.lq, p.lk = batch_q, kv_group, heads, head_dim, lq, lk
    p.scale = sc
    parts = dkv_partitions(batch_q, kv_group, heads, head_dim, lq, lk) if need_dkv else 1
    if parts > 1:   # the cross-frame form: too few (key block, head) workgroups for the chip; the frames are dealt out
        ws = torch.empty((2, parts, bkv * lk, Cc), dtype=torch.float32, device=q.device)
        p.kv_partitions, p.dkv_partial = parts, _p(ws)
    _lib.check(lib.i2v_attention_bwd_f16(C.byref(p), _stream()), "i2v_attention_bwd_f16")
    return dq, dk, dv


def dkv_partitions(batch_q, kv_group, heads, head_dim, lq, lk):
    """how many workgroups share the frames of one K / V in the dK / dV sweep (1 = off): the count the library's dispatch rule
    recommends (i2v_attn_bwd_route.kv_partitions); I2V_ATTN_BWD_PARTS=0 turns the partitions off."""
    if os.environ.get("I2V_ATTN_BWD_PARTS", "1") == "0":
        return 1
    return attn_bwd_route(batch_q, kv_group, heads, head_dim, lq, lk)["kv_partitions"]


def layernorm_bwd(x, dn, gamma, eps, add=None):
    """input gradient of LayerNorm (frozen affine): dx = LN'(x)[dn o gamma] (+ add, the residual path's gradient)."""
    lib = _lib.load()
    x, ldx = _mat(x, "x")
    dn, lddn = _mat(dn, "dn")
    _req(gamma, "gamma")
    rows, c = x.shape
    if tuple(dn.shape) != (rows, c) or gamma.numel() != c:
        raise ValueError("layernorm_bwd: shape mismatch")
    lda = 0
    if add is not None:
        add, lda = _mat(add, "add")
        if tuple(add.shape) != (rows, c):
            raise ValueError("layernorm_bwd: add shape mismatch")
    dx = torch.empty((rows, c), dtype=f16, device=x.device)
    _lib.check(lib.i2v_layernorm_bwd_f16(_p(x), ldx, _p(dn), lddn, _p(gamma.contiguous()), _p(add), lda, _p(dx), c, rows, c,
                                         float(eps), _stream()), "i2v_layernorm_bwd_f16")
    return dx


def geglu(h):
    """y [rows, inner] = value * gelu_erf(gate) from the interleaved (value, gate) pre-activation h [rows, 2 inner]
    (i2v_geglu_f16: what the I2V_EPI_GEGLU epilogue applies, run on a stored h)."""
    lib = _lib.load()
    h, ldh = _mat(h, "h")
    rows, two_inner = h.shape
    if two_inner % 16 != 0:
        raise ValueError("geglu: the inner width must be a multiple of 8")
    y = torch.empty((rows, two_inner // 2), dtype=f16, device=h.device)
    _lib.check(lib.i2v_geglu_f16(_p(h), ldh, _p(y), two_inner // 2, rows, two_inner // 2, _stream()), "i2v_geglu_f16")
    return y


def geglu_bwd(h, dy):
    """h [rows, 2 inner] interleaved (value, gate) pre-activation, dy [rows, inner] -> dh [rows, 2 inner] (same order)."""
    lib = _lib.load()
    h, ldh = _mat(h, "h")
    dy, lddy = _mat(dy, "dy")
    rows, two_inner = h.shape
    if dy.shape[0] != rows or dy.shape[1] * 2 != two_inner:
        raise ValueError("geglu_bwd: shape mismatch")
    dh = torch.empty((rows, two_inner), dtype=f16, device=h.device)
    _lib.check(lib.i2v_geglu_bwd_f16(_p(h), ldh, _p(dy), lddy, _p(dh), two_inner, rows, two_inner // 2, _stream()),
               "i2v_geglu_bwd_f16")
    return dh


_colsum_ws = {}


def _colsum_workspace(lib, rows, cols, device):
    """scratch of the fixed-order column sums, one per device, grown on demand (stream-ordered use)"""
    need = lib.i2v_colsum_workspace_bytes(rows, cols)
    ws = _colsum_ws.get(device)
    if ws is None or ws.numel() * 4 < need:
        ws = _colsum_ws[device] = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=device)
    return ws


def colsum(x, out=None):
    """fp32 [cols] += sum over the rows of fp16 x (bias gradient); block sums added in a fixed order: bit-reproducible."""
    lib = _lib.load()
    x, ldx = _mat(x, "x")
    if out is None:
        out = torch.zeros((x.shape[1],), dtype=torch.float32, device=x.device)
    _req(out, "out", dtype=torch.float32)
    ws = _colsum_workspace(lib, x.shape[0], x.shape[1], x.device)
    _lib.check(lib.i2v_colsum_det_f32(_p(x), ldx, None, 0, _p(out), x.shape[0], x.shape[1], _p(ws), _stream()), "i2v_colsum_det_f32")
    return out


def colsum_prod(a, b, out=None):
    """fp32 [cols] += sum over the rows of a o b (fp16 matrices of one shape): the gain gradient of a norm; fixed order."""
    lib = _lib.load()
    a, lda = _mat(a, "a")
    b, ldb = _mat(b, "b")
    if a.shape != b.shape:
        raise ValueError(f"colsum_prod: {tuple(a.shape)} vs {tuple(b.shape)}")
    if out is None:
        out = torch.zeros((a.shape[1],), dtype=torch.float32, device=a.device)
    _req(out, "out", dtype=torch.float32)
    ws = _colsum_workspace(lib, a.shape[0], a.shape[1], a.device)
    _lib.check(lib.i2v_colsum_det_f32(_p(a), lda, _p(b), ldb, _p(out), a.shape[0], a.shape[1], _p(ws), _stream()), "i2v_colsum_det_f32")
    return out


def masked_mse_grad(y, target, frames, coef):
    """seed gradient of the training loss (train_image_to_video.py:848-856): coef * (y - target) on the tokens of every
    frame but the first of each clip, 0 there.  y, target fp16 [n_img, tokens, C] contiguous."""
    lib = _lib.load()
    _req(y, "y")
    _req(target, "target")
    if y.dim() != 3 or y.shape != target.shape or not y.is_contiguous() or not target.is_contiguous():
        raise ValueError("masked_mse_grad: y / target must be equal-shape contiguous [n_img, tokens, C]")
    g = torch.empty_like(y)
    _lib.check(lib.i2v_masked_mse_grad_f16(_p(y), _p(target), _p(g), y.shape[0], y.shape[1], y.shape[2], frames, float(coef),
                                           _stream()), "i2v_masked_mse_grad_f16")
    return g


def masked_mse_grad_f32(y, target, frames, coef):
    """the same seed from an fp32 prediction and target [n_img, tokens, C] (train_image_to_video.py:848: the loss is taken in
    fp32).  Returns (fp16 gradient, fp32 [n_img * tokens] row sums of (y - target)^2 over the unmasked rows)."""
    lib = _lib.load()
    _req(y, "y", dtype=torch.float32)
    _req(target, "target", dtype=torch.float32)
    if y.dim() != 3 or y.shape != target.shape or not y.is_contiguous() or not target.is_contiguous():
        raise ValueError("masked_mse_grad_f32: y / target must be equal-shape contiguous [n_img, tokens, C]")
    g = torch.empty(y.shape, dtype=f16, device=y.device)
    rowsq = torch.empty((y.shape[0] * y.shape[1],), dtype=torch.float32, device=y.device)
    _lib.check(lib.i2v_masked_mse_grad_f32(_p(y), _p(target), _p(g), _p(rowsq), y.shape[0], y.shape[1], y.shape[2], frames,
                                           float(coef), _stream()), "i2v_masked_mse_grad_f32")
    return g, rowsq


def groupnorm_bwd(x, dy, gamma, beta, groups, eps, *, x2=None, silu=False, frames_per_stat=1):
    """input gradient of groupnorm(x [, x2], ...): dy [N, H, W, C1 + C2] -> dx [N, H, W, C1] (, dx2 [N, H, W, C2])."""
    lib = _lib.load()
    _req(x, "x")
    _req(dy, "dy")
    if x.dim() != 4 or not x.is_contiguous() or not dy.is_contiguous():
        raise ValueError("x / dy must be contiguous [N, H, W, C]")
    n, h, w, c1 = x.shape
    c2 = 0
    if x2 is not None:
        _req(x2, "x2")
        if x2.dim() != 4 or not x2.is_contiguous() or x2.shape[:3] != x.shape[:3]:
            raise ValueError("x2 must be contiguous [N, H, W, C2] with the same N, H, W as x")
        c2 = x2.shape[3]
    Cc = c1 + c2
    if tuple(dy.shape) != (n, h, w, Cc) or gamma.numel() != Cc or beta.numel() != Cc:
        raise ValueError("groupnorm_bwd: shape mismatch")
    ws = torch.empty((lib.i2v_groupnorm_bwd_workspace_bytes(n, h * w, Cc) + 3) // 4, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    dx2 = torch.empty_like(x2) if x2 is not None else None
    p = GnParams()
    p.x, p.c1, p.x2, p.c2 = _p(x), c1, _p(x2), c2
    p.gamma, p.beta = _p(_req(gamma, "gamma").contiguous()), _p(_req(beta, "beta").contiguous())
    p.n_img, p.hw, p.groups, p.frames_per_stat = n, h * w, groups, frames_per_stat
    p.eps, p.silu = eps, 1 if silu else 0
    p.workspace = _p(ws)
    _lib.check(lib.i2v_groupnorm_bwd_f16(C.byref(p), _p(dy), _p(dx), _p(dx2), _stream()), "i2v_groupnorm_bwd_f16")
    return (dx, dx2) if x2 is not None else dx


def add(a, b, out=None):
    """a + b (fp16, same shape, contiguous)."""
    lib = _lib.load()
    _req(a, "a")
    _req(b, "b")
    if a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous() or a.numel() % 8 != 0:
        raise ValueError("add: equal-shape contiguous tensors with a multiple of 8 elements expected")
    if out is None:
        out = torch.empty_like(a)
    _lib.check(lib.i2v_add_f16(_p(a), _p(b), _p(out), a.numel(), _stream()), "i2v_add_f16")
    return out


def permute_rows(x, batches, frames, hw, to_pixel_major):
    """[batches * frames * hw, C] rows (b, f, p) -> (b, p, f) (to_pixel_major) or back."""
    lib = _lib.load()
    x, ldx = _mat(x, "x")
    if x.shape[0] != batches * frames * hw or ldx != x.shape[1]:
        raise ValueError("permute_rows: contiguous [batches * frames * hw, C] expected")
    y = torch.empty_like(x)
    _lib.check(lib.i2v_permute_rows_f16(_p(x), _p(y), batches, frames, hw, x.shape[1], 1 if to_pixel_major else 0, _stream()),
               "i2v_permute_rows_f16")
    return y


def zero_insert2x(x):
    """[N, H, W, C] -> [N, 2H, 2W, C] with x at the even positions and zeros elsewhere."""
    lib = _lib.load()
    _req(x, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("zero_insert2x: contiguous [N, H, W, C] expected")
    n, h, w, c = x.shape
    y = torch.empty((n, 2 * h, 2 * w, c), dtype=f16, device=x.device)
    _lib.check(lib.i2v_zero_insert2x_f16(_p(x), _p(y), n, h, w, c, _stream()), "i2v_zero_insert2x_f16")
    return y


def sum_pool2x(x):
    """[N, 2H, 2W, C] -> [N, H, W, C]: sums of the 2 x 2 blocks."""
    lib = _lib.load()
    _req(x, "x")
    if x.dim() != 4 or not x.is_contiguous() or x.shape[1] % 2 or x.shape[2] % 2:
        raise ValueError("sum_pool2x: contiguous [N, 2H, 2W, C] expected")
    n, h2, w2, c = x.shape
    y = torch.empty((n, h2 // 2, w2 // 2, c), dtype=f16, device=x.device)
    _lib.check(lib.i2v_sum_pool2x_f16(_p(x), _p(y), n, h2 // 2, w2 // 2, c, _stream()), "i2v_sum_pool2x_f16")
    return y


def sumsq(x, out=None):
    """fp32 [1] += sum of squares of a flat fp32 tensor (the global gradient norm)."""
    lib = _lib.load()
    _req(x, "x", dtype=torch.float32)
    if not x.is_contiguous():
        raise ValueError("sumsq: contiguous tensor expected")
    if out is None:
        out = torch.zeros((1,), dtype=torch.float32, device=x.device)
    _lib.check(lib.i2v_sumsq_f32(_p(x), x.numel(), _p(out), _stream()), "i2v_sumsq_f32")
    return out


def adamw_step(param, grad, exp_avg, exp_avg_sq, *, lr, betas, eps, weight_decay, step, grad_coef=1.0, norm_sq=None,
               max_norm=0.0):
    """in-place AdamW update of a flat fp32 bucket (i2v_adamw_f32)."""
    lib = _lib.load()
    for t, name in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _req(t, name, dtype=torch.float32)
        if not t.is_contiguous() or t.numel() != param.numel():
            raise ValueError(f"adamw_step: {name} must be contiguous with {param.numel()} elements")
    _lib.check(lib.i2v_adamw_f32(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), float(lr), float(betas[0]),
                                 float(betas[1]), float(eps), float(weight_decay), int(step), float(grad_coef), _p(norm_sq),
                                 float(max_norm), _stream()), "i2v_adamw_f32")
    return param


def adamw_guarded_step(param, grad, exp_avg, exp_avg_sq, *, lr, betas, eps, weight_decay, grad_coef, max_norm, partials,
                       norm_sq, applied_steps, found_inf):
    """clip_grad_norm_ + AdamW of a flat fp32 bucket in one call, deterministic and overflow-safe (i2v_adamw_guarded_f32):
    `partials` fp32 [<= 1024] scratch, `norm_sq` fp32 [1] (out: sum grad^2), `applied_steps` int32 [1] (device step counter,
    advanced only by an applied step), `found_inf` int32 [1] (out: 1 = the gradients held inf / NaN and NOTHING was updated)."""
    lib = _lib.load()
    for t, name in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _req(t, name, dtype=torch.float32)
        if not t.is_contiguous() or t.numel() != param.numel():
            raise ValueError(f"adamw_guarded_step: {name} must be contiguous with {param.numel()} elements")
    _req(partials, "partials", dtype=torch.float32)
    _req(norm_sq, "norm_sq", dtype=torch.float32)
    _req(applied_steps, "applied_steps", dtype=torch.int32)
    _req(found_inf, "found_inf", dtype=torch.int32)
    if not partials.is_contiguous() or not 1 <= partials.numel() <= 1024:
        raise ValueError("adamw_guarded_step: partials must be a contiguous fp32 vector of 1 .. 1024 elements")
    _lib.check(lib.i2v_adamw_guarded_f32(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), float(lr),
                                         float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(grad_coef),
                                         float(max_norm), _p(partials), partials.numel(), _p(norm_sq), _p(applied_steps),
                                         _p(found_inf), _stream()), "i2v_adamw_guarded_f32")
    return param


def axpby(y, x, a, b):
    """y = a y + b x in place over flat fp32 tensors (i2v_axpby_f32: gradient accumulation, EMA of the trained weights)."""
    lib = _lib.load()
    _req(y, "y", dtype=torch.float32)
    _req(x, "x", dtype=torch.float32)
    if not y.is_contiguous() or not x.is_contiguous() or y.numel() != x.numel():
        raise ValueError("axpby: two contiguous fp32 tensors of equal size expected")
    _lib.check(lib.i2v_axpby_f32(_p(y), _p(x), float(a), float(b), y.numel(), _stream()), "i2v_axpby_f32")
    return y
