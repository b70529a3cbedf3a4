"""The motion module's attention sub-block at the 32^2 level in one launch (i2v_motion_attn_wide_f16: C = 640, 8 heads of 80, 16
frames, 64-row tiles, to_out + residual inside) against an fp32 torch restatement of the sub-block, and against the un-fused
chain of launches it replaces.

Tolerance: the SAME inputs go through the un-fused chain (LayerNorm + pe, q|k GEMM, V^T GEMM, temporal attention, to_out GEMM +
residual -- direct `kernels` calls) and are compared with the same fp32 reference; the fused form's max-abs and rms error may be
at most 1.5x the chain's.  Both round LayerNorm's output, q, k, v, P and o to fp16 and accumulate in fp32, so the 1.5x only allows
for a different but equivalent rounding order; a wrong fragment or a missed row shows as 10x or more.  Each measured pair is
printed and appended to the file $I2V_MOTION_WIDE_LOG names (profiles/motion_attn_wide_errors.jsonl is one such run on MI355X).

Shapes: 64 rows (one tile), 128 (both panels, one hand-over), 320 (an odd tile count), 64 x (CU count + 1) (the second round of
the persistent walk), each contiguous and with row strides of C + 64.
"""
import json
import os

import pytest
import torch

from tests.parity import compare, hip_model_random, host_threads, oracle_from_hip
from tests.test_full_width_gpu import MODULE_REL_TOL

pytestmark = pytest.mark.gpu

C_, HEADS, D, F = 640, 8, 80, 16
EPS = 1e-5
FACTOR = 1.5


def _K():
    from i2v_adapter_unofficial_amd import kernels
    return kernels


def _h(t):
    return t.half().float()


@pytest.fixture(scope="module")
def weights(dev):
    """fp16-representable constants of one sub-block (fp32 masters on the device) and their kernel-layout packs"""
    from i2v_adapter_unofficial_amd.blocks import SinusoidalPositionalEmbedding
    K = _K()
    g = torch.Generator().manual_seed(640)
    w = {n: _h(torch.randn(C_, C_, generator=g) * C_ ** -0.5).to(dev) for n in ("wq", "wk", "wv", "wo")}
    w["bo"] = _h(torch.randn(C_, generator=g) * 0.1).to(dev)
    w["gamma"] = _h(1.0 + 0.1 * torch.randn(C_, generator=g)).to(dev)
    w["beta"] = _h(0.1 * torch.randn(C_, generator=g)).to(dev)
    w["pe"] = _h(SinusoidalPositionalEmbedding(C_, max_seq_length=32).pe[0]).to(dev)
    w["tables"] = K.motion_attn_tables(w["gamma"].half(), w["beta"].half(), w["pe"].half(), F)
    w["wqkv"] = K.pack_motion_qkv(w["wq"].half(), w["wk"].half(), w["wv"].half(), HEADS)
    w["wo_frag"] = K.pack_attn_out(w["wo"].half(), w["bo"].half(), HEADS)
    return w


def _reference(x, w):
    """the sub-block in fp32: x [rows, C] fp16-representable, rows in (pixel, frame) order"""
    x = x.float()
    n = torch.nn.functional.layer_norm(x, (C_,), w["gamma"], w["beta"], EPS) + w["pe"][:F].repeat(x.shape[0] // F, 1)
    q, k, v = ((n @ w[m].T).view(-1, F, HEADS, D).transpose(1, 2) for m in ("wq", "wk", "wv"))      # [pixels, heads, F, d]
    p = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(-1, C_)
    return x + o @ w["wo"].T + w["bo"]


def _chain(x, w):
    """the launches the fused form replaces, as TemporalTransformerBlock._fwd_attn issues them without the LayerNorm fold"""
    K = _K()
    n = K.layernorm(x, w["gamma"].half(), w["beta"].half(), EPS, pe=w["pe"].half(), pe_period=F)
    vt = K.project_vt(n, w["wv"].half(), F)
    qk = K.gemm(n, torch.cat([w["wq"], w["wk"]], dim=0).half())
    o = K.temporal_attention(qk[:, :C_], qk[:, C_:], vt, n_pixels=x.shape[0] // F, frames=F, heads=HEADS, head_dim=D, scale=D ** -0.5)
    return K.gemm(o, w["wo"].half(), w["bo"].half(), residual=x)


_cases = {}


def _case(rows, dev, w):
    """(x fp16, fp32 reference, the chain's (max-abs, rms) error): computed once per row count, never modified"""
    if rows not in _cases:
        x = torch.randn(rows, C_, generator=torch.Generator().manual_seed(rows)).half().to(dev)
        ref = _reference(x, w)
        _cases[rows] = (x, ref, _errors(_chain(x, w), ref))
    return _cases[rows]


def _errors(got, ref):
    d = got.float() - ref
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def _row_counts(dev):
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    return {"one_tile": 64, "two_panels": 128, "odd_tiles": 64 * 5, "second_round": 64 * (min(cus, 512) + 1)}


@pytest.mark.parametrize("pad", [0, 64], ids=["contiguous", "strided"])
@pytest.mark.parametrize("shape", ["one_tile", "two_panels", "odd_tiles", "second_round"])
def test_wide_kernel_vs_fp32_and_chain(dev, weights, shape, pad):
    K = _K()
    rows = _row_counts(dev)[shape]
    assert K.motion_attn_wide_supported(rows, C_, HEADS, D, F)
    x, ref, (chain_max, chain_rms) = _case(rows, dev, weights)
    xb = torch.full((rows, C_ + pad), float("nan"), dtype=torch.float16, device=dev)
    xb[:, :C_] = x
    ob = torch.full((rows, C_ + pad), 7.0, dtype=torch.float16, device=dev)
    got = K.motion_attn_wide(xb[:, :C_], weights["tables"][0], weights["tables"][1], weights["wqkv"], heads=HEADS, head_dim=D, frames=F,
                             eps=EPS, out_proj=weights["wo_frag"], out=ob[:, :C_])
    assert torch.isfinite(got).all()
    assert pad == 0 or bool((ob[:, C_:] == 7.0).all())              # nothing written between the rows
    err_max, err_rms = _errors(got, ref)
    rec = dict(name=f"motion_attn_wide {rows}x{C_} F{F} {'ld' + str(C_ + pad)}", fused_max=err_max, fused_rms=err_rms,
               chain_max=chain_max, chain_rms=chain_rms, max_ref=ref.abs().max().item())
    print(json.dumps(rec))
    path = os.environ.get("I2V_MOTION_WIDE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert err_max <= FACTOR * chain_max, f"max-abs {err_max:.4e} > {FACTOR} x the un-fused chain's {chain_max:.4e}"
    assert err_rms <= FACTOR * chain_rms, f"rms {err_rms:.4e} > {FACTOR} x the un-fused chain's {chain_rms:.4e}"


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "switch_off"])
def test_motion_module_c640_routes(dev, wide):
    """TransformerTemporalModel at C = 640 on a 4 x 4 grid, 2 x 16 frames (512 rows) against the oracle module: through the wide
    kernel (the launch tags say that it ran) and with I2V_MOTION_FUSED_WIDE's switch off (the un-fused chain)."""
    from oracle.blocks import TransformerTemporalModel as O
    from i2v_adapter_unofficial_amd import TransformerTemporalModel, blocks, kernels as K
    from i2v_adapter_unofficial_amd.profiling import KernelProfile
    host_threads()
    hw = 4
    kw = dict(num_attention_heads=HEADS, attention_head_dim=D, in_channels=C_, norm_num_groups=32, attention_bias=False,
              activation_fn="geglu", positional_embeddings="sinusoidal", num_positional_embeddings=32)
    m = hip_model_random(kw, dev, seed=C_ + hw + 1, cls=TransformerTemporalModel)
    o = oracle_from_hip(m, O, kw)
    x = _h(torch.randn(2 * F, C_, hw, hw, generator=torch.Generator().manual_seed(C_ + 1)))
    assert K.motion_attn_wide_supported(2 * F * hw * hw, C_, HEADS, D, F) and not K.motion_attn_supported(2 * F * hw * hw, C_, HEADS, D, F)
    assert blocks.FUSED_MOTION_ATTN and blocks.FUSED_ATTN_OUT and blocks.FUSED_MOTION_ATTN_WIDE
    blocks.FUSED_MOTION_ATTN_WIDE = wide
    try:
        with torch.no_grad(), KernelProfile() as prof:
            got = m(x.half().to(dev), num_frames=F)[0]
    finally:
        blocks.FUSED_MOTION_ATTN_WIDE = True
    tags = [rec[5] for rec in prof.records]
    fused_tag = f"motion_attn {2 * F * hw * hw}x{C_} F{F} h{HEADS} d{D} (LN + q,k,v + attention + to_out + residual)"
    assert tags.count(fused_tag) == (2 if wide else 0), tags
    assert sum(t.startswith("temporal_attention ") for t in tags) == (0 if wide else 2), tags
    with torch.no_grad():
        ref = o(x, num_frames=F)[0]
    compare(got, ref, rel=MODULE_REL_TOL, name=f"motion module C={C_} {hw}x{hw} F={F}, {'wide kernel' if wide else 'un-fused chain'}")
