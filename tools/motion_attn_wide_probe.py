"""Time the 32^2 level's motion attention sub-block as one launch (i2v_motion_attn_wide_f16: 32768 rows = CFG 2 x 16 frames x 1024
pixels, C = 640, 8 heads of 80) against the launches it replaces, issued by the product's own route
(TemporalTransformerBlock._fwd_attn with I2V_MOTION_FUSED_WIDE's switch on and off: LN-folded q|k GEMM, LN-folded V^T GEMM, temporal
attention, to_out GEMM + residual).  Each figure is one sub-block: the mean of `--launches` (30) back-to-back launches between two
events, repeated `--repeats` (7) times; the spread of the repeats is printed beside the median, and the un-fused chain's launches
one by one (KernelProfile)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=32768)
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--repeats", type=int, default=7)
a = ap.parse_args()

import i2v_adapter_unofficial_amd as pkg  # noqa: E402
from i2v_adapter_unofficial_amd import blocks  # noqa: E402
from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_  # noqa: E402
from i2v_adapter_unofficial_amd.profiling import KernelProfile  # noqa: E402

dev = torch.device("cuda:0")
c, heads, d, F = 640, 8, 80, 16
with torch.device("meta"):
    m = pkg.TransformerTemporalModel(num_attention_heads=heads, attention_head_dim=d, in_channels=c, norm_num_groups=32, attention_bias=False,
                                     activation_fn="geglu", positional_embeddings="sinusoidal", num_positional_embeddings=32)
m = m.to_empty(device=dev).half()
init_random_weights_(m, seed=640, norm_jitter=0.1)
blk = m.eval().transformer_blocks[0]
x = torch.randn(a.rows, c, device=dev, generator=torch.Generator(device=dev).manual_seed(0)).half()
fold = blk._fold_ok(x, F, sites=("attn",))[0]


def sub_blocks(wide):
    blocks.FUSED_MOTION_ATTN_WIDE = wide
    with torch.no_grad():
        return blk._fwd_attn(x, a.rows // F, F, fold)          # both attention sub-blocks of the module


def timeit(wide):
    for _ in range(3):
        sub_blocks(wide)
    out = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches // 2):
            sub_blocks(wide)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / (2 * (a.launches // 2)) * 1e3)
    return out


ref, got = sub_blocks(False), sub_blocks(True)
print(f"rows {a.rows} C {c} F {F} h{heads} d{d}; LayerNorm fold in the un-fused chain: {fold}; wide kernel taken: "
      f"{pkg.kernels.motion_attn_wide_supported(a.rows, c, heads, d, F)}")
print(f"max |fused - un-fused| after both sub-blocks {(ref.float() - got.float()).abs().max().item():.3e}  (max |ref| {ref.float().abs().max().item():.3e})")
res = {}
for rnd in range(2):                     # un-fused, fused, un-fused, fused
    for wide in (False, True):
        res.setdefault(wide, []).extend(timeit(wide))
for wide, name in ((False, "un-fused chain (4 launches)"), (True, "i2v_motion_attn_wide_f16 (1 launch)")):
    t = res[wide]
    print(f"{name:38s} per sub-block: median {statistics.median(t):7.1f} us   min {min(t):7.1f}   max {max(t):7.1f}   ({len(t)} x {a.launches} launches)")
print(f"slowest fused {max(res[True]):.1f} us vs fastest un-fused {min(res[False]):.1f} us: "
      f"{'faster by more than the spread' if max(res[True]) < min(res[False]) else 'NOT separated from the spread'}")
for wide in (False, True):
    with KernelProfile() as prof:
        for _ in range(a.launches // 2):
            sub_blocks(wide)
    for tag, v in sorted(prof.by_shape().items(), key=lambda kv: -kv[1]["ms"]):
        print(f"  {'fused   ' if wide else 'un-fused'} {tag:100s} {v['calls']:4d} calls {v['ms'] / v['calls'] * 1e3:8.1f} us  {v['tflops']:6.0f} TFLOP/s {v['gbps']:6.0f} GB/s")
blocks.FUSED_MOTION_ATTN_WIDE = True
