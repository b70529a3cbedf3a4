"""FreeU on the GPU: `i2v_freeu_f16` against the literal FFT form in fp64 (tests/freeu_reference.py), the precise residual stream's
hi + lo pair through it, the reduced UNet's forward against the oracle with FreeU hooked into its up blocks, the switch's bit-exact
off state, the pipeline (captured graph == eager, re-capture when FreeU changes, trajectories with both schedulers) and a forward plan
recorded with FreeU replayed through the model handle's C entry point."""
import struct

import pytest
import torch

from tests.dpm_reference import ReferenceDPMSolver
from tests.freeu_reference import SD15_FREEU, hook_oracle_unet, tokens_reference
from tests.parity import (REL_TOL_TRAJECTORY, REL_TOL_UNET, compare, hip_unet_from_oracle, oracle_small_unet)
from tests.test_precise_stream_gpu import PAIR_TOL, check_pair, pair

pytestmark = pytest.mark.gpu


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h16(t):
    return t.half().float()


# ---------------------------------------------------------------------------------------------------------- the kernel
def _one_ulp_ok(got, ref64, name):
    """|out - ref| <= 2^-10 max(|ref|, 2^-14) elementwise: one fp16 ulp.  The kernel rounds once from fp32 (half an ulp); the fp32
    accumulation over <= 576 terms is orders of magnitude below that."""
    got64 = got.double().cpu()
    assert torch.isfinite(got64).all(), f"{name}: non-finite values"
    err = (got64 - ref64).abs()
    bound = 2.0 ** -10 * torch.clamp(ref64.abs(), min=2.0 ** -14)
    worst = (err / bound).max().item()
    print(f"{name}: max |err| / (one fp16 ulp) = {worst:.3f}")
    assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} elements off by more than one fp16 ulp (worst {worst:.3f} ulp)"
    return worst


KERNEL_CASES = [
    # n, h, w, c1 (hidden), c2 (skip), b, s
    (32, 8, 8, 1280, 1280, 1.2, 0.9),        # up block 0 at 16 f x 512^2 with CFG
    (32, 16, 16, 1280, 640, 1.4, 0.2),       # up block 1, its last resnet (skip of 640 channels)
    (32, 16, 16, 640, 640, 1.4, 0.2),
    (32, 8, 8, 640, 1280, 0.7, 1.6),         # b < 1, s > 1
    (4, 12, 12, 1280, 1280, 1.2, 0.9),       # 768^2
    (8, 24, 24, 1280, 640, 1.4, 0.2),
    (8, 5, 4, 128, 128, 1.2, 0.9),           # 36 x 28 latents: up block 0 ...
    (8, 9, 7, 128, 64, 1.4, 0.2),            # ... and up block 1
    (3, 9, 7, 24, 72, 1.4, 0.2),             # multiples of 8 that are not multiples of the 64-channel chunk; c1 / 2 = 12 splits a lane
    (2, 2, 2, 128, 128, 1.2, 0.9),           # the smallest plane (16 x 16 latents, up block 0 of the reduced UNet)
    (2, 4, 4, 128, 128, 1.0, 1.0),           # the identity
]


@pytest.mark.parametrize("n,hh,ww,c1,c2,b,s", KERNEL_CASES)
def test_kernel_against_the_fft_form(dev, n, hh, ww, c1, c2, b, s):
    K = pkg().kernels
    g = torch.Generator().manual_seed(n * 1000 + hh * 10 + ww + c1)
    hid, skip = torch.randn(n, hh, ww, c1, generator=g).half(), torch.randn(n, hh, ww, c2, generator=g).half()
    hd, sd = hid.to(dev), skip.to(dev)
    ho, so = K.freeu(hd, sd, b, s)
    torch.cuda.synchronize()
    assert ho.shape == hid.shape and so.shape == skip.shape and ho.dtype == so.dtype == torch.float16
    assert torch.equal(hd.cpu(), hid) and torch.equal(sd.cpu(), skip), "the inputs must not be modified"
    assert ho.data_ptr() != hd.data_ptr() and so.data_ptr() != sd.data_ptr() and K.lo_of(ho) is None
    ref_h, ref_s = tokens_reference(hid, skip, b, s)
    name = f"freeu {n}x{hh}x{ww} c1={c1} c2={c2} b={b} s={s}"
    _one_ulp_ok(ho, ref_h, name + " hidden")
    _one_ulp_ok(so, ref_s, name + " skip")
    assert torch.equal(ho[..., c1 // 2:].cpu(), hid[..., c1 // 2:]), "the untouched half of the hidden channels must be bit-identical"
    if b == 1.0 and s == 1.0:
        assert torch.equal(ho.cpu(), hid)
    else:
        assert (so.float().cpu() - skip.float()).abs().max().item() > 1e-2


def test_kernel_keeps_special_values_in_the_copied_half(dev):
    """the copied channels are moved, not computed with: -0, subnormals, inf and NaN payloads survive"""
    K = pkg().kernels
    hid = torch.randn(2, 4, 4, 16, generator=torch.Generator().manual_seed(2)).half()
    bits = hid.view(torch.int16)
    bits[..., 8] = -32768           # -0.0
    bits[..., 9] = 1                # the smallest subnormal
    bits[..., 10] = 0x7C00          # +inf
    bits[..., 11] = 0x7E01          # a NaN with a payload
    skip = torch.randn(2, 4, 4, 8, generator=torch.Generator().manual_seed(3)).half()
    ho, _ = K.freeu(hid.to(dev), skip.to(dev), 1.3, 0.5)
    assert torch.equal(ho.cpu().view(torch.int16)[..., 8:], bits[..., 8:])


def test_wrapper_rejects_what_the_kernel_does_not_take(dev):
    K = pkg().kernels
    z = lambda *s: torch.zeros(*s, dtype=torch.float16, device=dev)
    with pytest.raises(pkg()._lib.HipLibraryError, match="not implemented for this problem"):
        K.freeu(z(2, 1, 4, 16), z(2, 1, 4, 16), 1.2, 0.9)
    with pytest.raises(pkg()._lib.HipLibraryError, match="multiples of 8"):
        K.freeu(z(2, 4, 4, 12), z(2, 4, 4, 16), 1.2, 0.9)
    with pytest.raises(ValueError):
        K.freeu(z(2, 4, 4, 16), z(2, 4, 5, 16), 1.2, 0.9)
    with pytest.raises(ValueError):
        K.freeu(z(2, 4, 4, 32)[..., :16], z(2, 4, 4, 16), 1.2, 0.9)
    with pytest.raises(TypeError):
        K.freeu(z(2, 4, 4, 16).float(), z(2, 4, 4, 16), 1.2, 0.9)


@pytest.mark.parametrize("n,hh,ww,c1,c2,b", [(32, 8, 8, 1280, 1280, 1.2), (8, 16, 16, 1280, 640, 1.4), (3, 9, 7, 24, 72, 0.7)])
def test_kernel_precise_pair(dev, n, hh, ww, c1, c2, b):
    """a hidden tensor of the precise residual stream (hi + lo) is scaled as the pair's value and comes back as a pair -- checked at
    the precision the stream's other producers are held to (tests/test_precise_stream_gpu.py PAIR_TOL); the copied channels keep both
    halves bit for bit; the skip result does not depend on the low half being there"""
    K = pkg().kernels
    g = torch.Generator().manual_seed(n + hh + c1)
    hid32 = torch.randn(n, hh, ww, c1, generator=g)
    skip = torch.randn(n, hh, ww, c2, generator=g).half()
    hd, val64 = pair(hid32, dev)
    lo_in = K.lo_of(hd).clone()
    sd = skip.to(dev)
    ho, so = K.freeu(hd, sd, b, 0.2)
    torch.cuda.synchronize()
    ref_h, _ = tokens_reference(val64, skip, b, 0.2)
    half = c1 // 2
    lo = K.lo_of(ho)
    assert lo is not None and lo.data_ptr() != K.lo_of(hd).data_ptr(), "a low half in means a fresh low half out"
    scaled = ho[..., :half].contiguous()
    scaled._i2v_lo = lo[..., :half].contiguous()
    rel = check_pair(scaled, ref_h[..., :half].contiguous(), f"freeu precise pair {n}x{hh}x{ww}x{c1}")
    print(f"freeu precise pair {n}x{hh}x{ww}x{c1}: |hi + lo - ref| / max|ref| = {rel:.3e} (bound {PAIR_TOL:.1e})")
    assert torch.equal(ho[..., half:], hd[..., half:]) and torch.equal(lo[..., half:], lo_in[..., half:])
    assert torch.equal(K.lo_of(hd), lo_in), "the input's low half must not be modified"
    plain = hd.clone()                                     # (no low half attached)
    ho0, so0 = K.freeu(plain, sd, b, 0.2)
    assert K.lo_of(ho0) is None and torch.equal(so0, so)


# ---------------------------------------------------------------------------------------------------------- the UNet forward
@pytest.fixture(scope="module")
def small(dev):
    ou = oracle_small_unet()
    return ou, hip_unet_from_oracle(ou, dev)


def _forward_inputs(hh, ww, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    if cfg:                                                 # pipe:672-673: the same latents twice at one timestep, two prompts
        lat = h16(torch.randn(1, 4, 4, hh, ww, generator=g))
        sample, t = torch.cat([lat, lat]), torch.tensor([481, 481])
    else:
        sample, t = h16(torch.randn(2, 4, 4, hh, ww, generator=g)), torch.tensor([10, 500])
    return sample, t, h16(torch.randn(2, 7, 64, generator=g))


def _hip_forward(hu, dev, sample, t, ctx, cfg):
    kw = dict(cross_attention_kwargs={"cfg_shared_prefix": True}) if cfg else {}
    with torch.no_grad():
        return hu(sample.to(dev), t.to(dev), True, ctx.to(dev), **kw).sample


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("hh,ww", [(32, 32), (36, 28)])
def test_small_unet_forward_with_freeu(dev, small, hh, ww, cfg):
    """FreeU on (the paper's SD-1.5 values) against the oracle with the literal FFT form hooked into its up blocks, at the gate of
    the forward without FreeU (REL_TOL_UNET of max|ref|, tests/test_modules_gpu.py::test_small_unet_forward*).  36 x 28 takes the
    `forward_upsample_size` route (planes of 5 x 4 and 9 x 7).  In the same run FreeU off against the plain oracle: FreeU may not
    cost more than 1.5 x that error (both as fractions of their own max|ref|, the unit of the gate), and it must change the output by
    more than ten times the gate."""
    ou, hu = small
    sample, t, ctx = _forward_inputs(hh, ww, cfg, seed=hh * 31 + ww + int(cfg))
    with torch.no_grad():
        ref_off = ou(sample, t, True, ctx).sample
        hooks = hook_oracle_unet(ou, **SD15_FREEU)
        try:
            ref_on = ou(sample, t, True, ctx).sample
        finally:
            for hk in hooks:
                hk.remove()
    got_off = _hip_forward(hu, dev, sample, t, ctx, cfg)
    hu.enable_freeu(**SD15_FREEU)
    try:
        got_on = _hip_forward(hu, dev, sample, t, ctx, cfg)
    finally:
        hu.disable_freeu()
    name = f"small UNet {hh} x {ww} cfg={cfg}"
    e_off, s_off = compare(got_off, ref_off, rel=REL_TOL_UNET, name=name + ", FreeU off")
    err_on = (got_on.float().cpu() - ref_on).abs().max().item()
    s_on = ref_on.abs().max().item()
    diff = (got_on - got_off).abs().max().item()
    print(f"{name}: FreeU off err {e_off:.3e} (max|ref| {s_off:.3e}, rel {e_off / s_off:.3e}); FreeU on err {err_on:.3e} "
          f"(max|ref| {s_on:.3e}, rel {err_on / s_on:.3e}); max|y_freeu - y_plain| {diff:.3e}; gate {REL_TOL_UNET * s_on:.3e}")
    compare(got_on, ref_on, rel=REL_TOL_UNET, name=name + ", FreeU on")
    assert err_on / s_on <= 1.5 * e_off / s_off, f"{name}: FreeU on {err_on / s_on:.3e} of max|ref| vs off {e_off / s_off:.3e}"
    assert diff > 10 * REL_TOL_UNET * s_on, f"{name}: FreeU changed the output by {diff:.3e} only"
    assert (ref_on - ref_off).abs().max().item() > 10 * REL_TOL_UNET * s_on


def test_disable_restores_the_plain_forward_bit_for_bit(dev, small):
    _, hu = small
    sample, t, ctx = _forward_inputs(16, 16, False, seed=3)
    base = _hip_forward(hu, dev, sample, t, ctx, False)
    hu.enable_freeu(**SD15_FREEU)
    try:
        on = _hip_forward(hu, dev, sample, t, ctx, False)
        hu.enable_freeu(s1=0.9, s2=0.2, b1=0.0, b2=1.4)             # a zero among the four: off, as in the reference
        zeroed = _hip_forward(hu, dev, sample, t, ctx, False)
    finally:
        hu.disable_freeu()
    off = _hip_forward(hu, dev, sample, t, ctx, False)
    fresh = hip_unet_from_oracle(small[0], dev)                      # a model that never enabled it
    never = _hip_forward(fresh, dev, sample, t, ctx, False)
    assert torch.equal(off, base) and torch.equal(never, base) and torch.equal(zeroed, base)
    assert not torch.equal(on, base)


def test_small_unet_forward_with_freeu_precise_stream(dev, small):
    """the precise residual stream with FreeU: the mid block's hi + lo pair goes through the kernel, the forward stays inside the
    gate and is not farther from the oracle than the default stream is"""
    from i2v_adapter_unofficial_amd import blocks
    ou, hu = small
    sample, t, ctx = _forward_inputs(32, 32, False, seed=17)
    with torch.no_grad():
        hooks = hook_oracle_unet(ou, **SD15_FREEU)
        try:
            ref = ou(sample, t, True, ctx).sample
        finally:
            for hk in hooks:
                hk.remove()
    entry = blocks.set_precise_stream(False)
    hu.enable_freeu(**SD15_FREEU)
    try:
        base = _hip_forward(hu, dev, sample, t, ctx, False)
        blocks.set_precise_stream(True)
        got = _hip_forward(hu, dev, sample, t, ctx, False)
    finally:
        hu.disable_freeu()
        blocks.set_precise_stream(entry)
    e1, scale = compare(got, ref, rel=REL_TOL_UNET, name="small UNet + FreeU, precise stream")
    e0, _ = compare(base, ref, rel=REL_TOL_UNET, name="small UNet + FreeU, default stream")
    rms = lambda y: (y.float().cpu() - ref).pow(2).mean().sqrt().item()
    print(f"small UNet + FreeU vs oracle: default max {e0:.3e} rms {rms(base):.3e}; precise max {e1:.3e} rms {rms(got):.3e}")
    assert rms(got) < rms(base)


# ---------------------------------------------------------------------------------------------------------- the pipeline
def _problem(seed=31):
    g = torch.Generator().manual_seed(seed)
    return h16(torch.randn(1, 7, 64, generator=g)), h16(torch.randn(1, 7, 64, generator=g)), torch.randn(1, 4, 16, 16, generator=g)


def _gens():
    return dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _scheduler(kind):
    return pkg().DPMSolverMultistepScheduler() if kind == "dpmsolver++" else pkg().DDIMScheduler()


@pytest.mark.parametrize("kind", ["ddim", "dpmsolver++"])
def test_pipeline_routes_and_graph_key(dev, small, kind):
    """graph == eager (callback) bit for bit with FreeU on; enabling FreeU after a captured run of the same shape re-captures (the
    result changes and equals a fresh pipeline's); changing the scales and disabling re-capture too"""
    _, hu = small
    pe, ne, cond = _problem(seed=7)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=4, num_inference_steps=8,
              guidance_scale=7.5, frame_similarity_sample_ratio=0.9)
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=_scheduler(kind))
    try:
        plain = pipe(**kw, **_gens()).frames
        assert len(pipe._graph_cache) == 1
        pipe.enable_freeu(**SD15_FREEU)
        graph = pipe(**kw, **_gens()).frames
        assert len(pipe._graph_cache) == 1 and not torch.equal(graph, plain), "a stale graph was replayed"
        assert (graph - plain).abs().max().item() > 1e-2 and torch.equal(graph[:, 0], plain[:, 0])
        seen = []
        eager = pipe(**kw, callback=lambda i, t, lat: seen.append(i), **_gens()).frames
        assert seen == list(range(7)) and torch.equal(graph, eager)
        again = pipe(**kw, **_gens()).frames                              # a graph-cache hit
        assert torch.equal(again, graph)
        pipe.enable_freeu(0.8, 0.3, 1.1, 1.3)
        other = pipe(**kw, **_gens()).frames
        assert not torch.equal(other, graph) and not torch.equal(other, plain)
        fresh = pkg().I2VAdapterPipeline(unet=hu, scheduler=_scheduler(kind))(**kw, **_gens()).frames
        assert torch.equal(fresh, other)
        pipe.disable_freeu()
        back = pipe(**kw, **_gens()).frames
        assert torch.equal(back, plain)
    finally:
        hu.disable_freeu()


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("kind", ["ddim", "dpmsolver++"])
def test_pipeline_trajectory_against_the_hooked_oracle(dev, small, kind, use_graph):
    from oracle.pipeline_i2v_adapter import I2VAdapterPipeline as OP
    ou, hu = small
    pe, ne, cond = _problem()
    kw = dict(num_frames=4, num_inference_steps=10, guidance_scale=7.5, frame_similarity_sample_ratio=0.9)
    hooks = hook_oracle_unet(ou, **SD15_FREEU)
    try:
        op = OP(ou, scheduler=ReferenceDPMSolver()) if kind == "dpmsolver++" else OP(ou)
        ref = op(pe, ne, cond, **kw, **_gens()).frames
    finally:
        for hk in hooks:
            hk.remove()
    ref_plain = (OP(ou, scheduler=ReferenceDPMSolver()) if kind == "dpmsolver++" else OP(ou))(pe, ne, cond, **kw, **_gens()).frames
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=_scheduler(kind))
    pipe.enable_freeu(**SD15_FREEU)
    try:
        got = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, use_graph=use_graph, **kw, **_gens()).frames
    finally:
        pipe.disable_freeu()
    assert got.shape == (1, 4, 4, 16, 16) and torch.equal(got[:, 0].cpu(), cond)
    err, scale = compare(got, ref, rel=REL_TOL_TRAJECTORY, name=f"{kind} trajectory with FreeU (9 steps)")
    moved = (ref - ref_plain).abs().max().item()
    print(f"{kind} + FreeU use_graph={use_graph}: max abs latent err {err:.3e} (max|ref| {scale:.3e}); FreeU moves the oracle by {moved:.3e}")
    assert moved > 10 * REL_TOL_TRAJECTORY * scale


# ---------------------------------------------------------------------------------------------------------- the model handle
def _plan_entries(blob):
    hdr = struct.unpack_from("<6I6iQ2I6Q", blob, 0)
    n_ops, ops_off = hdr[3], hdr[16]
    return [struct.unpack_from("<I", blob, ops_off + 24 * i)[0] for i in range(n_ops)]


def test_forward_plan_with_freeu_through_the_c_abi(dev, monkeypatch, small):
    """a plan recorded with FreeU enabled carries six i2v_freeu_f16 launches and replays them through i2v_unet_forward with no
    kernels.py wrapper running; it equals the module API bit for bit, also on other inputs, and differs from the plan without"""
    p = pkg()
    H, K = p.handle, p.kernels
    _, hu = small
    g = torch.Generator().manual_seed(5)

    def inputs(seed):
        g.manual_seed(seed)
        return dict(sample=torch.randn(2, 4, 4, 16, 16, generator=g).half().to(dev), t=torch.tensor([481.0, 37.0], device=dev),
                    ctx=torch.randn(2, 7, 64, generator=g).half().to(dev))

    def module(inp):
        with torch.no_grad():
            return hu(inp["sample"], inp["t"], True, inp["ctx"]).sample
    inp, inp2 = inputs(5), inputs(6)
    plain = module(inp)
    hu.enable_freeu(**SD15_FREEU)
    try:
        ref, ref2 = module(inp), module(inp2)
        blob, weights = H.record_forward_plan(hu, inp["sample"], inp["t"], inp["ctx"])
    finally:
        hu.disable_freeu()
    entries = _plan_entries(blob)
    assert entries.count(H.entry_id("i2v_freeu_f16")) == 6
    blob_off, _ = H.record_forward_plan(hu, inp["sample"], inp["t"], inp["ctx"])
    assert _plan_entries(blob_off).count(H.entry_id("i2v_freeu_f16")) == 0 and len(_plan_entries(blob_off)) == len(entries) - 6
    hd = p.UNetHandle(hu)
    hd.plan(2, 4, 16, 16, ctx_len=7, has_ip=False)
    hd.set_plan(blob)
    hd.set_weights(weights)
    arena = torch.empty(hd.activation_bytes, dtype=torch.uint8, device=dev)
    hd.set_workspace(arena)
    out, out2 = torch.full_like(ref, float("nan")), torch.full_like(ref, float("nan"))

    def boom(*a, **k):
        raise AssertionError("a kernels.py wrapper ran during i2v_unet_forward")
    with monkeypatch.context() as m:
        for name in ("freeu", "gemm", "conv3x3", "attention", "groupnorm", "layernorm", "ff_fused", "motion_attn", "cross_attn_fused",
                     "ln_qkv", "temporal_attention", "nchw_to_tokens", "tokens_to_nchw", "timestep_embedding", "silu", "copy3d"):
            m.setattr(K, name, boom)
        hd.forward(inp["sample"], inp["t"], inp["ctx"], None, out)
        hd.forward(inp2["sample"], inp2["t"], inp2["ctx"], None, out2)
        torch.cuda.synchronize()
    assert torch.equal(out, ref), f"C-ABI forward differs from the module API: max |d| {(out.float() - ref.float()).abs().max().item():.3e}"
    assert torch.equal(out2, ref2) and not torch.equal(out, plain)
    hd.close()
