"""T2I-Adapter on the GPU: the four kernels of csrc/t2i_adapter.hip, `T2IAdapter.forward` against the fp32 restatement
(tests/t2i_adapter_reference.py), the UNet with `down_intrablock_additional_residuals` against the oracle, and the pipeline (scale 0 is
the pipeline without an adapter, the factor's step window, graph == eager under the three schedulers, graph-cache replay with other
frames, FreeInit, adapter + ControlNet, an odd latent size) and the driver.

Yardsticks.  The unshuffle moves values (bit equality with torch).  The pool is an fp32 sum of at most four fp16 values times an exact
factor and ONE rounding: whatever the order of the sum, the fp32 value is within a few 2^-24 relative of the exact mean, so the fp16
result is torch's or its neighbour -- at most 1 ulp, and exact where a window holds one tap.  The per-step add is held to the existing
kernel: bit equality with `kernels.add_residuals` on the repeated feature, no tolerance.  The model and the UNet use the gate the
ControlNet's residuals have, tests/parity.compare with REL_TOL_UNET (3e-3 of max|ref|).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import controlnet_reference as CR
from tests import t2i_adapter_reference as R
from tests.parity import REL_TOL_UNET, compare, hip_unet_from_oracle, oracle_small_unet, small_unet_inputs

pytestmark = pytest.mark.gpu

f16 = torch.float16


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h16(t):
    return t.half().float()


def bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------- the movers
@pytest.mark.parametrize("dtype", [torch.float32, f16])
@pytest.mark.parametrize("c", [1, 3])
def test_pixel_unshuffle8_is_torchs(dev, c, dtype):
    K = pkg().kernels
    g = torch.Generator().manual_seed(c)
    x = torch.rand(2, c, 16, 24, generator=g).to(dtype)
    want = F.pixel_unshuffle(x.float(), 8).half().permute(0, 2, 3, 1).contiguous()            # [N, H / 8, W / 8, 64 C]: token order
    got = K.pixel_unshuffle8(x.to(dev))
    assert got.shape == (2, 2, 3, 64 * c) and got.dtype == f16
    assert torch.equal(bits(got.cpu()), bits(want))


def _ulps(a, b):
    """distance in fp16 units in the last place between two fp16 tensors (finite values)"""
    def ordered(t):
        i = bits(t).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (ordered(a) - ordered(b)).abs()


@pytest.mark.parametrize("shape", [(2, 5, 7, 32), (2, 4, 6, 64)])
def test_avgpool2x_against_torch(dev, shape):
    K = pkg().kernels
    g = torch.Generator().manual_seed(shape[1])
    x = (torch.rand(shape, generator=g) * 8 - 4).half()
    want = F.avg_pool2d(x.float().permute(0, 3, 1, 2), 2, stride=2, ceil_mode=True).permute(0, 2, 3, 1).contiguous().half()
    got = K.avgpool2x(x.to(dev)).cpu()
    n, h, w, c = shape
    assert got.shape == want.shape == (n, (h + 1) // 2, (w + 1) // 2, c)
    worst = int(_ulps(got, want).max())
    print(f"i2v_avgpool2x_f16 {shape}: worst distance from torch {worst} ulp")
    assert worst <= 1
    if h % 2 and w % 2:                         # the corner window holds one tap, the last row / column two: no sum, no rounding
        assert torch.equal(bits(got[:, -1, -1]), bits(x[:, -1, -1]))
        pair = (x[:, -1, 0::2][:, :-1].float() + x[:, -1, 1::2].float()) * 0.5
        assert torch.equal(got[:, -1, :-1], pair.half())


def test_relu_is_torchs_in_and_out_of_place(dev):
    K = pkg().kernels
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(3, 5, 7, 8, generator=g) * 3).half()
    x[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 65504.0, -65504.0], dtype=f16)
    want = torch.relu(x.float()).half()
    d = x.to(dev)
    out = K.relu(d)
    assert out.data_ptr() != d.data_ptr() and torch.equal(out.cpu(), want) and torch.equal(d.cpu(), x)
    same = K.relu(d, out=d)
    assert same is d and torch.equal(d.cpu(), want)
    with pytest.raises(ValueError):
        K.relu(torch.zeros(12, dtype=f16, device=dev))


# ---------------------------------------------------------------------------------------------------------- the per-step add
TABLE = (0.5, -0.75, 1.25)


def _add_case(copies, feat_numel, seed=5):
    """x [copies, feat_numel] as a proper (hi, lo) pair, feat [1, feat_numel]"""
    g = torch.Generator().manual_seed(seed + feat_numel + copies)
    x = torch.randn(copies, feat_numel, generator=g) * 2.0
    hi = x.half()
    return hi, (x - hi.float()).half(), (torch.randn(1, feat_numel, generator=g) * 0.7).half()


@pytest.mark.parametrize("feat_numel", [8, 4200, 8200])         # one chunk; under one 1024-chunk tile; over one tile, the wrap unaligned to it
@pytest.mark.parametrize("copies", [1, 2, 3])
def test_add_broadcast_residual_equals_add_residuals_bit_for_bit(dev, copies, feat_numel):
    """the same bits as the existing kernel on the feature repeated `copies` times: no table, and a table at step 0, the last step and
    past the end (clamped); out of place and in place; default stream and precise pair (the low halves compared too)"""
    K = pkg().kernels
    hi, lo, feat = _add_case(copies, feat_numel)
    table = torch.tensor(TABLE, device=dev)
    scales = [None, (table, None)] + [(table, torch.tensor([i], dtype=torch.int32, device=dev)) for i in (0, len(TABLE) - 1, 7)]
    d_feat = feat.to(dev)
    rep = d_feat.repeat(copies, 1).contiguous()
    for precise in (False, True):
        def operand():
            t = hi.to(dev)
            if precise:
                t._i2v_lo = lo.to(dev)
            return t
        seen = set()
        for scale in scales:
            want, = K.add_residuals([operand()], [rep], scale=scale)
            x = operand()
            got = K.add_broadcast_residual(x, d_feat, scale=scale)
            assert got.data_ptr() != x.data_ptr() and torch.equal(x.cpu(), hi), "out of place changed x"
            assert torch.equal(bits(got), bits(want)), (precise, scale)
            assert (K.lo_of(got) is not None) == precise
            if precise:
                assert torch.equal(bits(K.lo_of(got)), bits(K.lo_of(want))) and torch.equal(K.lo_of(x).cpu(), lo)
            x = operand()
            own_lo = K.lo_of(x)
            same = K.add_broadcast_residual(x, d_feat, scale=scale, out=x)
            assert same is x and torch.equal(bits(x), bits(want))
            if precise:
                assert K.lo_of(x) is own_lo and torch.equal(bits(own_lo), bits(K.lo_of(want)))
            seen.add(bits(got).cpu().numpy().tobytes())
        # s = 1 (no table), 0.5 (row 0: no counter, step 0) and 1.25 (the last step, and past the end): the table and the counter are read
        assert len(seen) == 3, len(seen)


GUARD = 64          # fp16 values of poison on either side of every destination


def _guarded(n, dev, poison):
    buf = torch.full((n + 2 * GUARD,), poison, dtype=f16, device=dev)
    return buf, buf[GUARD: GUARD + n]


def _guards_intact(buf, n, poison):
    b = buf.cpu()
    return bool((b[:GUARD] == poison).all()) and bool((b[GUARD + n:] == poison).all())


@pytest.mark.parametrize("precise", [False, True])
def test_add_broadcast_residual_zero_scale_and_guard_bands(dev, precise):
    """s = 0 (a table row) leaves x's bits, -0 and the low half included; the launch writes nothing outside dst / dst_lo (poisoned
    guard bands on either side, through the ABI with the test's own buffers), and nothing into dst_lo without a low half"""
    K, L = pkg().kernels, pkg()._lib
    copies, feat_numel = 3, 8200
    hi, lo, feat = _add_case(copies, feat_numel)
    hi[0, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 6e-8, -6e-8, 65504.0, -65504.0], dtype=f16)
    n = hi.numel()
    x, x_lo, d_feat = hi.to(dev), lo.to(dev), feat.to(dev)
    table, idx = torch.tensor([1.0, 0.0, -0.75], device=dev), torch.tensor([1], dtype=torch.int32, device=dev)
    for row in (1, 2):
        idx.fill_(row)
        buf, out = _guarded(n, dev, 777.0)
        lbuf, out_lo = _guarded(n, dev, -555.0)
        rc = L.load().i2v_add_broadcast_residual_f16(x.data_ptr(), x_lo.data_ptr() if precise else None, d_feat.data_ptr(), out.data_ptr(),
                                                     out_lo.data_ptr() if precise else None, n, feat_numel, table.data_ptr(), 3,
                                                     idx.data_ptr(), K._stream())
        L.check(rc, "i2v_add_broadcast_residual_f16")
        torch.cuda.synchronize()
        assert _guards_intact(buf, n, 777.0), "dst written outside the tensor"
        assert _guards_intact(lbuf, n, -555.0) and (precise or bool((lbuf == -555.0).all())), "dst_lo written outside / without a low half"
        if row == 1:
            assert torch.equal(bits(out.cpu()), bits(hi.reshape(-1))), "s = 0: not x bit for bit"
            if precise:
                assert torch.equal(bits(out_lo.cpu()), bits(lo.reshape(-1))), "s = 0: the low half changed"
        else:
            t = x.clone()
            if precise:
                t._i2v_lo = x_lo.clone()
            want = K.add_broadcast_residual(t, d_feat, scale=(table, idx))
            assert torch.equal(bits(out), bits(want.reshape(-1))) and not torch.equal(out.cpu(), hi.reshape(-1))
            if precise:
                assert torch.equal(bits(out_lo), bits(K.lo_of(want).reshape(-1)))


def test_add_broadcast_residual_wrapper_refusals(dev):
    K = pkg().kernels
    x, feat = torch.zeros(4, 3, 5, 8, dtype=f16, device=dev), torch.zeros(2, 3, 5, 8, dtype=f16, device=dev)
    assert K.add_broadcast_residual(x, feat).shape == x.shape
    with pytest.raises(ValueError, match="divides"):
        K.add_broadcast_residual(x, torch.zeros(3, 3, 5, 8, dtype=f16, device=dev))
    with pytest.raises(ValueError, match="behind the batch"):
        K.add_broadcast_residual(x, torch.zeros(2, 5, 3, 8, dtype=f16, device=dev))
    with pytest.raises(ValueError, match="contiguous"):
        K.add_broadcast_residual(x, feat, out=torch.zeros(4, 3, 5, 16, dtype=f16, device=dev)[..., :8])
    with pytest.raises(ValueError, match="scale table"):
        K.add_broadcast_residual(x, feat, scale=(torch.zeros(2, 2, device=dev), None))


# ---------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module", params=[(3, 72, 104), (1, 64, 64)], ids=["rgb-72x104", "grey-64x64"])
def small_adapter(request, dev):
    """(HIP model with the reference's weights, frames, the reference's four feature maps): 72 x 104 gives the odd levels 9 x 13,
    5 x 7, 3 x 4, 2 x 2 (every edge form of the pool); the 1-channel model is the canny / sketch layout"""
    c, h, w = request.param
    ref = R.small_reference(c)
    m = pkg().T2IAdapter(**R.small_config(c))
    m.load_state_dict(ref.state_dict())
    m = m.to(dev, f16).eval()
    frames = R.small_frames(c, h, w)
    with torch.no_grad():
        want = ref(frames)
    return m, frames, want


def test_adapter_forward_against_the_reference(dev, small_adapter):
    m, frames, want = small_adapter
    with torch.no_grad():
        got = m(frames.to(dev))
    assert isinstance(got, list) and len(got) == 4
    sizes = R.feature_sizes(*frames.shape[-2:])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.float32 and tuple(g.shape) == (2, R.SMALL_CHANNELS[i]) + sizes[i] and w.abs().max().item() > 1e-2
        compare(g, w, rel=REL_TOL_UNET, name=f"T2IAdapter small, {tuple(frames.shape)}, feature {i}")


def test_adapter_embed_is_forward_in_token_form(dev, small_adapter):
    K = pkg().kernels
    m, frames, _ = small_adapter
    with torch.no_grad():
        nchw = m(frames.to(dev).half())
        tokens = m.embed(frames.to(dev))
    for a, t in zip(nchw, tokens):
        assert a.dtype == f16 and t.dtype == f16 and t.is_contiguous() and t.shape == (a.shape[0], a.shape[2], a.shape[3], a.shape[1])
        assert torch.equal(a, K.tokens_to_nchw(t))


# ---------------------------------------------------------------------------------------------------------- the UNet
def _oracle_with_intrablock(ou, inp, enable, feats):
    """the oracle UNet with diffusers' down_intrablock_additional_residuals: a block with cross-attention gets its tensor as
    `additional_residuals` (unet:329-330); for the block without, the tensor is added by hand to the hidden state it returns, which is
    also its last output state (UNet2DConditionModel's in-place `sample += ...`).  oracle/ is not edited: the blocks' forwards are
    wrapped for the call and restored."""
    wrapped = []
    try:
        for blk, feat in zip(ou.down_blocks, feats):
            orig = blk.forward
            if getattr(blk, "has_cross_attention", False):
                blk.forward = lambda *a, _f=feat, _o=orig, **k: _o(*a, additional_residuals=_f, **k)
            else:
                def fwd(*a, _f=feat, _o=orig, **k):
                    x, states = _o(*a, **k)
                    assert states[-1] is x or torch.equal(states[-1], x)
                    x = x + _f
                    return x, states[:-1] + (x,)
                blk.forward = fwd
            wrapped.append(blk)
        with torch.no_grad():
            return ou(inp["sample"], inp["timestep"], enable, inp["ctx"]).sample
    finally:
        for blk in wrapped:
            del blk.forward


@pytest.fixture(scope="module")
def small_unet(dev):
    """(oracle, HIP UNet, inputs, adapter-shaped features for B * F = 2 images, the oracle's outputs with them on the batch of 4)"""
    ou = oracle_small_unet()
    hu = hip_unet_from_oracle(ou, dev)
    inp = small_unet_inputs(b=2, f=2)
    same = inp["sample"][:1]
    inp["sample"], inp["timestep"] = torch.cat([same, same]), torch.tensor([481, 481])     # a CFG-shaped batch: cfg_shared_prefix applies
    g = torch.Generator().manual_seed(29)
    feats = [h16(torch.randn(2, c, 16 >> i, 16 >> i, generator=g) * 0.5) for i, c in enumerate(R.SMALL_CHANNELS)]
    full = [torch.cat([t, t]) for t in feats]                                               # what the modulo stands for
    want = {e: _oracle_with_intrablock(ou, inp, e, full) for e in (True, False)}
    with torch.no_grad():
        plain = ou(inp["sample"], inp["timestep"], True, inp["ctx"]).sample
    return ou, hu, inp, feats, full, want, plain


def _hip_unet(hu, dev, inp, enable, feats=None, **kw):
    with torch.no_grad():
        return hu(inp["sample"].to(dev), inp["timestep"].to(dev), enable, inp["ctx"].to(dev),
                  down_intrablock_additional_residuals=None if feats is None else [t.to(dev) for t in feats], **kw).sample


def test_unet_with_adapter_features_against_the_oracle(dev, small_unet):
    ou, hu, inp, feats, full, want, plain = small_unet
    moved = (plain - want[True]).abs().max().item()
    assert moved > 10 * REL_TOL_UNET * want[True].abs().max().item(), "the features move the output by less than 10 x the tolerance"
    # one copy of B * F features under the shared CFG prefix: the first block's add sees the full batch and wraps around
    got = _hip_unet(hu, dev, inp, True, feats, cross_attention_kwargs={"cfg_shared_prefix": True})
    compare(got, want[True], rel=REL_TOL_UNET, name="small UNet + adapter features, cross-frame, cfg_shared, B * F features")
    got = _hip_unet(hu, dev, inp, True, full)
    compare(got, want[True], rel=REL_TOL_UNET, name="small UNet + adapter features, cross-frame, full-batch features")
    got = _hip_unet(hu, dev, inp, False, feats)
    compare(got, want[False], rel=REL_TOL_UNET, name="small UNet + adapter features, no cross-frame")
    assert torch.equal(_hip_unet(hu, dev, inp, True, feats), _hip_unet(hu, dev, inp, True, full)), "the modulo is not the repeated feature"


def test_unet_with_adapter_features_precise_stream(dev, small_unet):
    from i2v_adapter_unofficial_amd import blocks
    _, hu, inp, feats, _, want, _ = small_unet
    prev = blocks.set_precise_stream(True)
    try:
        got = _hip_unet(hu, dev, inp, True, feats)
    finally:
        blocks.set_precise_stream(prev)
    compare(got, want[True], rel=REL_TOL_UNET, name="small UNet + adapter features, precise stream")


def test_unet_with_adapter_features_and_controlnet_residuals(dev, small_unet):
    """both kinds of residual in one forward: the adapter's inside the blocks, the ControlNet's on the skip tensors and the mid block"""
    ou, hu, inp, feats, full, _, _ = small_unet
    g = torch.Generator().manual_seed(23)
    shapes = [(4, 32, 16, 16)]
    for i, c in enumerate(R.SMALL_CHANNELS):
        shapes += [(4, c, 16 >> i, 16 >> i)] * 2 + ([(4, c, 8 >> i, 8 >> i)] if i < 3 else [])
    down = [h16(torch.randn(s, generator=g) * 0.5) for s in shapes]
    mid = h16(torch.randn((4, 128, 2, 2), generator=g) * 0.5)
    orig = ou.forward
    ou.forward = lambda *a, **k: orig(*a, down_block_additional_residuals=down, mid_block_additional_residual=mid, **k)
    try:
        want = _oracle_with_intrablock(ou, inp, True, full)
    finally:
        del ou.forward
    with torch.no_grad():
        got = hu(inp["sample"].to(dev), inp["timestep"].to(dev), True, inp["ctx"].to(dev), down_intrablock_additional_residuals=[t.to(dev) for t in feats],
                 down_block_additional_residuals=[d.to(dev) for d in down], mid_block_additional_residual=mid.to(dev)).sample
    compare(got, want, rel=REL_TOL_UNET, name="small UNet + adapter features + ControlNet residuals")


@pytest.mark.parametrize("precise", [False, True])
def test_unet_zero_features_are_bit_equal_to_none(dev, small_unet, precise):
    from i2v_adapter_unofficial_amd import blocks
    _, hu, inp, feats, _, _, _ = small_unet
    prev = blocks.set_precise_stream(precise)
    try:
        base = _hip_unet(hu, dev, inp, True)
        zero = _hip_unet(hu, dev, inp, True, [torch.zeros_like(t) for t in feats])
    finally:
        blocks.set_precise_stream(prev)
    assert torch.equal(base, zero)


# ---------------------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def pipe_parts(dev, small_unet):
    ref = R.small_reference(3)
    ad = pkg().T2IAdapter(**R.small_config(3))
    ad.load_state_dict(ref.state_dict())
    return small_unet[1], ad.to(dev, f16).eval()


def _problem(seed=31, frames=2, hw=(16, 16)):
    g = torch.Generator().manual_seed(seed)
    return dict(prompt_embeds=h16(torch.randn(1, 7, 64, generator=g)), negative_prompt_embeds=h16(torch.randn(1, 7, 64, generator=g)),
                condition_image_latents=torch.randn(1, 4, *hw, generator=g), num_frames=frames, guidance_scale=7.5,
                output_type="latent"), torch.rand(frames, 3, 8 * hw[0], 8 * hw[1], generator=g)


def _gens():
    return dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _sched(kind):
    p = pkg()
    return {"ddim": p.DDIMScheduler, "dpmsolver++": p.DPMSolverMultistepScheduler, "lcm": p.LCMScheduler}[kind]()


def test_pipeline_scale_zero_is_the_pipeline_without_an_adapter(dev, pipe_parts):
    hu, ad = pipe_parts
    kw, frames = _problem()
    plain = pkg().I2VAdapterPipeline(unet=hu)(**kw, num_inference_steps=3, **_gens()).frames
    pipe = pkg().I2VAdapterPipeline(unet=hu, t2i_adapter=ad)
    off = pipe(**kw, num_inference_steps=3, adapter_image=frames, adapter_conditioning_scale=0.0, **_gens()).frames
    assert torch.equal(off, plain)
    on = pipe(**kw, num_inference_steps=3, adapter_image=frames, **_gens()).frames          # scale 1: another table, the same graph
    assert len(pipe._graph_cache) == 1 and not torch.equal(on, plain) and torch.equal(on[:, 0], plain[:, 0])
    # a factor with int(n * f) == 0 switches every step off: the pipeline without an adapter again
    none = pipe(**kw, num_inference_steps=3, adapter_image=frames, adapter_conditioning_factor=0.3, **_gens()).frames
    assert torch.equal(none, plain) and len(pipe._graph_cache) == 1


def test_pipeline_factor_is_a_step_window(dev, pipe_parts):
    """factor 0.5 over 4 steps: the table is [1, 1, 0, 0] -- the latents after step 2 are the full-adapter run's, the result differs
    from both factor 0 and factor 1; graph == eager"""
    hu, ad = pipe_parts
    kw, frames = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=hu, t2i_adapter=ad)

    def run(factor):
        seen = {}
        out = pipe(**kw, num_inference_steps=4, adapter_image=frames, adapter_conditioning_factor=factor,
                   callback=lambda i, t, lat: seen.__setitem__(i, lat.clone()), **_gens()).frames
        return seen, out
    s0, o0 = run(0.0)
    sh, oh = run(0.5)
    s1, o1 = run(1.0)
    assert sorted(sh) == [0, 1, 2, 3]
    assert torch.equal(sh[0], s1[0]) and torch.equal(sh[1], s1[1]) and not torch.equal(sh[1], s0[1])
    assert not torch.equal(oh, o0) and not torch.equal(oh, o1)
    graph = pipe(**kw, num_inference_steps=4, adapter_image=frames, adapter_conditioning_factor=0.5, **_gens()).frames
    assert torch.equal(graph, oh)


@pytest.mark.parametrize("kind", ["ddim", "dpmsolver++", "lcm"])
def test_pipeline_graph_equals_eager(dev, pipe_parts, kind):
    hu, ad = pipe_parts
    kw, frames = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=hu, t2i_adapter=ad, scheduler=_sched(kind))
    graph = pipe(**kw, num_inference_steps=3, adapter_image=frames, **_gens()).frames
    eager = pipe(**kw, num_inference_steps=3, adapter_image=frames, use_graph=False, **_gens()).frames
    plain = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched(kind))(**kw, num_inference_steps=3, **_gens()).frames
    assert torch.equal(graph, eager) and not torch.equal(graph, plain)
    assert len(pipe._graph_cache) == 1, "the adapter's schedule did not stay one captured graph"


def test_pipeline_graph_cache_replays_for_other_frames(dev, pipe_parts):
    hu, ad = pipe_parts
    kw, frames = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=hu, t2i_adapter=ad)
    first_out = pipe(**kw, num_inference_steps=3, adapter_image=frames, **_gens()).frames
    first = pipe._graph
    kw2, frames2 = _problem(seed=77)
    import PIL.Image
    pil = [PIL.Image.fromarray((f.permute(1, 2, 0).numpy() * 255).astype("uint8")) for f in frames2]
    again = pipe(**kw2, num_inference_steps=3, adapter_image=pil, adapter_conditioning_scale=0.7, **_gens()).frames
    assert pipe._graph is first and len(pipe._graph_cache) == 1, "a second sample of the same shape re-captured the step"
    fresh = pkg().I2VAdapterPipeline(unet=hu, t2i_adapter=ad)(**kw2, num_inference_steps=3, adapter_image=pil, adapter_conditioning_scale=0.7,
                                                              **_gens()).frames
    assert torch.equal(again, fresh) and not torch.equal(again, first_out)
    other = pipe(**kw2, num_inference_steps=3, adapter_image=frames, adapter_conditioning_scale=0.7, **_gens()).frames
    assert not torch.equal(other, again), "the adapter frames do not reach the replayed graph"
    # with CFG off: one copy of the batch
    kw1 = dict(kw, guidance_scale=1.0)
    kw1.pop("negative_prompt_embeds")
    g1 = pipe(**kw1, num_inference_steps=3, adapter_image=frames, **_gens()).frames
    e1 = pipe(**kw1, num_inference_steps=3, adapter_image=frames, use_graph=False, **_gens()).frames
    assert torch.equal(g1, e1)


def test_pipeline_free_init_fast_sampling(dev, pipe_parts):
    hu, ad = pipe_parts
    kw, frames = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=hu, t2i_adapter=ad)
    pipe.enable_free_init(num_iters=2, use_fast_sampling=True)
    graph = pipe(**kw, num_inference_steps=4, adapter_image=frames, adapter_conditioning_factor=0.5, **_gens()).frames
    eager = pipe(**kw, num_inference_steps=4, adapter_image=frames, adapter_conditioning_factor=0.5, use_graph=False, **_gens()).frames
    full = pipe(**kw, num_inference_steps=4, adapter_image=frames, **_gens()).frames
    assert torch.isfinite(graph).all() and torch.equal(graph, eager) and not torch.equal(graph, full)


def test_pipeline_adapter_next_to_a_controlnet(dev, pipe_parts):
    hu, ad = pipe_parts
    ref = CR.small_reference()
    cn = pkg().ControlNetModel(**CR.small_config())
    cn.load_state_dict(ref.state_dict())
    cn = cn.to(dev, f16).eval()
    kw, frames = _problem()
    g = torch.Generator().manual_seed(41)
    control = torch.rand(2, 3, 128, 128, generator=g)
    both = pkg().I2VAdapterPipeline(unet=hu, controlnet=cn, t2i_adapter=ad)
    graph = both(**kw, num_inference_steps=3, adapter_image=frames, control_image=control, **_gens()).frames
    eager = both(**kw, num_inference_steps=3, adapter_image=frames, control_image=control, use_graph=False, **_gens()).frames
    assert torch.equal(graph, eager)
    plain = pkg().I2VAdapterPipeline(unet=hu)(**kw, num_inference_steps=3, **_gens()).frames
    off = both(**kw, num_inference_steps=3, adapter_image=frames, control_image=control, adapter_conditioning_scale=0.0,
               controlnet_conditioning_scale=0.0, **_gens()).frames
    assert torch.equal(off, plain)
    only_cn = pkg().I2VAdapterPipeline(unet=hu, controlnet=cn)(**kw, num_inference_steps=3, control_image=control, **_gens()).frames
    only_ad = pkg().I2VAdapterPipeline(unet=hu, t2i_adapter=ad)(**kw, num_inference_steps=3, adapter_image=frames, **_gens()).frames
    assert not torch.equal(graph, only_cn) and not torch.equal(graph, only_ad)
    cn_off = both(**kw, num_inference_steps=3, adapter_image=frames, control_image=control, controlnet_conditioning_scale=0.0, **_gens()).frames
    assert torch.equal(cn_off, only_ad)


def test_pipeline_odd_latent_size(dev, pipe_parts):
    """9 x 13 latents (72 x 104 pixels): the adapter's levels 9 x 13, 5 x 7, 3 x 4, 2 x 2 are the UNet's"""
    hu, ad = pipe_parts
    kw, frames = _problem(hw=(9, 13))
    pipe = pkg().I2VAdapterPipeline(unet=hu, t2i_adapter=ad)
    graph = pipe(**kw, num_inference_steps=3, adapter_image=frames, **_gens()).frames
    eager = pipe(**kw, num_inference_steps=3, adapter_image=frames, use_graph=False, **_gens()).frames
    plain = pkg().I2VAdapterPipeline(unet=hu)(**kw, num_inference_steps=3, **_gens()).frames
    assert graph.shape == (1, 2, 4, 9, 13) and torch.isfinite(graph).all()
    assert torch.equal(graph, eager) and not torch.equal(graph, plain)


# ---------------------------------------------------------------------------------------------------------- the driver
def test_eval_driver_with_a_t2i_adapter(dev, tmp_path, monkeypatch):
    """`--t2i_adapter PATH --adapter_column COL` on a one-row CSV whose column names a directory of frames"""
    import PIL.Image
    from safetensors.torch import save_file
    import i2v_adapter_unofficial_amd as p
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    from i2v_adapter_unofficial_amd.pipeline_i2v_adapter import I2VAdapterPipeline, main
    root = str(tmp_path)
    ch = (32, 64, 128, 128)
    kw = dict(sample_size=8, block_out_channels=ch, attention_head_dim=4, norm_num_groups=8, cross_attention_dim=64)
    init_random_weights_(p.UNet2DConditionModel(**kw), seed=1).save_pretrained(os.path.join(root, "sd", "unet"))
    init_random_weights_(p.AutoencoderKL(block_out_channels=(32, 64, 64, 64), norm_num_groups=8), seed=2) \
        .save_pretrained(os.path.join(root, "sd", "vae"))
    p.DDIMScheduler().save_pretrained(os.path.join(root, "sd", "scheduler"))
    init_random_weights_(p.MotionAdapter(block_out_channels=ch, motion_num_attention_heads=4, motion_norm_num_groups=8),
                         seed=3).save_pretrained(os.path.join(root, "motion"))
    init_random_weights_(p.I2VAdapterModule(2, ch, 4), seed=4).save_pretrained(
        os.path.join(root, "checkpoint", "demo", "epoch_3", "i2v_adapter"))
    init_random_weights_(p.T2IAdapter(**R.small_config(1)), seed=5).save_pretrained(os.path.join(root, "sketch"))
    rs = np.random.RandomState(0)
    img = lambda h, w: PIL.Image.fromarray((rs.rand(h, w, 3) * 255).astype("uint8"))
    os.makedirs(os.path.join(root, "data", "images"))
    os.makedirs(os.path.join(root, "data", "sketch0"))
    for j in range(5):                                    # more frames than the clip needs: the first four in sorted order
        img(48, 80).save(os.path.join(root, "data", "sketch0", f"{j:03d}.png"))
    name = "a cat on a boat"
    with open(os.path.join(root, "data", "eval.csv"), "w") as f:
        f.write("image_path,name,sketch\n")
        img(70, 90).save(os.path.join(root, "data", "images", "0.png"))
        f.write(f'images/0.png,"{name}",sketch0\n')
    g = torch.Generator().manual_seed(5)
    save_file({"prompt_embeds": torch.randn(1, 7, 64, generator=g), "negative_prompt_embeds": torch.randn(1, 7, 64, generator=g)},
              os.path.join(root, "embeds.safetensors"))
    seen = []
    call = I2VAdapterPipeline.__call__

    def spy(self, *a, **k):
        seen.append((len(k["adapter_image"]), k["adapter_image"][0].size, k["adapter_conditioning_scale"], k["adapter_conditioning_factor"],
                     type(self.t2i_adapter).__name__, self.t2i_adapter.config.in_channels, "control_image" in k))
        return call(self, *a, **k)
    monkeypatch.setattr(I2VAdapterPipeline, "__call__", spy)
    common = ["--task_name", "demo", "--checkpoint_epoch", "3", "--eval_data_path", os.path.join(root, "data", "eval.csv"),
              "--embeds", os.path.join(root, "embeds.safetensors"), "--model_path", os.path.join(root, "sd"),
              "--motion_adapter_path", os.path.join(root, "motion"), "--checkpoint_root", os.path.join(root, "checkpoint"),
              "--samples_root", os.path.join(root, "samples"), "--num_frames", "4", "--num_inference_steps", "4"]
    assert main(common + ["--t2i_adapter", os.path.join(root, "sketch"), "--adapter_column", "sketch", "--adapter_scale", "0.8",
                          "--adapter_factor", "0.5"]) == 0
    assert seen == [(4, (80, 48), 0.8, 0.5, "T2IAdapter", 1, False)]
    out = PIL.Image.open(os.path.join(root, "samples", "demo", "epoch_3", f"{name}.gif"))
    assert out.n_frames == 4 and out.size == (64, 64)
    assert main(common + ["--t2i_adapter", os.path.join(root, "sketch")]) == -1      # the two options come together
