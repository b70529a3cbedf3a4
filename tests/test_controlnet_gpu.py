"""ControlNet on the GPU: `i2v_add_residuals_f16` against fp64, `ControlNetModel.forward` against the fp32 reference
(tests/controlnet_reference.py), the UNet with residuals against the existing oracle, and the pipeline (graph == eager, the control
window over the schedule, graph-cache replay with other control frames, all three schedulers, FreeInit).

The bounds of the kernel test, per element, against the fp64 value `ref` of skip (+ lo) + s * res (derived here as
tests/tattn_bounds.py derives its own; rn32 / rn16 = round to nearest fp32 / fp16, relative error 2^-24 / 2^-11):
  default stream   out = rn16(rn32(skip + rn32(s res))).  The product: 2^-24 |s res|.  The sum: 2^-24 |skip + p| <= 2^-24 (|skip| + |s res|)
      (1 + 2^-24).  Together |e32| <= 2^-24 (|skip| + 2 |s res|) -- never more than the issue's 2^-23 (|skip| + |s res|), so that term is
      taken in the tighter form.  The rounding to fp16: 2^-11 |sum32| for a normal result, at most 2^-25 (half the subnormal spacing)
      below 2^-14, never both:
          |out - ref| <= 2^-11 |ref| + 2^-24 (|skip| + 2 |s res|) + 2^-24
      The last term keeps the issue's 2^-24 although the derivation needs 2^-25: the other 2^-25 pays for the second-order terms
      (2^-11 |e32| + 2^-48 (...) <= 2^-33 (|skip| + |s res|), below 2^-25 for |skip| + |s res| <= 256; the test's values stay below 16).
      Where s res == 0 the kernel returns skip's bits: error 0 (and the s = 0 cases are checked for bit equality instead).
  precise pair   sum32 = rn32(rn32(hi + lo) + rn32(s res)): |e32| <= 2^-24 (|hi| + |lo|) + 2^-24 |s res| + 2^-24 (|hi| + |lo| + |s res|)
      = 2^-23 (|hi| + |lo| + |s res|).  hi' = rn16(sum32); sum32 - hi' is exact in fp32 (at most 13 significant bits at sum32's last
      place); lo' = rn16 of it: 2^-11 |sum32 - hi'| <= 2^-22 |sum32|, or at most 2^-25 below 2^-14:
          |hi' + lo' - ref| <= 2^-22 |ref| + 2^-23 (|hi| + |lo| + |s res|) + 2^-24
      -- the issue's 2^-21 |ref| + 2^-22 (...) + 2^-24 with its first two terms halved; the last term as above.
Both are tests/controlnet_reference.add_residuals_bound; tests/test_controlnet.py checks on the same tensors that they pass the fp32
evaluation and reject the neighbouring table row, the neighbouring tensor's residual and a dropped `lo`.
"""
import os

import numpy as np
import pytest
import torch

from tests import controlnet_reference as R
from tests.parity import REL_TOL_UNET, compare, hip_unet_from_oracle, oracle_small_unet, small_unet_inputs

pytestmark = pytest.mark.gpu

f16 = torch.float16


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h16(t):
    return t.half().float()


# ---------------------------------------------------------------------------------------------------------- the kernel
GUARD = 64          # fp16 values of poison on either side of every destination


def _guarded(n, dev, poison):
    buf = torch.full((n + 2 * GUARD,), poison, dtype=f16, device=dev)
    return buf, buf[GUARD: GUARD + n]


def _guards_intact(buf, n, poison):
    b = buf.cpu()
    return bool((b[:GUARD] == poison).all()) and bool((b[GUARD + n:] == poison).all())


@pytest.fixture(scope="module")
def kcase():
    return R.kernel_case()


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("s", R.KERNEL_SCALES)
def test_add_residuals_kernel(dev, kcase, s, precise):
    """one launch, 13 tensors, a 3-row table read at row 2 through the device step counter; out of place into poisoned, guarded buffers"""
    K = pkg().kernels
    skips, lows, ress = kcase
    d = lambda ts: [t.to(dev) for t in ts]
    sk, rs = d(skips), d(ress)
    if precise:
        for t, lo in zip(sk, d(lows)):
            t._i2v_lo = lo
    table, idx = R.kernel_table(s).to(dev), torch.tensor([R.KERNEL_ROW], dtype=torch.int32, device=dev)
    runs = []
    for _ in range(2):
        bufs = [_guarded(t.numel(), dev, 777.0) for t in sk]
        lo_bufs = [_guarded(t.numel(), dev, -555.0) for t in sk]
        outs = [v for _, v in bufs]
        # (the wrapper allocates the low halves itself; to guard them too, the launch is issued with its own buffers through the ABI)
        L = pkg()._lib
        p = L.AddResidualsParams()
        for j, t in enumerate(sk):
            e = p.t[j]
            e.dst, e.skip, e.res, e.numel = outs[j].data_ptr(), t.data_ptr(), rs[j].data_ptr(), t.numel()
            if precise:
                e.dst_lo, e.skip_lo = lo_bufs[j][1].data_ptr(), K.lo_of(t).data_ptr()
        p.n, p.scale_table, p.scale_rows, p.step_idx = len(sk), table.data_ptr(), 3, idx.data_ptr()
        L.check(L.load().i2v_add_residuals_f16(p, K._stream()), "i2v_add_residuals_f16")
        torch.cuda.synchronize()
        for (buf, _), (lbuf, _), t in zip(bufs, lo_bufs, sk):
            assert _guards_intact(buf, t.numel(), 777.0), "dst written outside the tensor"
            assert _guards_intact(lbuf, t.numel(), -555.0) and (precise or bool((lbuf == -555.0).all())), "dst_lo written outside"
        runs.append(([o.cpu() for o in outs], [l.cpu() for _, l in lo_bufs]))
    for a, al, b, bl in zip(runs[0][0], runs[0][1], runs[1][0], runs[1][1]):
        assert torch.equal(a, b) and torch.equal(al, bl), "two runs differ"
    outs, louts = runs[0]
    worst = 0.0
    for i, (hi, lo, r, o, ol) in enumerate(zip(skips, lows, ress, outs, louts)):
        if s == 0.0:
            assert torch.equal(o.view(torch.int16), hi.view(torch.int16)), f"s = 0: tensor {i} is not the skip bit for bit"
            if precise:
                assert torch.equal(ol.view(torch.int16), lo.view(torch.int16)), f"s = 0: lo of tensor {i} changed"
            continue
        l = lo if precise else None
        ref, bound = R.add_residuals_fp64(hi, r, s, l), R.add_residuals_bound(hi, r, s, l)
        got = o.double() + (ol.double() if precise else 0.0)
        ratio = ((got - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"tensor {i} ({hi.numel()} values), s {s}, precise {precise}: worst |err| / bound = {ratio:.3f}"
    print(f"i2v_add_residuals_f16 s={s} precise={precise}: worst |err| / bound = {worst:.3f}")
    # the wrapper, same launch: equal to the raw call, lo attached
    w = K.add_residuals(sk, rs, scale=(table, idx))
    for o, g in zip(outs, w):
        assert torch.equal(o, g.cpu()) and (K.lo_of(g) is not None) == precise


@pytest.mark.parametrize("precise", [False, True])
def test_add_residuals_single_tensor_in_place_and_null_table(dev, kcase, precise):
    """n = 1: out of place == in place; scale None is s = 1, a table without a step counter reads row 0"""
    K = pkg().kernels
    skips, lows, ress = kcase
    i = 2
    mk = lambda: (skips[i].to(dev), lows[i].to(dev), ress[i].to(dev))
    hi, lo, r = mk()
    if precise:
        hi._i2v_lo = lo
    out, = K.add_residuals([hi], [r])
    assert out.data_ptr() != hi.data_ptr() and torch.equal(hi.cpu(), skips[i])
    hi2, lo2, r2 = mk()
    if precise:
        hi2._i2v_lo = lo2
    same, = K.add_residuals([hi2], [r2], out=[hi2])
    assert same is hi2 and torch.equal(same, out)
    if precise:
        assert K.lo_of(same).data_ptr() == lo2.data_ptr() and torch.equal(K.lo_of(same), K.lo_of(out))
    l = lows[i] if precise else None
    ref, bound = R.add_residuals_fp64(skips[i], ress[i], 1.0, l), R.add_residuals_bound(skips[i], ress[i], 1.0, l)
    got = out.double().cpu() + (K.lo_of(out).double().cpu() if precise else 0.0)
    assert bool(((got - ref).abs() <= bound).all())
    row0, = K.add_residuals([hi], [r], scale=(torch.tensor([1.0, 5.0], device=dev), None))
    assert torch.equal(row0, out)
    clamped, = K.add_residuals([hi], [r], scale=(torch.tensor([5.0, 1.0], device=dev), torch.tensor([7], dtype=torch.int32, device=dev)))
    assert torch.equal(clamped, out), "a step counter past the table reads its last row"


def test_add_residuals_more_than_sixteen_pairs(dev):
    K = pkg().kernels
    g = torch.Generator().manual_seed(9)
    sizes = [8 * (3 + 37 * j) for j in range(19)]
    sk = [torch.randn(n, generator=g).half() for n in sizes]
    rs = [torch.randn(n, generator=g).half() for n in sizes]
    table = torch.tensor([-0.75], device=dev)
    outs = K.add_residuals([t.to(dev) for t in sk], [t.to(dev) for t in rs], scale=(table, None))
    assert len(outs) == 19
    for a, b, o in zip(sk, rs, outs):
        assert bool(((o.double().cpu() - R.add_residuals_fp64(a, b, -0.75)).abs() <= R.add_residuals_bound(a, b, -0.75)).all())


def test_add_residuals_past_two_to_the_31(dev):
    """one tensor of 2^31 + 8 * 37 values (8.6 GB of operands, in place): chunk and element indices past 2^31 (and 2^32 bytes) address
    the right memory -- the head, the region around the 2^31-st value and the tail are checked against fp64, a second small tensor after
    the big one checks the prefix walk behind it"""
    K = pkg().kernels
    n = 2 ** 31 + 8 * 37
    g = torch.Generator(device=dev).manual_seed(4)
    skip = torch.randn(n, generator=g, device=dev, dtype=f16)
    res = torch.randn(n, generator=g, device=dev, dtype=f16)
    small, small_res = torch.randn(8 * 37, generator=g, device=dev, dtype=f16), torch.randn(8 * 37, generator=g, device=dev, dtype=f16)
    spans = [(0, 4096), (2 ** 30 - 2048, 2 ** 30 + 2048), (2 ** 31 - 4096, n)]
    want = [(skip[a:b].cpu(), res[a:b].cpu()) for a, b in spans]
    table = torch.tensor([-0.75], device=dev)
    untouched = skip[4096: 8192].clone()
    out, out_small = K.add_residuals([skip, small.clone()], [res, small_res], scale=(table, None), out=[skip, torch.empty_like(small)])
    assert out is skip
    for (a, b), (sk, rs) in zip(spans, want):
        ref, bound = R.add_residuals_fp64(sk, rs, -0.75), R.add_residuals_bound(sk, rs, -0.75)
        assert bool(((skip[a:b].double().cpu() - ref).abs() <= bound).all()), f"values {a} .. {b}"
    assert not torch.equal(skip[4096: 8192], untouched)
    ref, bound = R.add_residuals_fp64(small.cpu(), small_res.cpu(), -0.75), R.add_residuals_bound(small.cpu(), small_res.cpu(), -0.75)
    assert bool(((out_small.double().cpu() - ref).abs() <= bound).all())


def test_add_residuals_argument_errors(dev):
    """checked on the host with error codes, nothing launched"""
    L, K = pkg()._lib, pkg().kernels
    h = L.load()
    a = torch.zeros(32, dtype=f16, device=dev)
    p = L.AddResidualsParams()

    def one(**kw):
        q = L.AddResidualsParams()
        e = q.t[0]
        e.dst, e.skip, e.res, e.numel = a.data_ptr(), a.data_ptr(), a.data_ptr(), 16
        q.n = 1
        for k, v in kw.items():
            setattr(q if k in ("n", "scale_rows", "scale_table") else q.t[0], k, v)
        return h.i2v_add_residuals_f16(q, None)

    assert h.i2v_add_residuals_f16(None, None) == -1 and h.i2v_add_residuals_f16(p, None) == -1
    assert one(n=17) == -1 and one(numel=12) == -1 and one(numel=0) == -1 and one(res=None) == -1 and one(dst=None) == -1
    assert one(skip=a.data_ptr() + 2) == -1 and b"16-byte aligned" in h.i2v_last_error()
    assert one(skip_lo=a.data_ptr()) == -1 and b"come together" in h.i2v_last_error()
    assert one(scale_table=a.data_ptr(), scale_rows=0) == -1
    with pytest.raises(ValueError):
        K.add_residuals([a], [a[:16]])


# ---------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def small_cn(dev):
    """(reference, HIP model with the reference's weights, inputs, the reference's outputs at scale 1)"""
    ref = R.small_reference()
    cn = pkg().ControlNetModel(**R.small_config())
    cn.load_state_dict(ref.state_dict())
    cn = cn.to(dev, f16).eval()
    inp = R.small_inputs(batch=1)
    with torch.no_grad():
        want = ref(inp["sample"], inp["timestep"], inp["ctx"], inp["cond"])
    return ref, cn, inp, want


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_controlnet_forward_against_the_reference(dev, small_cn, scale):
    _, cn, inp, (down, mid) = small_cn
    with torch.no_grad():
        out = cn(inp["sample"].to(dev).view(1, R.SMALL_FRAMES, 4, R.SMALL_LATENT, R.SMALL_LATENT), inp["timestep"].to(dev),
                 inp["ctx"].to(dev), inp["cond"].to(dev), conditioning_scale=scale)
    assert len(out.down_block_res_samples) == 12
    for i, (g, w) in enumerate(zip(out.down_block_res_samples + (out.mid_block_res_sample,), down + (mid,))):
        assert g.dtype == torch.float32 and w.abs().max().item() > 1e-2
        compare(g, w * scale, rel=REL_TOL_UNET, name=f"ControlNet small, scale {scale}, tensor {i}")


def test_controlnet_module_api_equals_the_token_entry_points(dev, small_cn):
    K = pkg().kernels
    _, cn, inp, _ = small_cn
    with torch.no_grad():
        sample, ctx, cond = inp["sample"].to(dev), inp["ctx"].to(dev, f16), inp["cond"].to(dev)
        down, mid = cn(sample, inp["timestep"].to(dev), ctx, cond, return_dict=False)
        table = cn.project_time_table(torch.tensor([3.0, 481.0, 999.0], device=dev))
        temb = K.select_row(table, torch.tensor([1], dtype=torch.int32, device=dev))
        tdown, tmid = cn._fwd_tokens(K.nchw_to_tokens(sample, 8), temb, cn.project_context(ctx), cn.embed_condition(cond))
    assert tuple(cn.embed_condition(cond).shape) == (R.SMALL_FRAMES, R.SMALL_LATENT, R.SMALL_LATENT, 32)
    for a, b in zip(down + (mid,), tdown + (tmid,)):
        assert torch.equal(a, K.tokens_to_nchw(b, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------- the UNet
@pytest.fixture(scope="module")
def small_unet(dev):
    """(oracle, HIP UNet, inputs, random residuals shaped like the skip tensors, the oracle's outputs with them)"""
    ou = oracle_small_unet()
    hu = hip_unet_from_oracle(ou, dev)
    inp = small_unet_inputs(b=2, f=2)
    same = inp["sample"][:1]
    inp["sample"], inp["timestep"] = torch.cat([same, same]), torch.tensor([481, 481])     # a CFG-shaped batch: cfg_shared_prefix applies
    g = torch.Generator().manual_seed(23)
    n, ch = 4, (32, 64, 128, 128)
    shapes = [(n, 32, 16, 16)]
    for i, c in enumerate(ch):
        hw = 16 >> i
        shapes += [(n, c, hw, hw)] * 2
        if i < 3:
            shapes.append((n, c, hw // 2, hw // 2))
    down = [h16(torch.randn(s, generator=g) * 0.5) for s in shapes]
    mid = h16(torch.randn((n, 128, 2, 2), generator=g) * 0.5)
    with torch.no_grad():
        want = {e: ou(inp["sample"], inp["timestep"], e, inp["ctx"], down_block_additional_residuals=down,
                      mid_block_additional_residual=mid).sample for e in (True, False)}
    return ou, hu, inp, down, mid, want


def _hip_unet(hu, dev, inp, enable, down=None, mid=None, **kw):
    with torch.no_grad():
        return hu(inp["sample"].to(dev), inp["timestep"].to(dev), enable, inp["ctx"].to(dev),
                  down_block_additional_residuals=None if down is None else [d.to(dev) for d in down],
                  mid_block_additional_residual=None if mid is None else mid.to(dev), **kw).sample


def test_unet_with_residuals_against_the_oracle(dev, small_unet):
    """cross-frame attention on and the CFG prefix shared.  The mid block must read the last skip tensor WITHOUT its residual: an
    in-place add of the down residuals fails here"""
    ou, hu, inp, down, mid, want = small_unet
    assert len(down) == 12
    got = _hip_unet(hu, dev, inp, True, down, mid, cross_attention_kwargs={"cfg_shared_prefix": True})
    compare(got, want[True], rel=REL_TOL_UNET, name="small UNet + residuals, cross-frame, cfg_shared")
    plain = _hip_unet(hu, dev, inp, True)
    assert (plain.cpu() - want[True]).abs().max().item() > 10 * REL_TOL_UNET * want[True].abs().max().item(), "the residuals change nothing"
    got = _hip_unet(hu, dev, inp, False, down, mid)
    compare(got, want[False], rel=REL_TOL_UNET, name="small UNet + residuals, no cross-frame")
    only_mid = _hip_unet(hu, dev, inp, True, None, mid)
    with torch.no_grad():
        compare(only_mid, ou(inp["sample"], inp["timestep"], True, inp["ctx"], mid_block_additional_residual=mid).sample, rel=REL_TOL_UNET,
                name="small UNet + mid residual only")


def test_unet_with_residuals_precise_stream(dev, small_unet):
    from i2v_adapter_unofficial_amd import blocks
    _, hu, inp, down, mid, want = small_unet
    prev = blocks.set_precise_stream(True)
    try:
        got = _hip_unet(hu, dev, inp, True, down, mid)
    finally:
        blocks.set_precise_stream(prev)
    compare(got, want[True], rel=REL_TOL_UNET, name="small UNet + residuals, precise stream")


@pytest.mark.parametrize("precise", [False, True])
def test_unet_zero_residuals_are_bit_equal_to_none(dev, small_unet, precise):
    from i2v_adapter_unofficial_amd import blocks
    _, hu, inp, down, mid, _ = small_unet
    prev = blocks.set_precise_stream(precise)
    try:
        base = _hip_unet(hu, dev, inp, True)
        zero = _hip_unet(hu, dev, inp, True, [torch.zeros_like(d) for d in down], torch.zeros_like(mid))
    finally:
        blocks.set_precise_stream(prev)
    assert torch.equal(base, zero)


# ---------------------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def pipe_parts(dev, small_cn, small_unet):
    return small_unet[1], small_cn[1]


def _problem(seed=31, frames=R.SMALL_FRAMES):
    g = torch.Generator().manual_seed(seed)
    return dict(prompt_embeds=h16(torch.randn(1, 7, 64, generator=g)), negative_prompt_embeds=h16(torch.randn(1, 7, 64, generator=g)),
                condition_image_latents=torch.randn(1, 4, 16, 16, generator=g), num_frames=frames, guidance_scale=7.5,
                output_type="latent"), torch.rand(frames, 3, 128, 128, generator=g)


def _gens():
    return dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _sched(kind):
    p = pkg()
    return {"ddim": p.DDIMScheduler, "dpmsolver++": p.DPMSolverMultistepScheduler, "lcm": p.LCMScheduler}[kind]()


def test_pipeline_scale_zero_is_the_pipeline_without_a_controlnet(dev, pipe_parts):
    hu, cn = pipe_parts
    kw, frames = _problem()
    plain = pkg().I2VAdapterPipeline(unet=hu)(**kw, num_inference_steps=3, **_gens()).frames
    pipe = pkg().I2VAdapterPipeline(unet=hu, controlnet=cn)
    off = pipe(**kw, num_inference_steps=3, control_image=frames, controlnet_conditioning_scale=0.0, **_gens()).frames
    assert torch.equal(off, plain)
    on = pipe(**kw, num_inference_steps=3, control_image=frames, **_gens()).frames        # scale 1: another table, the same graph
    assert len(pipe._graph_cache) == 1 and (on - plain).abs().max().item() > 1e-2 and torch.equal(on[:, 0], plain[:, 0])


def test_pipeline_graph_equals_eager_and_replays_for_other_control_frames(dev, pipe_parts):
    hu, cn = pipe_parts
    kw, frames = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=hu, controlnet=cn)
    graph = pipe(**kw, num_inference_steps=3, control_image=frames, **_gens()).frames
    eager = pipe(**kw, num_inference_steps=3, control_image=frames, use_graph=False, **_gens()).frames
    assert torch.equal(graph, eager)
    first = pipe._graph
    kw2, frames2 = _problem(seed=77)
    import PIL.Image
    pil = [PIL.Image.fromarray((f.permute(1, 2, 0).numpy() * 255).astype("uint8")) for f in frames2]
    again = pipe(**kw2, num_inference_steps=3, control_image=pil, **_gens()).frames
    assert pipe._graph is first and len(pipe._graph_cache) == 1, "a second sample of the same shape re-captured the step"
    eager2 = pipe(**kw2, num_inference_steps=3, control_image=pil, use_graph=False, **_gens()).frames
    assert torch.equal(again, eager2) and not torch.equal(again, graph)
    other = pipe(**kw2, num_inference_steps=3, control_image=frames, **_gens()).frames
    assert not torch.equal(other, again), "the control frames do not reach the replayed graph"
    # with CFG off: one copy of the batch
    kw1 = dict(kw, guidance_scale=1.0)
    kw1.pop("negative_prompt_embeds")
    g1 = pipe(**kw1, num_inference_steps=3, control_image=frames, **_gens()).frames
    e1 = pipe(**kw1, num_inference_steps=3, control_image=frames, use_graph=False, **_gens()).frames
    assert torch.equal(g1, e1)


def test_pipeline_control_window(dev, pipe_parts):
    """control_guidance_start = 0.5 over 4 steps: the table is [0, 0, 1, 1] -- the latents after step 2 are the no-ControlNet run's,
    after step 4 they differ"""
    hu, cn = pipe_parts
    kw, frames = _problem()

    def run(pipe, **extra):
        seen = {}
        out = pipe(**kw, num_inference_steps=4, callback=lambda i, t, lat: seen.__setitem__(i, lat.clone()), **extra, **_gens()).frames
        return seen, out
    base, base_out = run(pkg().I2VAdapterPipeline(unet=hu))
    pipe = pkg().I2VAdapterPipeline(unet=hu, controlnet=cn)
    seen, out = run(pipe, control_image=frames, control_guidance_start=0.5)
    assert sorted(seen) == [0, 1, 2, 3]
    assert torch.equal(seen[0], base[0]) and torch.equal(seen[1], base[1])
    assert not torch.equal(seen[3], base[3]) and not torch.equal(out, base_out)
    graph = pipe(**kw, num_inference_steps=4, control_image=frames, control_guidance_start=0.5, **_gens()).frames
    assert torch.equal(graph, out)


@pytest.mark.parametrize("kind", ["dpmsolver++", "lcm"])
def test_pipeline_other_schedulers_graph_equals_eager(dev, pipe_parts, kind):
    hu, cn = pipe_parts
    kw, frames = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=hu, controlnet=cn, scheduler=_sched(kind))
    graph = pipe(**kw, num_inference_steps=3, control_image=frames, **_gens()).frames
    eager = pipe(**kw, num_inference_steps=3, control_image=frames, use_graph=False, **_gens()).frames
    plain = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched(kind))(**kw, num_inference_steps=3, **_gens()).frames
    assert torch.equal(graph, eager) and not torch.equal(graph, plain)


def test_pipeline_free_init_fast_sampling(dev, pipe_parts):
    hu, cn = pipe_parts
    kw, frames = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=hu, controlnet=cn)
    pipe.enable_free_init(num_iters=2, use_fast_sampling=True)
    graph = pipe(**kw, num_inference_steps=4, control_image=frames, control_guidance_end=0.5, **_gens()).frames
    eager = pipe(**kw, num_inference_steps=4, control_image=frames, control_guidance_end=0.5, use_graph=False, **_gens()).frames
    assert torch.isfinite(graph).all() and torch.equal(graph, eager)


# ---------------------------------------------------------------------------------------------------------- the driver
def test_eval_driver_with_a_controlnet(dev, tmp_path, monkeypatch):
    """`--controlnet PATH --control_column NAME` on a two-row CSV: a directory of frames and an animated GIF"""
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
    init_random_weights_(p.ControlNetModel(**R.small_config()), seed=5).save_pretrained(os.path.join(root, "control"))
    rs = np.random.RandomState(0)
    img = lambda h, w: PIL.Image.fromarray((rs.rand(h, w, 3) * 255).astype("uint8"))
    os.makedirs(os.path.join(root, "data", "images"))
    os.makedirs(os.path.join(root, "data", "pose0"))
    for j in range(5):                                    # more frames than the clip needs: the first four in sorted order
        img(48, 80).save(os.path.join(root, "data", "pose0", f"{j:03d}.png"))
    gif = [img(64, 64) for _ in range(4)]
    gif[0].save(os.path.join(root, "data", "pose1.gif"), save_all=True, append_images=gif[1:], duration=100, loop=0)
    names = ["a cat on a boat", "two dogs, running"]
    with open(os.path.join(root, "data", "eval.csv"), "w") as f:
        f.write("image_path,name,pose\n")
        for i, (nm, pose) in enumerate(zip(names, ("pose0", "pose1.gif"))):
            img(70, 90).save(os.path.join(root, "data", "images", f"{i}.png"))
            f.write(f'images/{i}.png,"{nm}",{pose}\n')
    g = torch.Generator().manual_seed(5)
    save_file({"prompt_embeds": torch.randn(2, 7, 64, generator=g), "negative_prompt_embeds": torch.randn(1, 7, 64, generator=g)},
              os.path.join(root, "embeds.safetensors"))
    seen = []
    call = I2VAdapterPipeline.__call__

    def spy(self, *a, **k):
        seen.append((len(k["control_image"]), k["control_image"][0].size, k["controlnet_conditioning_scale"], k["control_guidance_start"],
                     k["control_guidance_end"], type(self.controlnet).__name__))
        return call(self, *a, **k)
    monkeypatch.setattr(I2VAdapterPipeline, "__call__", spy)
    common = ["--task_name", "demo", "--checkpoint_epoch", "3", "--eval_data_path", os.path.join(root, "data", "eval.csv"),
              "--embeds", os.path.join(root, "embeds.safetensors"), "--model_path", os.path.join(root, "sd"),
              "--motion_adapter_path", os.path.join(root, "motion"), "--checkpoint_root", os.path.join(root, "checkpoint"),
              "--samples_root", os.path.join(root, "samples"), "--num_frames", "4", "--num_inference_steps", "4"]
    assert main(common + ["--controlnet", os.path.join(root, "control"), "--control_column", "pose", "--controlnet_scale", "0.8",
                          "--control_guidance_start", "0.25", "--control_guidance_end", "0.75"]) == 0
    assert seen == [(4, (80, 48), 0.8, 0.25, 0.75, "ControlNetModel"), (4, (64, 64), 0.8, 0.25, 0.75, "ControlNetModel")]
    for nm in names:
        out = PIL.Image.open(os.path.join(root, "samples", "demo", "epoch_3", f"{nm}.gif"))
        assert out.n_frames == 4 and out.size == (64, 64)
    assert main(common + ["--controlnet", os.path.join(root, "control")]) == -1      # the two options come together
