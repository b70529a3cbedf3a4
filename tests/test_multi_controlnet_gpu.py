"""Multi-ControlNet on the GPU: `i2v_add_multi_residuals_f16` against fp64 and its bit-level contracts, `MultiControlNetModel.forward`
against the sum of two fp32 references, and the pipeline (one net in a Multi == the plain net, a silent net changes no bit, graph ==
eager under every scheduler, graph-cache replay with other frames, scales and windows, the hires fix, mixed channel counts, the driver).

The bounds of the kernel test, per element, against the fp64 value `ref` of skip (+ lo) + sum_k s_k res_k (N nets; rn32 / rn16 = round
to nearest fp32 / fp16, relative error 2^-24 / 2^-11; S = sum_k |s_k res_k|).  They generalise tests/test_controlnet_gpu.py's: one
rounding per product, one per addition.
  the sum of the products   acc = rn32(... rn32(rn32(s_0 res_0) + rn32(s_1 res_1)) ... + rn32(s_N-1 res_N-1)).  The N products: 2^-24 S.
      The N - 1 additions: each 2^-24 |partial sum| <= 2^-24 S (1 + 2^-23).  Together |e_acc| <= N 2^-24 S.
  default stream   out = rn16(rn32(skip + acc)).  The addition: 2^-24 |skip + acc| <= 2^-24 (|skip| + S).  So
      |e32| <= 2^-24 (|skip| + (N + 1) S); the rounding to fp16 as for one net (2^-11 |sum32| for a normal result, at most 2^-25 below
      2^-14, never both):
          |out - ref| <= 2^-11 |ref| + 2^-24 (|skip| + (N + 1) S) + 2^-24
      -- the issue's bound as it stands; for N = 1 it is the single-net bound.  The last term pays the second-order terms as there
      (the test's values stay below 16).
  precise pair   sum32 = rn32(rn32(hi + lo) + acc): 2^-24 (|hi| + |lo|) for the pair, N 2^-24 S for acc, 2^-24 (|hi| + |lo| + S) for
      the addition: |e32| <= 2^-23 (|hi| + |lo|) + (N + 1) 2^-24 S.  hi' = rn16(sum32), sum32 - hi' exact, lo' = rn16 of it:
          |hi' + lo' - ref| <= 2^-22 |ref| + 2^-23 (|hi| + |lo|) + 2^-24 (N + 1) S + 2^-24
      -- the issue's 2^-23 (|hi| + |lo| + N S) has 2 N where the derivation gives N + 1: the tighter form is taken (equal for N = 1).
Where every product is zero the kernel returns the skip's bits: those cases are checked for bit equality instead.
Both bounds are tests/multi_controlnet_reference.bound; tests/test_multi_controlnet.py checks on the same tensors that they pass the
fp32 restatement (with and without an FMA chain) and reject five wrong evaluations.
"""
import os

import numpy as np
import pytest
import torch

from tests import controlnet_reference as R
from tests import multi_controlnet_reference as M
from tests.parity import REL_TOL_UNET, compare, hip_unet_from_oracle, oracle_small_unet

pytestmark = pytest.mark.gpu

f16 = torch.float16
i16 = torch.int16


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h16(t):
    return t.half().float()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(i16), b.view(i16))


# ---------------------------------------------------------------------------------------------------------- the kernel
GUARD = 64          # fp16 values of poison on either side of every destination


def _guarded(n, dev, poison):
    buf = torch.full((n + 2 * GUARD,), poison, dtype=f16, device=dev)
    return buf, buf[GUARD: GUARD + n]


def _guards_intact(buf, n, poison):
    b = buf.cpu()
    return bool((b[:GUARD] == poison).all()) and bool((b[GUARD + n:] == poison).all())


def _on(dev, n_nets, precise):
    """the shared case on the device: (skips with their low halves attached when precise, residual sets)"""
    K = pkg().kernels
    skips, lows, sets = M.case(n_nets)
    sk = [t.to(dev) for t in skips]
    if precise:
        for t, lo in zip(sk, lows):
            t._i2v_lo = lo.to(dev)
    assert all((K.lo_of(t) is not None) == precise for t in sk)
    return sk, [[t.to(dev) for t in rs] for rs in sets]


def _idx(dev, row):
    return torch.tensor([row], dtype=torch.int32, device=dev)


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("scales", [s for n in (1, 2, 3, 4) for s in M.SCALES[n]])
def test_add_multi_residuals_kernel(dev, scales, precise):
    """one launch, 13 tensors, N nets, a [N, 3] table read at row 2 through the device step counter; out of place into poisoned,
    guarded buffers (the low halves too: the launch is issued through the ABI with its own buffers)"""
    K, L = pkg().kernels, pkg()._lib
    n_nets = len(scales)
    skips, lows, sets = M.case(n_nets)
    sk, rs = _on(dev, n_nets, precise)
    tab, idx = M.table(scales).to(dev), _idx(dev, M.ROW)
    bufs = [_guarded(t.numel(), dev, 777.0) for t in sk]
    lo_bufs = [_guarded(t.numel(), dev, -555.0) for t in sk]
    p = L.AddMultiResidualsParams()
    for j, t in enumerate(sk):
        e = p.t[j]
        e.dst, e.skip, e.numel = bufs[j][1].data_ptr(), t.data_ptr(), t.numel()
        for k in range(n_nets):
            e.res[k] = rs[k][j].data_ptr()
        if precise:
            e.dst_lo, e.skip_lo = lo_bufs[j][1].data_ptr(), K.lo_of(t).data_ptr()
    p.n, p.n_nets, p.scale_table, p.scale_rows, p.step_idx = len(sk), n_nets, tab.data_ptr(), M.ROWS, idx.data_ptr()
    L.check(L.load().i2v_add_multi_residuals_f16(p, K._stream()), "i2v_add_multi_residuals_f16")
    torch.cuda.synchronize()
    worst = 0.0
    for i, ((buf, o), (lbuf, ol), hi, lo) in enumerate(zip(bufs, lo_bufs, skips, lows)):
        assert _guards_intact(buf, hi.numel(), 777.0), f"dst of tensor {i} written outside the tensor"
        assert _guards_intact(lbuf, hi.numel(), -555.0) and (precise or bool((lbuf == -555.0).all())), f"dst_lo of tensor {i} written outside"
        ress = [s[i] for s in sets]
        l = lo if precise else None
        ref, bound = M.fp64(hi, ress, scales, l), M.bound(hi, ress, scales, l)
        got = o.cpu().double() + (ol.cpu().double() if precise else 0.0)
        ratio = ((got - ref).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"tensor {i} ({hi.numel()} values), scales {scales}, precise {precise}: worst |err| / bound = {ratio:.3f}"
    print(f"i2v_add_multi_residuals_f16 N={n_nets} scales={scales} precise={precise}: worst |err| / bound = {worst:.4f}")
    # the wrapper issues the same launch: equal bits, the low halves attached
    w = K.add_multi_residuals(sk, rs, scale=(tab, idx))
    for (_, o), (_, ol), g in zip(bufs, lo_bufs, w):
        assert same_bits(o, g) and (K.lo_of(g) is not None) == precise
        assert not precise or same_bits(ol, K.lo_of(g))


# ---------------------------------------------------------------------------------------------------------- bit equalities
def _run(dev, n_nets, precise, table, idx=None, use=None):
    """add_multi_residuals on the shared case with residual sets `use` (indices into the case's sets) -> (outputs, their low halves)"""
    K = pkg().kernels
    sk, rs = _on(dev, n_nets, precise)
    rs = rs if use is None else [rs[k] for k in use]
    out = K.add_multi_residuals(sk, rs, scale=None if table is None else (torch.tensor(table, dtype=torch.float32, device=dev), idx))
    return out, [K.lo_of(o) for o in out]


def _assert_same(a, b, what):
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert same_bits(x, y), f"{what}: tensor {i} differs"
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert (x is None) == (y is None) and (x is None or same_bits(x, y)), f"{what}: the low half of tensor {i} differs"


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("s", [1.0, -0.75])
def test_one_net_is_add_residuals_bit_for_bit(dev, s, precise):
    K = pkg().kernels
    sk, rs = _on(dev, 1, precise)
    tab = torch.tensor([s + 1.0, s], dtype=torch.float32, device=dev)
    idx = _idx(dev, 1)
    want = K.add_residuals(sk, rs[0], scale=(tab, idx))
    got = K.add_multi_residuals(sk, rs, scale=(tab.view(1, 2), idx))
    _assert_same((got, [K.lo_of(o) for o in got]), (want, [K.lo_of(o) for o in want]), "out of place")
    # in place, each on its own copy of the skips
    mine, theirs = _on(dev, 1, precise)[0], _on(dev, 1, precise)[0]
    got = K.add_multi_residuals(mine, rs, scale=(tab.view(1, 2), idx), out=mine)
    K.add_residuals(theirs, rs[0], scale=(tab, idx), out=theirs)
    assert all(g is m for g, m in zip(got, mine))
    _assert_same((mine, [K.lo_of(o) for o in mine]), (theirs, [K.lo_of(o) for o in theirs]), "in place")
    _assert_same((mine, [K.lo_of(o) for o in mine]), (want, [K.lo_of(o) for o in want]), "in place against out of place")


@pytest.mark.parametrize("precise", [False, True])
def test_a_silent_net_changes_no_bit(dev, precise):
    a, b = -0.75, 0.5
    one = _run(dev, 2, precise, [[a]], use=[0])
    _assert_same(_run(dev, 2, precise, [[a], [0.0]]), one, "N = 2 with (a, 0) against N = 1 with a")
    _assert_same(_run(dev, 2, precise, [[0.0], [a]], use=[1, 0]), one, "N = 2 with (0, a) against N = 1 with a")
    two = _run(dev, 3, precise, [[a], [b]], use=[0, 2])
    _assert_same(_run(dev, 3, precise, [[a], [0.0], [b]]), two, "N = 3 with (a, 0, b) against N = 2 with (a, b)")
    _assert_same(_run(dev, 4, precise, [[a], [0.0], [b], [0.0]]), two, "N = 4 with (a, 0, b, 0) against N = 2 with (a, b)")


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("n_nets", [1, 2, 3, 4])
def test_all_zero_scales_return_the_skip_bits(dev, n_nets, precise):
    """-0 planted in the skip, its low half and the residuals: every product is +-0, and the skip's bits (and its low half's) come back"""
    K = pkg().kernels
    skips, lows, sets = M.case(n_nets)
    plant = lambda t: torch.where(torch.arange(t.numel()) % 5 == 0, torch.tensor(-0.0, dtype=f16), t)
    sk = [plant(t).to(dev) for t in skips]
    lo = [plant(t).to(dev) for t in lows]
    rs = [[plant(t).to(dev) for t in s] for s in sets]
    if precise:
        for t, l in zip(sk, lo):
            t._i2v_lo = l
    out = K.add_multi_residuals(sk, rs, scale=(torch.zeros(n_nets, 2, device=dev), None))
    for i, (o, t, l) in enumerate(zip(out, sk, lo)):
        assert o.data_ptr() != t.data_ptr() and same_bits(o, t), f"tensor {i}"
        assert bool((o.view(i16)[::5] == -32768).all()), "-0 did not survive"
        assert not precise or same_bits(K.lo_of(o), l), f"low half of tensor {i}"


def test_step_counter_clamp_null_table_and_null_counter(dev):
    a = -0.75
    rows = [[5.0, 3.0, a], [7.0, 2.0, 0.5]]
    first = _run(dev, 2, False, [[5.0], [7.0]])
    last = _run(dev, 2, False, [[a], [0.5]])
    _assert_same(_run(dev, 2, False, rows, _idx(dev, 2)), last, "row 2")
    _assert_same(_run(dev, 2, False, rows, _idx(dev, 9)), last, "a step counter past the table reads its last row")
    _assert_same(_run(dev, 2, False, rows, _idx(dev, -4)), first, "a negative step counter reads row 0")
    _assert_same(_run(dev, 2, False, rows, None), first, "no step counter reads row 0")
    assert not same_bits(first[0][4], last[0][4])
    _assert_same(_run(dev, 2, True, None), _run(dev, 2, True, [[1.0], [1.0]]), "no table is every s_k = 1")


def test_more_than_sixteen_tensors(dev):
    K = pkg().kernels
    g = torch.Generator().manual_seed(9)
    sizes = [8 * (3 + 37 * j) for j in range(20)]
    sk = [torch.randn(n, generator=g).half() for n in sizes]
    sets = [[torch.randn(n, generator=g).half() for n in sizes] for _ in range(3)]
    scales = (1.0, -0.75, 0.5)
    outs = K.add_multi_residuals([t.to(dev) for t in sk], [[t.to(dev) for t in s] for s in sets],
                                 scale=(torch.tensor(scales, device=dev).view(3, 1), None))
    assert len(outs) == 20
    for i, (a, o) in enumerate(zip(sk, outs)):
        ress = [s[i] for s in sets]
        assert bool(((o.double().cpu() - M.fp64(a, ress, scales)).abs() <= M.bound(a, ress, scales)).all()), f"tensor {i}"


# ---------------------------------------------------------------------------------------------------------- the model
SEEDS = (4321, 777)


@pytest.fixture(scope="module")
def small_nets(dev):
    """two (reference, HIP model with its weights) pairs with different seeds, and the inputs"""
    pairs = []
    for seed in SEEDS:
        ref = R.small_reference(seed)
        cn = pkg().ControlNetModel(**R.small_config())
        cn.load_state_dict(ref.state_dict())
        pairs.append((ref, cn.to(dev, f16).eval()))
    return pairs, R.small_inputs(batch=1)


def test_multi_forward_against_the_sum_of_two_references(dev, small_nets):
    """the tolerance is test_controlnet_forward_against_the_reference's for one net -- REL_TOL_UNET of the largest value of that net's
    (scaled) reference output -- once per net: the nets' errors add"""
    pairs, inp = small_nets
    scales = (1.0, -0.75)
    conds = [inp["cond"], h16(torch.rand(inp["cond"].shape, generator=torch.Generator().manual_seed(8)))]
    with torch.no_grad():
        wants = [ref(inp["sample"], inp["timestep"], inp["ctx"], c, conditioning_scale=s) for (ref, _), c, s in zip(pairs, conds, scales)]
        multi = pkg().MultiControlNetModel([cn for _, cn in pairs])
        out = multi(inp["sample"].to(dev).view(1, R.SMALL_FRAMES, 4, R.SMALL_LATENT, R.SMALL_LATENT), inp["timestep"].to(dev),
                    inp["ctx"].to(dev), [c.to(dev) for c in conds], list(scales))
    assert len(out.down_block_res_samples) == 12
    flat = [down + (mid,) for down, mid in wants]
    for i, g in enumerate(out.down_block_res_samples + (out.mid_block_res_sample,)):
        want = flat[0][i] + flat[1][i]
        tol = sum(REL_TOL_UNET * w[i].abs().max().item() for w in flat)
        assert g.dtype == torch.float32 and want.abs().max().item() > 1e-2
        compare(g, want, abs_tol=tol, name=f"MultiControlNet small, scales {scales}, tensor {i}")


# ---------------------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def parts(dev, small_nets):
    hu = hip_unet_from_oracle(oracle_small_unet(), dev)
    return hu, small_nets[0][0][1], small_nets[0][1][1]


def _problem(seed=31, frames=R.SMALL_FRAMES):
    g = torch.Generator().manual_seed(seed)
    kw = dict(prompt_embeds=h16(torch.randn(1, 7, 64, generator=g)), negative_prompt_embeds=h16(torch.randn(1, 7, 64, generator=g)),
              condition_image_latents=torch.randn(1, 4, 16, 16, generator=g), num_frames=frames, guidance_scale=7.5,
              output_type="latent", num_inference_steps=3)
    return kw, [torch.rand(frames, 3, 128, 128, generator=g), torch.rand(frames, 3, 128, 128, generator=g)]


def _gens():
    return dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


def _pipe(hu, nets, **kw):
    p = pkg()
    return p.I2VAdapterPipeline(unet=hu, controlnet=p.MultiControlNetModel(nets) if isinstance(nets, list) else nets, **kw)


def test_pipeline_one_net_in_a_multi_is_the_plain_net(dev, parts):
    hu, a, _ = parts
    kw, frames = _problem()
    single = _pipe(hu, a)(**kw, control_image=frames[0], controlnet_conditioning_scale=0.8, **_gens()).frames
    multi = _pipe(hu, [a])(**kw, control_image=[frames[0]], controlnet_conditioning_scale=0.8, **_gens()).frames
    listed = _pipe(hu, [a])(**kw, control_image=[frames[0]], controlnet_conditioning_scale=[0.8], use_graph=False, **_gens()).frames
    assert torch.equal(multi, single) and torch.equal(listed, single)


def test_pipeline_silent_nets_change_no_bit(dev, parts):
    hu, a, b = parts
    kw, frames = _problem()
    plain = pkg().I2VAdapterPipeline(unet=hu)(**kw, **_gens()).frames
    single = _pipe(hu, a)(**kw, control_image=frames[0], controlnet_conditioning_scale=0.8, **_gens()).frames
    pipe = _pipe(hu, [a, b])
    assert torch.equal(pipe(**kw, control_image=frames, controlnet_conditioning_scale=[0.8, 0.0], **_gens()).frames, single)
    assert torch.equal(pipe(**kw, control_image=frames, controlnet_conditioning_scale=0.0, **_gens()).frames, plain)
    both = pipe(**kw, control_image=frames, controlnet_conditioning_scale=[0.8, 0.8], **_gens()).frames
    assert len(pipe._graph_cache) == 1, "another scale table re-captured the step"
    assert not torch.equal(both, single) and (single - plain).abs().max().item() > 1e-2 and torch.equal(both[:, 0], plain[:, 0])


def test_pipeline_graph_equals_eager_and_replays_for_other_frames_scales_and_windows(dev, parts):
    hu, a, b = parts
    kw, frames = _problem()
    pipe = _pipe(hu, [a, b])
    windows = dict(control_guidance_start=[0.0, 0.5], control_guidance_end=[0.5, 1.0])
    graph = pipe(**kw, control_image=frames, **windows, **_gens()).frames
    eager = pipe(**kw, control_image=frames, **windows, use_graph=False, **_gens()).frames
    assert torch.equal(graph, eager)
    whole = pipe(**kw, control_image=frames, **_gens()).frames
    assert not torch.equal(whole, graph), "the windows do not reach the step"
    first = pipe._graph
    kw2, frames2 = _problem(seed=77)
    import PIL.Image
    pil = [PIL.Image.fromarray((f.permute(1, 2, 0).numpy() * 255).astype("uint8")) for f in frames2[0]]
    other = dict(control_image=[pil, frames2[1]], controlnet_conditioning_scale=[0.5, -0.75], control_guidance_start=[0.3, 0.0],
                 control_guidance_end=1.0)
    again = pipe(**kw2, **other, **_gens()).frames
    assert pipe._graph is first and len(pipe._graph_cache) == 1, "a second sample of the same shape re-captured the step"
    eager2 = pipe(**kw2, **other, use_graph=False, **_gens()).frames
    assert torch.equal(again, eager2) and not torch.equal(again, graph)
    swapped = pipe(**kw2, **dict(other, control_image=[frames2[1], pil]), **_gens()).frames
    assert not torch.equal(swapped, again), "the control frames do not reach the replayed graph"
    # with CFG off: one copy of the batch
    kw1 = dict(kw, guidance_scale=1.0)
    kw1.pop("negative_prompt_embeds")
    assert torch.equal(pipe(**kw1, control_image=frames, **windows, **_gens()).frames,
                       pipe(**kw1, control_image=frames, **windows, use_graph=False, **_gens()).frames)


@pytest.mark.parametrize("kind", ["dpmsolver++", "lcm", "euler_ancestral"])
def test_pipeline_other_schedulers_graph_equals_eager(dev, parts, kind):
    hu, a, b = parts
    p = pkg()
    sched = lambda: {"dpmsolver++": p.DPMSolverMultistepScheduler, "lcm": p.LCMScheduler,
                     "euler_ancestral": p.EulerAncestralDiscreteScheduler}[kind]()
    kw, frames = _problem()
    pipe = _pipe(hu, [a, b], scheduler=sched())
    args = dict(control_image=frames, controlnet_conditioning_scale=[1.0, -0.75], control_guidance_end=[1.0, 0.7])
    graph = pipe(**kw, **args, **_gens()).frames
    eager = pipe(**kw, **args, use_graph=False, **_gens()).frames
    plain = p.I2VAdapterPipeline(unet=hu, scheduler=sched())(**kw, **_gens()).frames
    assert torch.isfinite(graph).all() and torch.equal(graph, eager) and not torch.equal(graph, plain)


def test_pipeline_hires_fix(dev, parts):
    """the second pass prepares every net's frames again at the target size: with a silent second net it is the single net's call"""
    hu, a, b = parts
    kw, frames = _problem()
    single = _pipe(hu, a)
    single.enable_hires_fix(size=(192, 192), strength=0.5)
    want = single(**kw, control_image=frames[0], controlnet_conditioning_scale=0.8, **_gens()).frames
    pipe = _pipe(hu, [a, b])
    pipe.enable_hires_fix(size=(192, 192), strength=0.5)
    got = pipe(**kw, control_image=frames, controlnet_conditioning_scale=[0.8, 0.0], **_gens()).frames
    assert tuple(got.shape[-2:]) == (24, 24) and torch.equal(got, want)
    both = pipe(**kw, control_image=frames, controlnet_conditioning_scale=[0.8, 0.6], **_gens()).frames
    eager = pipe(**kw, control_image=frames, controlnet_conditioning_scale=[0.8, 0.6], use_graph=False, **_gens()).frames
    assert torch.equal(both, eager) and not torch.equal(both, want)


def test_pipeline_one_channel_net_beside_a_three_channel_net(dev, parts):
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    hu, a, _ = parts
    edges = init_random_weights_(pkg().ControlNetModel(**R.small_config(), conditioning_channels=1), seed=11).to(dev, f16).eval()
    kw, frames = _problem()
    pipe = _pipe(hu, [edges, a])
    images = [frames[1][:, :1], frames[0]]
    graph = pipe(**kw, control_image=images, **_gens()).frames
    eager = pipe(**kw, control_image=images, use_graph=False, **_gens()).frames
    assert torch.isfinite(graph).all() and torch.equal(graph, eager)
    single = _pipe(hu, a)(**kw, control_image=frames[0], **_gens()).frames
    assert torch.equal(pipe(**kw, control_image=images, controlnet_conditioning_scale=[0.0, 1.0], **_gens()).frames, single)
    assert not torch.equal(graph, single), "the 1-channel net contributes nothing"


# ---------------------------------------------------------------------------------------------------------- the driver
def test_eval_driver_with_two_controlnets(dev, tmp_path, monkeypatch):
    """`--controlnet A --control_column pose --controlnet B --control_column depth` on a two-row CSV, one scale per net"""
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
    init_random_weights_(p.ControlNetModel(**R.small_config()), seed=5).save_pretrained(os.path.join(root, "pose_net"))
    init_random_weights_(p.ControlNetModel(**R.small_config()), seed=6).save_pretrained(os.path.join(root, "depth_net"))
    rs = np.random.RandomState(0)
    img = lambda h, w: PIL.Image.fromarray((rs.rand(h, w, 3) * 255).astype("uint8"))
    os.makedirs(os.path.join(root, "data", "images"))
    for i in range(2):
        for col, (h, w) in (("pose", (48, 80)), ("depth", (64, 64))):
            os.makedirs(os.path.join(root, "data", f"{col}{i}"))
            for j in range(4):
                img(h, w).save(os.path.join(root, "data", f"{col}{i}", f"{j:03d}.png"))
    names = ["a cat on a boat", "two dogs, running"]
    with open(os.path.join(root, "data", "eval.csv"), "w") as f:
        f.write("image_path,name,pose,depth\n")
        for i, nm in enumerate(names):
            img(70, 90).save(os.path.join(root, "data", "images", f"{i}.png"))
            f.write(f'images/{i}.png,"{nm}",pose{i},depth{i}\n')
    g = torch.Generator().manual_seed(5)
    save_file({"prompt_embeds": torch.randn(2, 7, 64, generator=g), "negative_prompt_embeds": torch.randn(1, 7, 64, generator=g)},
              os.path.join(root, "embeds.safetensors"))
    seen = []
    call = I2VAdapterPipeline.__call__

    def spy(self, *a, **k):
        seen.append(([(len(c), c[0].size) for c in k["control_image"]], k["controlnet_conditioning_scale"], k["control_guidance_start"],
                     k["control_guidance_end"], type(self.controlnet).__name__, len(self.controlnet.nets)))
        return call(self, *a, **k)
    monkeypatch.setattr(I2VAdapterPipeline, "__call__", spy)
    common = ["--task_name", "demo", "--checkpoint_epoch", "3", "--eval_data_path", os.path.join(root, "data", "eval.csv"),
              "--embeds", os.path.join(root, "embeds.safetensors"), "--model_path", os.path.join(root, "sd"),
              "--motion_adapter_path", os.path.join(root, "motion"), "--checkpoint_root", os.path.join(root, "checkpoint"),
              "--samples_root", os.path.join(root, "samples"), "--num_frames", "4", "--num_inference_steps", "4"]
    two = ["--controlnet", os.path.join(root, "pose_net"), "--control_column", "pose", "--controlnet", os.path.join(root, "depth_net"),
           "--control_column", "depth"]
    assert main(common + two + ["--controlnet_scale", "0.8", "0.4", "--control_guidance_start", "0.25", "--control_guidance_end", "0.75",
                                "1.0"]) == 0
    row = ([(4, (80, 48)), (4, (64, 64))], [0.8, 0.4], 0.25, [0.75, 1.0], "MultiControlNetModel", 2)
    assert seen == [row, row]
    for nm in names:
        out = PIL.Image.open(os.path.join(root, "samples", "demo", "epoch_3", f"{nm}.gif"))
        assert out.n_frames == 4 and out.size == (64, 64)
    assert main(common + two[:6]) == -1                                             # two nets, one column
    assert main(common + two + ["--controlnet_scale", "1.0", "0.5", "0.25"]) == -1  # three scales for two nets
