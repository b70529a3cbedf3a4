"""LCMScheduler on the GPU: the `i2v_lcm_cfg_step` kernel against fp32 torch on the host (both forms, the noise row each step reads,
the last step's unread table), the kernel driven through a problem with a known model, the pipeline's trajectory on the reduced UNet
against the oracle loop with tests/lcm_reference.py as its scheduler, the routes that must agree bit for bit (graph / callback, eta, a
new seed on a cached graph, another step count, a scheduler swapped between calls) and an LCM step plan replayed through the model
handle's C entry point."""
import functools
import warnings

import pytest
import torch

from tests.lcm_reference import ReferenceLCMScheduler
from tests.parity import REL_TOL_TRAJECTORY, compare, hip_unet_from_oracle, oracle_small_unet, small_ip_state_dict

pytestmark = pytest.mark.gpu


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h(t):
    return t.half().float()


def _coef(N=4):
    s = pkg().LCMScheduler()
    s.set_timesteps(N)
    return s.step_coefficients(s.timesteps).contiguous()


def _host_step(x, z, np_tok, row, g, copies, c):
    """fp32 torch on the host: CFG combine, x0, boundary scalings, re-noise; latents [b, f, c, h, w], tokens [copies * b * f, h, w, ld]"""
    b, f, _, hh, ww = x.shape
    eps_tok = np_tok.float()[..., :c]
    if copies == 2:
        u, cn = eps_tok[: b * f], eps_tok[b * f:]
        eps_tok = u + g * (cn - u)
    eps = eps_tok.reshape(b, f, hh, ww, c).permute(0, 1, 4, 2, 3)
    sa_t, sb_t, c_skip, c_out, sa_p, sb_p = [float(v) for v in row]
    x0 = (x - sb_t * eps) / sa_t
    den = c_out * x0 + c_skip * x
    out = sa_p * den
    return out + sb_p * z if sb_p != 0.0 else out


def _run_kernel_case(dev, np_dtype, copies, hw, offset_view=False):
    K = pkg().kernels
    b, f, c, ld = 2, 3, 4, 8
    hh, ww = hw
    g = torch.Generator().manual_seed(3)
    coef = _coef(4)
    assert coef.shape == (4, 6) and coef[3, 4:].tolist() == [1.0, 0.0] and 14.0 < 1.0 / float(coef[0, 0]) < 15.5      # the t = 999 row
    x = torch.randn(b, f, c, hh, ww, generator=g)
    noise = torch.randn(3, b, f, c, hh, ww, generator=g)                     # three distinct rows
    if offset_view:
        flat = torch.zeros(noise.numel() + 1, device=dev)
        noise_d = flat[1:].view(noise.shape)
        noise_d.copy_(noise)
        assert noise_d.data_ptr() % 16 == 4 and noise_d.is_contiguous()
    else:
        noise_d = noise.to(dev)
        assert noise_d.data_ptr() % 16 == 0
    poison = torch.full_like(noise_d, float("nan"))
    lat = x.to(dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    coef_d = coef.to(dev)
    for k in [0, 1, 2, 3, 0]:
        np_tok = torch.randn(copies * b * f, hh, ww, ld, generator=g).to(np_dtype)
        x = _host_step(x, noise[k] if k < 3 else None, np_tok, coef[k], 1.5, copies, c)
        K.lcm_cfg_step(lat, poison if k == 3 else noise_d, np_tok.to(dev), coef_d, idx, 1.5, copies)     # the last row reads no noise
        torch.cuda.synchronize()
        assert torch.isfinite(lat).all(), k
        scale = x.abs().max().item()
        err = (lat.cpu() - x).abs().max().item()
        assert err <= 1e-5 * scale, (k, err, scale)
        assert int(idx.item()) == (k + 1) % 4
        x = lat.cpu().clone()            # each step is judged on its own: the next one starts from the device's latents
    return lat, np_tok, coef_d, idx, noise_d


@pytest.mark.parametrize("np_dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("hw", [(8, 8), (5, 7)])
def test_kernel_against_host(dev, np_dtype, copies, hw):
    """the rows of a real 4-step table (t = 999 first: 1 / sa_t = 14.7) in the order 0, 1, 2, 3, 0 -- the counter wraps --, each with
    its own noise row (a step that read another row misses the bound); the last step runs with a NaN-filled table; ld_np > c.
    hw = 5 x 7 takes the scalar form of the kernel."""
    K = pkg().kernels
    lat, np_tok, coef_d, idx, noise_d = _run_kernel_case(dev, np_dtype, copies, hw)
    with pytest.raises(ValueError):
        K.lcm_cfg_step(lat, noise_d, np_tok.to(dev), coef_d[:, :4].contiguous(), idx, 1.5, copies)
    with pytest.raises(ValueError):
        K.lcm_cfg_step(lat, noise_d[:, :, :2].contiguous(), np_tok.to(dev), coef_d, idx, 1.5, copies)
    with pytest.raises(ValueError):
        K.lcm_cfg_step(lat, noise_d[0], np_tok.to(dev), coef_d, idx, 1.5, copies)


def test_kernel_with_a_misaligned_noise_table(dev):
    """a noise table that starts 4 bytes into its buffer: hw = 64 would allow 16-byte accesses, the table's address does not"""
    _run_kernel_case(dev, torch.float16, 2, (8, 8), offset_view=True)


def test_single_step_schedule_takes_no_table(dev):
    K = pkg().kernels
    coef = _coef(1)
    assert coef.shape == (1, 6)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 2, 4, 8, 8, generator=g)
    tok = torch.randn(2, 8, 8, 4, generator=g)
    lat, idx = x.to(dev), torch.zeros(1, dtype=torch.int32, device=dev)
    K.lcm_cfg_step(lat, None, tok.to(dev), coef.to(dev), idx, 1.0, 1)
    want = _host_step(x, None, tok, coef[0], 1.0, 1, 4)
    assert (lat.cpu() - want).abs().max().item() <= 1e-5 * want.abs().max().item() and int(idx.item()) == 0


def test_gaussian_model_through_the_kernel(dev):
    """data ~ N(0, v) per element: eps(x, t) = s_t x / (a_t^2 v + s_t^2) exactly.  Six LCM steps of the kernel (the model evaluated on
    the device between them) equal the same rows and the same noise applied in float64 on the host to fp32 level."""
    K = pkg().kernels
    s = pkg().LCMScheduler()
    s.set_timesteps(6)
    coef = s.step_coefficients(s.timesteps)
    ac = s.alphas_cumprod.double()
    v = torch.tensor([0.25, 1.0, 4.0, 9.0], dtype=torch.float64).view(1, 1, 4, 1, 1)
    g = torch.Generator().manual_seed(5)
    xT = torch.randn(1, 2, 4, 16, 16, generator=g, dtype=torch.float64)
    noise = s.step_noise(s.timesteps, tuple(xT.shape), torch.Generator().manual_seed(6), "cpu")
    assert noise.shape[0] == 5
    lat = xT.float().to(dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    coef_d, v_d, noise_d = coef.to(dev), v.float().to(dev), noise.to(dev)
    x = xT.float().double()
    for k, t in enumerate(s.timesteps.tolist()):
        a, sg = float(ac[t]) ** 0.5, (1 - float(ac[t])) ** 0.5
        eps = sg * lat / (a * a * v_d + sg * sg)
        tok = eps.permute(0, 1, 3, 4, 2).reshape(2, 16, 16, 4).contiguous()
        K.lcm_cfg_step(lat, noise_d, tok, coef_d, idx, 1.0, 1)
        eps64 = sg * x / (a * a * v + sg * sg)
        r = [float(q) for q in coef[k]]
        x0 = (x - r[1] * eps64) / r[0]
        x = r[4] * (r[3] * x0 + r[2] * x) + (r[5] * noise[k].double() if k < 5 else 0.0)
    torch.cuda.synchronize()
    err = (lat.cpu().double() - x).abs().max().item()
    print(f"LCM gaussian model, 6 steps: max abs err {err:.3e} (max|x| {x.abs().max().item():.3e})")
    assert err <= 1e-5 * x.abs().max().item(), err


# ---------------------------------------------------------------------------------------------------------- the pipeline
def _problem(seed=31, samples=1, ip=False):
    g = torch.Generator().manual_seed(seed)
    pe, ne = h(torch.randn(samples, 7, 64, generator=g)), h(torch.randn(samples, 7, 64, generator=g))
    ie = h(torch.randn(samples, 48, generator=g)) if ip else None
    cond = torch.randn(samples, 4, 16, 16, generator=g)
    return pe, ne, ie, cond


def _gens(seed=5):
    return dict(generator=torch.Generator().manual_seed(seed), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


@pytest.fixture(scope="module")
def small(dev):
    ou = oracle_small_unet()
    return ou, hip_unet_from_oracle(ou, dev)


@pytest.fixture(scope="module")
def small_ip(dev):
    ou = oracle_small_unet(ip=True)
    return ou, hip_unet_from_oracle(ou, dev, ip_state_dict=small_ip_state_dict(ou))


_REFERENCES = {}


def _reference(key, make):
    """the oracle trajectory of a case, computed once and shared by its use_graph False / True runs"""
    if key not in _REFERENCES:
        _REFERENCES[key] = make()
    return _REFERENCES[key].clone()


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("N,ratio,guidance", [(4, 1.0, 1.0), (6, 0.9, 2.0)])
def test_pipeline_trajectory_against_the_oracle(dev, small, N, ratio, guidance, use_graph):
    """the oracle draws its noise inside the reference scheduler's `step`, the product reads its table: the same stream of `generator`, so
    only the UNet's fp16 error enters.  guidance 1.0 runs one copy; ratio 0.9 at N = 6 starts the loop at full-list index 1."""
    from oracle.pipeline_i2v_adapter import I2VAdapterPipeline as OP
    ou, hu = small
    pe, ne, _, cond = _problem()
    kw = dict(num_frames=4, num_inference_steps=N, guidance_scale=guidance, frame_similarity_sample_ratio=ratio)
    ref = _reference((N, ratio, guidance), lambda: OP(ou, scheduler=ReferenceLCMScheduler())(pe, ne, cond, **kw, **_gens()).frames)
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=pkg().LCMScheduler())
    got = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, use_graph=use_graph, **kw, **_gens()).frames
    steps = min(int(N * ratio), N)
    assert got.shape == (1, 4, 4, 16, 16)
    assert torch.equal(got[:, 0].cpu(), cond)
    err, scale = (got.float().cpu() - ref).abs().max().item(), ref.abs().max().item()
    print(f"LCM N={N} ratio={ratio} guidance={guidance} use_graph={use_graph}: max abs latent err {err:.3e} (max|ref| {scale:.3e}, "
          f"rel {err / scale:.3e}, gate {REL_TOL_TRAJECTORY:.1e})")
    compare(got, ref, rel=REL_TOL_TRAJECTORY, name=f"LCM trajectory ({steps} steps, guidance {guidance}, use_graph {use_graph})")


@pytest.mark.parametrize("use_graph", [False, True])
def test_pipeline_trajectory_two_samples_with_ip(dev, small_ip, use_graph):
    """two samples per call, one generator each (every sample's noise rows come from its own generator, as diffusers' randn_tensor
    draws them), with the IP-Adapter branch.  Both sides are handed `latents` (the prior overwrites them, pipe:656): the oracle's
    prepare_latents takes one generator only."""
    from oracle.pipeline_i2v_adapter import I2VAdapterPipeline as OP
    ou, hu = small_ip
    pe, ne, ie, cond = _problem(seed=41, samples=2, ip=True)
    gens = lambda: dict(_gens(), generator=[torch.Generator().manual_seed(51), torch.Generator().manual_seed(52)])
    kw = dict(num_frames=4, num_inference_steps=6, guidance_scale=2.0, frame_similarity_sample_ratio=0.9, image_embeds=ie,
              blur_sigma=0.8, latents=torch.zeros(2, 4, 4, 16, 16))
    ref = _reference("ip", lambda: OP(ou, scheduler=ReferenceLCMScheduler())(pe, ne, cond, **kw, **gens()).frames)
    got = pkg().I2VAdapterPipeline(unet=hu, scheduler=pkg().LCMScheduler())(
        prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, use_graph=use_graph, **kw, **gens()).frames
    assert got.shape == (2, 4, 4, 16, 16) and torch.equal(got[:, 0].cpu(), cond)
    err, scale = (got.float().cpu() - ref).abs().max().item(), ref.abs().max().item()
    print(f"LCM N=6 two samples + IP use_graph={use_graph}: max abs latent err {err:.3e} (max|ref| {scale:.3e}, rel {err / scale:.3e}, "
          f"gate {REL_TOL_TRAJECTORY:.1e})")
    compare(got, ref, rel=REL_TOL_TRAJECTORY, name=f"LCM trajectory, 2 samples per call + IP (5 steps, use_graph {use_graph})")
    assert (got[0] - got[1]).abs().max().item() > 0.1


def _call_kw(seed=7, N=6):
    pe, ne, _, cond = _problem(seed=seed)
    return dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=4, num_inference_steps=N,
                guidance_scale=2.0, frame_similarity_sample_ratio=0.9)


def test_every_route_gives_the_same_result(dev, small):
    """graph route == callback (eager) route bit for bit, on the same noise table; eta is ignored (no host noise, no warning, still
    captured, one cached graph)"""
    _, hu = small
    kw = _call_kw()
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=pkg().LCMScheduler())
    graph = pipe(**kw, **_gens()).frames
    seen = []
    eager = pipe(**kw, callback=lambda i, t, lat: seen.append(i), **_gens()).frames
    assert seen == list(range(5)) and torch.equal(graph, eager)           # int(6 * 0.9) steps (pipe:529-536)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        noisy = pipe(**kw, eta=0.5, **_gens()).frames
    assert torch.equal(noisy, graph) and len(pipe._graph_cache) == 1


def test_a_new_seed_on_the_cached_graph_gets_its_own_noise(dev, small):
    """the stale-noise-table case: a graph-cache hit must copy this call's table into the graph's static buffer"""
    _, hu = small
    kw = _call_kw(seed=8)
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=pkg().LCMScheduler())
    first = pipe(**kw, **_gens(5)).frames
    captured = pipe._graph
    second = pipe(**kw, **_gens(77)).frames
    assert pipe._graph is captured and len(pipe._graph_cache) == 1        # a hit: replayed, not re-captured
    assert (second - first).abs().max().item() > 1e-2
    eager = pipe(**kw, use_graph=False, **_gens(77)).frames
    assert torch.equal(second, eager)
    assert torch.equal(pipe(**kw, **_gens(5)).frames, first)


def test_another_step_count_recaptures(dev, small):
    _, hu = small
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=pkg().LCMScheduler())
    four = pipe(**_call_kw(seed=9, N=4), **_gens()).frames
    captured, key = pipe._graph, next(iter(pipe._graph_cache))
    six = pipe(**_call_kw(seed=9, N=6), **_gens()).frames
    assert pipe._graph is not captured and len(pipe._graph_cache) == 1 and next(iter(pipe._graph_cache)) != key
    assert torch.equal(six, pipe(**_call_kw(seed=9, N=6), use_graph=False, **_gens()).frames)
    assert torch.equal(four, pipe(**_call_kw(seed=9, N=4), **_gens()).frames)


def test_scheduler_swap_recaptures(dev, small):
    """one pipeline, DDIM -> LCM -> DDIM on the graph route: each swap re-captures; the two DDIM results are equal bit for bit"""
    p = pkg()
    _, hu = small
    kw = _call_kw(seed=10, N=6)
    pipe = p.I2VAdapterPipeline(unet=hu)
    first = pipe(**kw, **_gens()).frames
    pipe.scheduler = p.LCMScheduler.from_config(pipe.scheduler.config)
    lcm = pipe(**kw, **_gens()).frames
    pipe.scheduler = p.DDIMScheduler.from_config(pipe.scheduler.config)
    third = pipe(**kw, **_gens()).frames
    assert torch.equal(first, third)
    assert (lcm - first).abs().max().item() > 1e-3 and torch.equal(lcm[:, 0], first[:, 0])


# ---------------------------------------------------------------------------------------------------------- the model handle
def test_lcm_step_plan_through_the_c_abi(dev, monkeypatch):
    """`record_step_plan` of an LCM state carries the noise table as io slot STEP_NOISE (= 4); the plan replayed through ONE
    `i2v_unet_run` per step (captured), after `record_prepare_plan` refilled the scrambled per-sample buffers, equals the Python `_step`
    loop bit for bit over two consecutive steps (each reads its own row of the table)."""
    p = pkg()
    H = p.handle
    ou = oracle_small_unet(ip=True)
    hu = hip_unet_from_oracle(ou, dev, ip_state_dict=small_ip_state_dict(ou))
    pipe = p.I2VAdapterPipeline(unet=hu, scheduler=p.LCMScheduler())
    sch = pipe.scheduler
    sch.set_timesteps(4)
    ts = sch.timesteps
    g = torch.Generator().manual_seed(51)
    B, F, hh = 1, 4, 16
    ie = torch.randn(2 * B, 48, generator=g).half().to(dev)
    st = dict(latents=torch.randn(B, F, 4, hh, hh, generator=g).to(dev), cond=torch.randn(B, 4, hh, hh, generator=g).to(dev),
              copies=2, num_frames=F, guidance=2.0, t_table=ts.float().to(dev), coef=sch.step_coefficients(ts).to(dev),
              step_idx=torch.zeros(1, dtype=torch.int32, device=dev),
              ctx_text=torch.randn(2 * B, 7, 64, generator=g).half().to(dev),
              ctx_ip=hu._project_image_embeds({"image_embeds": ie}))
    st["noise"] = sch.step_noise(ts, (B, F, 4, hh, hh), torch.Generator().manual_seed(52), dev)
    assert st["noise"].shape == (3, B, F, 4, hh, hh)
    with torch.no_grad():
        st["ctx_proj"] = hu.project_context(st["ctx_text"], st["ctx_ip"])
        st["temb_table"] = hu.project_time_table(st["t_table"])
        step_blob, w_step = H.record_step_plan(pipe, st)
        prep_blob, w_prep = H.record_prepare_plan(pipe, st, image_embeds=ie)
    weights = {**w_step, **w_prep}
    problem = H._step_problem(st)
    handles = []
    for blob in (prep_blob, step_blob):
        hd = p.UNetHandle(hu, ip_num_tokens=4)
        hd.plan(*problem[:4], ctx_len=problem[4], has_ip=bool(problem[5]))
        hd.set_plan(blob)
        hd.set_weights(weights)
        handles.append(hd)
    hp, hs = handles
    arena = torch.empty(max(hp.activation_bytes, hs.activation_bytes), dtype=torch.uint8, device=dev)
    hp.set_workspace(arena)
    hs.set_workspace(arena)
    latents0 = torch.randn(st["latents"].shape, generator=g).to(dev)
    n_steps = 2
    with torch.no_grad():                              # the Python loop
        st["latents"].copy_(latents0)
        st["step_idx"].zero_()
        hu.project_context(st["ctx_text"], hu._project_image_embeds({"image_embeds": ie}), out=st["ctx_proj"])
        hu.project_time_table(st["t_table"], out=st["temb_table"])
        for _ in range(n_steps):
            pipe._step(st)
        torch.cuda.synchronize()
    ref = st["latents"].clone()
    assert torch.isfinite(ref).all()
    for t in H.sample_buffers(hu, st).values():
        t.fill_(float("nan"))
    st["latents"].copy_(latents0)
    st["step_idx"].zero_()
    K = p.kernels

    def boom(*a, **k):
        raise AssertionError("a kernels.py wrapper ran during i2v_unet_run")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with monkeypatch.context() as m:
        for name in ("gemm", "attention", "groupnorm", "ddim_prep", "lcm_cfg_step", "dpm_cfg_step", "ddim_cfg_step", "timestep_embedding"):
            m.setattr(K, name, boom)
        with torch.cuda.stream(s):
            hp.run({H.PREP_CONTEXT: st["ctx_text"], H.PREP_TIMESTEPS: st["t_table"], H.PREP_IMAGE_EMBEDS: ie}, stream=s)
        io = {H.STEP_LATENTS: st["latents"], H.STEP_COND: st["cond"], H.STEP_INDEX: st["step_idx"], H.STEP_COEF: st["coef"],
              H.STEP_NOISE: st["noise"]}
        hs.capture(s, lambda: hs.run(io, stream=s))
        for _ in range(n_steps):
            hs.replay(s)
        s.synchronize()
    assert torch.equal(st["latents"], ref), f"max |d| {(st['latents'] - ref).abs().max().item():.3e}"
    assert int(st["step_idx"].item()) == n_steps
    for hd in handles:
        hd.close()
