"""DPM-Solver++(2M) on the GPU: the `i2v_dpm_cfg_step` kernel against fp32 torch on the host, the kernel driven through a
problem with a known answer, the pipeline's trajectory on the reduced UNet against the oracle loop with tests/dpm_reference.py as
its scheduler, the routes that must agree bit for bit (graph / callback, eta, a scheduler swapped between calls) and a DPM
step plan replayed through the model handle's C entry point."""
import warnings

import pytest
import torch

from tests.dpm_reference import ReferenceDPMSolver
from tests.parity import REL_TOL_TRAJECTORY, compare, hip_unet_from_oracle, oracle_small_unet, small_ip_state_dict

pytestmark = pytest.mark.gpu


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h(t):
    return t.half().float()


def _coef(N=20, rows=3):
    """the first rows of a real table: order 1, then order 2"""
    s = pkg().DPMSolverMultistepScheduler()
    s.set_timesteps(N)
    return s.step_coefficients(s.timesteps)[:rows].contiguous()


def _host_step(x, x0_prev, np_tok, row, g, copies, c):
    """fp32 torch on the host: CFG combine, x0, update; latents [b, f, c, h, w], tokens [copies * b * f, h, w, ld]"""
    b, f, _, hh, ww = x.shape
    eps_tok = np_tok.float()[..., :c]
    if copies == 2:
        u, cn = eps_tok[: b * f], eps_tok[b * f:]
        eps_tok = u + g * (cn - u)
    eps = eps_tok.reshape(b, f, hh, ww, c).permute(0, 1, 4, 2, 3)
    a_s0, s_s0, ratio, c_cur, c_prev, order = [float(v) for v in row]
    x0 = (x - s_s0 * eps) / a_s0
    out = ratio * x + c_cur * x0
    if order > 1.5:
        out = out + c_prev * x0_prev
    return out, x0


@pytest.mark.parametrize("np_dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("hw", [(8, 8), (5, 7)])
def test_kernel_against_host(dev, np_dtype, copies, hw):
    """order-1 row with a NaN-filled x0_prev (it must not be read), then order-2 rows; ld_np > c; the step counter advances and
    wraps to 0 after the table (the next step reads row 0 again).  hw = 5 x 7 takes the scalar form of the kernel."""
    K = pkg().kernels
    b, f, c, ld = 2, 3, 4, 8
    hh, ww = hw
    g = torch.Generator().manual_seed(3)
    coef = _coef(rows=3)
    assert coef[:, 5].tolist() == [1, 2, 2]
    x = torch.randn(b, f, c, hh, ww, generator=g)
    x0p = torch.full_like(x, float("nan"))
    lat, hist = x.to(dev), x0p.to(dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    coef_d = coef.to(dev)
    for k in [0, 1, 2, 0]:
        np_tok = torch.randn(copies * b * f, hh, ww, ld, generator=g).to(np_dtype)
        x, x0p = _host_step(x, x0p, np_tok, coef[k], 7.5, copies, c)
        K.dpm_cfg_step(lat, hist, np_tok.to(dev), coef_d, idx, 7.5, copies)
        torch.cuda.synchronize()
        assert torch.isfinite(lat).all() and torch.isfinite(hist).all(), k
        scale = x.abs().max().item()
        assert (lat.cpu() - x).abs().max().item() <= 1e-5 * scale, k
        assert (hist.cpu() - x0p).abs().max().item() <= 1e-5 * x0p.abs().max().item(), k
        assert int(idx.item()) == (k + 1) % 3
    with pytest.raises(ValueError):
        K.dpm_cfg_step(lat, hist, np_tok.to(dev), coef_d[:, :4].contiguous(), idx, 7.5, copies)


def test_gaussian_ode_through_the_kernel(dev):
    """data ~ N(0, v) per element: eps(x, t) = s_t x / (a_t^2 v + s_t^2) exactly.  20 steps of the kernel (the model evaluated
    on the device between them) equal the same table applied in float64 on the host to fp32 level, and land close to the exact
    solution of the probability-flow ODE."""
    K = pkg().kernels
    s = pkg().DPMSolverMultistepScheduler()
    s.set_timesteps(20)
    coef = s.step_coefficients(s.timesteps)
    ac = s.alphas_cumprod.double()
    v = torch.tensor([0.25, 1.0, 4.0, 9.0], dtype=torch.float64).view(1, 1, 4, 1, 1)
    g = torch.Generator().manual_seed(5)
    xT = torch.randn(1, 2, 4, 16, 16, generator=g, dtype=torch.float64)
    lat, hist = xT.float().to(dev), torch.full(xT.shape, float("nan"), device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    coef_d, v_d = coef.to(dev), v.float().to(dev)
    x, x0p = xT.clone(), None
    for k, t in enumerate(s.timesteps.tolist()):
        a, sg = float(ac[t]) ** 0.5, (1 - float(ac[t])) ** 0.5
        eps = sg * lat / (a * a * v_d + sg * sg)
        tok = eps.permute(0, 1, 3, 4, 2).reshape(2, 16, 16, 4).contiguous()
        K.dpm_cfg_step(lat, hist, tok, coef_d, idx, 1.0, 1)
        eps64 = sg * x / (a * a * v + sg * sg)
        r = [float(q) for q in coef[k]]
        x0 = (x - r[1] * eps64) / r[0]
        x = r[2] * x + r[3] * x0 + (r[4] * x0p if r[5] > 1.5 else 0.0)
        x0p = x0
    torch.cuda.synchronize()
    err = (lat.cpu().double() - x).abs().max().item()
    assert err <= 1e-5 * x.abs().max().item(), err
    (aT, sT), (a0, s0) = (float(ac[999]) ** 0.5, (1 - float(ac[999])) ** 0.5), (float(ac[0]) ** 0.5, (1 - float(ac[0])) ** 0.5)
    exact = xT * torch.sqrt(a0 * a0 * v + s0 * s0) / torch.sqrt(aT * aT * v + sT * sT)
    assert (x - exact).abs().max().item() <= 0.05 * exact.abs().max().item()      # (2.4e-2 at N = 20)


# ---------------------------------------------------------------------------------------------------------- the pipeline
def _problem(seed=31, samples=1, ip=False):
    g = torch.Generator().manual_seed(seed)
    pe, ne = h(torch.randn(samples, 7, 64, generator=g)), h(torch.randn(samples, 7, 64, generator=g))
    ie = h(torch.randn(samples, 48, generator=g)) if ip else None
    cond = torch.randn(samples, 4, 16, 16, generator=g)
    return pe, ne, ie, cond


def _gens():
    return dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


@pytest.fixture(scope="module")
def small(dev):
    ou = oracle_small_unet()
    return ou, hip_unet_from_oracle(ou, dev)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("N", [10, 16])
def test_pipeline_trajectory_against_the_oracle(dev, small, N, use_graph):
    """ratio 0.9: the loop starts at full-list index 1 (first order); N = 10 ends with a first-order step (lower_order_final),
    N = 16 with a second-order one"""
    from oracle.pipeline_i2v_adapter import I2VAdapterPipeline as OP
    ou, hu = small
    pe, ne, _, cond = _problem()
    kw = dict(num_frames=4, num_inference_steps=N, guidance_scale=7.5, frame_similarity_sample_ratio=0.9)
    ref = OP(ou, scheduler=ReferenceDPMSolver())(pe, ne, cond, **kw, **_gens()).frames
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=pkg().DPMSolverMultistepScheduler())
    got = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, use_graph=use_graph, **kw, **_gens()).frames
    assert got.shape == (1, 4, 4, 16, 16)
    assert torch.equal(got[:, 0].cpu(), cond)
    orders = pipe.scheduler.step_orders(pipe.scheduler.timesteps[1:])
    assert orders[0] == 1 and orders[-1] == (1 if N == 10 else 2)
    err, scale = compare(got, ref, rel=REL_TOL_TRAJECTORY, name=f"DPM-Solver++ trajectory ({N - 1} steps)")
    print(f"DPM N={N} use_graph={use_graph}: max abs latent err {err:.3e} (max|ref| {scale:.3e})")


def test_pipeline_trajectory_two_samples_with_ip(dev):
    from oracle.pipeline_i2v_adapter import I2VAdapterPipeline as OP
    ou = oracle_small_unet(ip=True)
    hu = hip_unet_from_oracle(ou, dev, ip_state_dict=small_ip_state_dict(ou))
    pe, ne, ie, cond = _problem(seed=41, samples=2, ip=True)
    kw = dict(num_frames=4, num_inference_steps=16, guidance_scale=7.5, frame_similarity_sample_ratio=0.9, image_embeds=ie,
              blur_sigma=0.8)
    ref = OP(ou, scheduler=ReferenceDPMSolver())(pe, ne, cond, **kw, **_gens()).frames
    got = pkg().I2VAdapterPipeline(unet=hu, scheduler=pkg().DPMSolverMultistepScheduler())(
        prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, **kw, **_gens()).frames
    assert got.shape == (2, 4, 4, 16, 16) and torch.equal(got[:, 0].cpu(), cond)
    compare(got, ref, rel=REL_TOL_TRAJECTORY, name="DPM-Solver++ trajectory, 2 samples per call + IP (15 steps)")
    assert (got[0] - got[1]).abs().max().item() > 0.1


def test_every_route_gives_the_same_result(dev, small):
    """graph route == callback (eager) route bit for bit; eta is ignored (no host noise, no warning, still captured)"""
    _, hu = small
    pe, ne, _, cond = _problem(seed=7)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=4, num_inference_steps=12,
              guidance_scale=7.5, frame_similarity_sample_ratio=0.9)
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=pkg().DPMSolverMultistepScheduler())
    graph = pipe(**kw, **_gens()).frames
    seen = []
    eager = pipe(**kw, callback=lambda i, t, lat: seen.append(i), **_gens()).frames
    assert seen == list(range(10)) and torch.equal(graph, eager)        # int(12 * 0.9) steps (pipe:529-536)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        noisy = pipe(**kw, eta=0.5, **_gens()).frames
    assert torch.equal(noisy, graph) and len(pipe._graph_cache) == 1
    again = pipe(**kw, **_gens()).frames          # a graph-cache hit: x0_prev is not reset and must not matter
    assert torch.equal(again, graph)


def test_scheduler_swap_recaptures(dev, small):
    """one pipeline, DDIM -> DPM -> DDIM on the graph route: each swap re-captures; the two DDIM results are equal bit for bit"""
    p = pkg()
    _, hu = small
    pe, ne, _, cond = _problem(seed=9)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=4, num_inference_steps=10,
              guidance_scale=7.5, frame_similarity_sample_ratio=0.9)
    pipe = p.I2VAdapterPipeline(unet=hu)
    first = pipe(**kw, **_gens()).frames
    pipe.scheduler = p.DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    dpm = pipe(**kw, **_gens()).frames
    pipe.scheduler = p.DDIMScheduler.from_config(pipe.scheduler.config)
    third = pipe(**kw, **_gens()).frames
    assert torch.equal(first, third)
    assert (dpm - first).abs().max().item() > 1e-3 and torch.equal(dpm[:, 0], first[:, 0])


# ---------------------------------------------------------------------------------------------------------- the model handle
def test_dpm_step_plan_through_the_c_abi(dev, monkeypatch):
    """`record_step_plan` of a DPM state carries x0_prev as io slot STEP_HISTORY; the plan replayed through ONE `i2v_unet_run` per
    step (captured), after `record_prepare_plan` refilled the scrambled per-sample buffers, equals the Python `_step` loop bit for
    bit -- starting from a NaN-filled x0_prev, which the first (first-order) step must not read."""
    p = pkg()
    H = p.handle
    ou = oracle_small_unet(ip=True)
    hu = hip_unet_from_oracle(ou, dev, ip_state_dict=small_ip_state_dict(ou))
    pipe = p.I2VAdapterPipeline(unet=hu, scheduler=p.DPMSolverMultistepScheduler())
    sch = pipe.scheduler
    sch.set_timesteps(10)
    ts = sch.timesteps
    g = torch.Generator().manual_seed(51)
    B, F, hh = 1, 4, 16
    ie = torch.randn(2 * B, 48, generator=g).half().to(dev)
    st = dict(latents=torch.randn(B, F, 4, hh, hh, generator=g).to(dev), cond=torch.randn(B, 4, hh, hh, generator=g).to(dev),
              copies=2, num_frames=F, guidance=7.5, t_table=ts.float().to(dev), coef=sch.step_coefficients(ts).to(dev),
              step_idx=torch.zeros(1, dtype=torch.int32, device=dev),
              ctx_text=torch.randn(2 * B, 7, 64, generator=g).half().to(dev),
              ctx_ip=hu._project_image_embeds({"image_embeds": ie}))
    st["x0_prev"] = torch.zeros_like(st["latents"])
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
    n_steps = 4                                        # rows of order 1, 2, 2, 2
    with torch.no_grad():                              # the Python loop
        st["latents"].copy_(latents0)
        st["step_idx"].zero_()
        st["x0_prev"].fill_(float("nan"))
        hu.project_context(st["ctx_text"], hu._project_image_embeds({"image_embeds": ie}), out=st["ctx_proj"])
        hu.project_time_table(st["t_table"], out=st["temb_table"])
        for _ in range(n_steps):
            pipe._step(st)
        torch.cuda.synchronize()
    ref, ref_hist = st["latents"].clone(), st["x0_prev"].clone()
    assert torch.isfinite(ref).all()
    for t in H.sample_buffers(hu, st).values():
        t.fill_(float("nan"))
    st["latents"].copy_(latents0)
    st["step_idx"].zero_()
    st["x0_prev"].fill_(float("nan"))
    K = p.kernels

    def boom(*a, **k):
        raise AssertionError("a kernels.py wrapper ran during i2v_unet_run")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with monkeypatch.context() as m:
        for name in ("gemm", "attention", "groupnorm", "ddim_prep", "dpm_cfg_step", "ddim_cfg_step", "timestep_embedding"):
            m.setattr(K, name, boom)
        with torch.cuda.stream(s):
            hp.run({H.PREP_CONTEXT: st["ctx_text"], H.PREP_TIMESTEPS: st["t_table"], H.PREP_IMAGE_EMBEDS: ie}, stream=s)
        io = {H.STEP_LATENTS: st["latents"], H.STEP_COND: st["cond"], H.STEP_INDEX: st["step_idx"], H.STEP_COEF: st["coef"],
              H.STEP_HISTORY: st["x0_prev"]}
        hs.capture(s, lambda: hs.run(io, stream=s))
        for _ in range(n_steps):
            hs.replay(s)
        s.synchronize()
    assert torch.equal(st["latents"], ref), f"max |d| {(st['latents'] - ref).abs().max().item():.3e}"
    assert torch.equal(st["x0_prev"], ref_hist) and int(st["step_idx"].item()) == n_steps
    for hd in handles:
        hd.close()
