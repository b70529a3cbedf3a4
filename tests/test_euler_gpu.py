"""EulerDiscreteScheduler and EulerAncestralDiscreteScheduler on the GPU: `i2v_euler_cfg_step` against fp32 torch on the host (both
forms, the noise row each step reads, the rows that read none), `i2v_sigma_prep` bit for bit against the host's scaling and against
`i2v_ddim_prep`, both kernels driven through a problem with a known model, the pipeline's trajectories on the reduced UNet against the
oracle loop with tests/euler_reference.py as its scheduler, the routes that must agree bit for bit (graph / callback, a new seed on a
cached graph, another step count, a scheduler swapped between calls), the places where a clean clip is noised to a timestep's level
in sigma space (the prior, video-to-video, the mask's blend, FreeInit) and the C handle's refusal."""
import warnings

import pytest
import torch

from tests import freeinit_reference as FR
from tests.euler_reference import ReferenceEulerScheduler
from tests.parity import REL_TOL_TRAJECTORY, compare, hip_unet_from_oracle, oracle_small_unet, small_ip_state_dict

pytestmark = pytest.mark.gpu

SD15 = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h(t):
    return t.half().float()


def bits(t):
    return t.contiguous().view(torch.int32)


def _sched(ancestral=False, **kw):
    p = pkg()
    return (p.EulerAncestralDiscreteScheduler if ancestral else p.EulerDiscreteScheduler)(**SD15, **kw)


def _ref_sched(ancestral=False, **kw):
    return ReferenceEulerScheduler(ancestral=ancestral, **SD15, **kw)


def _coef(ancestral, N=4):
    s = _sched(ancestral)
    s.set_timesteps(N)
    return s.step_coefficients(s.timesteps).contiguous()


# ---------------------------------------------------------------------------------------------------------- the step kernel
def _host_step(x, z, np_tok, row, g, copies, c):
    """fp32 torch on the host: CFG combine, then x + eps (sigma_to - sigma) + sigma_up z; latents [b, f, c, h, w], tokens
    [copies * b * f, h, w, ld]"""
    b, f, _, hh, ww = x.shape
    eps_tok = np_tok.float()[..., :c]
    if copies == 2:
        u, cn = eps_tok[: b * f], eps_tok[b * f:]
        eps_tok = u + g * (cn - u)
    eps = eps_tok.reshape(b, f, hh, ww, c).permute(0, 1, 4, 2, 3)
    sigma_up = float(row[3])
    out = x + eps * float(row[2] - row[0])                   # the difference taken in fp32, as the kernel takes it
    return out + sigma_up * z if sigma_up != 0.0 else out


def _run_kernel_case(dev, ancestral, np_dtype, copies, hw, offset_view=False):
    K = pkg().kernels
    b, f, c, ld = 2, 3, 4, 8
    hh, ww = hw
    g = torch.Generator().manual_seed(3)
    coef = _coef(ancestral, 4)
    assert coef.shape == (4, 4) and 14.0 < float(coef[0, 0]) < 15.5                                 # the t = 999 row
    assert coef[3, 2:].tolist() == [0.0, 0.0] and bool((coef[:3, 3] > 0).all()) == ancestral
    x = torch.randn(b, f, c, hh, ww, generator=g) * 10
    noise = torch.randn(4, b, f, c, hh, ww, generator=g)                     # four distinct rows
    if not ancestral:
        noise_d = poison = None                                              # Euler: no table at all
    elif offset_view:
        flat = torch.zeros(noise.numel() + 1, device=dev)
        noise_d = flat[1:].view(noise.shape)
        noise_d.copy_(noise)
        assert noise_d.data_ptr() % 16 == 4 and noise_d.is_contiguous()
    else:
        noise_d = noise.to(dev)
        assert noise_d.data_ptr() % 16 == 0
    if ancestral:
        poison = torch.full_like(noise_d, float("nan"))
    lat = x.to(dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    coef_d = coef.to(dev)
    for k in [0, 1, 2, 3, 0]:
        np_tok = torch.randn(copies * b * f, hh, ww, ld, generator=g).to(np_dtype)
        x = _host_step(x, noise[k], np_tok, coef[k], 1.5, copies, c)
        K.euler_cfg_step(lat, poison if k == 3 else noise_d, np_tok.to(dev), coef_d, idx, 1.5, copies)   # the last row reads no noise
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
@pytest.mark.parametrize("ancestral", [False, True], ids=["euler", "ancestral"])
def test_kernel_against_host(dev, ancestral, np_dtype, copies, hw):
    """the rows of a real 4-step table (t = 999 first: sigma = 14.6) in the order 0, 1, 2, 3, 0 -- the counter wraps --, each with its own
    noise row (a step that read another row misses the bound); the last step runs with a NaN-filled table, Euler with no table; ld_np > c.
    hw = 5 x 7 takes the scalar form of the kernel.  Bound: 1e-5 max|ref| per step, the project's bound for this class of kernel (about
    ten times the worst case of the half-dozen fp32 roundings involved)."""
    K = pkg().kernels
    lat, np_tok, coef_d, idx, noise_d = _run_kernel_case(dev, ancestral, np_dtype, copies, hw)
    tok = np_tok.to(dev)
    with pytest.raises(ValueError):
        K.euler_cfg_step(lat, noise_d, tok, coef_d[:, :3].contiguous(), idx, 1.5, copies)                  # coefficient width
    with pytest.raises(ValueError):
        K.euler_cfg_step(lat, noise_d, tok, torch.zeros(4, 6, device=dev), idx, 1.5, copies)
    if ancestral:
        with pytest.raises(ValueError):
            K.euler_cfg_step(lat, noise_d[:3].contiguous(), tok, coef_d, idx, 1.5, copies)                 # too few rows
        with pytest.raises(ValueError):
            K.euler_cfg_step(lat, noise_d[:, :, :2].contiguous(), tok, coef_d, idx, 1.5, copies)
        with pytest.raises(ValueError):
            K.euler_cfg_step(lat, noise_d[0], tok, coef_d, idx, 1.5, copies)
        with pytest.raises(ValueError, match="sigma_up"):
            K.euler_cfg_step(lat, None, tok, coef_d, idx, 1.5, copies)                                     # an ancestral table, no noise
    assert int(idx.item()) == 1                                                                            # no refused call launched


def test_kernel_with_a_misaligned_noise_table(dev):
    """a noise table that starts 4 bytes into its buffer: hw = 64 would allow 16-byte accesses, the table's address does not"""
    _run_kernel_case(dev, True, torch.float16, 2, (8, 8), offset_view=True)


# ---------------------------------------------------------------------------------------------------------- the prep kernel
@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("hw,c_pad", [((8, 8), 8), ((5, 7), 8), ((5, 7), 4)])
def test_sigma_prep(dev, hw, c_pad, copies):
    """model_in = fp16(v * row[1]) bit for bit, both copies, zero padding channels; latents[:, 0] = cond unscaled; the counter is read
    (clamped to the table) and left as it is; with a scale column of exactly 1.0 the output is `ddim_prep`'s bit for bit"""
    K = pkg().kernels
    b, f, c = 2, 3, 4
    hh, ww = hw
    g = torch.Generator().manual_seed(8)
    coef = _coef(True, 4)
    coef_d = coef.to(dev)
    x = torch.randn(b, f, c, hh, ww, generator=g) * 10
    cond = torch.randn(b, c, hh, ww, generator=g)
    want_lat = x.clone()
    want_lat[:, 0] = cond
    tokens = want_lat.permute(0, 1, 3, 4, 2).reshape(b * f, hh, ww, c)
    for counter, row in ((0, 0), (1, 1), (2, 2), (3, 3), (9, 3), (-1, 0)):
        lat, idx = x.to(dev), torch.full((1,), counter, dtype=torch.int32, device=dev)
        out = K.sigma_prep(lat, cond.to(dev), coef_d, idx, c_pad, copies)
        torch.cuda.synchronize()
        assert out.shape == (copies * b * f, hh, ww, c_pad) and out.dtype == torch.float16
        want = (tokens.float() * coef[row, 1]).half()
        for k in range(copies):
            part = out[k * b * f: (k + 1) * b * f].cpu()
            assert torch.equal(part[..., :c].view(torch.int16), want.view(torch.int16)), (counter, k)
            assert bool((part[..., c:] == 0).all()), (counter, k)
        assert torch.equal(bits(lat.cpu()), bits(want_lat)), counter                    # frame 0 is the bare condition, the rest untouched
        assert int(idx.item()) == counter
    ones = coef.clone()
    ones[:, 1] = 1.0
    lat_a, lat_b = x.to(dev), x.to(dev)
    idx = torch.full((1,), 2, dtype=torch.int32, device=dev)
    got = K.sigma_prep(lat_a, cond.to(dev), ones.to(dev), idx, c_pad, copies)
    ref = K.ddim_prep(lat_b, cond.to(dev), c_pad, copies)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)) and torch.equal(lat_a, lat_b)
    # a two-column table (the scale is column 1 of whatever row width) reads the same scale
    got2 = K.sigma_prep(x.to(dev), cond.to(dev), coef_d[:, :2].contiguous(), idx, c_pad, copies)
    assert torch.equal(got2, K.sigma_prep(x.to(dev), cond.to(dev), coef_d, idx, c_pad, copies))
    with pytest.raises(ValueError):
        K.sigma_prep(x.to(dev), cond.to(dev), coef_d[:, :1].contiguous(), idx, c_pad, copies)
    with pytest.raises(ValueError):
        K.sigma_prep(x.to(dev), cond[:1].to(dev), coef_d, idx, c_pad, copies)


# ---------------------------------------------------------------------------------------------------------- a known model
@pytest.mark.parametrize("ancestral", [False, True], ids=["euler", "ancestral"])
def test_gaussian_model_through_both_kernels(dev, ancestral):
    """data ~ N(0, v) per element: eps(x, sigma) = sigma x / (v + sigma^2) exactly, evaluated on the device from the SCALED fp16 input the
    prep kernel wrote (x = model_in sqrt(sigma^2 + 1)).  Six steps through both kernels equal, for Euler, the float64 product
    x_T prod(1 + sigma (sigma_to - sigma) / (v + sigma^2)) and, for the ancestral sampler, the float64 linear recursion with the table's
    z.  Bound 1e-3 max|ref|: the model input is fp16 -- six steps of 2^-11 relative input error, each entering through eps with gain
    sigma (sigma - sigma_to) / (v + sigma^2) < 1."""
    K = pkg().kernels
    s = _sched(ancestral)
    s.set_timesteps(6)
    coef = s.step_coefficients(s.timesteps)
    v = torch.tensor([0.25, 1.0, 4.0, 9.0], dtype=torch.float64).view(1, 1, 4, 1, 1)
    g = torch.Generator().manual_seed(5)
    sig0 = float(coef[0, 0])
    xT = (torch.randn(1, 2, 4, 16, 16, generator=g, dtype=torch.float64) * (v + sig0 ** 2).sqrt()).float()
    noise = s.step_noise(s.timesteps, tuple(xT.shape), torch.Generator().manual_seed(6), "cpu") if ancestral else None
    lat, idx = xT.to(dev), torch.zeros(1, dtype=torch.int32, device=dev)
    cond = torch.empty(1, 4, 16, 16, device=dev)
    coef_d, v_tok = coef.to(dev), v.float().view(1, 1, 1, 4).to(dev)
    noise_d = noise.to(dev) if ancestral else None
    x = xT.double()
    for k in range(6):
        sigma, c_in, sigma_to, sigma_up = [float(q) for q in coef[k]]
        cond.copy_(lat[:, 0])                                                # frame 0 evolves with the rest: the overwrite is a no-op
        model_in = K.sigma_prep(lat, cond, coef_d, idx, 4, 1)                 # [2, 16, 16, 4] fp16, scaled
        tok = (sigma * (model_in.float() / c_in) / (v_tok + sigma * sigma)).contiguous()
        K.euler_cfg_step(lat, noise_d, tok, coef_d, idx, 1.0, 1)
        x = x * (1 + sigma * (sigma_to - sigma) / (v + sigma * sigma))
        if ancestral:
            x = x + sigma_up * noise[k].double()
    if not ancestral:
        prod = torch.ones_like(v)
        for k in range(6):
            sigma, _, sigma_to, _ = [float(q) for q in coef[k]]
            prod = prod * (1 + sigma * (sigma_to - sigma) / (v + sigma * sigma))
        assert (x - xT.double() * prod).abs().max().item() <= 1e-12 * x.abs().max().item()
    torch.cuda.synchronize()
    err, scale = (lat.cpu().double() - x).abs().max().item(), x.abs().max().item()
    print(f"Euler{' ancestral' if ancestral else ''} gaussian model, 6 steps: max abs err {err:.3e} (max|x| {scale:.3e}, rel {err / scale:.3e})")
    assert err <= 1e-3 * scale, (err, scale)
    assert int(idx.item()) == 0


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


CASES = {"euler": (dict(), 4, 1.0, 1.0), "ancestral": (dict(ancestral=True), 6, 0.9, 2.0), "karras": (dict(use_karras_sigmas=True), 5, 1.0, 2.0)}


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_pipeline_trajectory_against_the_oracle(dev, small, case, use_graph):
    """the oracle scales its model input, noises its prior and (ancestral) draws its noise inside the reference scheduler, the product
    reads its tables: the same stream of `generator`, so only the UNet's fp16 error enters.  guidance 1.0 runs one copy; ratio 0.9 at
    N = 6 starts the loop at full-list index 1; the Karras case has fractional timesteps from `_sigma_to_t`."""
    from oracle.pipeline_i2v_adapter import I2VAdapterPipeline as OP
    ou, hu = small
    skw, N, ratio, guidance = CASES[case]
    pe, ne, _, cond = _problem()
    kw = dict(num_frames=4, num_inference_steps=N, guidance_scale=guidance, frame_similarity_sample_ratio=ratio)
    ref = _reference(case, lambda: OP(ou, scheduler=_ref_sched(**skw))(pe, ne, cond, **kw, **_gens()).frames)
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched(**skw))
    got = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, use_graph=use_graph, **kw, **_gens()).frames
    assert got.shape == (1, 4, 4, 16, 16)
    assert torch.equal(got[:, 0].cpu(), cond)
    err, scale = (got.float().cpu() - ref).abs().max().item(), ref.abs().max().item()
    print(f"Euler {case} N={N} ratio={ratio} guidance={guidance} use_graph={use_graph}: max abs latent err {err:.3e} (max|ref| {scale:.3e}, "
          f"rel {err / scale:.3e}, gate {REL_TOL_TRAJECTORY:.1e})")
    compare(got, ref, rel=REL_TOL_TRAJECTORY, name=f"Euler trajectory ({case}, N {N}, guidance {guidance}, use_graph {use_graph})")


@pytest.mark.parametrize("use_graph", [False, True])
def test_pipeline_trajectory_two_samples_with_ip(dev, small_ip, use_graph):
    """two samples per call, one generator each (every sample's noise rows come from its own generator, as diffusers' randn_tensor
    draws them), with the IP-Adapter branch, under the ancestral sampler.  Both sides are handed `latents` (the prior overwrites them,
    pipe:656): the oracle's prepare_latents takes one generator only."""
    from oracle.pipeline_i2v_adapter import I2VAdapterPipeline as OP
    ou, hu = small_ip
    pe, ne, ie, cond = _problem(seed=41, samples=2, ip=True)
    gens = lambda: dict(_gens(), generator=[torch.Generator().manual_seed(51), torch.Generator().manual_seed(52)])
    kw = dict(num_frames=4, num_inference_steps=6, guidance_scale=2.0, frame_similarity_sample_ratio=0.9, image_embeds=ie,
              blur_sigma=0.8, latents=torch.zeros(2, 4, 4, 16, 16))
    ref = _reference("ip", lambda: OP(ou, scheduler=_ref_sched(ancestral=True))(pe, ne, cond, **kw, **gens()).frames)
    got = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched(ancestral=True))(
        prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, use_graph=use_graph, **kw, **gens()).frames
    assert got.shape == (2, 4, 4, 16, 16) and torch.equal(got[:, 0].cpu(), cond)
    err, scale = (got.float().cpu() - ref).abs().max().item(), ref.abs().max().item()
    print(f"Euler ancestral N=6 two samples + IP use_graph={use_graph}: max abs latent err {err:.3e} (max|ref| {scale:.3e}, "
          f"rel {err / scale:.3e}, gate {REL_TOL_TRAJECTORY:.1e})")
    compare(got, ref, rel=REL_TOL_TRAJECTORY, name=f"Euler ancestral trajectory, 2 samples per call + IP (5 steps, use_graph {use_graph})")
    assert (got[0] - got[1]).abs().max().item() > 0.1


# ---------------------------------------------------------------------------------------------------------- plumbing
def _call_kw(seed=7, N=6):
    pe, ne, _, cond = _problem(seed=seed)
    return dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=4, num_inference_steps=N,
                guidance_scale=2.0, frame_similarity_sample_ratio=0.9)


@pytest.mark.parametrize("ancestral", [False, True], ids=["euler", "ancestral"])
def test_every_route_gives_the_same_result(dev, small, ancestral):
    """graph route == eager route == callback route bit for bit, on the same noise table; eta is ignored (no host noise, no warning,
    still captured, one cached graph)"""
    _, hu = small
    kw = _call_kw()
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched(ancestral))
    graph = pipe(**kw, **_gens()).frames
    seen = []
    called = pipe(**kw, callback=lambda i, t, lat: seen.append((i, float(t))), **_gens()).frames
    assert [i for i, _ in seen] == list(range(5)) and torch.equal(graph, called)           # int(6 * 0.9) steps (pipe:529-536)
    assert [t for _, t in seen] == [float(t) for t in pipe.scheduler.timesteps[1:]]       # fractional timesteps reach the callback
    assert torch.equal(graph, pipe(**kw, use_graph=False, **_gens()).frames)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        noisy = pipe(**kw, eta=0.5, **_gens()).frames
    assert torch.equal(noisy, graph) and len(pipe._graph_cache) == 1


def test_a_new_seed_on_the_cached_graph_gets_its_own_noise(dev, small):
    """the stale-noise-table case: a graph-cache hit must copy this call's table into the graph's static buffer"""
    _, hu = small
    kw = _call_kw(seed=8)
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched(True))
    first = pipe(**kw, **_gens(5)).frames
    captured = pipe._graph
    second = pipe(**kw, **_gens(77)).frames
    assert pipe._graph is captured and len(pipe._graph_cache) == 1        # a hit: replayed, not re-captured
    assert (second - first).abs().max().item() > 1e-2
    eager = pipe(**kw, use_graph=False, **_gens(77)).frames
    assert torch.equal(second, eager)
    assert torch.equal(pipe(**kw, **_gens(5)).frames, first)


@pytest.mark.parametrize("ancestral", [False, True], ids=["euler", "ancestral"])
def test_another_step_count_recaptures(dev, small, ancestral):
    _, hu = small
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched(ancestral))
    four = pipe(**_call_kw(seed=9, N=4), **_gens()).frames
    captured, key = pipe._graph, next(iter(pipe._graph_cache))
    six = pipe(**_call_kw(seed=9, N=6), **_gens()).frames
    assert pipe._graph is not captured and len(pipe._graph_cache) == 1 and next(iter(pipe._graph_cache)) != key
    assert torch.equal(six, pipe(**_call_kw(seed=9, N=6), use_graph=False, **_gens()).frames)
    assert torch.equal(four, pipe(**_call_kw(seed=9, N=4), **_gens()).frames)


def test_scheduler_swap_recaptures(dev, small):
    """one pipeline, DDIM -> Euler -> Euler-ancestral -> DDIM on the graph route: each swap re-captures; the two DDIM results are equal
    bit for bit"""
    p = pkg()
    _, hu = small
    kw = _call_kw(seed=10, N=6)
    pipe = p.I2VAdapterPipeline(unet=hu)
    first = pipe(**kw, **_gens()).frames
    keys = [next(iter(pipe._graph_cache))]
    pipe.scheduler = p.EulerDiscreteScheduler.from_config(pipe.scheduler.config)
    euler = pipe(**kw, **_gens()).frames
    keys.append(next(iter(pipe._graph_cache)))
    pipe.scheduler = p.EulerAncestralDiscreteScheduler.from_config(pipe.scheduler.config)
    anc = pipe(**kw, **_gens()).frames
    keys.append(next(iter(pipe._graph_cache)))
    pipe.scheduler = p.DDIMScheduler.from_config(pipe.scheduler.config)
    third = pipe(**kw, **_gens()).frames
    assert len(set(keys)) == 3 and next(iter(pipe._graph_cache)) == keys[0]
    assert torch.equal(first, third)
    assert (euler - first).abs().max().item() > 1e-3 and torch.equal(euler[:, 0], first[:, 0])
    assert (anc - euler).abs().max().item() > 1e-3 and torch.equal(anc[:, 0], first[:, 0])


# ---------------------------------------------------------------------------------------------------------- sigma-space noising
def test_the_prior_is_noised_in_sigma_space(dev, small):
    """blurred strength 0 leaves the prior = the condition latents in every frame: the initial latents are cond + sigma_0 noise, with
    noise the draw of `prior_noise_generator` (two fp32 roundings); with ratio 0.5 sigma_0 is the level of the first EXECUTED step"""
    _, hu = small
    _, _, _, cond = _problem()
    for ratio, first in ((1.0, 0), (0.5, 2)):
        pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched())
        gens = _gens()
        lat, _, noise, source, ts = pipe._initial_latents(cond, None, 1, 4, 128, 128, 4, ratio, 0.0, gens["generator"], None,
                                                          gens["prior_mask_generator"], gens["prior_noise_generator"], 0.8)
        sigma = float(pipe.scheduler.sigmas[first])
        assert source is None and len(ts) == 4 - first and float(ts[0]) == float(pipe.scheduler.timesteps[first])
        z = torch.randn((1, 4, 4, 16, 16), generator=torch.Generator().manual_seed(7))
        assert torch.equal(noise.cpu(), z)
        want = cond[:, None].double() + sigma * z.double()
        bound = 2 * 2.0 ** -24 * (cond[:, None].double().abs() + (sigma * z.double()).abs())
        assert bool(((lat.cpu().double() - want).abs() <= bound).all())


@torch.no_grad()
def _v2v_reference(ou, sched, pe, ne, cond, src, noise, N, strength, guidance, mask=None):
    """video-to-video (and the inpainting blend) restated for a sigma-space scheduler on the oracle's UNet: the clip noised to the first
    executed timestep's level by `add_noise`, the reference loop, after every step the blend to the NEXT step's level"""
    sched.set_timesteps(N)
    ts = sched.timesteps[N - min(int(N * strength), N):]
    x = sched.add_noise(src, noise, ts[:1])
    ctx = torch.cat([ne, pe])
    for i, t in enumerate(ts):
        x[:, 0] = cond
        pred = ou(sched.scale_model_input(torch.cat([x] * 2), t), t, enable_cross_frame_attn=True, encoder_hidden_states=ctx).sample
        u, c = pred.chunk(2)
        x = sched.step(u + guidance * (c - u), t, x)
        if mask is not None:
            kept = sched.add_noise(src, noise, ts[i + 1: i + 2]) if i + 1 < len(ts) else src
            x = mask * x + (1 - mask) * kept
    x[:, 0] = cond
    return x


def _clip(seed=31):
    pe, ne, _, cond = _problem(seed)
    src = torch.randn(1, 3, 4, 16, 16, generator=torch.Generator().manual_seed(seed + 1))
    noise = torch.randn((1, 3, 4, 16, 16), generator=torch.Generator().manual_seed(7))          # the draw of `prior_noise_generator`
    return dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=3, guidance_scale=2.0), src, noise


def test_video_to_video_against_the_reference_loop(dev, small):
    """`video_latents=` with strength 0.5 of a 4-step Euler schedule: the source + sigma_t noise, then the last two steps"""
    ou, hu = small
    kw, src, noise = _clip()
    ref = _v2v_reference(ou, _ref_sched(), kw["prompt_embeds"], kw["negative_prompt_embeds"], kw["condition_image_latents"], src, noise,
                         4, 0.5, 2.0)
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched())
    got = pipe(**kw, video_latents=src, num_inference_steps=4, strength=0.5, **_gens()).frames
    err, scale = compare(got, ref, rel=REL_TOL_TRAJECTORY, name="Euler video-to-video (2 of 4 steps)")
    print(f"Euler video-to-video: max abs err {err:.3e} (max|ref| {scale:.3e}, rel {err / scale:.3e})")
    assert torch.equal(got, pipe(**kw, video_latents=src, num_inference_steps=4, strength=0.5, use_graph=False, **_gens()).frames)
    start = pipe.prepare_video_latents(src.to(dev), noise.to(dev), pipe.scheduler.timesteps[2]).cpu()
    want = src.double() + float(pipe.scheduler.sigmas[2]) * noise.double()
    assert bool(((start.double() - want).abs() <= 2 * 2.0 ** -24 * (src.double().abs() + (want - src.double()).abs())).all())


@pytest.mark.parametrize("ancestral", [False, True], ids=["euler", "ancestral"])
def test_mask_keeps_the_source_and_the_steps_bits(dev, small, ancestral):
    """m == 0 ends as the source bit for bit, m == 1 keeps the scheduler step's bits (a mask of ones is the call without a mask), and a
    half mask follows the reference loop's blend; graph == eager"""
    ou, hu = small
    kw, src, noise = _clip()
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched(ancestral))
    call = lambda **k: pipe(**kw, video_latents=src, num_inference_steps=4, strength=0.75, **k, **_gens()).frames
    plain = call()
    assert torch.equal(call(mask_image=torch.ones(16, 16)), plain)
    kept = call(mask_image=torch.zeros(16, 16)).cpu()
    assert torch.equal(bits(kept[:, 1:]), bits(src[:, 1:])) and torch.equal(kept[:, 0], kw["condition_image_latents"])
    m = torch.zeros(16, 16)
    m[:, 8:] = 1.0
    half = call(mask_image=m)
    assert torch.equal(half, call(mask_image=m, use_graph=False)) and torch.isfinite(half).all()
    assert torch.equal(bits(half[:, 1:, :, :, :8].cpu()), bits(src[:, 1:, :, :, :8])) and not torch.equal(half, plain)
    if not ancestral:
        ref = _v2v_reference(ou, _ref_sched(), kw["prompt_embeds"], kw["negative_prompt_embeds"], kw["condition_image_latents"], src, noise,
                             4, 0.75, 2.0, mask=m[None, None, None].expand(1, 3, 1, 16, 16))
        compare(half, ref, rel=REL_TOL_TRAJECTORY, name="Euler masked video-to-video (3 of 4 steps)")
    tab = pipe.renoise_table(pipe.scheduler.timesteps[1:])
    assert tab[0].tolist() == [1.0, 0.0] and torch.equal(tab[1:, 1], pipe.scheduler.sigmas[2:4]) and bool((tab[:, 0] == 1).all())


@torch.no_grad()
def _free_init_reference(ou, sched, pe, ne, cond, N, rounds, guidance, generator, prior_mask_generator, prior_noise_generator):
    """FreeInit restated for a sigma-space scheduler on the oracle's UNet (tests/freeinit_reference.py's loop, with the re-noising
    x0 + sigma_0 noise in place of the alpha pair): round 0 from the prior, every later round from the float64 mix"""
    from oracle.blocks import gaussian_blur3
    sched.set_timesteps(N)
    ts = sched.timesteps
    FR.randn((1, 4, 4, 16, 16), generator)                                                       # prepare_latents' draw
    blur_sigma = float(torch.empty(1).uniform_(0.1, 2.0, generator=prior_mask_generator).item())
    exp_blur = gaussian_blur3(cond, blur_sigma).unsqueeze(1).repeat(1, 4, 1, 1, 1)
    exp_cond = cond.unsqueeze(1).repeat(1, 4, 1, 1, 1)
    mask = (torch.rand(exp_cond.shape, generator=prior_mask_generator) < 0.6).to(exp_cond.dtype)
    init_noise = torch.randn(exp_cond.shape, generator=prior_noise_generator)
    x = sched.add_noise(mask * exp_blur + (1 - mask) * exp_cond, init_noise, ts[:1])
    lpf = FR.reference_filter((4, 16, 16))
    ctx = torch.cat([ne, pe])
    for rnd in range(rounds):
        if rnd > 0:
            z_rand = FR.randn(x.shape, generator)
            sched.set_timesteps(N)
            x = FR.reference_mix(x, init_noise, z_rand, lpf, 1.0, float(sched.sigmas[0])).to(torch.float32)
        for t in ts:
            x[:, 0] = cond
            pred = ou(sched.scale_model_input(torch.cat([x] * 2), t), t, enable_cross_frame_attn=True, encoder_hidden_states=ctx).sample
            u, c = pred.chunk(2)
            x = sched.step(u + guidance * (c - u), t, x, generator=generator)
        x[:, 0] = cond
    return x


def test_free_init_two_rounds_under_euler(dev, small):
    """two rounds of 3 Euler steps: the second round starts from the first's clip re-noised with the prior's noise to sigma_0 and
    low-passed against fresh noise; both rounds replay one captured step"""
    ou, hu = small
    pe, ne, _, cond = _problem()
    ref = _free_init_reference(ou, _ref_sched(), pe, ne, cond, 3, 2, 2.0, **_gens())
    one = _free_init_reference(ou, _ref_sched(), pe, ne, cond, 3, 1, 2.0, **_gens())
    assert (ref - one).abs().max().item() > 0.05                                                 # the second round does something
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=_sched())
    pipe.enable_free_init(num_iters=2)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=4, num_inference_steps=3,
              guidance_scale=2.0)
    got = pipe(**kw, **_gens()).frames
    assert torch.equal(got[:, 0].cpu(), cond) and len(pipe._graph_cache) == 1
    err, scale = compare(got, ref, rel=REL_TOL_TRAJECTORY, name="FreeInit under Euler (2 rounds x 3 steps, guidance 2)")
    print(f"FreeInit under Euler: max abs err {err:.3e} (max|ref| {scale:.3e}, rel {err / scale:.3e}, gate {REL_TOL_TRAJECTORY:.1e})")
    assert torch.equal(got, pipe(**kw, use_graph=False, **_gens()).frames)


# ---------------------------------------------------------------------------------------------------------- next to the rest
def _next_to(pipe, kw, **extra):
    """the ancestral sampler's captured route equals its eager route bit for bit, with one cached graph"""
    graph = pipe(**kw, num_inference_steps=3, **extra, **_gens()).frames
    eager = pipe(**kw, num_inference_steps=3, use_graph=False, **extra, **_gens()).frames
    assert torch.isfinite(graph).all() and torch.equal(graph, eager) and len(pipe._graph_cache) == 1
    assert torch.equal(graph[:, 0].cpu(), kw["condition_image_latents"])
    return graph


def test_ancestral_next_to_a_controlnet_and_a_t2i_adapter(dev, small):
    """the ControlNet reads the scaled model input the UNet reads; the adapter's features are added as under any scheduler"""
    from tests import controlnet_reference as CR
    from tests import t2i_adapter_reference as TR
    p = pkg()
    pe, ne, _, cond = _problem()
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=2, guidance_scale=2.0)
    frames = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(41))
    cn = p.ControlNetModel(**CR.small_config())
    cn.load_state_dict(CR.small_reference().state_dict())
    pipe = p.I2VAdapterPipeline(unet=small[1], controlnet=cn.to(dev, torch.float16).eval(), scheduler=_sched(True))
    on = _next_to(pipe, kw, control_image=frames)
    assert not torch.equal(on, pipe(**kw, num_inference_steps=3, control_image=frames, controlnet_conditioning_scale=0.0, **_gens()).frames)
    ad = p.T2IAdapter(**TR.small_config(3))
    ad.load_state_dict(TR.small_reference(3).state_dict())
    pipe = p.I2VAdapterPipeline(unet=small[1], t2i_adapter=ad.to(dev, torch.float16).eval(), scheduler=_sched(True))
    on = _next_to(pipe, kw, adapter_image=frames)
    assert not torch.equal(on, pipe(**kw, num_inference_steps=3, adapter_image=frames, adapter_conditioning_scale=0.0, **_gens()).frames)


def test_ancestral_under_free_noise_and_prompt_travel(dev, small):
    pe, ne, _, cond = _problem()
    pipe = pkg().I2VAdapterPipeline(unet=small[1], scheduler=_sched(True))
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=6, guidance_scale=2.0)
    plain = _next_to(pipe, kw)
    pipe.enable_free_noise(context_length=4, context_stride=2)
    try:
        windowed = _next_to(pipe, kw)
    finally:
        pipe.disable_free_noise()
    assert windowed.shape == (1, 6, 4, 16, 16) and not torch.equal(windowed, plain)
    g = torch.Generator().manual_seed(43)
    per_frame = h(torch.randn(1, 4, 7, 64, generator=g))
    kw = dict(kw, num_frames=4, prompt_embeds=per_frame)
    travelled = _next_to(pipe, kw)
    assert not torch.equal(travelled, _next_to(pipe, dict(kw, prompt_embeds=per_frame[:, 0])))


# ---------------------------------------------------------------------------------------------------------- the model handle
@pytest.mark.parametrize("ancestral", [False, True], ids=["euler", "ancestral"])
def test_the_c_handle_refuses_the_schedulers(dev, small, ancestral):
    p = pkg()
    pipe = p.I2VAdapterPipeline(unet=small[1], scheduler=_sched(ancestral))
    st = dict(latents=torch.zeros(1, 4, 4, 16, 16, device=dev), copies=2, ctx_text=torch.zeros(2, 7, 64, device=dev))
    with pytest.raises(NotImplementedError, match=type(pipe.scheduler).__name__):
        p.handle.record_step_plan(pipe, st)
    with pytest.raises(NotImplementedError, match=type(pipe.scheduler).__name__):
        p.handle.export_denoiser(pipe, "unused", num_frames=4, latent_height=16, latent_width=16)
