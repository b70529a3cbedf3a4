"""FreeInit on the GPU: `i2v_freeinit_mix` against the float64 three-transform reference (tests/freeinit_reference.py) at the smallest
shapes at which each index path can go wrong and at the product's shape, synthetic tables (zeros, ones, a single centre / off-centre
bin), a run over a NaN-filled workspace and output, the pipeline's trajectory on the reduced UNet against the oracle loop composed
with the reference mix, the routes that must agree bit for bit, and the one captured step every round replays.

The kernel's bound is max |out - ref| <= 1e-5 max |ref| (the bound of the DDIM / DPM / LCM step kernels' tests): an fp32 direct-DFT
emulation with exactly rounded twiddles lands at 3.6e-7 absolute for 16 x 64 x 64 (max |ref| 4.9), so a wrong twiddle, shift or scale
(errors of order 1) cannot pass and fp32 summation cannot fail."""
import ctypes as C

import pytest
import torch

from tests import freeinit_reference as R
from tests.lcm_reference import ReferenceLCMScheduler
from tests.parity import REL_TOL_TRAJECTORY, compare, hip_unet_from_oracle, oracle_small_unet

pytestmark = pytest.mark.gpu

KERNEL_REL = 1e-5
#          B   F  C    H    W
SHAPES = [(1, 16, 4, 8, 8),
          (2, 3, 4, 5, 7),          # all odd, B > 1
          (1, 8, 4, 12, 10),        # even, not a power of two
          (1, 1, 4, 8, 8),          # F = 1
          (1, 32, 1, 4, 4),         # F at its limit
          (1, 2, 1, 128, 4),        # H at its limit
          (1, 2, 1, 4, 128),        # W at its limit
          (1, 16, 4, 64, 64)]       # the product's shape
METHODS = ["butterworth", "gaussian", "ideal"]


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h(t):
    return t.half().float()


def _levels():
    """sqrt(a), sqrt(1 - a) at t = 999 (about 0.068 / 0.998)"""
    a = float(pkg().DDIMScheduler().alphas_cumprod[999])
    assert 0.06 < a ** 0.5 < 0.075
    return a ** 0.5, (1.0 - a) ** 0.5


_OPERANDS = {}


def _operands(shape):
    """latents (a clean clip's scale), init_noise, z_rand on the host: drawn once per shape, never modified"""
    if shape not in _OPERANDS:
        g = torch.Generator().manual_seed(17 + sum(shape))
        _OPERANDS[shape] = (2.0 * torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn(shape, generator=g))
    return _OPERANDS[shape]


def _check(got, ref, what):
    got = got.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"freeinit_mix {what}: max abs err {err:.3e}, max|ref| {scale:.3e}, rel {err / scale:.3e} (bound {KERNEL_REL:.0e})")
    assert err <= KERNEL_REL * scale, (what, err, scale)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_kernel_against_the_float64_reference(dev, shape, method):
    K, F = pkg().kernels, pkg().free_init
    lat, noise, zr = _operands(shape)
    sa, sb = _levels()
    fhw = (shape[1], shape[3], shape[4])
    lpf = F.free_init_filter(fhw, method, 4, 0.25, 0.25)
    ref = R.reference_mix(lat, noise, zr, lpf, sa, sb)
    lat_d, noise_d, zr_d = lat.to(dev), noise.to(dev), zr.to(dev)
    got = K.freeinit_mix(lat_d, noise_d, zr_d, lpf.to(dev), sa, sb)
    torch.cuda.synchronize()
    _check(got, ref, f"{shape} {method}")
    assert torch.equal(lat_d.cpu(), lat) and torch.equal(noise_d.cpu(), noise) and torch.equal(zr_d.cpu(), zr)       # inputs untouched
    assert got.data_ptr() not in (lat_d.data_ptr(), noise_d.data_ptr(), zr_d.data_ptr())


@pytest.mark.parametrize("shape", [(2, 3, 4, 5, 7), (1, 8, 4, 12, 10)], ids=["odd", "even"])
def test_synthetic_tables(dev, shape):
    """zeros -> z_rand bit for bit; ones -> z_t; the centre bin alone -> z_rand + the volume mean of z_t - z_rand; one off-centre bin ->
    the reference (at the odd shape its spectrum is not Hermitian: the dropped imaginary part is not zero)"""
    K = pkg().kernels
    lat, noise, zr = _operands(shape)
    sa, sb = _levels()
    b, f, c, hh, ww = shape
    d = [t.to(dev) for t in (lat, noise, zr)]
    run = lambda table: K.freeinit_mix(*d, table.to(dev), sa, sb)
    assert torch.equal(run(torch.zeros(f, hh, ww)).cpu(), zr)
    z_t = R.add_noise(lat, noise, sa, sb)
    _check(run(torch.ones(f, hh, ww)), z_t, f"{shape} all ones")
    centre = torch.zeros(f, hh, ww)
    centre[f // 2, hh // 2, ww // 2] = 1.0
    want = zr.double() + (z_t - zr.double()).mean(dim=(1, 3, 4), keepdim=True)
    _check(run(centre), want, f"{shape} centre bin")
    off = torch.zeros(f, hh, ww)
    off[(f // 2 + 1) % f, hh // 2 - 2, ww // 2 + 1] = 1.0
    _check(run(off), R.reference_mix(lat, noise, zr, off, sa, sb), f"{shape} off-centre bin")
    if all(v % 2 for v in (f, hh, ww)):
        assert R.reference_mix_one_transform(lat, noise, zr, off, sa, sb, return_complex=True).imag.abs().max().item() > 1e-3


def test_poisoned_workspace_and_output(dev):
    """through the C entry point with a caller-made workspace: NaN in every byte of the workspace and of `out` beforehand, a finite and
    correct result afterwards -- the kernels read nothing they did not write"""
    lib = pkg()._lib
    hnd = lib.load()
    shape = (2, 3, 4, 5, 7)
    lat, noise, zr = _operands(shape)
    sa, sb = _levels()
    lpf = pkg().free_init.free_init_filter((3, 5, 7), "butterworth", 4, 0.25, 0.25)
    need = hnd.i2v_freeinit_workspace_bytes(*shape)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4,), float("nan"), device=dev)
    out = torch.full(shape, float("nan"), device=dev)
    d = [t.to(dev) for t in (lat, noise, zr, lpf)]
    p = lambda t: C.c_void_p(t.data_ptr())
    lib.check(hnd.i2v_freeinit_mix(p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(out), p(ws), need, *shape, sa, sb,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "i2v_freeinit_mix")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(ws).all()
    _check(out, R.reference_mix(lat, noise, zr, lpf, sa, sb), f"{shape} poisoned workspace")


def test_wrapper_checks(dev):
    K = pkg().kernels
    lat, noise, zr = (t.to(dev) for t in _operands((1, 8, 4, 12, 10)))
    lpf = torch.ones(8, 12, 10, device=dev)
    with pytest.raises(ValueError):
        K.freeinit_mix(lat, noise, zr[:, :4].contiguous(), lpf, 0.1, 0.9)
    with pytest.raises(ValueError):
        K.freeinit_mix(lat, noise, zr, lpf[:, :, :8].contiguous(), 0.1, 0.9)
    with pytest.raises(ValueError):
        K.freeinit_mix(lat, noise, zr.transpose(3, 4), lpf, 0.1, 0.9)
    with pytest.raises(TypeError):
        K.freeinit_mix(lat.half(), noise, zr, lpf, 0.1, 0.9)
    with pytest.raises(pkg().HipLibraryError):
        K.freeinit_mix(lat.cpu(), noise, zr, lpf, 0.1, 0.9)
    big = torch.zeros(1, 33, 1, 4, 4, device=dev)
    with pytest.raises(pkg().HipLibraryError, match="not implemented for this problem"):
        K.freeinit_mix(big, big.clone(), big.clone(), torch.ones(33, 4, 4, device=dev), 0.1, 0.9)


# ---------------------------------------------------------------------------------------------------------- the pipeline
def _problem(seed=31, samples=1):
    g = torch.Generator().manual_seed(seed)
    pe, ne = h(torch.randn(samples, 7, 64, generator=g)), h(torch.randn(samples, 7, 64, generator=g))
    cond = torch.randn(samples, 4, 16, 16, generator=g)
    return pe, ne, cond


def _gens(seed=5):
    return dict(generator=torch.Generator().manual_seed(seed), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


@pytest.fixture(scope="module")
def small(dev):
    ou = oracle_small_unet()
    return ou, hip_unet_from_oracle(ou, dev)


def _schedulers(kind):
    from oracle.blocks import DDIMScheduler as OracleDDIM
    p = pkg()
    return (OracleDDIM(), p.DDIMScheduler()) if kind == "ddim" else (ReferenceLCMScheduler(), p.LCMScheduler())


@pytest.mark.parametrize("kind,samples", [("ddim", 1), ("lcm", 1), ("lcm", 2)])
def test_pipeline_trajectory_against_the_oracle(dev, small, kind, samples):
    """two rounds of 3 steps, guidance 2: the oracle loop with the float64 mix between its rounds, on the same host-generator draws
    (z_rand after round 0's draws, then an LCM round's noise -- a wrong order changes the clip by far more than the gate).  samples = 2
    draws every sample's noise from its own generator; both sides are then handed `latents` (the prior overwrites them)."""
    from oracle.pipeline_i2v_adapter import I2VAdapterPipeline as OP
    ou, hu = small
    pe, ne, cond = _problem(samples=samples)
    o_sch, p_sch = _schedulers(kind)
    if samples == 1:
        gens, extra = _gens, {}
    else:
        gens = lambda: dict(_gens(), generator=[torch.Generator().manual_seed(51 + i) for i in range(samples)])
        extra = dict(latents=torch.zeros(samples, 4, 4, 16, 16), blur_sigma=0.8)
    kw = dict(num_frames=4, num_inference_steps=3, guidance_scale=2.0, **extra)
    ref = R.oracle_free_init_call(OP(ou, scheduler=o_sch), pe, ne, cond, num_iters=2, **kw, **gens())
    if kind == "ddim":          # the second round does something
        assert (ref - OP(ou, scheduler=_schedulers(kind)[0])(pe, ne, cond, **kw, **gens()).frames).abs().max().item() > 0.05
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=p_sch)
    pipe.enable_free_init(num_iters=2)
    got = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, **kw, **gens()).frames
    assert got.shape == (samples, 4, 4, 16, 16) and torch.equal(got[:, 0].cpu(), cond)       # frame 0 is the condition latents
    err, scale = (got.float().cpu() - ref).abs().max().item(), ref.abs().max().item()
    print(f"FreeInit {kind} x{samples}: 2 rounds of 3 steps, max abs latent err {err:.3e} (max|ref| {scale:.3e}, rel {err / scale:.3e}, "
          f"gate {REL_TOL_TRAJECTORY:.1e})")
    compare(got, ref, rel=REL_TOL_TRAJECTORY, name=f"FreeInit trajectory ({kind}, {samples} sample(s), 2 rounds x 3 steps, guidance 2)")


def _call_kw(seed=7, N=3):
    pe, ne, cond = _problem(seed=seed)
    return dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=4, num_inference_steps=N,
                guidance_scale=2.0)


@pytest.mark.parametrize("kind", ["ddim", "lcm", "dpm"])
def test_graph_and_callback_routes_agree(dev, small, kind):
    p = pkg()
    _, hu = small
    sch = {"ddim": p.DDIMScheduler, "lcm": p.LCMScheduler, "dpm": p.DPMSolverMultistepScheduler}[kind]()
    pipe = p.I2VAdapterPipeline(unet=hu, scheduler=sch)
    pipe.enable_free_init(num_iters=2)
    kw = _call_kw()
    graph = pipe(**kw, **_gens()).frames
    seen = []
    eager = pipe(**kw, callback=lambda i, t, lat: seen.append(i), **_gens()).frames
    assert seen == [0, 1, 2, 0, 1, 2]                        # the callback's step index restarts every round
    assert torch.equal(graph, eager)
    assert torch.equal(graph, pipe(**kw, use_graph=False, **_gens()).frames)


def test_one_round_and_disabled_are_a_plain_call(dev, small):
    p = pkg()
    _, hu = small
    kw = _call_kw(seed=8)
    never = p.I2VAdapterPipeline(unet=hu)(**kw, **_gens()).frames
    pipe = p.I2VAdapterPipeline(unet=hu)
    pipe.enable_free_init(num_iters=1)
    assert torch.equal(pipe(**kw, **_gens()).frames, never)
    pipe.enable_free_init(num_iters=1, use_fast_sampling=True)
    assert torch.equal(pipe(**kw, **_gens()).frames, never)
    pipe.enable_free_init(num_iters=3)
    assert pipe.free_init_enabled and (pipe(**kw, **_gens()).frames - never).abs().max().item() > 1e-2
    pipe.disable_free_init()
    assert not pipe.free_init_enabled and torch.equal(pipe(**kw, **_gens()).frames, never)


def test_rounds_replay_one_captured_step(dev, small):
    """a plain call captures; enabling FreeInit neither re-captures nor adds a cache entry, and a later sample with a new seed on the
    cached graph equals its own eager run"""
    p = pkg()
    _, hu = small
    kw = _call_kw(seed=9)
    pipe = p.I2VAdapterPipeline(unet=hu)
    plain = pipe(**kw, **_gens()).frames
    captured, key = pipe._graph, next(iter(pipe._graph_cache))
    pipe.enable_free_init(num_iters=3)
    first = pipe(**kw, **_gens()).frames
    assert pipe._graph is captured and len(pipe._graph_cache) == 1 and next(iter(pipe._graph_cache)) == key
    second = pipe(**kw, **_gens(77)).frames
    assert pipe._graph is captured and len(pipe._graph_cache) == 1
    assert (second - first).abs().max().item() > 1e-2
    assert torch.equal(second, pipe(**kw, use_graph=False, **_gens(77)).frames)
    assert torch.equal(first, pipe(**kw, **_gens()).frames)
    pipe.disable_free_init()
    assert torch.equal(plain, pipe(**kw, **_gens()).frames) and pipe._graph is captured


@pytest.mark.parametrize("kind", ["ddim", "lcm"])
def test_fast_sampling_matches_its_eager_run(dev, small, kind):
    """6 steps over 3 rounds: 2, 4 and 6 steps, each round re-capturing the step (its tables change shape)"""
    p = pkg()
    _, hu = small
    kw = _call_kw(seed=10, N=6)
    pipe = p.I2VAdapterPipeline(unet=hu, scheduler=(p.DDIMScheduler if kind == "ddim" else p.LCMScheduler)())
    pipe.enable_free_init(num_iters=3, use_fast_sampling=True)
    seen = []
    eager = pipe(**kw, use_graph=False, **_gens()).frames
    graph = pipe(**kw, **_gens()).frames
    assert len(pipe._graph_cache) == 1
    assert torch.equal(graph, eager) and torch.isfinite(graph).all()
    assert torch.equal(graph, pipe(**kw, callback=lambda i, t, lat: seen.append(i), **_gens()).frames)
    assert seen == [0, 1, 0, 1, 2, 3, 0, 1, 2, 3, 4, 5]
    assert torch.equal(graph[:, 0].cpu(), kw["condition_image_latents"])
