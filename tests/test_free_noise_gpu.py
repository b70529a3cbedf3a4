"""FreeNoise on the GPU: the two row movers (`i2v_freenoise_gather_f16` bit for bit against torch indexing, `i2v_freenoise_blend_f16`
within one fp16 ulp of the fp64 sum), the motion module and the reduced UNet against the oracle running the literal FreeNoise loop
(tests/freenoise_reference.py), the switch's bit-exact off / one-window states, a forward recorded with FreeNoise replayed through
`i2v_unet_forward`, and the pipeline (graph == eager, re-capture on enable / disable, graph reuse, LCM's noise table, FreeInit's limit).
Every measured error is appended to profiles/freenoise_errors.jsonl ($I2V_FREENOISE_LOG names another file)."""
import json
import os
import struct

import pytest
import torch

from tests import freenoise_reference as R
from tests.parity import REL_TOL_MODULE, REL_TOL_UNET, ROOT, compare, hip_unet_from_oracle, oracle_small_unet, round_fp16_

pytestmark = pytest.mark.gpu

SCHEMES = ("flat", "pyramid", "delayed_reverse_sawtooth")


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h16(t):
    return t.half().float()


_LOG_STARTED = []


def _log(name, **values):
    """one JSON line per measured error; the file is started afresh by the first line of a test session, so a run of the suite
    rewrites it (the results are deterministic for a given binary) instead of growing it"""
    path = os.environ.get("I2V_FREENOISE_LOG") or os.path.join(ROOT, "profiles", "freenoise_errors.jsonl")
    with open(path, "a" if _LOG_STARTED else "w") as f:
        f.write(json.dumps(dict(name=name, **values)) + "\n")
    _LOG_STARTED.append(path)


def _settings(L, S, scheme="pyramid", noise="shuffle_context"):
    return pkg().free_noise.FreeNoiseSettings(L, S, scheme, noise)


# ---------------------------------------------------------------------------------------------------------- the kernels
KERNEL_CASES = [(320, 22, 8, 4), (1280, 22, 8, 4), (320, 40, 16, 4), (1280, 40, 16, 4)]
N_PIXELS = 6


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("c,F,L,S", KERNEL_CASES)
def test_gather_is_torch_indexing_bit_for_bit(dev, c, F, L, S, strided):
    K = pkg().kernels
    starts, _, _ = pkg().free_noise.tables(F, _settings(L, S), dev)
    g = torch.Generator().manual_seed(c + F)
    full = torch.randn(N_PIXELS * F, c + 64 if strided else c, generator=g).half()
    bits = full.view(torch.int16)
    bits[::7, 3] = -32768            # -0.0
    bits[::5, 9] = 0x7E01            # a NaN with a payload
    bits[::3, 17] = 1                # the smallest subnormal
    src = full.to(dev)[:, 8: 8 + c] if strided else full.to(dev)          # a strided source: rows c + 64 apart, 16 bytes in
    out = K.freenoise_gather(src, starts, n_pixels=N_PIXELS, frames=F, length=L)
    torch.cuda.synchronize()
    W = starts.numel()
    assert out.shape == (N_PIXELS * W * L, c) and out.is_contiguous() and out.dtype == torch.float16
    rows = torch.tensor([p * F + s + j for p in range(N_PIXELS) for s in starts.tolist() for j in range(L)])
    want = (full[:, 8: 8 + c] if strided else full)[rows]
    assert torch.equal(out.cpu().view(torch.int16), want.contiguous().view(torch.int16))
    assert torch.equal(src.cpu().view(torch.int16), (full[:, 8: 8 + c] if strided else full).view(torch.int16)), "the source is not modified"


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("c,F,L,S", KERNEL_CASES)
def test_blend_within_one_ulp_of_the_fp64_sum(dev, c, F, L, S, scheme):
    """one fp16 ulp of the reference everywhere, the ulp being the true spacing of fp16 at the reference, 2^(max(floor(log2 |ref|),
    -14) - 10).  At most ceil(L / S) + 1 <= 5 fp32 terms are accumulated: an error below 1e-6 of the LARGEST TERM, far below half an
    fp16 ulp of a result of the terms' size, so there only a value at a rounding boundary can move, and by one ulp.  Where the terms
    cancel to a result near zero the same absolute error (a few 1e-8 for terms of order 1) meets fp16's subnormal spacing 2^-24 = 6e-8,
    so the largest errors in ulps sit there (the figure is printed and logged).  Rows whose table holds the single coefficient 1.0 are
    the bits of their source row."""
    K = pkg().kernels
    st = _settings(L, S, scheme)
    starts, idx, coef = pkg().free_noise.tables(F, st, dev)
    W, pairs = starts.numel(), idx.shape[1]
    assert pairs <= -(-L // S) + 1 <= 5
    g = torch.Generator().manual_seed(c + F + len(scheme))
    tw = torch.randn(N_PIXELS, W * L, c, generator=g).half()
    out = K.freenoise_blend(tw.reshape(-1, c).to(dev), idx, coef, n_pixels=N_PIXELS, windows=W, length=L)
    torch.cuda.synchronize()
    assert out.shape == (N_PIXELS * F, c) and out.dtype == torch.float16
    idx_c, coef_c = idx.cpu().long(), coef.cpu().double()
    ref = sum(coef_c[None, :, k, None] * tw.double()[:, idx_c[:, k]] for k in range(pairs)).reshape(-1, c)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    exponent = torch.clamp(torch.floor(torch.log2(torch.clamp(ref.abs(), min=2.0 ** -30))), min=-14.0)
    bound = torch.pow(2.0, exponent - 10.0)                                      # one fp16 ulp at ref (2^-24 below 2^-14)
    assert bool((bound <= 2.0 ** -10 * torch.clamp(ref.abs(), min=2.0 ** -14)).all())
    ratio = err / bound
    worst = ratio.max().item()
    at = ref.reshape(-1)[ratio.argmax()].item()
    normal = ref.abs() >= 2.0 ** -14
    worst_normal = ratio[normal].max().item()
    print(f"blend c={c} F={F} L={L} S={S} {scheme}: max |err| / (one fp16 ulp) = {worst:.3f} at ref = {at:.3e}; "
          f"{worst_normal:.3f} over the normal range")
    _log("blend kernel", c=c, F=F, L=L, S=S, scheme=scheme, worst_ulp=worst, worst_at_ref=at, worst_ulp_normal_range=worst_normal)
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements off by more than one fp16 ulp (worst {worst:.3f})"
    single = [f for f in range(F) if int((coef_c[f] != 0).sum()) == 1]
    assert single and all(float(coef_c[f, 0]) == 1.0 for f in single)
    got16 = out.cpu().view(N_PIXELS, F, c)
    for f in single:
        assert torch.equal(got16[:, f].contiguous().view(torch.int16), tw[:, idx_c[f, 0]].contiguous().view(torch.int16)), f


def test_blend_single_rows_keep_special_values_and_padding_is_not_read(dev):
    """F = 22, L = 8, S = 4: frames 0 - 3 and 18 - 21 have one contributing window (coefficient 1.0, padding behind it).  Their source
    rows carry -0.0, a subnormal and inf and come back bit for bit; the padding's index-0 row is what frame 0 itself reads, so a
    second table whose padding points at a poisoned row nobody else reads proves padding is skipped, not multiplied by 0."""
    K = pkg().kernels
    F, L, S, c = 22, 8, 4, 320
    starts, idx, coef = pkg().free_noise.tables(F, _settings(L, S), dev)
    W = starts.numel()
    tw = torch.randn(N_PIXELS, W * L, c, generator=torch.Generator().manual_seed(9)).half()
    bits = tw.view(torch.int16)
    bits[:, :, 8] = -32768
    bits[:, :, 9] = 1
    bits[:, 0:4, 10] = 0x7C00
    out = K.freenoise_blend(tw.reshape(-1, c).to(dev), idx, coef, n_pixels=N_PIXELS, windows=W, length=L).cpu().view(N_PIXELS, F, c)
    for f in (0, 1, 2, 3, 18, 19, 20, 21):
        assert torch.equal(out[:, f].contiguous().view(torch.int16), tw[:, int(idx[f, 0])].contiguous().view(torch.int16)), f
    # the trailing window's rows 0 .. 5 (frames 14 .. 19 of window 4) contribute to nothing: poison them and point the padding there
    dead = 4 * L
    poisoned = tw.clone()
    poisoned[:, dead: dead + 6] = float("nan")
    idx2 = idx.clone()
    idx2[coef == 0] = dead
    out2 = K.freenoise_blend(poisoned.reshape(-1, c).to(dev), idx2, coef, n_pixels=N_PIXELS, windows=W, length=L).cpu().view(N_PIXELS, F, c)
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16))


def test_wrappers_reject_what_the_kernels_do_not_take(dev):
    K = pkg().kernels
    starts, idx, coef = pkg().free_noise.tables(22, _settings(8, 4), dev)
    z = lambda *s: torch.zeros(*s, dtype=torch.float16, device=dev)
    with pytest.raises(ValueError):
        K.freenoise_gather(z(6 * 22, 12), starts, n_pixels=6, frames=22, length=8)          # C not a multiple of 8
    with pytest.raises(ValueError):
        K.freenoise_gather(z(6 * 21, 16), starts, n_pixels=6, frames=22, length=8)          # rows
    with pytest.raises(TypeError):
        K.freenoise_gather(z(6 * 22, 16), starts.long(), n_pixels=6, frames=22, length=8)
    with pytest.raises(pkg()._lib.HipLibraryError, match="length"):
        K.freenoise_gather(z(6 * 4, 16), starts, n_pixels=6, frames=4, length=8)            # L > F
    with pytest.raises(ValueError):
        K.freenoise_blend(z(6 * 5 * 8, 16), idx, coef[:, :1], n_pixels=6, windows=5, length=8)
    with pytest.raises(TypeError):
        K.freenoise_blend(z(6 * 5 * 8, 16), idx, coef.half(), n_pixels=6, windows=5, length=8)


# ---------------------------------------------------------------------------------------------------------- the motion module
MODULE_KW = dict(num_attention_heads=8, in_channels=320, norm_num_groups=32, attention_bias=False, activation_fn="geglu",
                 positional_embeddings="sinusoidal", num_positional_embeddings=32, attention_head_dim=40)


@pytest.fixture(scope="module")
def module_pair(dev):
    from oracle.blocks import TransformerTemporalModel as OT
    torch.manual_seed(7)
    o = round_fp16_(OT(**MODULE_KW)).eval()
    m = pkg().TransformerTemporalModel(**MODULE_KW)
    m.load_state_dict(o.state_dict())
    return o, m.to(device=dev, dtype=torch.float16).eval()


def _module_input(batch, F, seed):
    return h16(torch.randn(batch * F, 320, 8, 8, generator=torch.Generator().manual_seed(seed)))


@pytest.mark.parametrize("batch,F,L,S,scheme,fused", [
    (2, 24, 16, 4, "pyramid", True),                       # window rows 2 * 64 * 3 * 16: the fused motion_attn launch
    (2, 22, 8, 4, "flat", False),                          # un-fused (LayerNorm / GEMMs / temporal attention), a trailing window
    (2, 40, 16, 4, "delayed_reverse_sawtooth", True),      # beyond the positional table, F not a power of two
    (1, 64, 16, 4, "pyramid", True),                       # beyond the table, the power-of-two feed-forward tail
])
def test_motion_module_against_the_reference_loop(dev, module_pair, monkeypatch, batch, F, L, S, scheme, fused):
    """REL_TOL_MODULE of max|ref|, the project's module tolerance: the window path adds one fp32 average and one fp16 rounding to the
    module's arithmetic.  (At this width every window count gives a multiple of 128 rows, which the fused launch takes at L = 8 too:
    the un-fused case switches it off, as I2V_MOTION_FUSED=0 does.)"""
    K = pkg().kernels
    o, m = module_pair
    if not fused:
        monkeypatch.setattr(pkg().blocks, "FUSED_MOTION_ATTN", False)
    x = _module_input(batch, F, seed=F + L)
    windows = len(R.ref_windows(F, L, S))
    rows = batch * 64 * windows * L
    if (batch, F, L) == (2, 24, 16):
        assert rows % 128 == 0 and K.motion_attn_supported(rows, 320, 8, 40, L), "this case is meant to run the fused motion_attn"
    with torch.no_grad():
        ref = R.ref_temporal_model(o, x, F, L, S, scheme)
        m.set_free_noise(_settings(L, S, scheme))
        try:
            got = m(x.half().to(dev), num_frames=F)[0]
        finally:
            m.set_free_noise(None)
    name = f"TransformerTemporalModel FreeNoise F={F} L={L} S={S} {scheme}"
    err, scale = compare(got, ref, rel=REL_TOL_MODULE, name=name)
    print(f"{name}: max abs err {err:.3e} (max|ref| {scale:.3e}, rel {err / scale:.3e}, gate {REL_TOL_MODULE:.1e})")
    _log(name, err=err, max_ref=scale, rel=err / scale, bound=REL_TOL_MODULE)


def test_one_window_is_bit_identical_and_the_plain_path_keeps_its_limit(dev, module_pair):
    _, m = module_pair
    x = _module_input(2, 16, seed=5).half().to(dev)
    with torch.no_grad():
        base = m(x, num_frames=16)[0]
        m.set_free_noise(_settings(16, 4))
        try:
            on = m(x, num_frames=16)[0]                        # F = L: today's path, unchanged
        finally:
            m.set_free_noise(None)
        assert torch.equal(on, base)
        x40 = _module_input(1, 40, seed=6).half().to(dev)
        with pytest.raises(ValueError, match="exceeds the positional table"):
            m(x40, num_frames=40)
        m.set_free_noise(_settings(16, 4))
        try:
            assert torch.isfinite(m(x40, num_frames=40)[0]).all()
        finally:
            m.set_free_noise(None)
        with pytest.raises(ValueError, match="exceeds the positional table"):
            m(x40, num_frames=40)


# ---------------------------------------------------------------------------------------------------------- the reduced UNet
@pytest.fixture(scope="module")
def small(dev):
    ou = oracle_small_unet()
    return ou, hip_unet_from_oracle(ou, dev)


def _unet_inputs(F, seed, hw=16):
    g = torch.Generator().manual_seed(seed)
    return h16(torch.randn(2, F, 4, hw, hw, generator=g)), torch.tensor([10, 500]), h16(torch.randn(2, 7, 64, generator=g))


def test_small_unet_forward_with_free_noise(dev, small):
    """F = 24, L = 16, S = 4 against the oracle UNet whose motion blocks run the reference loop, at the forward's gate REL_TOL_UNET;
    FreeNoise must move the output by far more than the gate, and disabling it restores the plain forward bit for bit"""
    ou, hu = small
    sample, t, ctx = _unet_inputs(24, seed=24)
    with torch.no_grad():
        ref_off = ou(sample, t, True, ctx).sample
        with R.hooked_blocks(ou, 16, 4, "pyramid") as n:
            assert n > 0
            ref_on = ou(sample, t, True, ctx).sample
        base = hu(sample.to(dev), t.to(dev), True, ctx.to(dev)).sample
        hu.enable_free_noise(16, 4, "pyramid")
        try:
            got = hu(sample.to(dev), t.to(dev), True, ctx.to(dev)).sample
        finally:
            hu.disable_free_noise()
        back = hu(sample.to(dev), t.to(dev), True, ctx.to(dev)).sample
    err, scale = compare(got, ref_on, rel=REL_TOL_UNET, name="small UNet F=24 FreeNoise L=16 S=4")
    e_off, _ = compare(base, ref_off, rel=REL_TOL_UNET, name="small UNet F=24 plain")
    moved = (ref_on - ref_off).abs().max().item()
    print(f"small UNet F=24: FreeNoise err {err:.3e} (max|ref| {scale:.3e}), plain err {e_off:.3e}; FreeNoise moves the oracle by {moved:.3e}")
    _log("small UNet F=24 L=16 S=4", err=err, max_ref=scale, rel=err / scale, bound=REL_TOL_UNET, plain_err=e_off, moved=moved)
    assert moved > 10 * REL_TOL_UNET * scale and torch.equal(back, base) and not torch.equal(got, base)
    s8, t8, c8 = _unet_inputs(8, seed=8)
    hu.enable_free_noise(16, 4)
    try:
        with pytest.raises(ValueError, match="below `context_length`"), torch.no_grad():
            hu(s8.to(dev), t8.to(dev), True, c8.to(dev))
    finally:
        hu.disable_free_noise()


def _plan_entries(blob):
    hdr = struct.unpack_from("<6I6iQ2I6Q", blob, 0)
    n_ops, ops_off = hdr[3], hdr[16]
    return [struct.unpack_from("<I", blob, ops_off + 24 * i)[0] for i in range(n_ops)]


def test_forward_plan_with_free_noise_through_the_c_abi(dev, monkeypatch, small):
    """a forward recorded with FreeNoise (F = 24 <= motion_max_seq_length) carries one gather and one blend per motion module and
    replays through i2v_unet_forward with no kernels.py wrapper running: bit-identical to the module API, also on other inputs"""
    p = pkg()
    H, K = p.handle, p.kernels
    _, hu = small

    def inputs(seed):
        s, t, c = _unet_inputs(24, seed)
        return dict(sample=s.half().to(dev), t=t.float().to(dev), ctx=c.half().to(dev))

    def module(inp):
        with torch.no_grad():
            return hu(inp["sample"], inp["t"], True, inp["ctx"]).sample
    inp, inp2 = inputs(5), inputs(6)
    plain = module(inp)
    hu.enable_free_noise(16, 4)
    try:
        ref, ref2 = module(inp), module(inp2)
        blob, weights = H.record_forward_plan(hu, inp["sample"], inp["t"], inp["ctx"])
    finally:
        hu.disable_free_noise()
    entries = _plan_entries(blob)
    n_motion = sum(len(m.transformer_blocks) for m in hu._motion_modules())
    assert entries.count(H.entry_id("i2v_freenoise_gather_f16")) == n_motion == entries.count(H.entry_id("i2v_freenoise_blend_f16"))
    assert any(k.startswith("free_noise#") for k in weights)
    hd = p.UNetHandle(hu)
    hd.plan(2, 24, 16, 16, ctx_len=7, has_ip=False)
    hd.set_plan(blob)
    hd.set_weights(weights)
    arena = torch.empty(hd.activation_bytes, dtype=torch.uint8, device=dev)
    hd.set_workspace(arena)
    out, out2 = torch.full_like(ref, float("nan")), torch.full_like(ref, float("nan"))

    def boom(*a, **k):
        raise AssertionError("a kernels.py wrapper ran during i2v_unet_forward")
    with monkeypatch.context() as mp:
        for name in ("freenoise_gather", "freenoise_blend", "gemm", "conv3x3", "attention", "groupnorm", "layernorm", "ff_fused", "motion_attn",
                     "temporal_attention", "nchw_to_tokens", "tokens_to_nchw", "timestep_embedding", "silu", "copy3d"):
            mp.setattr(K, name, boom)
        hd.forward(inp["sample"], inp["t"], inp["ctx"], None, out)
        hd.forward(inp2["sample"], inp2["t"], inp2["ctx"], None, out2)
        torch.cuda.synchronize()
    assert torch.equal(out, ref), f"C-ABI forward differs from the module API: max |d| {(out.float() - ref.float()).abs().max().item():.3e}"
    assert torch.equal(out2, ref2) and not torch.equal(out, plain)
    hd.close()


# ---------------------------------------------------------------------------------------------------------- the pipeline
def _problem(seed=31):
    g = torch.Generator().manual_seed(seed)
    return h16(torch.randn(1, 7, 64, generator=g)), h16(torch.randn(1, 7, 64, generator=g)), torch.randn(1, 4, 16, 16, generator=g)


def _gens(seed=5):
    return dict(generator=torch.Generator().manual_seed(seed), prior_mask_generator=torch.Generator().manual_seed(seed + 1),
                prior_noise_generator=torch.Generator().manual_seed(seed + 2))


def test_pipeline_graph_eager_recapture_and_reuse(dev, small):
    """F = 24, 3 DDIM steps: the replayed graph equals the eager steps bit for bit; enabling, then disabling FreeNoise re-captures and
    the disabled result equals a pipeline that never enabled it; a second sample of the same shape reuses the captured graph"""
    _, hu = small
    pe, ne, cond = _problem(seed=7)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=24, num_inference_steps=3,
              guidance_scale=7.5)
    pipe = pkg().I2VAdapterPipeline(unet=hu, scheduler=pkg().DDIMScheduler())
    try:
        plain = pipe(**kw, **_gens()).frames
        assert len(pipe._graph_cache) == 1
        g_plain = pipe._graph
        pipe.enable_free_noise(context_length=16, context_stride=4)
        assert pipe.free_noise_enabled
        graph = pipe(**kw, **_gens()).frames
        g_on = pipe._graph
        assert len(pipe._graph_cache) == 1 and g_on is not g_plain and not torch.equal(graph, plain), "a stale graph was replayed"
        assert graph.shape == (1, 24, 4, 16, 16) and torch.equal(graph[:, 0].cpu(), cond)
        seen = []
        eager = pipe(**kw, callback=lambda i, t, lat: seen.append(i), **_gens()).frames
        assert seen == [0, 1, 2] and torch.equal(graph, eager)
        second = pipe(**kw, **_gens(seed=50)).frames                          # another sample of the same shape: the same graph
        assert len(pipe._graph_cache) == 1 and pipe._graph is g_on and not torch.equal(second, graph)
        assert torch.equal(pipe(**kw, **_gens()).frames, graph)
        pipe.enable_free_noise(context_length=16, context_stride=4, noise_type="random")      # another initial noise, the same launches
        rnd = pipe(**kw, **_gens()).frames
        assert pipe._graph is g_on and len(pipe._graph_cache) == 1 and not torch.equal(rnd, graph)
        pipe.disable_free_noise()
        back = pipe(**kw, **_gens()).frames
        assert pipe._graph is not g_on and torch.equal(back, plain)
        never = pkg().I2VAdapterPipeline(unet=hu, scheduler=pkg().DDIMScheduler())(**kw, **_gens()).frames
        assert torch.equal(never, back)
    finally:
        hu.disable_free_noise()


def test_pipeline_noise_is_rescheduled_and_lcm_table_is_not(dev, small, monkeypatch):
    """the tensor handed to the first-frame prior is the rescheduled noise (every frame >= L a copy of a frame < L); LCM's per-step
    noise table is drawn as without FreeNoise"""
    p = pkg()
    _, hu = small
    pe, ne, cond = _problem(seed=9)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=24, num_inference_steps=3,
              guidance_scale=2.0)
    K = p.kernels
    prior_noise, tables = [], []
    real_prior = K.first_frame_prior
    monkeypatch.setattr(K, "first_frame_prior", lambda cond_, mask, noise, *a, **k: (prior_noise.append((mask.cpu(), noise.cpu())),
                                                                                     real_prior(cond_, mask, noise, *a, **k))[1])
    sched = p.LCMScheduler()
    real_table = sched.step_noise
    sched.step_noise = lambda *a, **k: (lambda t: (tables.append(None if t is None else t.cpu()), t)[1])(real_table(*a, **k))
    pipe = p.I2VAdapterPipeline(unet=hu, scheduler=sched)
    try:
        pipe(**kw, **_gens()).frames
        pipe.enable_free_noise(16, 4)
        pipe(**kw, **_gens()).frames
    finally:
        hu.disable_free_noise()
    (mask_off, noise_off), (mask_on, noise_on) = prior_noise
    assert torch.equal(mask_on, mask_off), "the mask draw covers all F frames, unchanged"
    want, src = R.ref_noise(tuple(noise_off.shape), 16, 4, "shuffle_context", 7)         # (_gens: the prior noise generator's seed)
    assert torch.equal(noise_on, want) and not torch.equal(noise_on, noise_off)
    assert all(any(torch.equal(noise_on[0, f], noise_on[0, k]) for k in range(16)) for f in range(16, 24))
    assert tables[0] is not None and torch.equal(tables[0], tables[1]), "LCM's noise table is not rescheduled"
    tab = tables[1]
    assert not any(torch.equal(tab[0, 0, f], tab[0, 0, k]) for f in range(16, 24) for k in range(16))


def test_free_init_with_free_noise_beyond_32_frames_raises_before_any_launch(dev, small, monkeypatch):
    p = pkg()
    _, hu = small
    pe, ne, cond = _problem(seed=3)
    pipe = p.I2VAdapterPipeline(unet=hu, scheduler=p.DDIMScheduler())
    pipe.enable_free_noise(16, 4)
    pipe.enable_free_init(num_iters=2)

    def boom(*a, **k):
        raise AssertionError("a kernel was launched")
    try:
        with monkeypatch.context() as mp:
            for name in ("first_frame_prior", "gemm", "conv3x3", "freenoise_gather", "freeinit_mix"):
                mp.setattr(p.kernels, name, boom)
            with pytest.raises(ValueError, match="32 x 128 x 128"):
                pipe(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=40, num_inference_steps=2,
                     guidance_scale=7.5, **_gens())
            with pytest.raises(ValueError, match="below `context_length`"):
                pipe(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, num_frames=8, num_inference_steps=2,
                     guidance_scale=7.5, **_gens())
    finally:
        hu.disable_free_noise()
