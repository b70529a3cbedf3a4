"""EulerDiscreteScheduler and EulerAncestralDiscreteScheduler on the host (no GPU): the timestep and sigma tables against
tests/euler_reference.py, the coefficient table of `i2v_sigma_prep` / `i2v_euler_cfg_step` against the reference's `step`, the ancestral
noise table, configuration handling, the pipeline's and the driver's view of the schedulers, the ABI version and the C entry points'
argument checks.  The contract is diffusers 0.24's two classes as tests/euler_reference.py restates them."""
import ctypes as C
import json
import os
import re
import sys

import pytest
import torch

from tests.euler_reference import ReferenceEulerScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD15 = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SD15_JSON = {"_class_name": "PNDMScheduler", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085,
             "num_train_timesteps": 1000, "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None}


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def E(**kw):
    return pkg().EulerDiscreteScheduler(**kw)


def A(**kw):
    return pkg().EulerAncestralDiscreteScheduler(**kw)


def make(ancestral, **kw):
    return (A if ancestral else E)(**kw), ReferenceEulerScheduler(ancestral=ancestral, **kw)


# ------------------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("N", [1, 4, 25])
@pytest.mark.parametrize("spacing", ["linspace", "leading", "trailing"])
@pytest.mark.parametrize("beta_schedule", ["linear", "scaled_linear"])
@pytest.mark.parametrize("variant", ["euler", "euler_karras", "ancestral"])
def test_timesteps_and_sigmas_are_the_references(N, spacing, beta_schedule, variant):
    kw = dict(timestep_spacing=spacing, beta_schedule=beta_schedule, steps_offset=1 if spacing == "leading" else 0)
    if variant == "euler_karras":
        kw["use_karras_sigmas"] = True
    s, ref = make(variant == "ancestral", **kw)
    assert s.timesteps.dtype == torch.float32 and len(s.timesteps) == 1000 and s.sigmas[-1] == 0        # before set_timesteps
    assert s.init_noise_sigma == ref.init_noise_sigma
    s.set_timesteps(N)
    ref.set_timesteps(N)
    assert s.timesteps.dtype == torch.float32 and s.sigmas.dtype == torch.float32
    assert s.timesteps.shape == (N,) and s.sigmas.shape == (N + 1,) and s.num_inference_steps == N
    assert torch.equal(s.timesteps, ref.timesteps) and torch.equal(s.sigmas, ref.sigmas)
    assert s.init_noise_sigma == ref.init_noise_sigma
    top = float(s.sigmas.max())
    assert s.init_noise_sigma == (top if spacing != "leading" else (top ** 2 + 1) ** 0.5)
    x = torch.randn(2, 3, generator=torch.Generator().manual_seed(N))
    for t in s.timesteps:
        assert torch.equal(s.scale_model_input(x, t), ref.scale_model_input(x, t))
        ref.step_index = None
        assert torch.equal(s.add_noise(x, x + 1, t.repeat(2)), ref.add_noise(x, x + 1, t.repeat(2)))
        assert s.noise_level(t) == (1.0, float(s.sigmas[s.timesteps.tolist().index(float(t))]))


def test_hand_checked_anchors():
    """SD-1.5 betas, linspace: the schedule starts at the last training step, sigma there is sqrt((1 - abar_999) / abar_999) with
    abar_999 = 0.00466 (about 14.6), the list of sigmas ends in the appended 0, and interior timesteps are fractional whenever
    999 / (N - 1) is not whole -- N = 4 divides (999 = 3 * 333: 999, 666, 333, 0, checked as such), N = 5 does not (749.25, ...)."""
    for s in (E(**SD15), A(**SD15)):
        s.set_timesteps(4)
        assert s.timesteps[0] == 999 and s.timesteps.tolist() == [999.0, 666.0, 333.0, 0.0]
        assert 14.0 < float(s.sigmas[0]) < 15.5 and float(s.sigmas[-1]) == 0.0
        assert s.init_noise_sigma == float(s.sigmas[0]) and s.order == 1
        s.set_timesteps(5)
        assert s.timesteps.tolist() == [999.0, 749.25, 499.5, 249.75, 0.0]
        # an interpolated level lies between its neighbours' on the training schedule
        train = ((1 - s.alphas_cumprod) / s.alphas_cumprod) ** 0.5
        assert float(train[749]) < float(s.sigmas[1]) < float(train[750])
        s.set_timesteps(25)
        assert s.timesteps[0] == 999 and any(float(t) != int(t) for t in s.timesteps[1:-1])
        assert torch.all(s.sigmas[:-1] > s.sigmas[1:])
    k = E(use_karras_sigmas=True, **SD15)
    k.set_timesteps(5)
    e = E(**SD15)
    e.set_timesteps(5)
    # the ramp keeps the ends and is linear in sigma^(1/7): its middle entry is the mean of the ends' seventh roots, to the 7th power
    assert k.sigmas[0] == e.sigmas[0] and abs(float(k.sigmas[4]) - float(e.sigmas[4])) < 1e-6 and torch.all(k.sigmas[:-1] > k.sigmas[1:])
    mid = ((float(e.sigmas[0]) ** (1 / 7) + float(e.sigmas[4]) ** (1 / 7)) / 2) ** 7
    assert abs(float(k.sigmas[2]) - mid) < 1e-6 * mid
    assert abs(float(k.timesteps[0]) - 999) < 1e-3 and torch.all(k.timesteps[:-1] > k.timesteps[1:])


# ------------------------------------------------------------------------------------------------------------ coefficients
def _apply(row, x, eps, z):
    sigma, _, sigma_to, sigma_up = [float(v) for v in row]
    out = x + eps * (sigma_to - sigma)
    return out + sigma_up * z if sigma_up != 0.0 else out


@pytest.mark.parametrize("variant,N,start", [("euler", 4, 0), ("euler", 25, 0), ("euler", 8, 3), ("euler_karras", 5, 0), ("euler_karras", 8, 2),
                                             ("ancestral", 4, 0), ("ancestral", 25, 0), ("ancestral", 8, 3)])
@pytest.mark.parametrize("beta_schedule", ["scaled_linear", "linear"])
def test_rows_reproduce_the_reference_step(variant, N, start, beta_schedule):
    """every row applied in float64 to random x, eps and the reference's own draw z equals the reference's `step` to 1e-12 relative: the
    rows hold the fp32-rounded sigmas exactly (sigma, sigma_next) or float64 functions of them rounded to fp32 (sigma_down, sigma_up), so
    the comparison is made with the rows' float64 source, `_step_sigmas`; the fp32 table itself is within its own rounding (6e-8
    relative per entry) of that."""
    kw = dict(beta_schedule=beta_schedule, use_karras_sigmas=True) if variant == "euler_karras" else dict(beta_schedule=beta_schedule)
    s, ref = make(variant == "ancestral", **kw)
    s.set_timesteps(N)
    ref.set_timesteps(N)
    ts = s.timesteps[start:]
    tab = s.step_coefficients(ts, eta=0.7)                     # eta is ignored
    assert tab.shape == (N - start, 4) and tab.dtype == torch.float32 and torch.equal(tab, s.step_coefficients(ts))
    assert torch.equal(tab[:, 0], s.sigmas[start:-1])
    assert torch.equal(tab[:, 1], (1.0 / (s.sigmas[start:-1].double() ** 2 + 1).sqrt()).float())
    if variant == "ancestral":
        assert tab[-1, 2:].tolist() == [0.0, 0.0] and torch.all(tab[:-1, 3] > 0)
    else:
        assert torch.equal(tab[:, 2], s.sigmas[start + 1:]) and torch.all(tab[:, 3] == 0)
    g = torch.Generator().manual_seed(N + start)
    gz, gz_mine = torch.Generator().manual_seed(99), torch.Generator().manual_seed(99)
    for k, t in enumerate(ts):
        x = torch.randn(2, 257, generator=g, dtype=torch.float64)
        eps = torch.randn(2, 257, generator=g, dtype=torch.float64)
        want = ref.step(eps, t, x, eta=0.7, generator=gz)
        z = torch.randn(2, 257, generator=gz_mine, dtype=torch.float64) if variant == "ancestral" else None
        exact = s._step_sigmas(start + k)
        got = _apply([exact[0], 0.0, exact[1], exact[2]], x, eps, z)
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item(), k
        row = [float(v) for v in tab[k]]
        for a, b in zip((row[0], row[2], row[3]), exact):
            assert abs(a - b) <= 2.0 ** -24 * abs(b), (k, a, b)
    assert torch.equal(torch.randn(3, generator=gz), torch.randn(3, generator=gz_mine))      # the same number of draws: one per step


def test_the_host_step_is_the_references():
    for ancestral in (False, True):
        s, ref = make(ancestral, **SD15)
        s.set_timesteps(6)
        ref.set_timesteps(6)
        g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
        x = torch.randn(1, 2, 4, 3, 3, generator=torch.Generator().manual_seed(1))          # fp32: both draw their noise in it
        for t in s.timesteps:                        # every step from the reference's state: one step's roundings each
            y, mag = s.step(0.3 * x, t, x, generator=g2), x.abs().max().item()
            x = ref.step(0.3 * x, t, x, generator=g1)
            # a few fp32 roundings, differently ordered, at the size of the step's input (the update cancels most of it)
            assert (x - y).abs().max().item() <= 4 * 2.0 ** -24 * max(mag, x.abs().max().item())
        with pytest.raises(NotImplementedError, match="s_churn"):
            s.step(y, s.timesteps[0], y, s_churn=0.5)


def test_coefficients_take_a_tail_only():
    for s in (E(**SD15), A(**SD15)):
        s.set_timesteps(6)
        full = s.step_coefficients(s.timesteps)
        pipe = object.__new__(pkg().I2VAdapterPipeline)
        pipe.scheduler = s
        ts, n = pipe.get_timesteps(6, 0.9)                         # pipe:529-536: int(6 * 0.9) = 5 steps
        assert n == 5 and ts.tolist() == s.timesteps.tolist()[1:]
        assert torch.equal(s.step_coefficients(ts), full[1:])
        # fractional timesteps are compared as floats: 799.2 is in the list, 799 is not
        assert 799.0 < float(s.timesteps[1]) < 800.0
        for bad in ([998.0, 500.0], [999.0, 799.0], [float(s.timesteps[1]), float(s.timesteps[3])], [799.0], []):
            with pytest.raises(ValueError):
                s.step_coefficients(torch.tensor(bad, dtype=torch.float32))
        with pytest.raises(ValueError):
            s.noise_level(799)
        assert pipe._noise_level(ts[0]) == (1.0, float(s.sigmas[1])) == pipe._prior_level(ts[0])
        tab = pipe.renoise_table(ts)
        assert tab[0].tolist() == [1.0, 0.0] and torch.equal(tab[1:, 1], s.sigmas[2:-1]) and torch.all(tab[1:, 0] == 1)


# ------------------------------------------------------------------------------------------------------------ noise table
def test_step_noise_is_what_the_reference_draws_over_a_loop():
    s, ref = make(True, **SD15)
    s.set_timesteps(4)
    ref.set_timesteps(4)
    shape = (2, 3, 4, 5, 7)
    g_mine, g_ref = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    tab = s.step_noise(s.timesteps, shape, g_mine, "cpu")
    assert tab.shape == (4,) + shape and tab.dtype == torch.float32 and tab.is_contiguous()
    drawn, randn = [], ref.randn
    ref.randn = lambda *a: drawn.append(randn(*a)) or drawn[-1]          # what the reference's `step` draws, recorded
    x = torch.ones(shape)
    for t in ref.timesteps:
        x = ref.step(0.5 * x, t, x, generator=g_ref)
    assert len(drawn) == 4 and all(torch.equal(tab[k], drawn[k]) for k in range(4))               # the last step drew too
    assert torch.equal(g_mine.get_state(), g_ref.get_state())
    g = torch.Generator().manual_seed(11)
    for k in range(4):
        assert torch.equal(tab[k], torch.randn(shape, generator=g)), k
    # a tail of the list draws its own length
    assert s.step_noise(s.timesteps[1:], shape, torch.Generator().manual_seed(11), "cpu").shape[0] == 3
    assert s.step_noise(s.timesteps[3:], shape, None, "cpu").shape[0] == 1
    assert not hasattr(E(), "step_noise")


def test_step_noise_with_one_generator_per_sample():
    s, ref = make(True, **SD15)
    s.set_timesteps(6)
    ref.set_timesteps(6)
    shape = (2, 3, 4, 5, 7)
    gens = [torch.Generator().manual_seed(21), torch.Generator().manual_seed(22)]
    ref_gens = [torch.Generator().manual_seed(21), torch.Generator().manual_seed(22)]
    tab = s.step_noise(s.timesteps, shape, gens, "cpu")
    assert tab.shape == (6,) + shape
    for k in range(6):
        assert torch.equal(tab[k], ref.randn(shape, ref_gens, torch.float32)), k
    for a, b in zip(gens, ref_gens):
        assert torch.equal(a.get_state(), b.get_state())
    with pytest.raises(ValueError):
        s.step_noise(s.timesteps, shape, gens[:1], "cpu")


# ------------------------------------------------------------------------------------------------------------ configuration
def test_defaults_are_diffusers():
    common = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                  prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0)
    assert A().config == common
    assert E().config == dict(common, interpolation_type="linear", use_karras_sigmas=False)
    assert torch.equal(E().betas, torch.linspace(0.0001, 0.02, 1000))


@pytest.mark.parametrize("cls", ["EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler"])
@pytest.mark.parametrize("key,value", [("prediction_type", "v_prediction"), ("prediction_type", "sample"), ("trained_betas", [0.1, 0.2]),
                                       ("interpolation_type", "log_linear"), ("beta_schedule", "squaredcos_cap_v2"),
                                       ("timestep_spacing", "karras")])
def test_unsupported_options_raise(cls, key, value):
    if key == "interpolation_type" and cls == "EulerAncestralDiscreteScheduler":
        getattr(pkg(), cls)(**{key: value})           # not a key of the ancestral class: ignored like any unknown key
        return
    with pytest.raises(NotImplementedError, match=key):
        getattr(pkg(), cls)(**{key: value})


@pytest.mark.parametrize("cls", ["EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler"])
def test_from_config_of_other_schedulers(cls, tmp_path):
    p = pkg()
    K = getattr(p, cls)
    ddim = p.DDIMScheduler()
    s = K.from_config(ddim.config)
    assert type(s) is K and torch.equal(s.alphas_cumprod, ddim.alphas_cumprod)
    assert s.config["timestep_spacing"] == "linspace" and s.config["steps_offset"] == 1 and "clip_sample" not in s.config
    s.set_timesteps(4)
    assert s.timesteps.tolist() == [999.0, 666.0, 333.0, 0.0]
    for other in (p.DPMSolverMultistepScheduler(), p.LCMScheduler()):
        assert torch.equal(K.from_config(other.config).alphas_cumprod, ddim.alphas_cumprod)
    s = K.from_config(SD15_JSON, timestep_spacing="trailing")
    assert torch.equal(s.alphas_cumprod, ddim.alphas_cumprod) and "skip_prk_steps" not in s.config and "_class_name" not in s.config
    assert s.config["timestep_spacing"] == "trailing"
    os.makedirs(tmp_path / "scheduler")
    json.dump(SD15_JSON, open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    r = K.from_pretrained(str(tmp_path), subfolder="scheduler")
    assert type(r) is K and torch.equal(r.alphas_cumprod, ddim.alphas_cumprod) and r.config["steps_offset"] == 1
    # and back from its own config to the others
    assert torch.equal(p.DDIMScheduler.from_config(r.config).alphas_cumprod, ddim.alphas_cumprod)


def test_save_and_load_round_trip(tmp_path):
    p = pkg()
    for s in (E(use_karras_sigmas=True, timestep_spacing="trailing", **SD15), A(beta_schedule="linear", timestep_spacing="leading", steps_offset=1)):
        d = tmp_path / type(s).__name__
        s.save_pretrained(str(d / "scheduler"))
        cfg = json.load(open(d / "scheduler" / "scheduler_config.json"))
        assert cfg["_class_name"] == type(s).__name__
        r = type(s).from_pretrained(str(d), subfolder="scheduler")
        assert r.config == s.config
        r.set_timesteps(6)
        s.set_timesteps(6)
        assert torch.equal(r.timesteps, s.timesteps) and torch.equal(r.step_coefficients(r.timesteps), s.step_coefficients(s.timesteps))
    assert p.EulerDiscreteScheduler is p.blocks.EulerDiscreteScheduler
    assert p.EulerAncestralDiscreteScheduler is p.blocks.EulerAncestralDiscreteScheduler


# ------------------------------------------------------------------------------------------------------------ pipeline, driver
def test_the_pipeline_knows_the_schedulers():
    p = pkg()
    pipe = object.__new__(p.I2VAdapterPipeline)
    pipe.scheduler = E()
    assert pipe._scheduler_kind() == "euler"
    pipe.scheduler = A()
    assert pipe._scheduler_kind() == "euler_ancestral"
    # a foreign object that is merely named like them (diffusers' own class) is refused as before, with a pointer to the package's
    for name in ("EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler"):
        pipe.scheduler = type(name, (), {})()
        with pytest.raises(NotImplementedError, match="DDIMScheduler or DPMSolverMultistepScheduler") as e:
            pipe._scheduler_kind()
        assert "this package's own EulerDiscreteScheduler" in str(e.value)
    assert p.pipeline_i2v_adapter.UNSUPPORTED_SCHEDULERS == ("EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler",
                                                             "LMSDiscreteScheduler", "PNDMScheduler")
    pipe.scheduler = p.DDIMScheduler()
    assert pipe._scheduler_kind() == "ddim" and not hasattr(pipe.scheduler, "noise_level")
    a = float(pipe.scheduler.alphas_cumprod[500])
    assert pipe._prior_level(torch.tensor(500)) == (a ** 0.5, (1.0 - a) ** 0.5)


def test_the_c_handle_refuses_the_schedulers():
    p = pkg()
    pipe = object.__new__(p.I2VAdapterPipeline)
    pipe.controlnet = pipe.t2i_adapter = None
    for s in (E(), A()):
        pipe.scheduler = s
        with pytest.raises(NotImplementedError, match=type(s).__name__):
            p.handle.export_denoiser(pipe, "unused", num_frames=2, latent_height=8, latent_width=8)


def test_driver_builds_the_schedulers(tmp_path):
    p = pkg()
    os.makedirs(tmp_path / "scheduler")
    json.dump(dict(SD15_JSON, timestep_spacing="leading"), open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    drv = p.pipeline_i2v_adapter
    assert drv.SIGMA_SCHEDULERS == ("euler_discrete", "euler_ancestral")
    s = drv.load_scheduler(str(tmp_path), "euler_discrete")
    assert type(s) is p.EulerDiscreteScheduler and torch.equal(s.alphas_cumprod, p.DDIMScheduler().alphas_cumprod)
    assert s.config["timestep_spacing"] == "linspace" and s.config["steps_offset"] == 1 and s.config["use_karras_sigmas"] is False
    assert drv.load_scheduler(str(tmp_path), "euler_discrete", karras_sigmas=True).config["use_karras_sigmas"] is True
    s = drv.load_scheduler(str(tmp_path), "euler_ancestral")
    assert type(s) is p.EulerAncestralDiscreteScheduler and torch.equal(s.alphas_cumprod, p.DDIMScheduler().alphas_cumprod)
    assert s.config["timestep_spacing"] == "linspace" and s.config["steps_offset"] == 1
    with pytest.raises(ValueError, match="ddim, dpmsolver\\+\\+, lcm, euler_discrete, euler_ancestral"):
        drv.load_scheduler(str(tmp_path), "euler")


def test_the_driver_command_line(capsys):
    drv = pkg().pipeline_i2v_adapter
    parser = drv.build_parser()
    assert tuple(next(a.choices for a in parser._actions if a.dest == "sampler")) == drv.SIGMA_SCHEDULERS
    args = parser.parse_args(["--embeds", "e.safetensors"])
    assert args.sampler is None and args.karras_sigmas is False and args.scheduler == "ddim"
    args = parser.parse_args(["--embeds", "e.safetensors", "--sampler", "euler_discrete", "--karras_sigmas"])
    assert args.sampler == "euler_discrete" and args.karras_sigmas is True
    assert parser.parse_args(["--sampler", "euler_ancestral"]).sampler == "euler_ancestral"
    assert drv.main(["--embeds", "e.safetensors", "--sampler", "euler_ancestral"]) == -1                  # parsed; no --task_name
    assert drv.main(["--task_name", "t", "--embeds", "e.safetensors", "--sampler", "euler_ancestral", "--karras_sigmas"]) == -1
    for bad in (["--sampler", "euler"], ["--scheduler", "euler"]):
        with pytest.raises(SystemExit):
            drv.main(["--embeds", "e.safetensors"] + bad)
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------ no GPU needed
@pytest.fixture(scope="module")
def lib():
    p = pkg()
    if not os.path.exists(p._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return p._lib


def test_abi_version_and_symbols(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 29
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for name in ("i2v_sigma_prep", "i2v_euler_cfg_step"):
        assert hasattr(h, name) and name in lib.SIGNATURES and name in src
    from i2v_adapter_unofficial_amd import kernels, profiling
    assert callable(kernels.sigma_prep) and callable(kernels.euler_cfg_step)
    assert "sigma_prep" in profiling._WRAPPED and "euler_cfg_step" in profiling._WRAPPED


def test_entry_points_reject_bad_arguments_without_a_gpu(lib):
    h = lib.load()
    buf = (C.c_float * 64)()
    idx = (C.c_int32 * 1)()
    ptr, iptr = C.cast(buf, C.c_void_p), C.cast(idx, C.c_void_p)
    #       latents noise n_noise np  f32 ld coef n_steps step_index g    b  f  c  hw copies stream
    good = [ptr, ptr, 4, ptr, 1, 4, ptr, 4, iptr, 7.5, 1, 1, 4, 16, 2, None]
    bad_args = [(0, None), (3, None), (6, None), (8, None),      # NULL latents / noise_pred / coef / step_index
                (2, 3), (2, 0), (2, -1),                          # a table with fewer rows than steps
                (7, 0), (7, -2),                                  # n_steps
                (14, 0), (14, 3),                                 # cfg_copies
                (5, 3),                                           # ld_np < c
                (10, 0), (13, 0)]                                 # sizes
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert h.i2v_euler_cfg_step(*args) == -1, (i, bad)
        assert b"i2v_euler_cfg_step" in h.i2v_last_error(), (i, bad)
    #       latents cond model_in coef ld_coef n_steps step_index b  f  c  hw c_pad copies stream
    good = [ptr, ptr, ptr, ptr, 4, 4, iptr, 1, 1, 4, 16, 8, 2, None]
    bad_args = [(0, None), (1, None), (2, None), (3, None), (6, None),      # NULL pointers
                (4, 1), (4, 0),                                              # the scale is column 1
                (5, 0),                                                      # n_steps
                (7, 0), (10, 0), (11, 3),                                    # sizes; c_pad < c
                (12, 0), (12, 3)]                                            # cfg_copies
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert h.i2v_sigma_prep(*args) == -1, (i, bad)
        assert b"i2v_sigma_prep" in h.i2v_last_error(), (i, bad)
