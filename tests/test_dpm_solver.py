"""DPMSolverMultistepScheduler on the host (no GPU): the schedule, the per-step solver order, the coefficient table of
`i2v_dpm_cfg_step` (identities, and convergence of its order on a problem with a known answer), configuration handling, the
C entry point's argument checks and the evaluation driver's `--scheduler` helper.  The contract is diffusers 0.24.0's
DPMSolverMultistepScheduler for algorithm_type="dpmsolver++", solver_type="midpoint" (DESIGN.md "DPM-Solver++")."""
import ctypes as C
import json
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def S(**kw):
    return pkg().DPMSolverMultistepScheduler(**kw)


def table(N, **kw):
    s = S(**kw)
    s.set_timesteps(N)
    return s, s.step_coefficients(s.timesteps)


# ------------------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("N,last", [(20, 50), (25, 40)])
def test_linspace_schedule(N, last):
    s = S()
    s.set_timesteps(N)
    ts = s.timesteps.tolist()
    assert s.timesteps.dtype == torch.int64 and len(ts) == N
    assert ts[0] == 999 and ts[-1] == last
    assert all(a > b for a, b in zip(ts, ts[1:]))


def test_leading_and_trailing_schedules():
    s = S(timestep_spacing="leading")
    s.set_timesteps(20)                  # ratio 1000 // 21 = 47, entries 20 .. 1 of the 21-point grid, + steps_offset
    assert s.timesteps.tolist() == [47 * k + 1 for k in range(20, 0, -1)]
    s = S(timestep_spacing="trailing")
    s.set_timesteps(20)                  # 1000, 950, .., 50 minus one
    assert s.timesteps.tolist() == list(range(999, 0, -50))
    s.set_timesteps(3)                   # round(arange(1000, 0, -333.33)) - 1
    assert s.timesteps.tolist() == [999, 666, 332]


# ------------------------------------------------------------------------------------------------------------ order pattern
def test_order_pattern():
    _, t10 = table(10)
    assert t10[:, 5].tolist() == [1] + [2] * 8 + [1]          # lower_order_final: a list shorter than 15 ends first order
    _, t20 = table(20)
    assert t20[:, 5].tolist() == [1] + [2] * 19
    _, t1 = table(20, solver_order=1)
    assert t1[:, 5].tolist() == [1] * 20 and torch.all(t1[:, 4] == 0)
    assert torch.all(t10[t10[:, 5] == 1][:, 4] == 0)


def test_truncated_schedule_starts_first_order():
    """frame_similarity_sample_ratio 0.9 (pipe:529-536) at N = 10 starts the loop at full-list index 1: that step is the first
    executed, so first order; the rest are the full table's rows (the last still first order: lower_order_final counts the full list)"""
    p = pkg()
    s, full = table(10)
    pipe = object.__new__(p.I2VAdapterPipeline)
    pipe.scheduler = s
    ts, n = pipe.get_timesteps(10, 0.9)
    assert n == 9 and int(ts[0]) == int(s.timesteps[1])
    sub = s.step_coefficients(ts)
    assert sub.shape == (9, 6)
    assert sub[:, 5].tolist() == [1] + [2] * 7 + [1]
    ac = s.alphas_cumprod.double()
    assert sub[0, 0].item() == pytest.approx(float(ac[int(ts[0])]) ** 0.5, rel=1e-6)
    assert torch.equal(sub[1:], full[2:])
    with pytest.raises(ValueError):
        s.step_coefficients(torch.tensor([998, 500]))


# ------------------------------------------------------------------------------------------------------------ identities
def _apply(row, x, eps, x0_prev=None):
    a_s0, s_s0, ratio, c_cur, c_prev, order = [float(v) for v in row]
    x0 = (x - s_s0 * eps) / a_s0
    out = ratio * x + c_cur * x0
    if order > 1.5:
        out = out + c_prev * x0_prev
    return out, x0


def _ddim_target(ac, t_next, x, eps, t_now):
    """sqrt(a_next) x0 + sqrt(1 - a_next) eps: the deterministic DDIM step, which DPM-Solver++'s first-order step is"""
    a0 = float(ac[t_now])
    x0 = (x - (1 - a0) ** 0.5 * eps) / a0 ** 0.5
    a1 = float(ac[t_next])
    return a1 ** 0.5 * x0 + (1 - a1) ** 0.5 * eps


def test_first_order_row_is_the_ddim_step():
    s, tab = table(20, solver_order=1)
    ac = s.alphas_cumprod.double()
    g = torch.Generator().manual_seed(0)
    x, eps = torch.randn(4096, generator=g, dtype=torch.float64), torch.randn(4096, generator=g, dtype=torch.float64)
    ts = [int(t) for t in s.timesteps] + [0]           # the last step lands on alphas_cumprod[0]
    for k in range(20):
        got, _ = _apply(tab[k], x, eps)
        ref = _ddim_target(ac, ts[k + 1], x, eps, ts[k])
        assert (got - ref).abs().max().item() <= 2e-6 * ref.abs().max().item(), k
    # N = 10: the default solver's last row is first order and lands on alphas_cumprod[0] as well
    s, tab = table(10)
    last = [int(t) for t in s.timesteps][-1]
    got, _ = _apply(tab[-1], x, eps)
    ref = _ddim_target(s.alphas_cumprod.double(), 0, x, eps, last)
    assert (got - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()


def test_second_order_with_equal_history_is_first_order():
    s, tab = table(20)
    ac = s.alphas_cumprod.double()
    ts = [int(t) for t in s.timesteps] + [0]
    g = torch.Generator().manual_seed(1)
    x, eps = torch.randn(4096, generator=g, dtype=torch.float64), torch.randn(4096, generator=g, dtype=torch.float64)
    for k in range(1, 20):
        assert tab[k, 5] == 2
        x0 = (x - float(tab[k, 1]) * eps) / float(tab[k, 0])
        got, _ = _apply(tab[k], x, eps, x0_prev=x0)
        ref = _ddim_target(ac, ts[k + 1], x, eps, ts[k])
        assert (got - ref).abs().max().item() <= 2e-6 * ref.abs().max().item(), k


# ------------------------------------------------------------------------------------------------------------ convergence
def _gaussian_end_error(N, v, order):
    """1-D data ~ N(0, v): eps(x, t) = s_t x / (a_t^2 v + s_t^2) exactly, and the probability-flow ODE's solution is
    x_t = x_T sqrt(a_t^2 v + s_t^2) / sqrt(a_T^2 v + s_T^2).  The product's table applied in float64 from x_T = 1."""
    s, tab = table(N, solver_order=order)
    ac = s.alphas_cumprod.double()
    ts = [int(t) for t in s.timesteps]
    a_s = lambda t: (float(ac[t]) ** 0.5, (1 - float(ac[t])) ** 0.5)
    x, x0_prev = 1.0, float("nan")
    for k, t in enumerate(ts):
        a, sg = a_s(t)
        eps = sg * x / (a * a * v + sg * sg)
        x, x0_prev = _apply(tab[k], x, eps, x0_prev)
    (aT, sT), (a0, s0) = a_s(ts[0]), a_s(0)
    exact = math.sqrt(a0 * a0 * v + s0 * s0) / math.sqrt(aT * aT * v + sT * sT)
    return abs(x - exact)


@pytest.mark.parametrize("v", [1.0, 4.0])
def test_convergence_order_on_gaussian_data(v):
    e2 = [_gaussian_end_error(N, v, 2) for N in (20, 40, 80)]
    e1 = [_gaussian_end_error(N, v, 1) for N in (20, 40, 80)]
    r2 = [e2[i] / e2[i + 1] for i in range(2)]
    r1 = [e1[i] / e1[i + 1] for i in range(2)]
    print(f"v={v}: order 2 errors {e2} ratios {r2}; order 1 errors {e1} ratios {r1}")
    assert all(r >= 2.6 for r in r2), r2
    assert all(1.8 <= r <= 2.1 for r in r1), r1
    assert all(a < b for a, b in zip(e2, e1))


# ------------------------------------------------------------------------------------------------------------ configuration
def test_from_config_of_ddim_and_defaults():
    p = pkg()
    ddim = p.DDIMScheduler()
    s = p.DPMSolverMultistepScheduler.from_config(ddim.config)          # clip_sample / set_alpha_to_one: unknown here, ignored
    assert torch.equal(s.alphas_cumprod, ddim.alphas_cumprod)
    assert torch.equal(S().alphas_cumprod, ddim.alphas_cumprod)          # this repository's beta defaults, not diffusers'
    assert s.order == 1 and s.init_noise_sigma == 1.0
    x = torch.randn(2, 3)
    assert s.scale_model_input(x, 999) is x
    t = torch.tensor([999])
    assert torch.equal(s.add_noise(x, x, t), ddim.add_noise(x, x, t))
    # an SD-1.5 scheduler_config.json (PNDM's) loads, and DDIM gained the same constructor
    sd15 = {"_class_name": "PNDMScheduler", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085,
            "num_train_timesteps": 1000, "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None}
    assert torch.equal(p.DPMSolverMultistepScheduler.from_config(sd15).alphas_cumprod, ddim.alphas_cumprod)
    assert p.DDIMScheduler.from_config(sd15, timestep_spacing="leading").timestep_spacing == "leading"
    assert p.DPMSolverMultistepScheduler.from_config(ddim.config, solver_order=1).solver_order == 1


def test_save_and_load_round_trip(tmp_path):
    p = pkg()
    s = S(solver_order=1, timestep_spacing="trailing")
    s.save_pretrained(str(tmp_path / "scheduler"))
    cfg = json.load(open(tmp_path / "scheduler" / "scheduler_config.json"))
    assert cfg["_class_name"] == "DPMSolverMultistepScheduler" and cfg["lambda_min_clipped"] == -math.inf
    r = p.DPMSolverMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    assert r.config == s.config
    r.set_timesteps(12)
    s.set_timesteps(12)
    assert torch.equal(r.timesteps, s.timesteps) and torch.equal(r.step_coefficients(r.timesteps), s.step_coefficients(s.timesteps))


@pytest.mark.parametrize("key,value", [("algorithm_type", "dpmsolver"), ("algorithm_type", "sde-dpmsolver++"),
                                       ("solver_type", "heun"), ("solver_order", 3), ("prediction_type", "v_prediction"),
                                       ("lower_order_final", False), ("thresholding", True), ("use_karras_sigmas", True),
                                       ("timestep_spacing", "karras"), ("lambda_min_clipped", -5.1)])
def test_unsupported_options_raise(key, value):
    with pytest.raises(NotImplementedError, match=key):
        S(**{key: value})


def test_pipeline_names_the_supported_schedulers():
    p = pkg()
    pipe = object.__new__(p.I2VAdapterPipeline)
    for name in ("EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler", "LMSDiscreteScheduler", "PNDMScheduler"):
        pipe.scheduler = type(name, (), {})()
        with pytest.raises(NotImplementedError, match="DDIMScheduler or DPMSolverMultistepScheduler"):
            pipe._scheduler_kind()
    pipe.scheduler = S()
    assert pipe._scheduler_kind() == "dpmsolver++"
    pipe.scheduler = p.DDIMScheduler()
    assert pipe._scheduler_kind() == "ddim"


# ------------------------------------------------------------------------------------------------------------ no GPU needed
@pytest.fixture(scope="module")
def lib():
    p = pkg()
    if not os.path.exists(p._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return p._lib


def test_dpm_step_rejects_bad_arguments_without_a_gpu(lib):
    h = lib.load()
    buf = (C.c_float * 64)()
    idx = (C.c_int32 * 1)()
    ptr = C.cast(buf, C.c_void_p)
    good = [ptr, ptr, ptr, 1, 4, ptr, 4, C.cast(idx, C.c_void_p), 7.5, 1, 1, 4, 16, 2, None]
    for i, bad in [(1, None), (0, None), (4, 3), (6, 0), (9, 0), (13, 3)]:
        args = list(good)
        args[i] = bad
        assert h.i2v_dpm_cfg_step(*args) == -1, i
        assert b"i2v_dpm_cfg_step" in h.i2v_last_error()
    assert pkg().handle.ENTRY_IDS["i2v_dpm_cfg_step"] == len(pkg().handle.ENTRY_IDS) - 1


def test_driver_builds_the_dpm_scheduler(tmp_path):
    p = pkg()
    os.makedirs(tmp_path / "scheduler")
    json.dump({"_class_name": "PNDMScheduler", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085,
               "num_train_timesteps": 1000, "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 0,
               "timestep_spacing": "leading", "trained_betas": None}, open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    load = p.pipeline_i2v_adapter.load_scheduler
    s = load(str(tmp_path), "dpmsolver++")
    assert isinstance(s, p.DPMSolverMultistepScheduler)
    assert s.config["timestep_spacing"] == "linspace" and s.config["steps_offset"] == 1 and s.config["solver_order"] == 2
    d = load(str(tmp_path), "ddim")
    assert type(d) is p.DDIMScheduler and d.timestep_spacing == "linspace" and d.steps_offset == 1
    with pytest.raises(ValueError):
        load(str(tmp_path), "euler")
    assert p.pipeline_i2v_adapter.SCHEDULERS == ("ddim", "dpmsolver++")


@pytest.mark.parametrize("N,start", [(10, 1), (16, 1), (20, 0)])
def test_table_agrees_with_the_reference_solver(N, start):
    """the product's table (combined coefficients) against tests/dpm_reference.py (diffusers' D0 / D1 form) over a whole
    schedule with arbitrary model outputs, in float64"""
    from tests.dpm_reference import ReferenceDPMSolver
    s, ref = S(), ReferenceDPMSolver()
    s.set_timesteps(N)
    ref.set_timesteps(N)
    assert torch.equal(s.timesteps, ref.timesteps)
    ts = s.timesteps[start:]
    tab = s.step_coefficients(ts)
    g = torch.Generator().manual_seed(N)
    x = torch.randn(256, generator=g, dtype=torch.float64)
    xr, x0_prev = x.clone(), None
    for k, t in enumerate(ts):
        eps = torch.randn(256, generator=g, dtype=torch.float64)
        x, x0_prev = _apply(tab[k], x, eps, x0_prev)
        xr = ref.step(eps, t, xr)
        assert (x - xr).abs().max().item() <= 1e-5 * xr.abs().max().item(), k
