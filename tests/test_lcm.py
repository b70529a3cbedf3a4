"""LCMScheduler on the host (no GPU): the timestep tables, the coefficient table of `i2v_lcm_cfg_step` against tests/lcm_reference.py,
the noise table, configuration handling, the pipeline's and the driver's view of the scheduler, the ABI version, the handle's entry id
and the C entry point's argument checks.  The contract is diffusers 0.24's LCMScheduler ("LCM")."""
import ctypes as C
import json
import os
import re
import sys

import pytest
import torch

from tests.lcm_reference import ReferenceLCMScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def S(**kw):
    return pkg().LCMScheduler(**kw)


# ------------------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("N,expected", [(3, [999, 679, 339]), (4, [999, 759, 499, 259]), (6, [999, 839, 679, 499, 339, 179]),
                                        (8, [999, 879, 759, 639, 499, 379, 259, 139])])
def test_timestep_tables(N, expected):
    s, ref = S(), ReferenceLCMScheduler()
    s.set_timesteps(N)
    ref.set_timesteps(N)
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == expected == ref.timesteps.tolist()
    assert s.num_inference_steps == N


def test_the_whole_origin_list_and_its_limits():
    s = S()
    s.set_timesteps(50)
    assert s.timesteps.tolist() == [20 * i - 1 for i in range(50, 0, -1)]
    with pytest.raises(ValueError):
        s.set_timesteps(51)
    with pytest.raises(ValueError):
        S(original_inference_steps=2000).set_timesteps(1001)
    s = S(original_inference_steps=1000)
    with pytest.raises(ValueError):
        s.set_timesteps(1001)


# ------------------------------------------------------------------------------------------------------------ coefficients
def _apply(row, x, eps, z):
    sa_t, sb_t, c_skip, c_out, sa_p, sb_p = [float(v) for v in row]
    x0 = (x - sb_t * eps) / sa_t
    den = c_out * x0 + c_skip * x
    out = sa_p * den
    return out + sb_p * z if sb_p != 0.0 else out


@pytest.mark.parametrize("N,start", [(4, 0), (8, 0), (8, 3)])
@pytest.mark.parametrize("beta_schedule", ["scaled_linear", "linear"])
def test_rows_agree_with_the_reference_step(N, start, beta_schedule):
    """every row applied in float64 to random x, eps and the reference's own draw z equals the reference's `step`: the rows are fp32,
    so 1e-6 relative is their rounding"""
    s, ref = S(beta_schedule=beta_schedule), ReferenceLCMScheduler(beta_schedule=beta_schedule)
    s.set_timesteps(N)
    ref.set_timesteps(N)
    ts = s.timesteps[start:]
    tab = s.step_coefficients(ts, eta=0.7)                     # eta is ignored
    assert tab.shape == (N - start, 6) and tab.dtype == torch.float32
    assert torch.equal(tab, s.step_coefficients(ts))
    assert tab[-1, 4:].tolist() == [1.0, 0.0] and torch.all(tab[:-1, 5] > 0)
    g = torch.Generator().manual_seed(N + start)
    gz, gz_mine = torch.Generator().manual_seed(99), torch.Generator().manual_seed(99)
    for k, t in enumerate(ts):
        x = torch.randn(2, 257, generator=g, dtype=torch.float64)
        eps = torch.randn(2, 257, generator=g, dtype=torch.float64)
        want = ref.step(eps, t, x, eta=0.7, generator=gz)
        z = torch.randn(2, 257, generator=gz_mine, dtype=torch.float64) if k < len(ts) - 1 else None
        got = _apply(tab[k], x, eps, z)
        assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item(), k
    assert torch.equal(torch.randn(3, generator=gz), torch.randn(3, generator=gz_mine))      # the last step drew nothing


def test_coefficients_take_a_tail_only():
    s = S()
    s.set_timesteps(6)
    full = s.step_coefficients(s.timesteps)
    pipe = object.__new__(pkg().I2VAdapterPipeline)
    pipe.scheduler = s
    ts, n = pipe.get_timesteps(6, 0.9)                         # pipe:529-536: int(6 * 0.9) = 5 steps
    assert n == 5 and ts.tolist() == s.timesteps.tolist()[1:]
    assert torch.equal(s.step_coefficients(ts), full[1:])
    for bad in ([998, 500], [999, 839], [839, 499], []):
        with pytest.raises(ValueError):
            s.step_coefficients(torch.tensor(bad, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------------------ noise table
def test_step_noise_is_the_sequence_of_per_step_draws():
    s = S()
    s.set_timesteps(4)
    shape = (2, 3, 4, 5, 7)
    tab = s.step_noise(s.timesteps, shape, torch.Generator().manual_seed(11), "cpu")
    assert tab.shape == (3,) + shape and tab.dtype == torch.float32 and tab.is_contiguous()
    g = torch.Generator().manual_seed(11)
    for k in range(3):
        assert torch.equal(tab[k], torch.randn(shape, generator=g)), k
    # a tail of the list draws one row fewer; a single step draws nothing
    assert s.step_noise(s.timesteps[1:], shape, torch.Generator().manual_seed(11), "cpu").shape[0] == 2
    g1 = torch.Generator().manual_seed(11)
    assert s.step_noise(s.timesteps[3:], shape, g1, "cpu") is None
    assert torch.equal(torch.randn(3, generator=g1), torch.randn(3, generator=torch.Generator().manual_seed(11)))
    s.set_timesteps(1)
    assert s.step_noise(s.timesteps, shape, None, "cpu") is None and s.step_coefficients(s.timesteps)[0, 4:].tolist() == [1.0, 0.0]


def test_step_noise_with_one_generator_per_sample():
    s = S()
    s.set_timesteps(6)
    shape = (2, 3, 4, 5, 7)
    gens = [torch.Generator().manual_seed(21), torch.Generator().manual_seed(22)]
    tab = s.step_noise(s.timesteps, shape, gens, "cpu")
    assert tab.shape == (5,) + shape
    for b, seed in enumerate((21, 22)):
        g = torch.Generator().manual_seed(seed)
        for k in range(5):
            assert torch.equal(tab[k, b], torch.randn((1,) + shape[1:], generator=g)[0]), (b, k)
    with pytest.raises(ValueError):
        s.step_noise(s.timesteps, shape, gens[:1], "cpu")


def test_the_table_is_the_stream_the_reference_step_draws():
    s, ref = S(), ReferenceLCMScheduler()
    s.set_timesteps(4)
    ref.set_timesteps(4)
    shape = (1, 2, 4, 3, 3)
    tab = s.step_noise(s.timesteps, shape, torch.Generator().manual_seed(5), "cpu")
    coef = s.step_coefficients(s.timesteps)
    g = torch.Generator().manual_seed(5)
    x = torch.ones(shape)
    for k, t in enumerate(ref.timesteps):
        eps = torch.full(shape, 0.5)
        want = ref.step(eps, t, x, generator=g)
        got = _apply(coef[k], x.double(), eps.double(), tab[k].double() if k < 3 else None)
        assert (got - want.double()).abs().max().item() <= 1e-5 * want.abs().max().item(), k
        x = want


# ------------------------------------------------------------------------------------------------------------ configuration
def test_defaults_are_diffusers():
    c = S().config
    want = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", original_inference_steps=50,
                timestep_scaling=10.0, prediction_type="epsilon", clip_sample=False, thresholding=False, set_alpha_to_one=True,
                steps_offset=0, timestep_spacing="leading", rescale_betas_zero_snr=False, trained_betas=None)
    assert c == want
    s = S()
    assert s.order == 1 and s.init_noise_sigma == 1.0
    x = torch.randn(2, 3)
    assert s.scale_model_input(x, 999) is x
    t = torch.tensor([999])
    assert torch.equal(s.add_noise(x, x, t), pkg().DDIMScheduler().add_noise(x, x, t))


@pytest.mark.parametrize("key,value", [("clip_sample", True), ("thresholding", True), ("prediction_type", "v_prediction"),
                                       ("prediction_type", "sample"), ("rescale_betas_zero_snr", True),
                                       ("trained_betas", [0.1, 0.2])])
def test_unsupported_options_raise(key, value):
    with pytest.raises(NotImplementedError, match=key):
        S(**{key: value})


def test_from_config_of_other_schedulers():
    p = pkg()
    ddim = p.DDIMScheduler()
    s = p.LCMScheduler.from_config(ddim.config)
    assert isinstance(s, p.LCMScheduler) and torch.equal(s.alphas_cumprod, ddim.alphas_cumprod)
    assert s.config["timestep_spacing"] == "linspace" and s.config["steps_offset"] == 1            # carried, not used
    s.set_timesteps(4)
    assert s.timesteps.tolist() == [999, 759, 499, 259]
    dpm = p.DPMSolverMultistepScheduler()
    assert torch.equal(p.LCMScheduler.from_config(dpm.config).alphas_cumprod, ddim.alphas_cumprod)
    sd15 = {"_class_name": "PNDMScheduler", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085,
            "num_train_timesteps": 1000, "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None}
    s = p.LCMScheduler.from_config(sd15, timestep_scaling=5.0)
    assert torch.equal(s.alphas_cumprod, ddim.alphas_cumprod) and s.timestep_scaling == 5.0 and "skip_prk_steps" not in s.config
    lin = p.LCMScheduler.from_config(dict(sd15, beta_schedule="linear"))                             # AnimateLCM's
    assert torch.equal(lin.betas, torch.linspace(0.00085, 0.012, 1000))


def test_save_and_load_round_trip(tmp_path):
    p = pkg()
    s = S(beta_schedule="linear", original_inference_steps=100, timestep_scaling=8.0)
    s.save_pretrained(str(tmp_path / "scheduler"))
    cfg = json.load(open(tmp_path / "scheduler" / "scheduler_config.json"))
    assert cfg["_class_name"] == "LCMScheduler" and cfg["original_inference_steps"] == 100
    r = p.LCMScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    assert r.config == s.config
    r.set_timesteps(6)
    s.set_timesteps(6)
    assert torch.equal(r.timesteps, s.timesteps) and torch.equal(r.step_coefficients(r.timesteps), s.step_coefficients(s.timesteps))


# ------------------------------------------------------------------------------------------------------------ pipeline, driver
def test_the_pipeline_knows_the_scheduler():
    p = pkg()
    pipe = object.__new__(p.I2VAdapterPipeline)
    pipe.scheduler = S()
    assert pipe._scheduler_kind() == "lcm"
    for name in ("EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler", "LMSDiscreteScheduler", "PNDMScheduler"):
        pipe.scheduler = type(name, (), {})()
        with pytest.raises(NotImplementedError, match="DDIMScheduler or DPMSolverMultistepScheduler"):
            pipe._scheduler_kind()
    pipe.scheduler = p.DDIMScheduler()
    assert pipe._scheduler_kind() == "ddim"
    pipe.scheduler = p.DPMSolverMultistepScheduler()
    assert pipe._scheduler_kind() == "dpmsolver++"


def test_driver_builds_the_lcm_scheduler(tmp_path):
    p = pkg()
    os.makedirs(tmp_path / "scheduler")
    json.dump({"_class_name": "PNDMScheduler", "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085,
               "num_train_timesteps": 1000, "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1,
               "timestep_spacing": "leading", "trained_betas": None}, open(tmp_path / "scheduler" / "scheduler_config.json", "w"))
    drv = p.pipeline_i2v_adapter
    s = drv.load_scheduler(str(tmp_path), "lcm")
    assert type(s) is p.LCMScheduler and torch.equal(s.alphas_cumprod, p.DDIMScheduler().alphas_cumprod)
    assert s.config["original_inference_steps"] == 50 and s.config["timestep_scaling"] == 10.0
    with pytest.raises(ValueError, match="ddim, dpmsolver\\+\\+, lcm"):
        drv.load_scheduler(str(tmp_path), "euler")
    assert drv.SCHEDULERS == ("ddim", "dpmsolver++") and drv.STOCHASTIC_SCHEDULERS == ("lcm",)


def test_the_driver_command_line(capsys):
    drv = pkg().pipeline_i2v_adapter
    parser = drv.build_parser()
    choices = next(a.choices for a in parser._actions if a.dest == "scheduler")
    assert tuple(choices) == ("ddim", "dpmsolver++", "lcm")
    args = parser.parse_args(["--embeds", "e.safetensors"])
    assert args.guidance_scale == 7.5 and args.scheduler == "ddim"
    args = parser.parse_args(["--embeds", "e.safetensors", "--scheduler", "lcm", "--guidance_scale", "1.5", "--num_inference_steps", "4"])
    assert args.scheduler == "lcm" and args.guidance_scale == 1.5
    assert drv.main(["--embeds", "e.safetensors", "--scheduler", "lcm", "--guidance_scale", "1"]) == -1      # parsed; no --task_name
    with pytest.raises(SystemExit):
        drv.main(["--embeds", "e.safetensors", "--scheduler", "euler"])
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


def test_abi_version_and_entry_id(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 14
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION and hasattr(h, "i2v_lcm_cfg_step")
    assert "i2v_lcm_cfg_step" in lib.SIGNATURES and "i2v_lcm_cfg_step" in src
    H = pkg().handle
    assert H.entry_id("i2v_lcm_cfg_step") == H.entry_id("i2v_freeu_f16") + 1
    assert H.entry_name(H.entry_id("i2v_lcm_cfg_step")) == "i2v_lcm_cfg_step" and "i2v_lcm_cfg_step" not in H.ENTRY_IDS
    assert H.STEP_NOISE == H.STEP_HISTORY == 4
    hip = open(os.path.join(ROOT, "i2v-adapter-unofficial_amd", "csrc", "handle.hip")).read()
    enum = re.search(r"enum Entry \{(.*?)\};", hip, re.S).group(1)
    names = [n.split("=")[0].strip() for n in re.sub(r"//[^\n]*", "", enum).split(",") if n.strip()]
    assert names.index("E_LCM_CFG_STEP") == H.entry_id("i2v_lcm_cfg_step") and names[-1] == "E_COUNT"
    from i2v_adapter_unofficial_amd import profiling
    assert "lcm_cfg_step" in profiling._WRAPPED


def test_lcm_step_rejects_bad_arguments_without_a_gpu(lib):
    h = lib.load()
    buf = (C.c_float * 64)()
    idx = (C.c_int32 * 1)()
    ptr = C.cast(buf, C.c_void_p)
    #       latents noise n_noise np  f32 ld coef n_steps step_index            g    b  f  c  hw copies stream
    good = [ptr, ptr, 3, ptr, 1, 4, ptr, 4, C.cast(idx, C.c_void_p), 7.5, 1, 1, 4, 16, 2, None]
    bad_args = [(0, None), (3, None), (6, None), (8, None),      # NULL latents / noise_pred / coef / step_index
                (1, None),                                        # NULL noise table with a 4-step schedule
                (2, 0), (2, -1),                                  # an empty table
                (7, 0), (7, -2),                                  # n_steps
                (14, 0), (14, 3),                                 # cfg_copies
                (5, 3),                                           # ld_np < c
                (10, 0), (13, 0)]                                 # sizes
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert h.i2v_lcm_cfg_step(*args) == -1, (i, bad)
        assert b"i2v_lcm_cfg_step" in h.i2v_last_error(), (i, bad)
    # (a NULL table with n_steps == 1 passes the checks: it is not tried here, where a launch has no device to go to)
