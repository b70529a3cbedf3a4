"""Video-to-video and masked editing on the host: the new arguments and every refusal before anything is launched, the mask preparation
and the coefficient table against the restatement (tests/video2video_reference.py), the ABI of i2v_masked_renoise_f32 with its
host-side argument checks, the handle's refusal, the driver's flags -- and the error bound the GPU test holds the kernel to, shown
here to pass a faithful fp32 evaluation and to reject two wrong ones.  No kernel is launched."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import video2video_reference as R
from tests.parity import ROOT, SMALL_UNET


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _cpu_pipe(scheduler=None):
    p = pkg()
    return p.I2VAdapterPipeline(unet=p.UNetMotionCrossFrameAttnModel(**SMALL_UNET), scheduler=scheduler)


def _call(pipe, **kw):
    base = dict(condition_image_latents=torch.zeros(1, 4, 16, 16), num_frames=4, num_inference_steps=4, output_type="latent")
    return pipe(**{**base, **kw})


# ---------------------------------------------------------------------------------------------------------- the interface
def test_the_new_arguments_exist_and_default_to_none():
    sig = inspect.signature(pkg().I2VAdapterPipeline.__call__).parameters
    names = list(sig)
    assert names[-4:] == ["video", "video_latents", "strength", "mask_image"]          # after the existing arguments
    assert all(sig[n].default is None for n in names[-4:])
    assert sig["frame_similarity_sample_ratio"].default == 1 and sig["num_inference_steps"].default == 50
    for fn in ("encode_video", "prepare_video_latents", "prepare_mask_latents"):
        assert callable(getattr(pkg().I2VAdapterPipeline, fn))
    assert list(inspect.signature(pkg().I2VAdapterPipeline.encode_video).parameters) == ["self", "video", "height", "width", "generator"]


def test_every_refusal_is_raised_before_anything_is_launched():
    pipe = _cpu_pipe()                # no VAE, no text encoder, no GPU: anything behind the checks would raise something else
    clip, mask = torch.zeros(1, 4, 4, 16, 16), torch.ones(16, 16)
    frames = torch.zeros(4, 3, 128, 128)
    with pytest.raises(ValueError, match="both `video` and `video_latents`"):
        _call(pipe, video=frames, video_latents=clip)
    with pytest.raises(ValueError, match=r"holds 3 frames, `num_frames` is 4"):
        _call(pipe, video_latents=clip[:, :3])
    with pytest.raises(ValueError, match=r"holds 2 frames, `num_frames` is 4"):
        _call(pipe, video=frames[:2])
    with pytest.raises(ValueError, match=r"holds 1 frames, `num_frames` is 4"):
        _call(pipe, video=[object()])
    with pytest.raises(ValueError, match="`strength` = 0.5 was passed without a source clip"):
        _call(pipe, strength=0.5)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"strength should in \(0.0, 1.0\]"):
            _call(pipe, video_latents=clip, strength=bad)
    with pytest.raises(ValueError, match=r"strength parameter: 0.2, the number of pipeline steps is 0 which is < 1"):
        _call(pipe, video_latents=clip, strength=0.2)                                      # int(4 * 0.2) = 0
    with pytest.raises(ValueError, match="`frame_similarity_sample_ratio` = 0.9 with a source clip"):
        _call(pipe, video_latents=clip, frame_similarity_sample_ratio=0.9)
    with pytest.raises(ValueError, match="`mask_image` was passed without a source clip"):
        _call(pipe, mask_image=mask)
    with pytest.raises(ValueError, match="eta = 0.5 > 0"):
        _call(pipe, video_latents=clip, mask_image=mask, eta=0.5)
    with pytest.raises(ValueError, match="needs a `vae`"):
        _call(pipe, video=frames)
    pipe.enable_free_init(num_iters=2)
    with pytest.raises(ValueError, match="FreeInit is enabled"):
        _call(pipe, video_latents=clip)
    pipe.disable_free_init()
    # a valid call goes on: past the prompt check to the missing GPU
    with pytest.raises(ValueError, match="Provide either `prompt` or `prompt_embeds`"):
        _call(pipe, video_latents=clip, mask_image=mask)
    pe = torch.zeros(1, 7, 64)
    for kw in (dict(video_latents=clip), dict(video_latents=clip[:, :4].repeat(1, 2, 1, 1, 1), strength=1.0, mask_image=mask),
               dict(video_latents=clip, eta=0.5)):                                         # (eta without a mask is allowed)
        with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
            _call(pipe, prompt_embeds=pe, negative_prompt_embeds=pe, **kw)
    # under DPM-Solver++ and LCM `eta` is ignored, so a mask next to it is not refused
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        _call(_cpu_pipe(pkg().DPMSolverMultistepScheduler()), prompt_embeds=pe, negative_prompt_embeds=pe, video_latents=clip,
              mask_image=mask, eta=0.5)


def test_the_condition_defaults_to_the_sources_first_frame_and_strength_to_08():
    """host side of the call: without a condition image the first source frame is the condition, and `strength` None is 0.8"""
    pipe = _cpu_pipe()
    v, vl, s = pipe._check_video_args(None, torch.zeros(1, 6, 4, 8, 8), None, None, 4, 10, 1, 0.0)
    assert v is None and vl.shape[1] == 4 and s == 0.8                                     # frames beyond num_frames are dropped
    assert pipe._check_video_args(None, None, None, None, 4, 10, 0.9, 0.0) == (None, None, None)
    pe = torch.zeros(1, 7, 64)
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):                    # no "condition_image is required" error
        pipe(prompt_embeds=pe, negative_prompt_embeds=pe, video_latents=torch.zeros(1, 4, 4, 8, 8), num_frames=4, num_inference_steps=4)


# ---------------------------------------------------------------------------------------------------------- schedule and table
def _scheduler(kind):
    p = pkg()
    return {"ddim": p.DDIMScheduler, "dpmsolver++": p.DPMSolverMultistepScheduler, "lcm": p.LCMScheduler}[kind]()


@pytest.mark.parametrize("kind", ["ddim", "dpmsolver++", "lcm"])
@pytest.mark.parametrize("steps", [1, 2, 5])
def test_renoise_table_equals_the_reference(kind, steps):
    pipe = _cpu_pipe(_scheduler(kind))
    pipe.scheduler.set_timesteps(steps)
    ac = R.alphas_cumprod()
    assert torch.equal(pipe.scheduler.alphas_cumprod, ac)
    ts = pipe.scheduler.timesteps
    table = pipe.renoise_table(ts)
    assert table.dtype == torch.float32 and tuple(table.shape) == (steps, 2)
    assert torch.equal(table, R.renoise_table(ac, ts))
    assert table[0].tolist() == [1.0, 0.0]                                                 # the clean source after the last step
    for r in range(1, steps):
        want = pipe.scheduler.add_noise(torch.ones(1), torch.zeros(1), ts[r: r + 1]), pipe.scheduler.add_noise(torch.zeros(1), torch.ones(1), ts[r: r + 1])
        assert table[r].tolist() == [float(want[0]), float(want[1])]                       # add_noise's own coefficients of timesteps[r]
    # the tail that `strength` leaves: the table follows the executed timesteps
    for strength in (1.0, 0.8, 0.5):
        if int(steps * strength) < 1:
            continue
        tail, n = pipe.get_timesteps(steps, strength)
        want, n_ref = R.get_timesteps(ts, steps, strength)
        assert torch.equal(tail, want) and n == n_ref == len(tail) == min(int(steps * strength), steps)
        assert torch.equal(pipe.renoise_table(tail), R.renoise_table(ac, want))


# ---------------------------------------------------------------------------------------------------------- the mask
def _pil(arr):
    import PIL.Image
    return PIL.Image.fromarray((np.asarray(arr) * 255).round().astype("uint8"))


def test_prepare_mask_latents_equals_the_reference_for_every_form():
    pipe = _cpu_pipe()
    g = torch.Generator().manual_seed(3)
    B, Fr, H, W = 2, 3, 24, 40
    edge = torch.zeros(H, W)
    edge[:, :12] = 1.0                                    # the edge at column 12 falls inside the 8-pixel cell 8 .. 15
    soft = torch.rand(Fr, 1, H, W, generator=g)
    batch = torch.rand(B, Fr + 1, 1, H, W, generator=g)   # one frame too many: dropped
    small = torch.rand(B, Fr, 1, H // 8, W // 8, generator=g)          # already at the latent size: taken as it is, unbinarised
    other = torch.rand(50, 30, generator=g)               # another size: nearest to H x W first
    pil_one = _pil(torch.rand(31, 57, generator=g).numpy())            # resized (Lanczos) then binarised
    pil_rgb = _pil(torch.rand(H, W, 3, generator=g).numpy())           # converted to grey
    pil_list = [_pil(torch.rand(H, W, generator=g).numpy()) for _ in range(Fr)]
    for form in (edge, soft, batch, small, other, pil_one, pil_rgb, pil_list):
        got = pipe.prepare_mask_latents(form, B, Fr, H, W)
        want = R.prepare_mask(form, B, Fr, H, W)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, Fr, 1, 3, 5) and got.is_contiguous()
        assert torch.equal(got, want)
    got = pipe.prepare_mask_latents(edge, B, Fr, H, W)
    assert got[1, 2, 0].tolist() == [[1.0, 1.0, 0.0, 0.0, 0.0]] * 3                        # nearest takes pixels 0, 8, 16, 24, 32
    assert torch.equal(pipe.prepare_mask_latents(small, B, Fr, H, W), small)
    assert set(pipe.prepare_mask_latents(soft, B, Fr, H, W).unique().tolist()) <= {0.0, 1.0}
    with pytest.raises(ValueError, match="holds 2 frames, `num_frames` is 3"):
        pipe.prepare_mask_latents(soft[:2], B, Fr, H, W)
    with pytest.raises(ValueError, match=r"must be \[H, W\]"):
        pipe.prepare_mask_latents(torch.zeros(3, H, W), B, Fr, H, W)
    with pytest.raises(ValueError, match="does not match batch"):
        pipe.prepare_mask_latents(torch.zeros(3, Fr, 1, H, W), B, Fr, H, W)


# ---------------------------------------------------------------------------------------------------------- the bound
def _operands(shape=(3, 4, 35), seed=9):
    g = torch.Generator().manual_seed(seed)
    n, c, hw = shape
    l, s, z = (torch.randn(n, c, hw, generator=g) for _ in range(3))
    m = torch.rand(n, 1, hw, generator=g)
    return l, s, z, m


def test_the_kernels_bound_accepts_an_fp32_evaluation_and_rejects_two_wrong_ones():
    l, s, z, m = _operands()
    a, b = np.float32(0.8), np.float32(0.6)
    for good in (R.blend(l, s, z, m, float(a), float(b)),                                  # torch's fp32, unfused
                 torch.addcmul(m * l, 1 - m, torch.addcmul(float(a) * s, z, torch.tensor(float(b))))):
        worst, ok = R.check_blend(good, l, s, z, m, a, b)
        assert ok and worst <= 1.0, worst
    wrong_mask = R.blend(l, s, z, torch.roll(m, 1, dims=-1), float(a), float(b))           # the neighbouring pixel's mask
    wrong_row = R.blend(l, s, z, m, 0.6, 0.8)                                              # the next table row
    for wrong in (wrong_mask, wrong_row):
        worst, ok = R.check_blend(wrong, l, s, z, m, a, b)
        assert not ok and worst > 100, worst
    # the exact cases: m == 1 and m == 0 have a bound that allows no other value than the term itself
    ones, zeros = torch.ones_like(m), torch.zeros_like(m)
    assert R.check_blend(l, l, s, z, ones, a, b)[1] and not R.check_blend(l + 1e-6, l, s, z, ones, a, b)[1]
    assert R.check_blend(s, l, s, z, zeros, 1.0, 0.0)[1]


# ---------------------------------------------------------------------------------------------------------- ABI
def test_abi_26_declares_exports_and_binds_masked_renoise():
    lib = pkg()._lib
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 26
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    from i2v_adapter_unofficial_amd import handle as H
    name = "i2v_masked_renoise_f32"
    assert re.search(rf"\bint {name}\(", src) and name in lib.SIGNATURES and hasattr(h, name)
    assert name not in H.ENTRY_IDS                              # the C handle's plan format is unchanged: it refuses a mask
    assert len(lib.SIGNATURES[name][1]) == 11
    assert callable(pkg().kernels.masked_renoise)
    # the table's convention is promised where a caller reads it
    for text in (src, pkg().kernels.masked_renoise.__doc__, open(os.path.join(ROOT, "i2v-adapter-unofficial_amd", "csrc", "video2video.hip")).read()):
        assert "(1, 0)" in text and "wrap" in text


def test_masked_renoise_bad_arguments_are_refused_on_the_host():
    """I2V_ERR_INVALID_ARG before anything is launched: callable without a GPU (the pointers are never dereferenced)"""
    h = pkg()._lib.load()
    L, S, N, M, C, I = 1 << 40, 1 << 41, 1 << 42, 1 << 43, 1 << 44, (1 << 44) + 4096
    ok = dict(latents=L, source=S, noise=N, mask=M, coef=C, coef_rows=3, step_idx=I, images=3, channels=4, hw=35)
    nbytes, mbytes = 3 * 4 * 35 * 4, 3 * 35 * 4
    cases = [(dict(latents=None), b"null"), (dict(source=None), b"null"), (dict(noise=None), b"null"), (dict(mask=None), b"null"),
             (dict(coef=None), b"null"), (dict(step_idx=None), b"null"),
             (dict(images=0), b"images 0"), (dict(channels=0), b"channels 0"), (dict(hw=0), b"hw 0"), (dict(coef_rows=0), b"coef_rows 0"),
             (dict(images=-1), b"positive"), (dict(hw=-35), b"positive"),
             (dict(latents=L + 4), b"16-byte"), (dict(source=S + 8), b"16-byte"), (dict(noise=N + 12), b"16-byte"), (dict(mask=M + 4), b"16-byte"),
             (dict(coef=C + 2), b"4-byte"), (dict(step_idx=I + 1), b"4-byte"),
             (dict(source=L), b"overlaps"), (dict(source=L + nbytes - 16), b"overlaps"), (dict(noise=L - nbytes + 16), b"overlaps"),
             (dict(mask=L + nbytes - 16), b"overlaps"), (dict(mask=L - mbytes + 4), b"overlaps"),           # (its last 4 bytes)
             (dict(images=1 << 20, channels=4, hw=512), b"too large"), (dict(images=(1 << 31) - (1 << 19), channels=1, hw=1), b"too large"),
             (dict(images=1 << 40, channels=1 << 20, hw=1 << 20), b"too large")]
    for kw, msg in cases:
        args = tuple({**ok, **kw}.values())
        assert h.i2v_masked_renoise_f32(*args, None) == -1, kw
        assert msg in h.i2v_last_error(), (kw, h.i2v_last_error())


def test_masked_renoise_wrapper_refuses_host_tensors():
    z = torch.zeros(1, 2, 4, 4, 4)
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        pkg().kernels.masked_renoise(z, z.clone(), z.clone(), torch.zeros(1, 2, 1, 4, 4), torch.zeros(3, 2), torch.zeros(1, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------- refusals, driver
def test_the_c_handle_refuses_a_step_with_a_mask():
    from i2v_adapter_unofficial_amd import handle
    pipe = _cpu_pipe()
    st = dict(latents=torch.zeros(1, 4, 4, 16, 16), copies=2, ctx_text=torch.zeros(2, 7, 64, dtype=torch.float16), ctx_ip=None,
              v2v_mask=torch.zeros(1, 4, 1, 16, 16))
    for fn in (handle.record_step_plan, handle.record_prepare_plan):
        with pytest.raises(NotImplementedError, match=fn.__name__ + ".*mask"):
            fn(pipe, st)


def test_driver_flags():
    P = pkg().pipeline_i2v_adapter
    parser = P.build_parser()
    a = parser.parse_args(["--task_name", "t"])
    assert a.video_column is None and a.strength is None and a.mask_column is None
    a = parser.parse_args(["--task_name", "t", "--video_column", "clip", "--strength", "0.6", "--mask_column", "mask"])
    assert (a.video_column, a.strength, a.mask_column) == ("clip", 0.6, "mask")
    assert P.SCHEDULERS == ("ddim", "dpmsolver++") and P.STOCHASTIC_SCHEDULERS == ("lcm",)
    # a mask or a strength without a clip ends the driver before anything is loaded
    assert P.main(["--task_name", "t", "--mask_column", "mask"]) == -1
    assert P.main(["--task_name", "t", "--strength", "0.5"]) == -1


def test_load_mask_frames_one_image_or_a_clip(tmp_path):
    P = pkg().pipeline_i2v_adapter
    rs = np.random.RandomState(0)
    one = os.path.join(str(tmp_path), "one.png")
    _pil(rs.rand(16, 24)).save(one)
    m = P.load_mask_frames(one, 3)
    assert m.mode == "L" and m.size == (24, 16)
    folder = os.path.join(str(tmp_path), "masks")
    os.makedirs(folder)
    for j in range(4):
        _pil(rs.rand(16, 24)).save(os.path.join(folder, f"{j}.png"))
    frames = P.load_mask_frames(folder, 3)
    assert len(frames) == 3 and frames[0].size == (24, 16)
