"""Multi-ControlNet on the host: the power of the kernel test's bounds (tests/test_multi_controlnet_gpu.py's header) to accept the fp32
restatement and to reject wrong evaluations, the entry point's argument errors, `MultiControlNetModel`'s constructor, folder names and
signature, and the pipeline's per-net arguments (lists, lengths, broadcasting, the [N, steps] table).  No kernel is launched."""
import ctypes as C
import os

import pytest
import torch

from tests import controlnet_reference as R
from tests import multi_controlnet_reference as M
from tests.parity import SMALL_UNET


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


# ---------------------------------------------------------------------------------------------------------- the bounds
@pytest.mark.parametrize("n_nets", [1, 2, 3, 4])
def test_kernel_bounds_accept_the_fp32_restatement_and_reject_wrong_evaluations(n_nets):
    skips, lows, sets = M.case(n_nets)
    for scales in M.SCALES[n_nets]:
        tab = M.table(scales)
        assert tuple(tab[:, M.ROW].tolist()) == scales and tab.shape == (n_nets, M.ROWS)
        wrong_row = tuple(tab[:, M.ROW - 1].tolist())
        live = [k for k, s in enumerate(scales) if s != 0.0]
        swapped = list(scales)
        if n_nets > 1:
            a, b = live[0], (live[0] + 1) % n_nets
            swapped[a], swapped[b] = swapped[b], swapped[a]
        worst = {False: 0.0, True: 0.0}
        for i, (hi, lo) in enumerate(zip(skips, lows)):
            ress = [s[i] for s in sets]
            for precise in (False, True):
                l = lo if precise else None
                ref, bnd = M.fp64(hi, ress, scales, l), M.bound(hi, ress, scales, l)
                for fma in (False, True):
                    ratio = ((M.restate(hi, ress, scales, l, fma=fma) - ref).abs() / bnd).max().item()
                    worst[precise] = max(worst[precise], ratio)
                    assert ratio <= 1.0, (i, scales, precise, fma, ratio)
                fails = lambda v: bool(((v - ref).abs() > bnd).any())
                tag = (i, scales, precise)
                assert fails(M.fp64(hi, ress, wrong_row, l)), ("neighbouring row",) + tag
                assert fails(M.fp64(hi, [R.neighbour_residual(sets[live[0]], i) if k == live[0] else r for k, r in enumerate(ress)],
                                    scales, l)), ("neighbouring tensor's residual",) + tag
                if n_nets > 1:
                    assert fails(M.fp64(hi, ress, swapped, l)), ("two nets' scales swapped",) + tag
                    dropped = [0.0 if k == live[-1] else s for k, s in enumerate(scales)]
                    assert fails(M.fp64(hi, ress, dropped, l)), ("one net dropped",) + tag
                if precise:
                    assert fails(M.fp64(hi, ress, scales, None)), ("dropped lo",) + tag
        print(f"N={n_nets} scales={scales}: fp32 restatement worst |err| / bound = {worst[False]:.4f} (default), {worst[True]:.4f} (pair)")


def test_restatement_with_one_net_is_the_single_net_evaluation():
    """N = 1 of the restatement is the expression tests/test_controlnet.py evaluates for i2v_add_residuals_f16, and its bounds are that
    test's bounds"""
    skips, lows, ress = R.kernel_case()
    for hi, lo, r in zip(skips, lows, ress):
        good32 = hi.float() + torch.tensor(-0.75) * r.float()
        assert torch.equal(M.restate(hi, [r], (-0.75,)), good32.half().double())
        for l in (None, lo):
            assert torch.equal(M.bound(hi, [r], (-0.75,), l), R.add_residuals_bound(hi, r, -0.75, l))
            assert torch.equal(M.fp64(hi, [r], (-0.75,), l), R.add_residuals_fp64(hi, r, -0.75, l))


# ---------------------------------------------------------------------------------------------------------- the entry point
def test_entry_point_argument_errors_without_a_gpu():
    """every refusal of include/i2v_hip.h's list: I2V_ERR_INVALID_ARG on the host, nothing launched (the addresses are never read)"""
    L = pkg()._lib
    h = L.load()
    assert L.ABI_VERSION >= 33 and L.I2V_ADD_RES_NETS_MAX == 4
    A, B, D, LO, T = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    top = ("n", "n_nets", "scale_rows", "scale_table", "step_idx")

    def call(res=(B,), **kw):
        q = L.AddMultiResidualsParams()
        e = q.t[0]
        e.dst, e.skip, e.numel = D, A, 16
        for k, r in enumerate(res):
            e.res[k] = r
        q.n, q.n_nets = 1, len(res)
        for k, v in kw.items():
            setattr(q if k in top else e, k, v)
        return h.i2v_add_multi_residuals_f16(C.byref(q), None)

    def refused(msg, *a, **kw):
        assert call(*a, **kw) == -1, (a, kw)
        assert msg in h.i2v_last_error(), (msg, h.i2v_last_error())

    assert h.i2v_add_multi_residuals_f16(None, None) == -1
    refused(b"n 0 outside", n=0)
    refused(b"n 17 outside", n=17)
    refused(b"n_nets 0 outside", n_nets=0)
    refused(b"n_nets 5 outside", n_nets=5)
    refused(b"null pointer", dst=None)
    refused(b"null pointer", skip=None)
    refused(b"null pointer (res[1]", res=(B, None))
    refused(b"null pointer (res[2]", res=(B, B + 64, None, B + 128))
    refused(b"positive multiple of 8", numel=12)
    refused(b"positive multiple of 8", numel=0)
    refused(b"positive multiple of 8", numel=-8)
    refused(b"16-byte aligned", skip=A + 2)
    refused(b"16-byte aligned", dst=D + 8)
    refused(b"16-byte aligned", res=(B, B + 4))
    refused(b"16-byte aligned", skip_lo=LO + 2, dst_lo=LO + 1024)
    refused(b"come together", skip_lo=LO)
    refused(b"come together", dst_lo=LO)
    refused(b"same memory", skip_lo=LO, dst_lo=D)
    refused(b"is its res", res=(B, D))
    refused(b"0 rows", scale_table=T, scale_rows=0)
    refused(b"4-byte aligned", scale_table=T + 2, scale_rows=3)
    refused(b"4-byte aligned", step_idx=T + 1)
    # the second tensor is checked like the first
    q = L.AddMultiResidualsParams()
    for j in range(2):
        q.t[j].dst, q.t[j].skip, q.t[j].numel = D + 64 * j, A + 64 * j, 16
        q.t[j].res[0] = B + 64 * j
    q.n, q.n_nets, q.t[1].numel = 2, 1, 20
    assert h.i2v_add_multi_residuals_f16(C.byref(q), None) == -1 and b"tensor 1 has 20 values" in h.i2v_last_error()


def test_wrapper_argument_errors_mirror_add_residuals():
    K = pkg().kernels
    a = torch.zeros(32, dtype=torch.float16)
    with pytest.raises(ValueError, match="0 residual sets"):
        K.add_multi_residuals([a], [])
    with pytest.raises(ValueError, match="5 residual sets"):
        K.add_multi_residuals([a], [[a]] * 5)
    with pytest.raises(ValueError, match="1 skip tensors and 2 residuals in set 1"):
        K.add_multi_residuals([a], [[a], [a, a]])
    with pytest.raises(ValueError, match="0 skip tensors"):
        K.add_multi_residuals([], [[]])
    with pytest.raises(ValueError, match="2 outputs for 1 skip"):
        K.add_multi_residuals([a], [[a]], out=[a, a])
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        K.add_multi_residuals([a], [[a], [a]])


# ---------------------------------------------------------------------------------------------------------- the model
def _net(seed, **kw):
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    return init_random_weights_(pkg().ControlNetModel(**R.small_config(), **kw), seed=seed)


def test_constructor_refusals_and_signature():
    p = pkg()
    a, b = _net(1), _net(2)
    with pytest.raises(ValueError, match="got 5"):
        p.MultiControlNetModel([a] * 5)
    with pytest.raises(ValueError, match="got 0"):
        p.MultiControlNetModel([])
    with pytest.raises(TypeError, match="entry 1 is a Linear"):
        p.MultiControlNetModel([a, torch.nn.Linear(2, 2)])
    with pytest.raises(TypeError, match="list of ControlNetModels"):
        p.MultiControlNetModel(a)
    m = p.MultiControlNetModel([a, b])
    assert isinstance(m.nets, torch.nn.ModuleList) and len(m.nets) == 2 and m.nets[0] is a and m.nets[1] is b
    assert m.weight_signature() == a.weight_signature() + b.weight_signature()
    before = m.weight_signature()
    with torch.no_grad():
        b.controlnet_mid_block.bias.add_(1.0)
    assert m.weight_signature() != before, "a change of the second net's weights must re-capture the step"
    with pytest.raises(NotImplementedError, match="guess_mode"):
        m(torch.zeros(2, 4, 16, 16), 1, torch.zeros(1, 7, 64), [torch.zeros(2, 3, 128, 128)] * 2, [1.0, 1.0], guess_mode=True)
    with pytest.raises(ValueError, match="3 entries for 2 ControlNets"):
        m(torch.zeros(2, 4, 16, 16), 1, torch.zeros(1, 7, 64), [torch.zeros(2, 3, 128, 128)] * 3, [1.0, 1.0])
    with pytest.raises(ValueError, match="1 entries for 2 ControlNets"):
        m(torch.zeros(2, 4, 16, 16), 1, torch.zeros(1, 7, 64), [torch.zeros(2, 3, 128, 128)] * 2, [1.0])


def test_save_and_load_use_diffusers_folder_names(tmp_path):
    p = pkg()
    nets = [_net(1), _net(2, conditioning_channels=1), _net(3)]
    root = os.path.join(str(tmp_path), "control")
    p.MultiControlNetModel(nets).save_pretrained(root)
    assert sorted(os.listdir(str(tmp_path))) == ["control", "control_1", "control_2"]
    back = p.MultiControlNetModel.from_pretrained(root)
    assert len(back.nets) == 3 and [n.config.conditioning_channels for n in back.nets] == [3, 1, 3]
    for mine, theirs in zip(nets, back.nets):
        a, b = mine.state_dict(), theirs.state_dict()
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    # reading stops at the first missing name
    os.rename(root + "_1", root + "_9")
    assert len(p.MultiControlNetModel.from_pretrained(root).nets) == 1
    with pytest.raises(ValueError, match="No ControlNets found"):
        p.MultiControlNetModel.from_pretrained(os.path.join(str(tmp_path), "absent"))


# ---------------------------------------------------------------------------------------------------------- the pipeline
def _cpu_pipe(n_nets=2, channels=(3, 3, 3, 3)):
    p = pkg()
    unet = p.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    nets = [p.ControlNetModel(**R.small_config(), conditioning_channels=channels[k]) for k in range(n_nets)]
    return p.I2VAdapterPipeline(unet=unet, controlnet=p.MultiControlNetModel(nets))


def test_pipeline_argument_errors_come_before_any_gpu_call():
    p = pkg()
    g = torch.Generator().manual_seed(0)
    kw = dict(prompt_embeds=torch.randn(1, 7, 64, generator=g), negative_prompt_embeds=torch.randn(1, 7, 64, generator=g),
              condition_image_latents=torch.randn(1, 4, 16, 16, generator=g), num_frames=2, num_inference_steps=3)
    frames = torch.rand(2, 3, 128, 128, generator=g)
    pipe = _cpu_pipe()
    with pytest.raises(ValueError, match="`control_image` is required"):
        pipe(**kw)
    with pytest.raises(ValueError, match="holds 1 entries, the pipeline has 2 ControlNets"):
        pipe(**kw, control_image=frames)
    with pytest.raises(ValueError, match="holds 3 entries, the pipeline has 2 ControlNets"):
        pipe(**kw, control_image=[frames] * 3)
    with pytest.raises(ValueError, match=r"`control_image\[1\]` holds 3 frames"):
        pipe(**kw, control_image=[frames, torch.rand(3, 3, 128, 128)])
    with pytest.raises(ValueError, match=r"`control_image\[0\]` has 1 channels"):
        pipe(**kw, control_image=[frames[:, :1], frames])
    for name in ("controlnet_conditioning_scale", "control_guidance_start", "control_guidance_end"):
        with pytest.raises(ValueError, match=f"`{name}` holds 3 values, the pipeline has 2 ControlNets"):
            pipe(**kw, control_image=[frames, frames], **{name: [0.1, 0.2, 0.3]})
    with pytest.raises(ValueError, match="start"):                       # each net's window is checked
        pipe(**kw, control_image=[frames, frames], control_guidance_start=[0.0, 0.6], control_guidance_end=0.5)
    with pytest.raises(NotImplementedError, match="guess_mode"):
        pipe(**kw, control_image=[frames, frames], guess_mode=True)
    with pytest.raises(NotImplementedError, match="list of ControlNets") as err:
        p.I2VAdapterPipeline(unet=pipe.unet, controlnet=list(pipe.controlnet.nets))
    assert "MultiControlNetModel([" in str(err.value)
    with pytest.raises(p.HipLibraryError, match="no CPU fallback"):      # only a valid call reaches the device
        pipe(**kw, control_image=[frames, frames], controlnet_conditioning_scale=[1.0, 0.5])
    # a 1-channel net beside a 3-channel one: each entry is checked against its own net
    mixed = _cpu_pipe(channels=(1, 3))
    with pytest.raises(ValueError, match=r"`control_image\[0\]` has 3 channels"):
        mixed(**kw, control_image=[frames, frames])
    with pytest.raises(p.HipLibraryError, match="no CPU fallback"):
        mixed(**kw, control_image=[frames[:, :1], frames])
    # the C handle refuses a Multi pipeline through the check it has
    from i2v_adapter_unofficial_amd import handle
    with pytest.raises(NotImplementedError, match="ControlNet"):
        handle.record_step_plan(pipe, {})


def test_control_image_preprocessing_per_net_channels():
    import numpy as np
    import PIL.Image
    pipe = _cpu_pipe(channels=(1, 3))
    rs = np.random.RandomState(0)
    imgs = [PIL.Image.fromarray((rs.rand(40, 56, 3) * 255).astype("uint8")) for _ in range(3)]
    one = pipe.prepare_control_image(imgs, 2, 3, 32, 48, 1)
    three = pipe.prepare_control_image(imgs, 2, 3, 32, 48, 3)
    assert one.shape == (6, 1, 32, 48) and three.shape == (6, 3, 32, 48) and torch.equal(one[:3], one[3:])
    assert 0.0 <= one.min().item() and one.max().item() <= 1.0 and one.mean().item() > 0.3
    assert torch.equal(three, pipe.prepare_control_image(imgs, 2, 3, 32, 48))
    f = torch.rand(3, 1, 32, 48)
    assert torch.equal(pipe.prepare_control_image(f, 2, 3, 32, 48, 1), torch.cat([f, f]))
    with pytest.raises(ValueError, match="has 3 channels"):
        pipe.prepare_control_image(torch.rand(3, 3, 32, 48), 1, 3, 32, 48, 1)


@pytest.mark.parametrize("scale,start,end", [(0.7, 0.0, 1.0), ([0.7, 0.2, 0.0], 0.25, 1.0), (0.7, [0.0, 0.1, 0.2], 0.9),
                                             ([1.0, 0.5, 0.25], [0.0, 0.1, 0.2], [0.5, 0.6, 1.0]), (1.0, 0.5, [0.75, 0.8, 1.0])])
def test_scale_and_window_broadcasting_is_diffusers(scale, start, end):
    pipe = _cpu_pipe(n_nets=3)
    want = list(zip(*M.diffusers_broadcast(3, scale, start, end)))
    assert list(pipe._control_args(scale, start, end)) == want


def test_scale_table_for_two_windows():
    """[N, steps]: net 0 on the first half at 0.5, net 1 on the second half at -2 (diffusers' controlnet_keep, per net)"""
    pipe = _cpu_pipe()
    st = dict(latents=torch.zeros(1), cn_cond=(torch.zeros(1), torch.zeros(1)),
              cn_args=pipe._control_args([0.5, -2.0], [0.0, 0.5], [0.5, 1.0]))
    timesteps = pipe.scheduler.set_timesteps(4) or pipe.scheduler.timesteps
    pipe._schedule_tables(st, timesteps, 0.0)
    assert st["cn_scale"].dtype == torch.float32 and st["cn_scale"].tolist() == [[0.5, 0.5, 0.0, 0.0], [0.0, 0.0, -2.0, -2.0]]
    # a single ControlNet keeps its vector
    p = pkg()
    single = p.I2VAdapterPipeline(unet=pipe.unet, controlnet=pipe.controlnet.nets[0], scheduler=pipe.scheduler)
    st = dict(latents=torch.zeros(1), cn_cond=torch.zeros(1), cn_args=single._control_args(0.5, 0.5, 1.0))
    single._schedule_tables(st, timesteps, 0.0)
    assert st["cn_scale"].tolist() == [0.0, 0.0, 0.5, 0.5]


def test_driver_flags_repeat():
    parser = pkg().pipeline_i2v_adapter.build_parser()
    a = parser.parse_args(["--task_name", "t", "--controlnet", "/m/pose", "--control_column", "pose", "--controlnet", "/m/depth",
                           "--control_column", "depth", "--controlnet_scale", "1.0", "0.5", "--control_guidance_end", "0.8"])
    assert (a.controlnet, a.control_column) == (["/m/pose", "/m/depth"], ["pose", "depth"])
    assert (a.controlnet_scale, a.control_guidance_start, a.control_guidance_end) == ([1.0, 0.5], 0.0, [0.8])
    main = pkg().pipeline_i2v_adapter.main
    assert main(["--task_name", "t", "--controlnet", "/m/pose", "--controlnet", "/m/depth", "--control_column", "pose"]) == -1
    assert main(["--task_name", "t", "--controlnet", "/m/pose", "--control_column", "pose", "--controlnet_scale", "1.0", "0.5"]) == -1
