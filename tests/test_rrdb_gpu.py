"""RRDBNet (Real-ESRGAN x4plus) on the GPU against tests/rrdb_reference.py.

* i2v_conv3x3_dense_f16: every case of DENSE_CASES (sizes x cin x {in-place grow, close, close of an RRDB apart / in place} x pixel
  strides 192 / 200) against the fp64 launch with its per-element bound, inside NaN-poisoned buffers with guard rows: channels >= cin
  hold NaN before the launch (the kernel reads none of them), channels < cin are bit-unchanged after it, everything outside the written
  channels is still NaN.  The multi-tile walk bit for bit, and the argument errors.  tests/test_rrdb.py shows that the bound rejects
  the wrong evaluations of every case.
* i2v_conv3x3_c64_up2_prelu_f16 against fp64 and, bit for bit, against the PReLU launch on a repeat-interleaved input; conv_last's route;
  i2v_rgb_exit_f32 against fp64 between NaN guards.
* the model: teacher-forced (every launch against its layer's bound given the launch's own input), the launch count, end to end against
  the fp32 restatement with the fp16-storage variant as the yardstick, batch = frames bit for bit.
* the pipeline and the driver.
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import gemm_bounds as B
from tests import rrdb_reference as R
from tests import srvgg_reference as S
from tests import taesd_reference as T

pytestmark = pytest.mark.gpu
GUARD = 24       # guard pixels on either side of a token-major buffer
f16 = torch.float16
NAN = float("nan")


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def K():
    return pkg().kernels


def _buffer(n_pix, ld, dev):
    return torch.full((n_pix + 2 * GUARD, ld), NAN, dtype=f16, device=dev)


def _view(buf, shape, c0=0):
    n, h, w, c = shape
    return buf[GUARD: GUARD + n * h * w, c0: c0 + c].view(n, h, w, c)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _nan_except(buf, n_pix, c0, c1):
    """everything but channels c0 .. c1 - 1 of the inner pixels is NaN, and those hold none"""
    inner = buf[GUARD: GUARD + n_pix]
    return (bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n_pix:]).all()) and bool(torch.isnan(inner[:, :c0]).all())
            and bool(torch.isnan(inner[:, c1:]).all()) and not bool(torch.isnan(inner[:, c0:c1]).any()))


# ------------------------------------------------------------------------------------------------------------- the dense launch
@functools.lru_cache(maxsize=None)
def _dense_ref(key):
    """the reference of a case, shared by the strides (the reference does not depend on them); read-only"""
    return R.dense_case_inputs(key) + R.dense_case_reference(key)


def _in_place(case):
    """the 32-channel configuration writes the buffer it reads, at channel offset cin -- where the buffer has the channels"""
    return case[2][1] == 32 and case[1] + 32 <= 192


def _dense_launch(case, dev, **kw):
    """the case inside poisoned buffers.  Returns (block buffer, its x view, out buffer or None, out view)"""
    (n, h, w), cin, (name, cout, slope, s1, r1, s2, r2), ld = case
    buf, wt, bias, res2, _, _ = _dense_ref(case[:3] + (R.DENSE_STRIDES[0],))
    k, npix = K(), n * h * w
    block = _buffer(npix, ld, dev)
    _view(block, (n, h, w, cin)).copy_(buf[..., :cin].to(dev))                 # channels >= cin and the padding stay NaN
    xv = _view(block, (n, h, w, 192))
    wp, b = k.pack_conv_dense(wt.to(dev)), bias.to(dev)
    if cout == 32:
        if _in_place(case):
            ov, obuf = _view(block, (n, h, w, 32), cin), None                 # in place, at channel offset cin
        else:
            obuf = _buffer(npix, ld - 160, dev)                               # 192 channels leave no room behind them: pixel stride 32 / 40
            ov = _view(obuf, (n, h, w, 32))
        assert bool(torch.isnan(ov).all())
        out = k.conv3x3_dense(xv, cin, wp, b, out=ov, slope=slope, **kw)
    else:
        obuf = _buffer(npix, ld - 128, dev)                                   # pixel stride 64 / 72
        ov = _view(obuf, (n, h, w, 64))
        own = _view(block, (n, h, w, 64)) if r1 else None
        res = None
        if r2 == "own":
            res = res2.to(dev)
        elif r2 == "out":
            ov.copy_(res2.to(dev))
            res = ov
        out = k.conv3x3_dense(xv, cin, wp, b, out=ov, slope=slope, s1=s1, r1=own, s2=s2, r2=res, **kw)
    assert out is ov
    return block, xv, obuf, ov


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=R.dense_case_id)
def test_dense_conv_obeys_the_bound_and_stays_inside_its_channels(dev, case):
    (n, h, w), cin, cfg, ld = case
    cout, npix = cfg[1], n * h * w
    buf, wt, bias, res2, ref, tol = _dense_ref(case[:3] + (R.DENSE_STRIDES[0],))
    block, xv, obuf, ov = _dense_launch(case, dev)
    got = ov.cpu()
    ex = B.excess(got, ref, tol)
    print(f"{R.dense_case_id(case)}: largest excess {float(ex.max()):.3e} (<= 0 passes), max |err| {float((got.double() - ref).abs().max()):.3e}")
    assert bool(torch.isfinite(got.float()).all())
    assert not bool((ex > 0).any()), f"{int((ex > 0).sum())}/{ex.numel()} elements miss the bound, largest excess {float(ex.max()):.3e}"
    # channels < cin are bit-unchanged; beyond what was written -- channels >= cin (+ 32 in place), the stride padding, the guard rows --
    # everything is still NaN
    assert torch.equal(_bits(xv[..., :cin].cpu()), _bits(buf[..., :cin]))
    assert _nan_except(block, npix, 0, cin + 32 if _in_place(case) else cin)
    if obuf is not None:
        assert _nan_except(obuf, npix, 0, cout)


@pytest.mark.parametrize("cfg", R.DENSE_CONFIGS, ids=[c[0] for c in R.DENSE_CONFIGS])
@pytest.mark.parametrize("cin", (64, 192))
def test_dense_multi_tile_walk_is_bit_equal(dev, cin, cfg):
    """(3, T_h + 1, T_w + 1) is 12 tiles (24 half-tiles at 64 output channels): max_workgroups 5 and 1, and a repeat, give the
    unconstrained launch's bits"""
    case = (R.DENSE_SIZES[-1], cin, cfg, 200)
    free = _dense_launch(case, dev)[3].clone()
    walk = _dense_launch(case, dev, max_workgroups=5)
    again = _dense_launch(case, dev, max_workgroups=5)[3]
    one = _dense_launch(case, dev, max_workgroups=1)[3]
    two = _dense_launch(case, dev, max_workgroups=2)[3]
    for other in (walk[3], again, one, two):
        assert torch.equal(_bits(other), _bits(free))
    assert _nan_except(walk[0], 3 * 17 * 17, 0, cin + 32 if _in_place(case) else cin)


def test_dense_bad_operands_are_the_librarys_argument_error(dev):
    k, E = K(), pkg().HipLibraryError
    block = torch.full((2, 16, 16, 192), 7.0, dtype=f16, device=dev)
    numel = 2 * 16 * 16 * 64
    flat = torch.full((numel + 64,), 7.0, dtype=f16, device=dev)
    other, shifted = flat[:numel].view(2, 16, 16, 64), flat[64:].view(2, 16, 16, 64)      # one pixel apart: overlapping, not the same
    w32 = k.pack_conv_dense(torch.zeros(32, 64, 3, 3, device=dev))
    w64 = k.pack_conv_dense(torch.zeros(64, 192, 3, 3, device=dev))
    b32 = torch.zeros(32, dtype=f16, device=dev)
    with pytest.raises(E, match=r"i2v_conv3x3_dense_f16: out overlaps channels 0\.\.63 of x"):
        k.conv3x3_dense(block, 64, w32, b32, out=block[..., 32:64])
    with pytest.raises(E, match=r"out overlaps channels 0\.\.63 of x"):
        k.conv3x3_dense(block, 64, w32, b32, out=block[..., 48:80])
    with pytest.raises(E, match=r"out overlaps channels 0\.\.191 of x"):
        k.conv3x3_dense(block, 192, w64, out=block[..., :64], slope=1.0)
    with pytest.raises(E, match="out overlaps r1 without being it"):
        k.conv3x3_dense(block, 192, w64, out=other, slope=1.0, r1=shifted)
    with pytest.raises(E, match="out overlaps r2 without being it"):
        k.conv3x3_dense(block, 192, w64, out=other, slope=1.0, r2=shifted)
    with pytest.raises(E, match="16-byte"):
        k.conv3x3_dense(block, 64, w32, b32, out=block[..., 68:100])
    with pytest.raises(E, match="ldx 196"):
        k.conv3x3_dense(torch.zeros((2, 16, 16, 196), dtype=f16, device=dev)[..., :192], 64, w32, b32, out=other[..., :32])
    with pytest.raises(ValueError, match="cin must be one of"):
        k.conv3x3_dense(block, 80, w32, b32, out=block[..., 80:112])
    with pytest.raises(ValueError, match="w_packed must be"):
        k.conv3x3_dense(block, 96, w32, b32, out=block[..., 96:128])
    with pytest.raises(ValueError, match="out must be"):
        k.conv3x3_dense(block, 64, w32, b32, out=block[..., 64:128])
    with pytest.raises(ValueError, match="max_workgroups"):
        k.conv3x3_dense(block, 64, w32, b32, out=block[..., 64:96], max_workgroups=0)
    torch.cuda.synchronize()
    assert bool((block == 7.0).all()) and bool((flat == 7.0).all())                      # nothing was launched


def test_exit_bad_operands_are_the_librarys_argument_error(dev):
    k, E = K(), pkg().HipLibraryError
    sentinel = torch.full((2, 3, 5, 7), 7.0, device=dev)
    narrow = torch.zeros(2 * 5 * 7 * 2 + 1, dtype=f16, device=dev).as_strided((2, 5, 7, 3), (70, 14, 2, 1))      # three channels, pixel stride 2
    with pytest.raises(E, match="ld 2 must be >= 3"):
        k.rgb_exit(narrow, out=sentinel)
    with pytest.raises(E, match="out overlaps y"):
        k.rgb_exit(sentinel.view(f16).view(-1)[: 2 * 5 * 7 * 3].view(2, 5, 7, 3), out=sentinel)
    with pytest.raises(ValueError, match="at least 3 channels"):
        k.rgb_exit(torch.zeros((2, 5, 7, 2), dtype=f16, device=dev), out=sentinel)
    with pytest.raises(ValueError, match="out must be"):
        k.rgb_exit(torch.zeros((2, 5, 7, 3), dtype=f16, device=dev), out=sentinel[:, :2])
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())


# ------------------------------------------------------------------------------------------------------------- the tail's launches
@pytest.mark.parametrize("case", R.UP2_CASES, ids=R.up2_case_id)
def test_up2_conv_obeys_the_bound_and_is_the_prelu_launch_on_the_upsampled_input(dev, case):
    (n, h, w), ldx, ldo = case
    x, wt, b = R.up2_case_inputs(case)
    ref, tol = R.up2_layer_fp64(x, wt, b)
    k = K()
    xbuf = _buffer(n * h * w, ldx, dev)
    xv = _view(xbuf, (n, h, w, 64))
    xv.copy_(x.to(dev))
    obuf = _buffer(4 * n * h * w, ldo, dev)
    ov = _view(obuf, (n, 2 * h, 2 * w, 64))
    wp, slope = k.pack_conv_c64(wt.to(dev)), torch.full((64,), R.LRELU, dtype=torch.float32, device=dev)
    assert k.conv3x3_c64_up2(xv, wp, b.to(dev), slope, out=ov) is ov
    got = ov.cpu()
    ex = B.excess(got, ref, tol)
    print(f"{R.up2_case_id(case)}: largest excess {float(ex.max()):.3e} (<= 0 passes)")
    assert bool(torch.isfinite(got.float()).all()) and not bool((ex > 0).any()), f"largest excess {float(ex.max()):.3e}"
    assert _nan_except(obuf, 4 * n * h * w, 0, 64) and _nan_except(xbuf, n * h * w, 0, 64)
    up = x.to(dev).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous()
    assert torch.equal(_bits(k.conv3x3_c64(up, wp, b.to(dev), slope=slope)), _bits(ov))
    assert torch.equal(_bits(k.conv3x3_c64_up2(xv, wp, b.to(dev), slope, max_workgroups=1)), _bits(ov))


def test_conv_last_takes_the_narrow_output_kernel(dev):
    from i2v_adapter_unofficial_amd.blocks import pack_conv3x3
    g = torch.Generator().manual_seed(9)
    wt = ((torch.rand((3, 64, 3, 3), generator=g) * 2 - 1) * (3.0 / 576) ** 0.5).half()
    b = torch.rand(3, generator=g).half()
    # conv_last runs at 4 H x 4 W: the halo-tile kernel takes images that are whole 8 x 16 tiles (H even, W a multiple of 4 -- every
    # size the VAE decodes to); any other size is `K.conv3x3`'s implicit-GEMM kernel, the same result within the same bound
    for shape, family in (((2, 16, 32), pkg()._lib.I2V_ROUTE_CONV_THIN), ((1, 36, 68), pkg()._lib.I2V_ROUTE_GENERIC)):
        x = torch.randn(shape + (64,), generator=g).half()
        got = K().conv3x3(x.to(dev), pack_conv3x3(wt.to(dev)), b.to(dev))
        assert K().last_gemm_route()["family"] == family, shape
        ref, tol = T.layer_fp64(x, wt, b)
        assert got.shape == shape + (3,) and not bool((B.excess(got.cpu(), ref, tol) > 0).any())


@pytest.mark.parametrize("case", R.EXIT_CASES, ids=R.exit_case_id)
def test_exit_obeys_the_bound_and_stays_inside_its_buffer(dev, case):
    (n, h, w), signed, ld = case
    y = R.exit_case_inputs(case)
    ref, tol = R.exit_fp64(y, True, signed)
    ybuf = _buffer(n * h * w, ld, dev)
    yv = _view(ybuf, (n, h, w, 3))
    yv.copy_(y.to(dev))
    numel, g = n * 3 * h * w, 64
    obuf = torch.full((g + numel + g,), NAN, dtype=torch.float32, device=dev)
    ov = obuf[g: g + numel].view(n, 3, h, w)
    assert K().rgb_exit(yv, clamp=True, signed_out=signed, out=ov) is ov
    got = ov.cpu()
    assert bool(torch.isfinite(got).all()) and bool(torch.isnan(obuf[:g]).all()) and bool(torch.isnan(obuf[g + numel:]).all())
    assert not bool(((got.double() - ref).abs() > tol).any())
    assert float(got.min()) == (-1.0 if signed else 0.0) and float(got.max()) == 1.0          # the clamp has work on both sides
    assert _nan_except(ybuf, n * h * w, 0, 3)
    free, _ = R.exit_fp64(y, False, False)
    assert torch.equal(K().rgb_exit(yv, clamp=False).cpu().double(), free)


# ------------------------------------------------------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _pair(num_block):
    ref = R.seeded_reference(num_block)
    hv = pkg().RRDBNet.from_pretrained(ref.state_dict())
    return ref, hv.to(torch.device("cuda:0"))


def _pad64(conv):
    w16, b16 = conv.weight.detach().half(), conv.bias.detach().half()
    return torch.nn.functional.pad(w16, (0, 0, 0, 0, 0, 64 - w16.shape[1])), b16


@pytest.mark.parametrize("case", R.TEACHER_CASES, ids=str)
def test_every_launch_binds_teacher_forced(dev, case):
    num_block, _ = case
    ref, hv = _pair(num_block)
    t = R.e2e_frames(case)
    hv._trace = []
    try:
        hv(t.to(dev), signed=True)
    finally:
        trace, hv._trace = hv._trace, None
    kinds = [e[1] for e in trace]
    assert len(trace) == 15 * num_block + pkg().upscaler.RRDB_TAIL_LAUNCHES
    assert kinds == ["prep", "c64"] + ["dense"] * (15 * num_block) + ["c64_res", "up2", "up2", "prelu", "last", "exit"]
    names = [e[0] for e in trace if e[1] == "dense"]
    assert names == [f"body.{i}.rdb{j}.conv{k}" for i in range(num_block) for j in (1, 2, 3) for k in range(1, 6)]
    for name, kind, x, y, extra in trace:
        x, y = x.cpu(), y.cpu()
        if kind == "prep":
            want = R.entry_map(x.double()).permute(0, 2, 3, 1)
            assert bool((y[..., 3:] == 0).all())
            y = y[..., :3]
            ex = (y.double() - want).abs() - ((2.0 ** -11 + 2.0 ** -23) * want.abs() + 2.0 ** -25)
        elif kind == "exit":
            want, tol = R.exit_fp64(x, True, True)
            ex = (y.double() - want).abs() - tol
        elif kind == "dense":
            conv = ref.get_submodule(name)
            k = int(name[-1])
            assert extra["cin"] == 64 + 32 * (k - 1) == conv.weight.shape[1]
            last, closing = k == 5, name.endswith("rdb3.conv5")
            assert (extra.get("slope"), extra.get("s1", 1.0), extra.get("s2", 1.0)) == ((1.0, 0.2, 0.2 if closing else 1.0) if last else (0.2, 1.0, 1.0))
            assert (extra.get("r1") is not None) == last and (extra.get("r2") is not None) == closing
            r1, r2 = (None if extra.get(q) is None else extra[q].cpu() for q in ("r1", "r2"))
            if last:
                assert torch.equal(r1, x[..., :64])                       # the block's own input
            want, tol = R.dense_layer_fp64(x, extra["cin"], conv.weight.detach().half(), conv.bias.detach().half(), extra["slope"],
                                           extra.get("s1", 1.0), r1, extra.get("s2", 1.0), r2)
            ex = B.excess(y, want, tol)
        elif kind == "up2":
            conv = ref.get_submodule(name)
            want, tol = R.up2_layer_fp64(x, conv.weight.detach().half(), conv.bias.detach().half())
            ex = B.excess(y, want, tol)
        elif kind == "last":
            conv = ref.get_submodule(name)
            want, tol = T.layer_fp64(x, conv.weight.detach().half(), conv.bias.detach().half())
            ex = B.excess(y, want, tol)
        else:
            w16, b16 = _pad64(ref.get_submodule(name))
            slope = torch.full((64,), R.LRELU) if kind == "prelu" else None
            want, tol = S.layer_fp64(x, w16, b16, slope, extra.cpu() if kind == "c64_res" else None)
            ex = B.excess(y, want, tol)
        assert tuple(y.shape) == tuple(want.shape), name
        assert bool(torch.isfinite(y.float()).all()) and not bool((ex > 0).any()), \
            f"{name} ({kind}) at {tuple(x.shape)}: {int((ex > 0).sum())}/{ex.numel()} elements miss the bound, largest excess {float(ex.max()):.3e}"


@pytest.mark.parametrize("case", R.E2E_CASES, ids=str)
def test_end_to_end_within_twice_the_fp16_storage_error(dev, case):
    """max-abs and rms error of the HIP model against the fp32 restatement on [-1, 1] outputs, each at most twice the yardstick: what
    the fp16-storage variant (fp64 accumulation) makes against the fp64 evaluation of the same network on the same input.  The
    summation order differs and ties round either way; a wrong slope, scale or channel is orders of magnitude above.  At most 10 %
    of the reference's outputs saturate, so the clamp cannot hide an error.
    Measured on one MI355X (HIP max / rms, yardstick max / rms): see DESIGN 4.19."""
    num_block, (n, h, w) = case
    ref, hv = _pair(num_block)
    t = R.e2e_frames(case)
    x = R.entry_map(t)
    with torch.no_grad():
        assert R.saturated_fraction(ref, x) <= 0.10
        exact = R.leave_map(ref(x), True)
        ref64 = R.seeded_reference(num_block).double()
        yard = R.leave_map(R.run_fp16_storage(ref, x, accumulate=torch.float64).double(), True) - R.leave_map(ref64(x.double()), True)
    got = hv(t.to(dev), signed=True).cpu()
    assert got.dtype == torch.float32 and got.shape == exact.shape == (n, 3, 4 * h, 4 * w)
    err = got - exact
    pairs = (float(err.abs().max()), float(err.pow(2).mean().sqrt())), (float(yard.abs().max()), float(yard.pow(2).mean().sqrt()))
    print(f"num_block {num_block} {(n, h, w)}: HIP vs fp32 max {pairs[0][0]:.3e} rms {pairs[0][1]:.3e}; fp16-storage vs fp64 "
          f"max {pairs[1][0]:.3e} rms {pairs[1][1]:.3e}")
    assert bool(torch.isfinite(got).all()) and float(got.min()) >= -1 and float(got.max()) <= 1
    assert pairs[0][0] <= 2 * pairs[1][0] and pairs[0][1] <= 2 * pairs[1][1], pairs


def test_a_batch_is_its_frames(dev):
    _, hv = _pair(2)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand((3, 3, 9, 17), generator=g) * 2 - 1).to(dev)
    whole = hv(x)
    for i in range(3):
        assert torch.equal(whole[i: i + 1], hv(x[i: i + 1])), i
    assert torch.equal(torch.cat([hv(x[:2]), hv(x[2:])]), whole)
    assert torch.equal(hv(x.half()), hv(x.half().float()))                   # an fp16 source is read as it is


# ------------------------------------------------------------------------------------------------------------- the pipeline
def _small_pipe(dev):
    from tests.parity import hip_unet_from_oracle, oracle_small_unet
    hv = pkg().AutoencoderTiny()
    hv.load_state_dict(T.seeded_reference(0).state_dict())
    return pkg().I2VAdapterPipeline(vae=hv.to(dev).eval(), unet=hip_unet_from_oracle(oracle_small_unet(), dev))


def _call_args():
    g = torch.Generator().manual_seed(3)
    h = lambda t: t.half().float()
    kw = dict(prompt_embeds=h(torch.randn(1, 7, 64, generator=g)), negative_prompt_embeds=h(torch.randn(1, 7, 64, generator=g)),
              condition_image_latents=h(torch.randn(1, 4, 8, 8, generator=g)), num_frames=3, num_inference_steps=2, guidance_scale=7.5,
              frame_similarity_sample_ratio=1.0)
    gens = lambda: dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                        prior_noise_generator=torch.Generator().manual_seed(7))
    return kw, gens


def test_pipeline_upscales_the_decoded_frames(dev):
    from tests.parity import host_threads
    host_threads()
    pipe = _small_pipe(dev)
    kw, gens = _call_args()
    plain = pipe(output_type="pt", **kw, **gens()).frames
    assert plain.shape == (1, 3, 3, 64, 64)
    model = pkg().RRDBNet.from_pretrained(R.seeded_reference(1).state_dict()).to(dev)
    pipe.enable_upscaler(model)
    assert pipe.upscaler_enabled and pipe._upscaler[0] is model
    up = pipe(output_type="pt", **kw, **gens()).frames
    assert up.shape == (1, 3, 3, 256, 256) and up.dtype == torch.float32 and bool(torch.isfinite(up).all())
    assert torch.equal(up, pipe.upscale_frames(plain)) and torch.equal(up[0], model(plain[0].to(dev), signed=True))
    assert float(up.min()) >= -1 and float(up.max()) <= 1
    with pytest.raises(ValueError, match="output_type='latent' with the upscaler enabled"):
        pipe(output_type="latent", **kw, **gens())
    pipe.enable_upscaler(R.seeded_reference(1).state_dict(), frames_per_batch=1)            # a state dict: an RRDBNet by its keys
    assert isinstance(pipe._upscaler[0], pkg().RRDBNet) and pipe._upscaler[0].device.type == "cuda"
    assert torch.equal(pipe(output_type="pt", **kw, **gens()).frames, up)
    pipe.enable_upscaler(model, frames_per_batch=2)
    assert torch.equal(pipe.upscale_frames(plain), up)
    pipe.enable_upscaler(model)
    pipe.enable_vae_slicing()
    assert torch.equal(pipe(output_type="pt", **kw, **gens()).frames, up)
    pipe.disable_vae_slicing()
    pipe.disable_upscaler()
    assert torch.equal(pipe(output_type="pt", **kw, **gens()).frames, plain)


def test_eval_driver_with_an_rrdbnet_upscaler(dev, tmp_path):
    """`--upscaler FILE` with a `save_pretrained` RRDBNet on a one-row CSV: the GIF is 4 x the size"""
    import PIL.Image
    from safetensors.torch import save_file
    import i2v_adapter_unofficial_amd as p
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    from i2v_adapter_unofficial_amd.pipeline_i2v_adapter import main
    root = str(tmp_path)
    ch = (32, 64, 128, 128)
    kw = dict(sample_size=8, block_out_channels=ch, attention_head_dim=4, norm_num_groups=8, cross_attention_dim=64)
    init_random_weights_(p.UNet2DConditionModel(**kw), seed=1).save_pretrained(os.path.join(root, "sd", "unet"))
    init_random_weights_(p.AutoencoderKL(block_out_channels=(32, 64, 64, 64), norm_num_groups=8), seed=2) \
        .save_pretrained(os.path.join(root, "sd", "vae"))
    p.DDIMScheduler().save_pretrained(os.path.join(root, "sd", "scheduler"))
    init_random_weights_(p.MotionAdapter(block_out_channels=ch, motion_num_attention_heads=4, motion_norm_num_groups=8),
                         seed=3).save_pretrained(os.path.join(root, "motion"))
    init_random_weights_(p.I2VAdapterModule(2, ch, 4), seed=4).save_pretrained(
        os.path.join(root, "checkpoint", "demo", "epoch_3", "i2v_adapter"))
    p.RRDBNet.from_pretrained(R.seeded_reference(1).state_dict()).save_pretrained(os.path.join(root, "x4plus-tiny.safetensors"))
    rs = np.random.RandomState(0)
    data = os.path.join(root, "data")
    os.makedirs(os.path.join(data, "images"))
    PIL.Image.fromarray((rs.rand(70, 90, 3) * 255).astype("uint8")).save(os.path.join(data, "images", "0.png"))
    with open(os.path.join(data, "eval.csv"), "w") as f:
        f.write('image_path,name\nimages/0.png,"a cat on a boat"\n')
    g = torch.Generator().manual_seed(5)
    save_file({"prompt_embeds": torch.randn(1, 7, 64, generator=g), "negative_prompt_embeds": torch.randn(1, 7, 64, generator=g)},
              os.path.join(root, "embeds.safetensors"))
    common = ["--task_name", "demo", "--checkpoint_epoch", "3", "--eval_data_path", os.path.join(data, "eval.csv"),
              "--embeds", os.path.join(root, "embeds.safetensors"), "--model_path", os.path.join(root, "sd"),
              "--motion_adapter_path", os.path.join(root, "motion"), "--checkpoint_root", os.path.join(root, "checkpoint"),
              "--samples_root", os.path.join(root, "samples"), "--num_frames", "3", "--num_inference_steps", "2"]
    assert main(common + ["--upscaler", os.path.join(root, "x4plus-tiny.safetensors")]) == 0
    out = PIL.Image.open(os.path.join(root, "samples", "demo", "epoch_3", "a cat on a boat.gif"))
    assert out.n_frames == 3 and out.size == (256, 256)
