"""FreeInit without a GPU: the low-pass table against the triple-loop formula, the reference's own sanity checks (tests/freeinit_reference.py
is what the GPU tests hold the kernel to), `enable_free_init`'s arguments, the fast-sampling step counts, the driver's flags and the C
entry points' argument checks through ctypes (no launch)."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from tests import freeinit_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(16, 64, 64), (3, 5, 7), (8, 12, 10), (1, 8, 8)]
METHODS = ["butterworth", "gaussian", "ideal"]
STOPS = [(0.25, 0.25), (0.5, 0.1)]


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


@pytest.mark.parametrize("stops", STOPS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES)
def test_filter_equals_the_triple_loop(shape, method, stops):
    d_s, d_t = stops
    got = pkg().free_init.free_init_filter(shape, method, 4, d_s, d_t)
    want = R.reference_filter(shape, method, 4, d_s, d_t).to(torch.float32)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == shape
    assert torch.equal(got, want), (got - want).abs().max().item()
    if method == "ideal":
        assert set(got.unique().tolist()) <= {0.0, 1.0}
        if not any(v % 2 for v in shape):      # (an odd axis has no bin at distance 0: 2 t / F - 1 != 0 for every t)
            assert got[shape[0] // 2, shape[1] // 2, shape[2] // 2] == 1.0


def test_filter_order_zero_stops_and_bad_arguments():
    F = pkg().free_init.free_init_filter
    assert torch.equal(F((8, 12, 10), "butterworth", 2, 0.25, 0.25), R.reference_filter((8, 12, 10), "butterworth", 2, 0.25, 0.25).float())
    for d_s, d_t in ((0.0, 0.25), (0.25, 0.0), (0, 0)):
        for method in METHODS:
            z = F((3, 5, 7), method, 4, d_s, d_t)
            assert z.shape == (3, 5, 7) and z.dtype == torch.float32 and not z.any()
    assert F((3, 5, 7), "gaussian", 4, 0.25, 0.25) is F((3, 5, 7), "gaussian", 4, 0.25, 0.25)        # kept per (shape, parameters)
    with pytest.raises(ValueError):
        F((3, 5, 7), "box")
    with pytest.raises(ValueError):
        F((3, 5, 7), "ideal", 4, -0.1, 0.25)
    with pytest.raises(ValueError):
        F((0, 5, 7))


def _operands(shape, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g) for _ in range(3)]


@pytest.mark.parametrize("shape", [(1, 16, 4, 8, 8), (2, 3, 4, 5, 7), (1, 8, 4, 12, 10), (1, 1, 4, 8, 8)])
def test_reference_sanity(shape):
    """one-transform form == three-transform form; an all-ones table returns z_t, an all-zeros table z_rand; at an odd size the
    imaginary part the last step drops is not zero (the kernel's inverse has to be a complex one)"""
    lat, noise, zr = _operands(shape)
    sa, sb = 0.068, 0.998
    fhw = (shape[1], shape[3], shape[4])
    for method in METHODS:
        lpf = R.reference_filter(fhw, method)
        three = R.reference_mix(lat, noise, zr, lpf, sa, sb)
        one = R.reference_mix_one_transform(lat, noise, zr, lpf, sa, sb)
        assert (three - one).abs().max().item() <= 1e-12
    z_t = R.add_noise(lat, noise, sa, sb)
    assert (R.reference_mix(lat, noise, zr, torch.ones(fhw), sa, sb) - z_t).abs().max().item() <= 1e-12
    assert (R.reference_mix(lat, noise, zr, torch.zeros(fhw), sa, sb) - zr.double()).abs().max().item() <= 1e-12
    if all(v % 2 for v in fhw):
        lpf = R.reference_filter(fhw, "butterworth")
        assert R.reference_mix_one_transform(lat, noise, zr, lpf, sa, sb, return_complex=True).imag.abs().max().item() > 1e-3


def _pipe():
    p = pkg()
    pipe = p.I2VAdapterPipeline.__new__(p.I2VAdapterPipeline)
    pipe._free_init = None
    return pipe


def test_enable_free_init_arguments():
    pipe = _pipe()
    assert pipe.free_init_enabled is False
    pipe.enable_free_init()
    assert pipe.free_init_enabled is True
    assert pipe._free_init == dict(num_iters=3, use_fast_sampling=False, method="butterworth", order=4, spatial_stop_frequency=0.25,
                                   temporal_stop_frequency=0.25)
    with pytest.raises(AttributeError):
        pipe.free_init_enabled = False
    for bad in (dict(num_iters=0), dict(num_iters=-1), dict(method="box"), dict(order=0), dict(spatial_stop_frequency=-0.1),
                dict(temporal_stop_frequency=-1.0)):
        with pytest.raises(ValueError):
            pipe.enable_free_init(**bad)
    assert pipe._free_init["num_iters"] == 3          # a refused call changes nothing
    pipe.enable_free_init(num_iters=2, use_fast_sampling=True, method="ideal", order=2, spatial_stop_frequency=0.5,
                          temporal_stop_frequency=0.1)
    assert pipe._free_init["method"] == "ideal" and pipe._free_init["use_fast_sampling"] is True
    pipe.disable_free_init()
    assert pipe.free_init_enabled is False and pipe._free_init is None
    import inspect
    sig = inspect.signature(pkg().I2VAdapterPipeline.enable_free_init)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:]] == [
        ("num_iters", 3), ("use_fast_sampling", False), ("method", "butterworth"), ("order", 4), ("spatial_stop_frequency", 0.25),
        ("temporal_stop_frequency", 0.25)]


def test_fast_sampling_step_counts():
    f = pkg().free_init.round_inference_steps
    assert [f(25, 3, i) for i in range(3)] == [8, 16, 25]
    assert [f(2, 3, i) for i in range(3)] == [1, 1, 2]
    assert [f(25, 1, 0)] == [25]
    assert [R.round_steps(25, 3, i) for i in range(3)] == [8, 16, 25]


def test_the_driver_flags():
    parser = pkg().pipeline_i2v_adapter.build_parser()
    a = parser.parse_args(["--embeds", "e.safetensors"])
    assert a.free_init is None and a.free_init_method == "butterworth" and a.free_init_fast is False
    assert parser.parse_args(["--embeds", "e.safetensors", "--free_init"]).free_init == 3
    a = parser.parse_args(["--embeds", "e.safetensors", "--free_init", "2", "--free_init_method", "gaussian", "--free_init_fast"])
    assert a.free_init == 2 and a.free_init_method == "gaussian" and a.free_init_fast is True


# ------------------------------------------------------------------------------------------------------------ the C entry points
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
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 15
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for name in ("i2v_freeinit_mix", "i2v_freeinit_workspace_bytes"):
        assert hasattr(h, name) and name in lib.SIGNATURES and name in src
    assert hasattr(pkg().kernels, "freeinit_mix")


def test_workspace_bytes_is_positive_and_monotone(lib):
    ws = lib.load().i2v_freeinit_workspace_bytes
    base = (1, 16, 4, 64, 64)
    assert ws(*base) >= 8 * 16 * 4 * 64 * 64
    for axis in range(5):
        prev = 0
        for v in (1, 2, 3, 5, 16, 31, 32):
            args = list(base)
            args[axis] = v
            cur = ws(*args)
            assert cur > prev, (axis, v, cur, prev)
            prev = cur
    for bad in ((1, 33, 4, 8, 8), (1, 4, 4, 129, 8), (1, 4, 4, 8, 129), (0, 4, 4, 8, 8), (1, 0, 4, 8, 8), (1, 4, 0, 8, 8),
                (1, 4, 4, 0, 8), (1, 4, 4, 8, -1), (2 ** 20, 32, 2 ** 11, 128, 128)):
        assert ws(*bad) == -1 and b"i2v_freeinit_workspace_bytes" in lib.load().i2v_last_error(), bad


def test_mix_rejects_bad_arguments_without_a_gpu(lib):
    h = lib.load()
    b, f, c, hh, ww = 1, 4, 2, 8, 8
    n = b * f * c * hh * ww
    need = h.i2v_freeinit_workspace_bytes(b, f, c, hh, ww)
    bufs = [(C.c_float * n)() for _ in range(4)]                 # latents, init_noise, z_rand, out
    lpf = (C.c_float * (f * hh * ww))()
    ws = (C.c_double * (need // 8))()
    lat, noise, zr, out = (C.cast(x, C.c_void_p) for x in bufs)
    #       latents noise z_rand lpf                      out  workspace              bytes  b  f  c  h   w   sa     sb     stream
    good = [lat, noise, zr, C.cast(lpf, C.c_void_p), out, C.cast(ws, C.c_void_p), need, b, f, c, hh, ww, 0.068, 0.998, None]
    bad_args = [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None),       # NULL operands
                (8, 33), (10, 129), (11, 129),                                          # F, H, W beyond the limits
                (7, 0), (8, 0), (9, 0), (10, 0), (11, -3),                              # sizes
                (4, lat), (4, noise), (4, zr),                                          # out equal to an input
                (6, need - 1), (6, 0)]                                                  # a workspace one byte short
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert h.i2v_freeinit_mix(*args) == -1, (i, bad)
        assert b"i2v_freeinit_mix" in h.i2v_last_error(), (i, bad)
    args = list(good)
    args[5] = C.c_void_p(C.addressof(ws) + 4)                                           # a misaligned workspace
    args[6] = need + 8
    assert h.i2v_freeinit_mix(*args) == -1
    args = list(good)
    args[5], args[6] = out, 4 * n                                                       # (too small, and on top of out)
    assert h.i2v_freeinit_mix(*args) == -1
