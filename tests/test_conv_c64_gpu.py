"""i2v_conv3x3_c64_f16 and i2v_taesd_prep_f16 on the GPU.

The convolution runs every case of tests/taesd_reference.py (CASES: four image sizes around the 8 x 16 tile x five epilogue / stride
configurations) against the fp64 layer with the per-element bound of tests/gemm_bounds.py -- K = 576, the residual's term, carried
through the 1-Lipschitz ReLU; tests/test_autoencoder_tiny.py shows that this bound rejects five wrong evaluations of every case.
Inputs and outputs are views with pixel strides 64 / 72 inside NaN-filled buffers with guard rows: everything the kernel does not own
must still be NaN afterwards."""
import functools

import pytest
import torch

from tests import gemm_bounds as B
from tests import taesd_reference as R

pytestmark = pytest.mark.gpu
GUARD = 24       # guard pixels on either side of a buffer


def K():
    import i2v_adapter_unofficial_amd as pkg
    return pkg.kernels


@functools.lru_cache(maxsize=None)
def _ref(case):
    x, w, b, r = R.case_inputs(case)
    _, (name, bias, relu_mid, relu_out, residual, ldx, ldo) = case
    return (x, w, b, r) + R.layer_fp64(x, w, b, r, relu_mid, relu_out)


def _strided(values, ld, dev, shape=None):
    """(NaN-filled buffer [GUARD + pixels + GUARD, ld], its [N, H, W, 64] view holding `values` (or uninitialised NaN))"""
    n, h, w, c = shape if values is None else values.shape
    buf = torch.full((n * h * w + 2 * GUARD, ld), float("nan"), dtype=torch.float16, device=dev)
    view = buf[GUARD: GUARD + n * h * w, :c].view(n, h, w, c)
    if values is not None:
        view.copy_(values.to(dev))
    return buf, view


def _outside_is_nan(buf, n_pix, c=64):
    inner = buf[GUARD: GUARD + n_pix]
    return (bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n_pix:]).all())
            and bool(torch.isnan(inner[:, c:]).all()) and not bool(torch.isnan(inner[:, :c]).any()))


def _launch(case, dev, **kw):
    (n, h, w), (name, bias, relu_mid, relu_out, residual, ldx, ldo) = case
    x, wt, b, r, ref, tol = _ref(case)
    xbuf, xv = _strided(x, ldx, dev)
    obuf, ov = _strided(r if residual == "out" else None, ldo, dev, shape=(n, h, w, 64))
    res = ov if residual == "out" else (r.to(dev) if residual else None)
    out = K().conv3x3_c64(xv, K().pack_conv_c64(wt.to(dev)), None if b is None else b.to(dev), relu_mid=relu_mid, relu_out=relu_out,
                          residual=res, out=ov, **kw)
    assert out is ov
    return xbuf, obuf, ov


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_conv_c64_obeys_the_bound_and_stays_inside_its_buffers(dev, case):
    (n, h, w), cfg = case
    x, wt, b, r, ref, tol = _ref(case)
    xbuf, obuf, ov = _launch(case, dev)
    got = ov.cpu()
    ex = B.excess(got, ref, tol)
    print(f"{R.case_id(case)}: largest excess {float(ex.max()):.3e} (<= 0 passes), max |err| {float((got.double() - ref).abs().max()):.3e}")
    assert bool(torch.isfinite(got.float()).all())
    assert not bool((ex > 0).any()), f"{int((ex > 0).sum())}/{ex.numel()} elements miss the bound, largest excess {float(ex.max()):.3e}"
    assert _outside_is_nan(obuf, n * h * w), "the kernel wrote outside its 64 channels / pixels, or left a NaN inside"
    assert _outside_is_nan(xbuf, n * h * w) and torch.equal(xbuf[GUARD: GUARD + n * h * w, :64].cpu().view(n, h, w, 64), x)


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=[c[0] for c in R.CONFIGS])
def test_multi_tile_walk_is_bit_equal(dev, cfg):
    """(3, 9, 17) is 12 tiles: with max_workgroups = 5 the workgroups take 3 and 2 tiles and the walk crosses image boundaries; the
    result must be the unconstrained launch's, and a repeat's, bit for bit"""
    case = ((3, 9, 17), cfg)
    free = _launch(case, dev)[2].clone()
    walk = _launch(case, dev, max_workgroups=5)
    again = _launch(case, dev, max_workgroups=5)[2]
    one = _launch(case, dev, max_workgroups=1)[2]
    assert torch.equal(walk[2], free) and torch.equal(again, free) and torch.equal(one, free)
    assert _outside_is_nan(walk[1], 3 * 9 * 17)
    ex = B.excess(walk[2].cpu(), *_ref(case)[4:])
    assert not bool((ex > 0).any())


def test_bad_operands_are_the_librarys_argument_error(dev):
    import i2v_adapter_unofficial_amd as pkg
    k = K()
    w = k.pack_conv_c64(torch.zeros(64, 64, 3, 3, device=dev))
    x = torch.zeros((2, 8, 16, 64), dtype=torch.float16, device=dev)
    sentinel = torch.full((2, 8, 16, 64), 7.0, dtype=torch.float16, device=dev)
    with pytest.raises(pkg.HipLibraryError, match="out overlaps x"):
        k.conv3x3_c64(x, w, out=x)
    mis = torch.zeros(2 * 8 * 16 * 64 + 8, dtype=torch.float16, device=dev)[4: 4 + 2 * 8 * 16 * 64].view(2, 8, 16, 64)
    with pytest.raises(pkg.HipLibraryError, match="16-byte"):
        k.conv3x3_c64(mis, w, out=sentinel)
    with pytest.raises(pkg.HipLibraryError, match="16-byte"):
        k.conv3x3_c64(x, w, out=mis)
    with pytest.raises(pkg.HipLibraryError, match="64 -> 64"):
        k.conv3x3_c64(torch.zeros((2, 8, 16, 32), dtype=torch.float16, device=dev), w)
    with pytest.raises(pkg.HipLibraryError, match="pixel strides"):
        k.conv3x3_c64(torch.zeros((2, 8, 16, 68), dtype=torch.float16, device=dev)[..., :64], w, out=sentinel)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())                      # nothing was launched


# ------------------------------------------------------------------------------------------------------------- the entry mover
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("f32", "f16"))
@pytest.mark.parametrize("shape", ((1, 3, 1, 1), (2, 4, 5, 3), (3, 3, 40, 24), (1, 64, 3, 5), (2, 13, 7, 9)), ids=str)
def test_taesd_prep(dev, shape, dtype):
    """identity and the padding zeros are exact.  The other two maps against fp64, per element:
        |got - ref| <= (2^-11 + e) |ref| + 2^-25
    2^-11 |ref| + 2^-25 is the one rounding to fp16 (2^-25: half a subnormal step); e is the fp32 arithmetic in front of it:
      unit   (v + 1) / 2: one rounded add (2^-24 relative), the halving is exact:                       e = 2^-23 (with slack for |ref|)
      clamp  3 tanh(v / 3): a correctly rounded division (2^-24, which tanh -- relative condition number x / (sinh x cosh x) <= 1 --
             does not amplify), tanhf within the 5 ulp OpenCL allows it (5 * 2^-23), a rounded product (2^-24):   e = 2^-20."""
    g = torch.Generator().manual_seed(shape[1] * 100 + shape[2])
    n, c, h, w = shape
    src = (torch.randn(shape, generator=g) * 2).to(dtype)
    src.view(-1)[0] = 0.0
    k = K()
    for mode, e in (("identity", 0.0), ("unit", 2.0 ** -23), ("clamp", 2.0 ** -20)):
        for ld in (64, 72):
            buf, view = _strided(None, ld, dev, shape=(n, h, w, 64))
            out = k.taesd_prep(src.to(dev), mode, out=view)
            assert out is view and _outside_is_nan(buf, n * h * w)
            got = view.cpu()
            assert bool((got[..., c:] == 0).all())
            x = src.double().permute(0, 2, 3, 1)
            if mode == "identity":
                assert torch.equal(got[..., :c], src.permute(0, 2, 3, 1).half())
                continue
            ref = (x + 1) / 2 if mode == "unit" else 3 * torch.tanh(x / 3)
            ex = (got[..., :c].double() - ref).abs() - ((2.0 ** -11 + e) * ref.abs() + 2.0 ** -25)
            assert not bool((ex > 0).any()), (mode, float(ex.max()))
