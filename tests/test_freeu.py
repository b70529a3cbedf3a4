"""FreeU without a GPU: the four-frequency form the HIP kernel implements equals diffusers' literal FFT form, the switches of the
product UNet / pipeline follow the reference (attributes on every up block, the truthiness rule), and `i2v_freeu_f16` validates its
arguments on the host."""
import ctypes as C
import os
import sys

import pytest
import torch

from tests.freeu_reference import SD15_FREEU, apply_freeu, fourier_filter, four_mode_filter, hook_oracle_unet
from tests.parity import SMALL_UNET, oracle_small_unet, small_unet_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


@pytest.mark.parametrize("hw", [(8, 8), (16, 16), (64, 32),            # powers of two
                                (12, 12), (24, 24), (6, 10),           # even, not powers of two
                                (9, 7), (5, 4), (5, 8), (3, 2), (2, 5), (7, 7),   # odd sizes (5 x 4, 9 x 7: 36 x 28 latents)
                                (2, 2)])
@pytest.mark.parametrize("scale", [0.2, 0.9, 1.0, 1.7])
def test_four_mode_form_equals_the_fft_form(hw, scale):
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    x = torch.randn(2, 3, *hw, generator=g, dtype=torch.float64)
    ref = fourier_filter(x, 1, scale)
    got = four_mode_filter(x, scale)
    assert ref.dtype == torch.float64 and (got - ref).abs().max().item() <= 1e-12
    if scale == 1.0:
        assert (ref - x).abs().max().item() <= 1e-12
    else:
        assert (ref - x).abs().max().item() > 1e-3


def test_the_identity_needs_two_rows_and_columns():
    """at H = 1 the reference's box slice starts at -1 and wraps: the closed form is a different function there, which is why the
    library refuses such planes instead of computing something"""
    x = torch.randn(1, 1, 1, 6, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    assert (four_mode_filter(x, 0.2) - fourier_filter(x, 1, 0.2)).abs().max().item() > 1e-3


def test_apply_freeu_scales_half_the_backbone_and_leaves_its_inputs():
    g = torch.Generator().manual_seed(1)
    hid, skip = torch.randn(2, 10, 4, 4, generator=g), torch.randn(2, 6, 4, 4, generator=g)
    h0, s0 = hid.clone(), skip.clone()
    for ridx, (b, s) in ((0, (1.2, 0.9)), (1, (1.4, 0.2))):
        ho, so = apply_freeu(ridx, hid, skip, **SD15_FREEU)
        assert torch.equal(ho[:, :5], hid[:, :5] * b) and torch.equal(ho[:, 5:], hid[:, 5:])
        assert torch.allclose(so, fourier_filter(skip, 1, s))
    ho, so = apply_freeu(2, hid, skip, **SD15_FREEU)
    assert ho is hid and so is skip and torch.equal(hid, h0) and torch.equal(skip, s0)


def test_hooked_oracle_changes_the_forward_and_unhooks():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ou = oracle_small_unet()
    inp = small_unet_inputs(b=1, f=2, hw=8)
    with torch.no_grad():
        plain = ou(inp["sample"], inp["timestep"], True, inp["ctx"]).sample
        hooks = hook_oracle_unet(ou, **SD15_FREEU)
        assert len(hooks) == 6
        on = ou(inp["sample"], inp["timestep"], True, inp["ctx"]).sample
        for hk in hooks:
            hk.remove()
        off = ou(inp["sample"], inp["timestep"], True, inp["ctx"]).sample
    assert torch.equal(off, plain) and (on - plain).abs().max().item() > 1e-3 * plain.abs().max().item()


def _product_unet():
    with torch.device("meta"):
        return pkg().UNetMotionCrossFrameAttnModel(**SMALL_UNET)


def test_enable_and_disable_set_the_reference_attributes():
    from i2v_adapter_unofficial_amd.blocks import freeu_scales
    u = _product_unet()
    assert u.freeu_signature() == (None,) * 4
    u.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
    for blk in u.up_blocks:
        assert (blk.s1, blk.s2, blk.b1, blk.b2) == (0.9, 0.2, 1.2, 1.4)
    assert [freeu_scales(b) for b in u.up_blocks] == [(1.2, 0.9), (1.4, 0.2), None, None]
    u.enable_freeu(0.8, 0.3, 1.1, 1.3)                                       # the reference's positional order: s1, s2, b1, b2
    assert u.freeu_signature() == ((1.1, 0.8), (1.3, 0.3), None, None)
    u.disable_freeu()
    for blk in u.up_blocks:
        assert blk.s1 is None and blk.s2 is None and blk.b1 is None and blk.b2 is None
    assert u.freeu_signature() == (None,) * 4
    u.disable_freeu()                                                        # (idempotent)


@pytest.mark.parametrize("zero", ["s1", "s2", "b1", "b2"])
def test_a_zero_among_the_four_leaves_freeu_off(zero):
    u = _product_unet()
    kw = dict(SD15_FREEU)
    kw[zero] = 0.0
    u.enable_freeu(**kw)
    assert getattr(u.up_blocks[0], zero) == 0.0                              # the attribute is set, as in the reference ...
    assert u.freeu_signature() == (None,) * 4                                # ... and `s1 and s2 and b1 and b2` is falsy


def test_pipeline_delegates_and_needs_a_unet():
    p = pkg()
    u = _product_unet()
    pipe = p.I2VAdapterPipeline(unet=u)
    key_off = u.freeu_signature()
    pipe.enable_freeu(0.9, 0.2, 1.2, 1.4)
    assert u.freeu_signature() == ((1.2, 0.9), (1.4, 0.2), None, None) != key_off
    pipe.disable_freeu()
    assert u.freeu_signature() == key_off
    pipe.unet = None
    with pytest.raises(ValueError, match="must have `unet`"):
        pipe.enable_freeu(0.9, 0.2, 1.2, 1.4)


def test_training_refuses_freeu():
    from i2v_adapter_unofficial_amd import training
    u = _product_unet()
    u.enable_freeu(**SD15_FREEU)
    tr = training.UNetAdapterTrainer(u)
    with pytest.raises(NotImplementedError, match="FreeU"):
        tr.forward(torch.zeros(1, 2, 4, 8, 8), 10, torch.zeros(1, 7, 64))


@pytest.fixture(scope="module")
def lib():
    p = pkg()
    if not os.path.exists(p._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return p._lib


def test_bad_arguments_return_error_codes_without_a_gpu(lib):
    h = lib.load()
    assert lib.ABI_VERSION >= 11 and h.i2v_abi_version() == lib.ABI_VERSION
    buf = (C.c_uint16 * 4096)()
    a = C.cast(buf, C.c_void_p)
    q = lambda off: C.c_void_p(a.value + off)                # distinct, 16-byte aligned, never dereferenced: every call is refused
    hid, hid_o, skip, skip_o, lo, lo_o = q(0), q(1024), q(2048), q(3072), q(4096), q(5120)
    call = lambda *args: h.i2v_freeu_f16(*args, None)
    ok_dims = (1, 4, 4, 16, 16, 1.2, 0.9)
    for nulled in range(4):
        ptrs = [hid, None, hid_o, None, skip, skip_o]
        ptrs[(0, 2, 4, 5)[nulled]] = None
        assert call(*ptrs, *ok_dims) == -1 and b"null pointer" in h.i2v_last_error()
    assert call(hid, lo, hid_o, None, skip, skip_o, *ok_dims) == -1 and b"low half" in h.i2v_last_error()
    assert call(hid, None, hid_o, lo_o, skip, skip_o, *ok_dims) == -1 and b"low half" in h.i2v_last_error()
    for hh, ww in ((1, 4), (4, 1), (1, 1)):
        assert call(hid, None, hid_o, None, skip, skip_o, 1, hh, ww, 16, 16, 1.2, 0.9) == -1
        assert b"not implemented for this problem" in h.i2v_last_error()
    assert call(hid, None, hid_o, None, skip, skip_o, 1, 300, 4, 16, 16, 1.2, 0.9) == -1
    assert b"not implemented for this problem" in h.i2v_last_error()
    for c1, c2 in ((12, 16), (16, 20), (4, 16)):
        assert call(hid, None, hid_o, None, skip, skip_o, 1, 4, 4, c1, c2, 1.2, 0.9) == -1
        assert b"not implemented for this problem" in h.i2v_last_error() and b"multiples of 8" in h.i2v_last_error()
    assert call(hid, None, hid_o, None, skip, skip_o, 0, 4, 4, 16, 16, 1.2, 0.9) == -1
    assert call(hid, None, hid, None, skip, skip_o, *ok_dims) == -1 and b"not in place" in h.i2v_last_error()
    assert call(hid, None, hid_o, None, skip, skip, *ok_dims) == -1 and b"not in place" in h.i2v_last_error()
    assert call(q(2), None, hid_o, None, skip, skip_o, *ok_dims) == -1 and b"aligned" in h.i2v_last_error()


def test_the_handle_knows_the_entry_point():
    H = pkg().handle
    assert H.entry_id("i2v_freeu_f16") == 21 and H.ENTRY_NAMES[21] == "i2v_freeu_f16"        # appended: no earlier id moved
    assert H.entry_id("i2v_dpm_cfg_step") == H.ENTRY_IDS["i2v_dpm_cfg_step"] == 20 and "i2v_freeu_f16" not in H.ENTRY_IDS
    assert sorted(H.ENTRY_NAMES) == list(range(22)) and H.entry_id("i2v_unet_forward") is None
