"""The 64-row-tile form of the fused motion attention sub-block (ABI 28: i2v_motion_attn_wide_supported / i2v_motion_attn_wide_f16)
without a GPU: the ABI, the shape query's truth table beside the unchanged narrow query, the host-side argument checks, the handle's
entry id and the routing switch.  The kernel and its numbers are tests/test_motion_attn_wide_gpu.py's."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


@pytest.fixture(scope="module")
def lib():
    return pkg()._lib


def test_abi_28_declares_exports_and_binds_the_two_entry_points(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 28
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for name, ret in (("i2v_motion_attn_wide_supported", "int32_t"), ("i2v_motion_attn_wide_f16", "int")):
        assert re.search(rf"\b{ret} {name}\(", src) and name in lib.SIGNATURES and hasattr(h, name)
    assert lib.SIGNATURES["i2v_motion_attn_wide_f16"] == lib.SIGNATURES["i2v_motion_attn_f16"]          # the same params struct
    assert lib.SIGNATURES["i2v_motion_attn_wide_supported"] == lib.SIGNATURES["i2v_motion_attn_supported"]
    assert callable(pkg().kernels.motion_attn_wide) and callable(pkg().kernels.motion_attn_wide_supported)


def test_supported_truth_table(lib):
    q = lib.load().i2v_motion_attn_wide_supported
    assert q(64, 640, 8, 80, 16) == 1 and q(32768, 640, 8, 80, 16) == 1
    assert q(64 + 16, 640, 8, 80, 16) == 0 and q(0, 640, 8, 80, 16) == 0 and q(64 << 24, 640, 8, 80, 16) == 0
    assert q(64, 320, 8, 40, 16) == 0 and q(64, 320, 8, 80, 16) == 0
    assert q(64, 640, 8, 80, 8) == 0 and q(64, 640, 8, 80, 32) == 0
    assert q(64, 640, 4, 80, 16) == 0 and q(64, 640, 4, 160, 16) == 0 and q(64, 640, 8, 40, 16) == 0


def test_the_narrow_query_answers_as_before(lib):
    h = lib.load()
    q = h.i2v_motion_attn_supported
    assert q(131072, 320, 8, 40, 16) == 1 and q(131072 + 16, 320, 8, 40, 16) == 0
    assert q(32768, 640, 8, 80, 16) == 0 and q(65536, 320, 8, 40, 4) == 0
    assert q(65536, 320, 8, 40, 8) == 1 and q(65536, 320, 8, 40, 32) == 1
    assert q(64, 320, 8, 40, 16) == 0 and q(128, 320, 8, 40, 16) == 1         # its tiles are still 128 rows
    assert h.i2v_motion_attn_pack_rows(8, 40) == 1152 and h.i2v_motion_attn_pack_rows(8, 80) == 8 * 3 * 80


def test_bad_arguments_are_refused_on_the_host(lib):
    """I2V_ERR_INVALID_ARG before anything is launched: callable without a GPU (the pointers are never dereferenced)"""
    h = lib.load()
    assert h.i2v_motion_attn_wide_f16(None, None) == -1 and b"i2v_motion_attn_wide_f16: null params" in h.i2v_last_error()
    ok = dict(x=1 << 40, ldx=640, gamma=1 << 41, shift=1 << 42, ld_shift=640, w_qkv=1 << 43, out=1 << 44, ldo=640, rows=128,
              channels=640, heads=8, head_dim=80, frames=16, eps=1e-5, scale=80 ** -0.5, w_o=1 << 45, b_o=1 << 46)
    for kw, msg in ((dict(x=None), b"null pointer"), (dict(gamma=None), b"null pointer"), (dict(shift=None), b"null pointer"),
                    (dict(w_qkv=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(w_o=None), b"required"), (dict(b_o=None), b"required"), (dict(w_o=None, b_o=None), b"required"),
                    (dict(rows=128 + 16), b"not a fused shape"), (dict(channels=320, head_dim=40), b"not a fused shape"),
                    (dict(frames=8), b"not a fused shape"), (dict(frames=32), b"not a fused shape"), (dict(heads=4), b"not a fused shape"),
                    (dict(ldx=632), b"row strides"), (dict(ldx=644), b"row strides"), (dict(ldo=636), b"row strides"),
                    (dict(ldo=644), b"row strides"), (dict(ld_shift=638), b"row strides"), (dict(ld_shift=0), b"row strides"),
                    (dict(x=(1 << 40) + 8), b"16-byte"), (dict(w_o=(1 << 45) + 2), b"16-byte"), (dict(b_o=(1 << 46) + 4), b"16-byte"),
                    (dict(ldx=1 << 23), b"below 2^23")):
        p = lib.MotionAttnParams()
        for name, v in {**ok, **kw}.items():
            setattr(p, name, v)
        assert h.i2v_motion_attn_wide_f16(C.byref(p), None) == -1, kw
        err = h.i2v_last_error()
        assert err.startswith(b"i2v_motion_attn_wide_f16:") and msg in err, (kw, err)


def test_wrapper_requires_out_proj():
    import torch
    with pytest.raises(ValueError, match="out_proj is required"):
        pkg().kernels.motion_attn_wide(torch.zeros(64, 640), None, None, None, heads=8, head_dim=80, frames=16, eps=1e-5, out_proj=None)


def test_handle_entry_id_continues_the_numbering():
    from i2v_adapter_unofficial_amd import handle as H
    name = "i2v_motion_attn_wide_f16"
    assert name not in H.ENTRY_IDS and H.LATER_ENTRY_IDS[name] == 25 == H.entry_id(name) and H.entry_name(25) == name
    hip = open(os.path.join(ROOT, "i2v-adapter-unofficial_amd", "csrc", "handle.hip")).read()
    enum = re.search(r"enum Entry \{(.*?)\};", hip, re.S).group(1)
    names = [n.split("=")[0].strip() for n in re.sub(r"//[^\n]*", "", enum).split(",") if n.strip()]
    assert names.index("E_MOTION_ATTN_WIDE") == 25 and names[-1] == "E_COUNT"
    assert f'{{"{name}", sizeof(i2v_motion_attn_params), 0}}' in hip


def test_routing_switch_is_read_once_like_its_neighbours():
    from i2v_adapter_unofficial_amd import blocks
    assert blocks.FUSED_MOTION_ATTN_WIDE is (os.environ.get("I2V_MOTION_FUSED_WIDE", "1") != "0")
    src = open(blocks.__file__).read()
    assert src.count('os.environ.get("I2V_MOTION_FUSED_WIDE"') == 1
