"""FreeNoise without a GPU: windows, weights and coefficients against the lists of the specification and against the literal reference
(tests/freenoise_reference.py), the reference block loop pinned by hand arithmetic and against the oracle's plain block, the noise
rescheduling, `enable_free_noise`'s validation, the driver's flags and the ABI (version 16, the two symbols, the entry ids, the C entry
points' argument checks through ctypes -- no launch)."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from tests import freenoise_reference as R
from tests.parity import SMALL_UNET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def fn():
    return pkg().free_noise


# ------------------------------------------------------------------------------------------------------------ windows / coefficients
@pytest.mark.parametrize("F,L,S,starts,trailing", [
    (20, 8, 4, [0, 4, 8, 12], None),
    (22, 8, 4, [0, 4, 8, 12, 14], (14, 20, 22)),
    (16, 16, 4, [0], None),
    (25, 16, 4, [0, 4, 8, 9], (9, 24, 25)),
])
def test_windows(F, L, S, starts, trailing):
    wins = fn().windows(F, L, S)
    assert [w[0] for w in wins] == starts
    assert [(s, e, first) for s, first, e in wins] == R.ref_windows(F, L, S)
    regular = wins if trailing is None else wins[:-1]
    assert all(first == s and e == s + L for s, first, e in regular)
    if trailing is not None:
        assert wins[-1] == trailing and wins[-1][2] - wins[-1][0] == L
    covered = set()
    for s, first, e in wins:
        covered |= set(range(first, e))
    assert covered == set(range(F))


@pytest.mark.parametrize("scheme", ["flat", "pyramid", "delayed_reverse_sawtooth"])
@pytest.mark.parametrize("F,L,S", [(20, 8, 4), (22, 8, 4), (16, 16, 4), (25, 16, 4), (40, 16, 4), (64, 16, 4), (24, 16, 4), (11, 5, 2)])
def test_coefficients(F, L, S, scheme):
    starts, idx, coef = fn().coefficients(F, L, S, scheme)
    ref = R.ref_coefficients(F, L, S, scheme)
    pairs = len(idx[0])
    assert pairs <= -(-L // S) + 1 and all(len(i) == pairs == len(c) for i, c in zip(idx, coef))
    c32 = torch.tensor(coef, dtype=torch.float64).to(torch.float32)
    for f in range(F):
        live = [(i, c) for i, c in zip(idx[f], coef[f]) if c != 0.0]
        assert [(i // L, i % L) for i, _ in live] == [(w, j) for w, j, _ in ref[f]]
        assert [c for _, c in live] == [c for _, _, c in ref[f]]
        assert all(i == 0 for i, c in zip(idx[f], coef[f]) if c == 0.0), "padding carries index 0"
        assert all(c == 0.0 for c in coef[f][len(live):]), "padding sits behind the contributions"
        assert all(starts[i // L] + i % L == f for i, _ in live), "every pair points at this frame inside its window"
        assert abs(float(c32[f].double().sum()) - 1.0) <= 1e-6
        if len(live) == 1:
            assert coef[f][0] == 1.0 and float(c32[f, 0]) == 1.0
    if (F, L, S) == (22, 8, 4):
        assert [len([c for c in coef[f] if c]) for f in (20, 21)] == [1, 1] and idx[20][0] == 4 * L + 6 and idx[21][0] == 4 * L + 7
    if (F, L, S) == (25, 16, 4):
        assert [c for c in coef[24] if c] == [1.0] and idx[24][0] == 3 * L + 15


def test_weights_match_the_specification():
    W = fn().weights
    assert W(4, "flat") == [1, 1, 1, 1] and W(5, "flat") == [1] * 5 and W(16, "flat") == [1] * 16
    assert W(4, "pyramid") == [1, 2, 2, 1]
    assert W(5, "pyramid") == [1, 2, 3, 2, 1]
    assert W(16, "pyramid") == [1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 6, 5, 4, 3, 2, 1]
    assert W(4, "delayed_reverse_sawtooth") == [0.01, 2, 2, 1]
    assert W(5, "delayed_reverse_sawtooth") == [0.01, 0.01, 3, 2, 1]
    assert W(16, "delayed_reverse_sawtooth") == [0.01] * 7 + [8, 8, 7, 6, 5, 4, 3, 2, 1]
    for L in (4, 5, 16):
        for scheme in fn().WEIGHTING_SCHEMES:
            assert W(L, scheme) == R.ref_weights(L, scheme) and len(W(L, scheme)) == L
    with pytest.raises(ValueError):
        W(8, "triangle")


# ------------------------------------------------------------------------------------------------------------ the reference loop
class _ToyBlock:
    """identity attention output (attn(n) = n), identity norms, zero positions, zero feed-forward: a window's result is
    c -> c + c = 2c -> 2c + 2c = 4c, so the blended frame is 4 x[f] whatever the weights -- unless the positions are non-zero"""

    def __init__(self, pos=None):
        self.norm1 = self.norm2 = self.norm3 = lambda x: x
        self.attn1 = self.attn2 = lambda n: n
        self.pos_embed = (lambda x: x) if pos is None else (lambda x: x + pos[: x.shape[1]][None, :, None])
        self.ff = lambda x: torch.zeros_like(x)


def test_reference_loop_by_hand():
    x = torch.arange(6, dtype=torch.float64).reshape(1, 6, 1) + 1.0           # frames 1 .. 6, one pixel, one channel
    out = R.ref_block_forward(_ToyBlock(), x, 4, 2, "pyramid")
    assert torch.equal(out, 4 * x)
    # positions p_j = 10 j restart in every window: c -> 2c + p -> 2 (2c + p) + p = 4c + 3p.  Windows [0, 4) and [2, 6), weights 1 2 2 1:
    #   frames 0, 1: window 0 only, j = 0, 1                      -> 4x + 0, 4x + 30
    #   frames 2, 3: window 0 (j = 2, 3; weights 2, 1) and window 1 (j = 0, 1; weights 1, 2)
    #       frame 2: (2 (4x + 60) + 1 (4x + 0)) / 3 = 4x + 40;    frame 3: (1 (4x + 90) + 2 (4x + 30)) / 3 = 4x + 50
    #   frames 4, 5: window 1 only, j = 2, 3                      -> 4x + 60, 4x + 90
    pos = torch.tensor([0.0, 10.0, 20.0, 30.0], dtype=torch.float64)
    out = R.ref_block_forward(_ToyBlock(pos), x, 4, 2, "pyramid")
    want = 4 * x + torch.tensor([0.0, 30.0, 40.0, 50.0, 60.0, 90.0], dtype=torch.float64).reshape(1, 6, 1)
    assert torch.allclose(out, want, rtol=0, atol=1e-12), (out - want).abs().max()
    # a trailing window: F = 7, L = 4, S = 2 -> windows 0, 2 and the trailing [3, 7) that gives frame 6 only (j = 3)
    x7 = torch.arange(7, dtype=torch.float64).reshape(1, 7, 1) + 1.0
    out = R.ref_block_forward(_ToyBlock(pos), x7, 4, 2, "flat")
    want = 4 * x7 + torch.tensor([0.0, 30.0, (60 + 0) / 2, (90 + 30) / 2, 60.0, 90.0, 90.0], dtype=torch.float64).reshape(1, 7, 1)
    assert torch.allclose(out, want, rtol=0, atol=1e-12), (out - want).abs().max()


def test_reference_with_one_window_is_the_plain_block():
    from oracle.blocks import BasicTransformerBlock
    torch.manual_seed(3)
    blk = BasicTransformerBlock(32, 4, 8, double_self_attention=True, positional_embeddings="sinusoidal",
                                num_positional_embeddings=32).double().eval()
    x = torch.randn(5, 8, 32, dtype=torch.float64)
    with torch.no_grad():
        # one window, weight 1: (c * 1) / 1 is exact, so the loop IS the plain block.  With other weights (c * w) / w rounds twice
        # (2^-53 relative each) ahead of the feed-forward: equal to a few fp64 ulps, not bit for bit
        assert torch.equal(R.ref_block_forward(blk, x, 8, 4, "flat"), blk(x))
        for scheme in ("pyramid", "delayed_reverse_sawtooth"):
            assert torch.allclose(R.ref_block_forward(blk, x, 8, 4, scheme), blk(x), rtol=1e-13, atol=1e-13)
        assert not torch.allclose(R.ref_block_forward(blk, x, 4, 2, "pyramid"), blk(x))


def test_blend_coefficients_reproduce_the_reference_loop():
    """the gather -> per-window -> coefficient sum form the device runs, in fp64 torch, equals accumulated / total_weight"""
    from oracle.blocks import BasicTransformerBlock
    torch.manual_seed(4)
    blk = BasicTransformerBlock(16, 2, 8, double_self_attention=True, positional_embeddings="sinusoidal",
                                num_positional_embeddings=32).double().eval()
    F, L, S = 22, 8, 4
    x = torch.randn(3, F, 16, dtype=torch.float64)
    starts, idx, coef = fn().coefficients(F, L, S, "pyramid")
    with torch.no_grad():
        c = torch.cat([x[:, s: s + L] for s in starts], dim=1)                 # [pixels, windows * L, C]
        c = c.reshape(3 * len(starts), L, 16)
        c = blk.attn1(blk.pos_embed(blk.norm1(c))) + c
        c = blk.attn2(blk.pos_embed(blk.norm2(c))) + c
        c = c.reshape(3, len(starts) * L, 16)
        out = sum(torch.tensor(coef, dtype=torch.float64)[None, :, k, None] * c[:, torch.tensor(idx)[:, k]] for k in range(len(idx[0])))
        out = blk.ff(blk.norm3(out)) + out
        want = R.ref_block_forward(blk, x, L, S, "pyramid")
    assert torch.allclose(out, want, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------ noise
def _draw(shape, g):
    return torch.randn(shape, generator=g, dtype=torch.float32)


@pytest.mark.parametrize("noise_type", ["repeat_context", "shuffle_context"])
def test_noise_rescheduling(noise_type):
    F, L, S = 22, 8, 4
    shape = (2, F, 4, 6, 5)
    st = fn().FreeNoiseSettings(L, S, "pyramid", noise_type)
    got = fn().reschedule_noise(_draw, shape, st, torch.Generator().manual_seed(11))
    again = fn().reschedule_noise(_draw, shape, st, torch.Generator().manual_seed(11))
    other = fn().reschedule_noise(_draw, shape, st, torch.Generator().manual_seed(12))
    assert got.shape == shape and got.dtype == torch.float32 and torch.equal(got, again) and not torch.equal(got, other)
    plain = torch.randn((2, L) + shape[2:], generator=torch.Generator().manual_seed(11), dtype=torch.float32)
    assert torch.equal(got[:, :L], plain), "the first L frames are the plain draw of L frames"
    want, src = R.ref_noise(shape, L, S, noise_type, 11)
    assert torch.equal(got, want)
    for f in range(L, F):
        for b in range(2):
            hits = [k for k in range(L) if torch.equal(got[b, f], got[b, k])]
            assert hits == [src[f]], (f, hits)
    if noise_type == "repeat_context":
        assert src == [f % L for f in range(F)]
    else:
        # frame f >= L sits in the destination block [i, i + S) of i = L + S ((f - L) // S) and comes from [i - L, i - L + S)
        for f in range(L, F):
            i = L + S * ((f - L) // S)
            lo, hi = i - L, min(F, i - L + S)
            assert any(torch.equal(got[0, f], got[0, k]) for k in range(lo, hi)), f
        blocks = [sorted(src[i: min(F, i + S)]) for i in range(L, F, S)]
        assert all(len(set(b)) == len(b) for b in blocks), "a block is a permutation: no frame of its window twice"


def test_noise_random_and_generator_lists():
    st = fn().FreeNoiseSettings(8, 4, "pyramid", "random")
    shape = (2, 22, 4, 3, 3)
    got = fn().reschedule_noise(_draw, shape, st, torch.Generator().manual_seed(5))
    assert torch.equal(got, torch.randn(shape, generator=torch.Generator().manual_seed(5), dtype=torch.float32))
    st = st._replace(noise_type="shuffle_context")
    gens = [torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)]
    both = fn().reschedule_noise(_draw, shape, st, gens)
    one = fn().reschedule_noise(_draw, (1,) + shape[1:], st, torch.Generator().manual_seed(2))
    assert torch.equal(both[1:], one), "a sample's noise depends on its own generator only"
    with pytest.raises(ValueError):
        fn().reschedule_noise(_draw, shape, st, gens[:1])
    with pytest.raises(ValueError):
        fn().reschedule_noise(_draw, (1, 7, 4, 3, 3), st, None)                # F < L


# ------------------------------------------------------------------------------------------------------------ the switches
def _product_unet():
    with torch.device("meta"):
        return pkg().UNetMotionCrossFrameAttnModel(**SMALL_UNET)


def test_enable_disable_and_signature():
    u = _product_unet()
    blocks = [b for m in u._motion_modules() for b in m.transformer_blocks]
    assert blocks and u.free_noise_signature() is None and all(b.free_noise is None for b in blocks)
    u.enable_free_noise()
    assert u.free_noise_signature() == (16, 4, "pyramid", "shuffle_context")                   # diffusers' defaults
    assert all(tuple(b.free_noise) == (16, 4, "pyramid", "shuffle_context") for b in blocks)
    u.enable_free_noise(context_length=8, context_stride=2, weighting_scheme="flat", noise_type="random")
    assert u.free_noise_signature() == (8, 2, "flat", "random")
    assert u.free_noise_launch_signature() == (8, 2, "flat")            # the captured step's key: noise_type launches nothing
    u.disable_free_noise()
    assert u.free_noise_signature() is None and u.free_noise_launch_signature() is None and all(b.free_noise is None for b in blocks)
    u.disable_free_noise()                                                                      # (idempotent)
    pipe = pkg().I2VAdapterPipeline(unet=u)
    assert pipe.free_noise_enabled is False
    pipe.enable_free_noise(context_length=12)
    assert pipe.free_noise_enabled is True and u.free_noise_signature() == (12, 4, "pyramid", "shuffle_context")
    pipe.disable_free_noise()
    assert pipe.free_noise_enabled is False
    pipe.unet = None
    with pytest.raises(ValueError, match="must have `unet`"):
        pipe.enable_free_noise()


@pytest.mark.parametrize("kw", [dict(context_length=33), dict(context_length=1), dict(context_stride=0), dict(context_stride=-2),
                                dict(weighting_scheme="triangle"), dict(noise_type="white"), dict(context_length=8.5)])
def test_enable_rejects_bad_settings(kw):
    u = _product_unet()
    with pytest.raises(ValueError):
        u.enable_free_noise(**kw)
    assert u.free_noise_signature() is None, "a refused call leaves FreeNoise off"


def test_num_frames_is_checked_against_the_settings():
    st = fn().check_free_noise_args(16, 4, "pyramid", "shuffle_context", 32)
    with pytest.raises(ValueError, match="below `context_length`"):
        fn().check_num_frames(12, st)
    fn().check_num_frames(16, st)
    for bad in ((12, 16, 4), (16, 1, 4), (16, 8, 0)):
        with pytest.raises(ValueError):
            fn().windows(*bad)
    m = pkg().TransformerTemporalModel(num_attention_heads=2, in_channels=16, norm_num_groups=4, attention_head_dim=8,
                                       positional_embeddings="sinusoidal", num_positional_embeddings=8)
    with pytest.raises(ValueError, match="num_positional_embeddings"):
        m.set_free_noise(st)                                                                    # L = 16 above this module's 8 positions


def test_tables_are_one_block_named_without_the_device():
    st = fn().FreeNoiseSettings(8, 4, "pyramid", "random")
    starts, idx, coef = fn().tables(22, st, torch.device("cpu"))
    s, i, c = fn().coefficients(22, 8, 4, "pyramid")
    assert starts.dtype == idx.dtype == torch.int32 and coef.dtype == torch.float32
    assert starts.tolist() == s and idx.tolist() == i and torch.equal(coef, torch.tensor(c, dtype=torch.float64).float())
    assert fn().tables(22, st._replace(noise_type="repeat_context"), torch.device("cpu"))[0] is starts     # kept per (F, L, S, scheme)
    named = fn().persistent_tables(torch.device("cpu"))
    block = named["free_noise#22.8.4.pyramid"]
    assert block.dtype == torch.float32 and block.numel() == len(s) + 2 * 22 * len(i[0])
    assert starts.untyped_storage().data_ptr() == idx.untyped_storage().data_ptr() == coef.untyped_storage().data_ptr() == block.data_ptr()
    assert fn().persistent_tables(torch.device("meta")) == {}


def test_training_refuses_free_noise():
    from i2v_adapter_unofficial_amd import training
    u = _product_unet()
    u.enable_free_noise()
    tr = training.UNetAdapterTrainer(u)
    with pytest.raises(NotImplementedError, match="FreeNoise"):
        tr.forward(torch.zeros(1, 2, 4, 8, 8), 10, torch.zeros(1, 7, 64))


def test_driver_flags():
    parser = pkg().pipeline_i2v_adapter.build_parser()
    a = parser.parse_args(["--embeds", "e.safetensors"])
    assert a.free_noise is None and a.free_noise_stride == 4 and a.free_noise_weighting == "pyramid" and a.free_noise_noise == "shuffle_context"
    assert parser.parse_args(["--embeds", "e.safetensors", "--free_noise"]).free_noise == 16
    a = parser.parse_args(["--embeds", "e.safetensors", "--free_noise", "8", "--free_noise_stride", "2", "--free_noise_weighting", "flat",
                           "--free_noise_noise", "repeat_context"])
    assert (a.free_noise, a.free_noise_stride, a.free_noise_weighting, a.free_noise_noise) == (8, 2, "flat", "repeat_context")


# ------------------------------------------------------------------------------------------------------------ the ABI
@pytest.fixture(scope="module")
def lib():
    p = pkg()
    if not os.path.exists(p._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return p._lib


def test_abi_version_symbols_and_entry_ids(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 16
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    H = pkg().handle
    for name in ("i2v_freenoise_gather_f16", "i2v_freenoise_blend_f16"):
        assert hasattr(h, name) and name in lib.SIGNATURES and name in src
        assert H.entry_name(H.entry_id(name)) == name and name not in H.ENTRY_IDS and name in H.LATER_ENTRY_IDS
    assert H.entry_id("i2v_freenoise_gather_f16") == H.entry_id("i2v_lcm_cfg_step") + 1 == 23
    assert H.entry_id("i2v_freenoise_blend_f16") == 24
    # the old tables are unchanged
    assert H.ENTRY_IDS["i2v_dpm_cfg_step"] == len(H.ENTRY_IDS) - 1 == 20 and sorted(H.ENTRY_NAMES) == list(range(22))
    assert H.entry_id("i2v_freeu_f16") == 21 and H.entry_id("i2v_lcm_cfg_step") == 22
    hip = open(os.path.join(ROOT, "i2v-adapter-unofficial_amd", "csrc", "handle.hip")).read()
    enum = re.search(r"enum Entry \{(.*?)\};", hip, re.S).group(1)
    names = [n.split("=")[0].strip() for n in re.sub(r"//[^\n]*", "", enum).split(",") if n.strip()]
    assert names.index("E_FREENOISE_GATHER") == 23 and names.index("E_FREENOISE_BLEND") == 24 and names[-1] == "E_COUNT"
    assert hasattr(pkg().kernels, "freenoise_gather") and hasattr(pkg().kernels, "freenoise_blend")


def test_entry_points_reject_bad_arguments_without_a_gpu(lib):
    h = lib.load()
    n_pix, F, W, L, c, pairs = 3, 10, 3, 4, 16, 2
    src = (C.c_uint16 * (n_pix * F * c + 8))()
    win = (C.c_uint16 * (n_pix * W * L * c + 8))()
    starts = (C.c_int32 * W)(0, 3, 6)
    idx = (C.c_int32 * (F * pairs))()
    coef = (C.c_float * (F * pairs))()
    P = lambda a: C.cast(a, C.c_void_p)
    #        src     ld dst     ld starts     pixels F  W  L  c  stream
    good = [P(src), c, P(win), c, P(starts), n_pix, F, W, L, c, None]
    bad_args = [(0, None), (2, None), (4, None), (5, 0), (7, 0), (7, F + 1), (8, 0), (8, F + 1), (9, 12), (9, 0), (1, c - 8), (1, c + 4),
                (3, c + 2), (0, C.c_void_p(C.addressof(src) + 2)), (2, P(src)), (5, 2 ** 40)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert h.i2v_freenoise_gather_f16(*args) == -1, (i, bad)
        assert b"i2v_freenoise_gather_f16" in h.i2v_last_error(), (i, bad)
    #        src     ld dst     ld idx     coef     pixels F  W  L  pairs c  stream
    good = [P(win), c, P(src), c, P(idx), P(coef), n_pix, F, W, L, pairs, c, None]
    bad_args = [(0, None), (2, None), (4, None), (5, None), (6, 0), (8, 0), (9, F + 1), (10, 0), (10, 34), (11, 20), (1, c - 8),
                (3, c + 4), (2, P(win)), (2, C.c_void_p(C.addressof(src) + 6))]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert h.i2v_freenoise_blend_f16(*args) == -1, (i, bad)
        assert b"i2v_freenoise_blend_f16" in h.i2v_last_error(), (i, bad)
