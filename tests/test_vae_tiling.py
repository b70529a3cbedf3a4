"""Tiled VAE without a GPU: the tile planner, the geometry diffusers derives from the config, the closed four-tile form the HIP kernel
implements against diffusers' literal in-place loops, the refusal of overlap factors it does not hold for, the switches, the driver's
flag, and `i2v_vae_tile_blend`'s declaration / binding / host-side argument checks."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from tests import vae_tiling_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def _vae(**kw):
    with torch.device("meta"):
        return pkg().AutoencoderKL(**kw)


def _covered(size, tile, overlap, limit, out_len=lambda v: v):
    """how often each output element is kept: tile k covers [offset, offset + min(out_len(length), limit))"""
    count, off = [0] * out_len(size), 0
    for start, length in pkg().vae.plan_tiles(size, tile, overlap):
        assert 0 <= start and 0 < length <= tile and start + length <= size
        keep = min(out_len(length), limit)
        assert off == out_len(start)                       # the kept piece sits where the tile starts: no shift in the stitched image
        for k in range(off, off + keep):
            count[k] += 1
        off += keep
    return count


def test_planner_covers_every_latent_exactly_once():
    plan = pkg().vae.plan_tiles
    assert plan(96, 64, 48) == [(0, 64), (48, 48)] and plan(64, 64, 48) == [(0, 64), (48, 16)] and plan(1, 64, 48) == [(0, 1)]
    assert plan(100, 64, 48) == [(0, 64), (48, 52), (96, 4)]
    for h in range(1, 201):
        assert _covered(h, 64, 48, 48) == [1] * h, h
        # decode: the tiles come out 8x as long and are cropped to 384 px
        assert _covered(h, 64, 48, 384, lambda v: 8 * v) == [1] * (8 * h), h
    with pytest.raises(ValueError):
        plan(10, 64, 0)


def test_planner_covers_the_pixel_geometry_on_multiples_of_8():
    for px in range(8, 1601, 8):                           # encode: 512 px tiles every 384, 64 latents cropped to 48
        assert _covered(px, 512, 384, 48, lambda v: v // 8) == [1] * (px // 8), px
    for px in range(8, 201, 8):                            # sample_size 32: 32 px tiles every 24, 4 latents cropped to 3
        assert _covered(px, 32, 24, 3, lambda v: v // 8) == [1] * (px // 8), px


def test_default_geometry_comes_from_the_config():
    v = _vae()
    assert (v.use_tiling, v.tile_sample_min_size, v.tile_latent_min_size, v.tile_overlap_factor) == (False, 512, 64, 0.25)
    g = pkg().vae.tile_geometry
    assert g(v.tile_latent_min_size, v.tile_sample_min_size, 0.25) == (48, 128, 384) == R.geometry(64, 512)        # decode
    assert g(v.tile_sample_min_size, v.tile_latent_min_size, 0.25) == (384, 16, 48) == R.geometry(512, 64)         # encode
    s = _vae(block_out_channels=(32, 64, 64, 64), norm_num_groups=8, sample_size=32)
    assert (s.tile_sample_min_size, s.tile_latent_min_size, s.tile_overlap_factor) == (32, 4, 0.25)
    assert g(4, 32, 0.25) == (3, 8, 24) and g(32, 4, 0.25) == (24, 1, 3)
    assert _vae(block_out_channels=(128, 256, 512, 512), sample_size=64).tile_latent_min_size == 8


def test_switches():
    v = _vae()
    v.enable_tiling()
    assert v.use_tiling is True
    v.enable_tiling(False)
    assert v.use_tiling is False
    v.enable_tiling(True)
    v.disable_tiling()
    assert v.use_tiling is False
    v.disable_tiling()                                     # (idempotent)
    from tests.parity import SMALL_UNET
    p = pkg()
    with torch.device("meta"):
        u = p.UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    pipe = p.I2VAdapterPipeline(vae=v, unet=u)
    pipe.enable_vae_tiling()
    assert v.use_tiling is True
    pipe.disable_vae_tiling()
    assert v.use_tiling is False
    bare = p.I2VAdapterPipeline(unet=u)
    with pytest.raises(ValueError, match="vae"):
        bare.enable_vae_tiling()
    with pytest.raises(ValueError, match="vae"):
        bare.disable_vae_tiling()


# (tile heights, tile widths, E, limit): what the decoder / encoder hands the stitcher -- full tiles and the remainder at the end
GRIDS = [
    ((32, 16), (32, 16), 8, 24),                  # 2 x 2, 16 px remainder
    ((64, 64, 8), (64, 64, 8), 16, 48),           # 3 x 3 with a remainder NARROWER than E in both axes (e = 8 < E)
    ((32,), (32, 32, 8), 8, 24),                  # 1 x 3
    ((32, 32, 8), (32,), 8, 24),                  # 3 x 1
    ((32, 24), (32, 32, 16), 8, 24),              # 2 x 3, different remainders per axis
    ((64, 52, 4), (64, 64, 64, 16), 16, 48),      # a second-to-last tile that is not full (100 = 48 + 48 + 4) and a 4-wide remainder
    ((4, 4, 2), (4, 3), 1, 3),                    # the encode geometry of sample_size 32: E = 1 latent
    ((512, 384), (512, 384), 128, 384),           # the SD VAE's real geometry at 768 px
]


@pytest.mark.parametrize("heights,widths,extent,limit", GRIDS)
def test_closed_form_equals_the_in_place_loops(heights, widths, extent, limit):
    n, c = (1, 1) if heights[0] >= 512 else (2, 3)
    rows = R.random_grid(heights, widths, n=n, c=c, seed=len(heights) * 10 + len(widths))
    keep = [[t.clone() for t in row] for row in rows]
    ref = R.stitch(rows, extent, limit)
    got = R.closed_form_stitch(rows, extent, limit)
    assert all(torch.equal(a, b) for ra, rb in zip(rows, keep) for a, b in zip(ra, rb))      # neither form touched the raw tiles
    assert got.shape == ref.shape == (n, c, sum(min(h, limit) for h in heights), sum(min(w, limit) for w in widths))
    assert (got - ref).abs().max().item() <= 1e-12
    if len(heights) > 1 and len(widths) > 1:      # the corner of tile (1, 1) really mixes four tiles: it moves with the diagonal one
        rows[0][0] = rows[0][0] + 1.0
        moved = R.closed_form_stitch(rows, extent, limit)
        oy, ox = min(heights[0], limit), min(widths[0], limit)
        assert (moved - got)[:, :, oy, ox].abs().min().item() > 0.5


def test_a_factor_above_one_third_is_refused():
    g = pkg().vae.tile_geometry
    assert g(64, 512, 1 / 3) == (42, 170, 342)
    for f in (0.34, 0.5, 0.75):
        with pytest.raises(NotImplementedError, match="1/3"):
            g(64, 512, f)
        with pytest.raises(NotImplementedError, match="1/3"):
            g(512, 64, f)
    with pytest.raises(NotImplementedError):               # no cross-fade at all: the kernel takes a positive blend extent only
        g(64, 512, 0.0)
    v = _vae()
    v.enable_tiling()
    v.tile_overlap_factor = 0.5
    with pytest.raises(NotImplementedError, match="1/3"):
        v.tiled_decode(torch.zeros(1, 4, 96, 96, device="meta"))
    with pytest.raises(NotImplementedError, match="1/3"):
        v.tiled_encode(torch.zeros(1, 3, 768, 768, device="meta"))


def test_the_driver_takes_vae_tiling(capsys):
    main = pkg().pipeline_i2v_adapter.main
    assert main(["--embeds", "e.safetensors", "--vae_tiling"]) == -1          # parsed; stops at the missing --task_name
    with pytest.raises(SystemExit):
        main(["--embeds", "e.safetensors", "--vae_tiling", "1"])              # a switch, not a value
    capsys.readouterr()


@pytest.fixture(scope="module")
def lib():
    p = pkg()
    if not os.path.exists(p._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return p._lib


CTYPE = {"const void*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "i2v_stream_t": C.c_void_p}


def test_header_and_binding_agree_on_the_symbol(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1) == str(lib.ABI_VERSION) and lib.ABI_VERSION >= 12
    comment = src[:src.index("int i2v_vae_tile_blend(")].rsplit("/*", 1)[1]           # the entry's own comment block
    assert comment.lstrip().startswith("(ABI 12)") and "pipe:139-153" in comment and comment.rstrip().endswith("*/")
    decl = re.search(r"\bint i2v_vae_tile_blend\(([^)]*)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S)).group(1)
    types = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0] for a in decl.split(",")]
    res, args = lib.SIGNATURES["i2v_vae_tile_blend"]
    assert res is C.c_int and args == [CTYPE[t] for t in types] and len(args) == 20
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION and hasattr(h, "i2v_vae_tile_blend")
    assert "i2v_vae_tile_blend" not in pkg().handle.ENTRY_IDS          # glue outside the captured step: the plan format is unchanged


def test_bad_arguments_return_error_codes_without_a_gpu(lib):
    h = lib.load()
    buf = (C.c_float * 4096)()
    a = C.cast(buf, C.c_void_p)
    q = lambda off: C.c_void_p(a.value + off)                # never dereferenced: every call is refused before the launch
    t, u, l, ul, out = q(0), q(1024), q(2048), q(3072), q(4096)
    #            f32 n th tw ld c up_h left_w E limit | out_h out_w oy ox
    good = dict(f32=1, n=1, th=8, tw=8, ld=3, c=3, up_h=8, left_w=8, e=2, limit=6, out_h=12, out_w=12, oy=6, ox=6)

    def call(tile=t, up=u, left=l, upleft=ul, dst=out, **kw):
        k = dict(good, **kw)
        return h.i2v_vae_tile_blend(tile, up, left, upleft, k["f32"], k["n"], k["th"], k["tw"], k["ld"], k["c"], k["up_h"], k["left_w"],
                                    k["e"], k["limit"], dst, k["out_h"], k["out_w"], k["oy"], k["ox"], None)

    assert call(tile=None) == -1 and b"null pointer" in h.i2v_last_error()
    assert call(dst=None) == -1 and b"null pointer" in h.i2v_last_error()
    assert call(c=4) == -1 and b"> ld" in h.i2v_last_error()
    assert call(limit=0) == -1 and b"limit" in h.i2v_last_error()
    assert call(limit=-3) == -1 and b"limit" in h.i2v_last_error()
    assert call(e=0) == -1 and b"blend_extent" in h.i2v_last_error()
    for kw in (dict(oy=7), dict(ox=7), dict(oy=-1), dict(ox=-1), dict(out_h=11), dict(out_w=11), dict(limit=7)):
        assert call(**kw) == -1 and b"leaves the" in h.i2v_last_error(), kw
    assert call(up=None) == -1 and b"upleft comes with both" in h.i2v_last_error()
    assert call(left=None) == -1 and b"upleft comes with both" in h.i2v_last_error()
    assert call(up=None, left=None) == -1 and b"upleft comes with both" in h.i2v_last_error()
    assert call(up_h=0) == -1 and call(left_w=0) == -1 and call(n=0) == -1 and call(th=0) == -1 and call(tw=0) == -1
