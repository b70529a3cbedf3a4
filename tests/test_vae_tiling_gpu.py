"""GPU tests of the tiled VAE (enable_vae_tiling, pipe:139-153): `i2v_vae_tile_blend` against diffusers' literal in-place loops on
synthetic raw tiles, its exact pass-through and its confinement to the crop rectangle, `AutoencoderKL.tiled_decode` / `tiled_encode`
against the oracle VAE run through the literal loops (tests/vae_tiling_reference.py), the switch, and the pipeline."""
import pytest
import torch

from tests import vae_tiling_reference as R
from tests.parity import compare, hip_model_random, host_threads, oracle_from_hip

pytestmark = pytest.mark.gpu
SMALL_VAE = dict(block_out_channels=(32, 64, 64, 64), norm_num_groups=8, sample_size=32)      # tiles of 4 latents / 32 px
SD_VAE = dict(block_out_channels=(128, 256, 512, 512), norm_num_groups=32, sample_size=64)    # tiles of 8 latents / 64 px
SENTINEL = 12345.0


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def K():
    return pkg().kernels


def h(t):
    return t.half().float()


def _pair(cfg, dev, seed):
    from oracle.vae import AutoencoderKL as O
    hv = hip_model_random(cfg, dev, seed=seed, cls=pkg().AutoencoderKL)
    return oracle_from_hip(hv, O, cfg), hv


@pytest.fixture(scope="module")
def small_pair(dev):
    host_threads()
    return _pair(SMALL_VAE, dev, seed=31)


def _tokens(t, ld, dtype, dev, seed=0):
    """[N, C, h, w] -> token-major [N, h, w, ld] on the device; the channels >= C hold junk the kernel must not use"""
    n, c, hh, ww = t.shape
    tok = torch.randn(n, hh, ww, ld, generator=torch.Generator().manual_seed(seed)) * 100
    tok[..., :c] = t.permute(0, 2, 3, 1)
    return tok.to(dtype).contiguous().to(dev)


def _device_grid(rows, ld, dtype, dev):
    return [[_tokens(t, ld, dtype, dev, seed=7 * i + j) for j, t in enumerate(row)] for i, row in enumerate(rows)]


def _rect(rows, i, j, limit):
    oy = sum(min(r[0].shape[2], limit) for r in rows[:i])
    ox = sum(min(t.shape[3], limit) for t in rows[i][:j])
    return oy, ox, min(rows[i][j].shape[2], limit), min(rows[i][j].shape[3], limit)


def _launch(dgrid, i, j, out, oy, ox, extent, limit, c):
    up = dgrid[i - 1][j] if i else None
    left = dgrid[i][j - 1] if j else None
    K().vae_tile_blend(dgrid[i][j], out, oy, ox, extent, limit, up=up, left=left, upleft=dgrid[i - 1][j - 1] if i and j else None, c=c)


def _stitch_on_device(rows, dgrid, extent, limit, c, dev):
    n = rows[0][0].shape[0]
    hh = sum(min(r[0].shape[2], limit) for r in rows)
    ww = sum(min(t.shape[3], limit) for t in rows[0])
    out = torch.full((n, c, hh, ww), SENTINEL, dtype=torch.float32, device=dev)
    for i in range(len(rows)):
        for j in range(len(rows[0])):
            oy, ox, _, _ = _rect(rows, i, j, limit)
            _launch(dgrid, i, j, out, oy, ox, extent, limit, c)
    return out


# (name, tile heights, tile widths, E, limit, n): the raw tiles a decoder / encoder hands the stitcher
KERNEL_GRIDS = [
    ("2x2 at 32/8/24, 16 px remainder", (32, 16), (32, 16), 8, 24, 2),
    ("3x3 at 64/16/48, 8 px remainder (e = 8 < E)", (64, 64, 8), (64, 64, 8), 16, 48, 1),
    ("1x3 at 32/8/24", (32,), (32, 32, 8), 8, 24, 1),
    ("3x1 at 32/8/24", (32, 32, 8), (32,), 8, 24, 1),
    ("2x3, remainders 24 and 16", (32, 24), (32, 32, 16), 8, 24, 1),
    ("2x2 at the real 512/128/384, 384 px second tile", (512, 384), (512, 384), 128, 384, 1),
]
# (source dtype, c, ld): the decoder's fp32 conv_out (ld = c = 3: 12-byte loads) and quant_conv's fp16 GEMM output (16-byte loads);
# on the small grids also the 16-byte fp32 form (ld 4) and the scalar forms (ld no multiple of the vector, c < ld)
LAYOUTS = [(torch.float32, 3, 3), (torch.float16, 8, 8)]
EXTRA_LAYOUTS = [(torch.float32, 3, 4), (torch.float32, 5, 7), (torch.float16, 5, 12), (torch.float16, 11, 16)]


@pytest.mark.parametrize("name,heights,widths,extent,limit,n", KERNEL_GRIDS, ids=[g[0] for g in KERNEL_GRIDS])
def test_kernel_against_the_literal_loops(dev, name, heights, widths, extent, limit, n):
    """|out - ref64| <= 16 * 2^-24 * max|inputs|: an output is two nested lerps a (1 - w) + b w, each with at most three fp32
    roundings (two products, one sum) and two of the weight (y / e and 1 - y / e)."""
    big = heights[0] >= 512
    for dtype, c, ld in LAYOUTS + ([] if big else EXTRA_LAYOUTS):
        rows = [[t.to(dtype).double() for t in row] for row in R.random_grid(heights, widths, n=n, c=c, seed=len(heights) + c)]
        ref = R.stitch(rows, extent, limit)
        dgrid = _device_grid(rows, ld, dtype, dev)
        got = _stitch_on_device(rows, dgrid, extent, limit, c, dev).cpu().double()
        assert got.shape == ref.shape
        peak = max(t.abs().max().item() for row in rows for t in row)
        err, bound = (got - ref).abs().max().item(), 16 * 2.0 ** -24 * peak
        print(f"vae_tile_blend {name}, {dtype} c {c} ld {ld}: max |err| {err:.3e}, bound {bound:.3e} (max|input| {peak:.3f})")
        assert err <= bound, (name, dtype, c, ld, err, bound)


@pytest.mark.parametrize("dtype,c,ld", LAYOUTS, ids=["fp32", "fp16"])
def test_exactness_and_confinement(dev, dtype, c, ld):
    heights, widths, extent, limit = (64, 64, 8), (64, 64, 8), 16, 48
    rows = [[t.to(dtype) for t in row] for row in R.random_grid(heights, widths, n=2, c=c, seed=5, dtype=torch.float32)]
    dgrid = _device_grid(rows, ld, dtype, dev)
    before = [[t.clone() for t in row] for row in dgrid]
    hh, ww = sum(min(v, limit) for v in heights), sum(min(v, limit) for v in widths)
    for i in range(3):
        for j in range(3):
            out = torch.full((2, c, hh, ww), SENTINEL, dtype=torch.float32, device=dev)
            oy, ox, ch, cw = _rect(rows, i, j, limit)
            _launch(dgrid, i, j, out, oy, ox, extent, limit, c)                   # ONE launch into a fresh destination
            got = out.cpu()
            inside = torch.zeros(hh, ww, dtype=torch.bool)
            inside[oy: oy + ch, ox: ox + cw] = True
            assert (got[:, :, ~inside] == SENTINEL).all(), f"tile ({i}, {j}) wrote outside its crop rectangle"
            assert (got[:, :, inside] != SENTINEL).all(), f"tile ({i}, {j}) left part of its crop rectangle unwritten"
            crop = got[:, :, oy: oy + ch, ox: ox + cw]
            T = rows[i][j].float()
            ev = min(rows[i - 1][j].shape[2], T.shape[2], extent) if i else 0
            eh = min(rows[i][j - 1].shape[3], T.shape[3], extent) if j else 0
            # outside both blend zones the source passes through bit for bit
            assert torch.equal(crop[:, :, ev:, eh:], T[:, :, ev:ch, eh:cw])
            if i:       # weight 0: row 0 outside the corner IS the neighbour's row
                U = rows[i - 1][j].float()
                assert torch.equal(crop[:, :, 0, eh:], U[:, :, U.shape[2] - ev, eh:cw])
            if j:
                L = rows[i][j - 1].float()
                assert torch.equal(crop[:, :, ev:, 0], L[:, :, ev:ch, L.shape[3] - eh])
    assert all(torch.equal(a, b) for ra, rb in zip(dgrid, before) for a, b in zip(ra, rb)), "a source tile was modified"


def test_bad_arguments_write_nothing(dev):
    from i2v_adapter_unofficial_amd._lib import HipLibraryError
    mk = lambda hh, ww, ld=3: torch.randn(1, hh, ww, ld, device=dev)
    t, u, l, ul = mk(8, 8), mk(8, 8), mk(8, 8), mk(8, 8)
    out = torch.full((1, 3, 12, 12), SENTINEL, dtype=torch.float32, device=dev)
    kw = dict(up=u, left=l, upleft=ul, c=3)
    K().vae_tile_blend(t, out.clone(), 6, 6, 2, 6, **kw)                                        # the good call the bad ones vary
    bad = [
        ("> ld", lambda: K().vae_tile_blend(t, torch.full((1, 4, 12, 12), SENTINEL, device=dev), 6, 6, 2, 6, up=u, left=l, upleft=ul, c=4)),
        ("limit", lambda: K().vae_tile_blend(t, out, 6, 6, 2, 0, **kw)),
        ("blend_extent", lambda: K().vae_tile_blend(t, out, 6, 6, 0, 6, **kw)),
        ("blend_extent", lambda: K().vae_tile_blend(t, out, 6, 6, -1, 6, **kw)),
        ("leaves the", lambda: K().vae_tile_blend(t, out, 7, 6, 2, 6, **kw)),
        ("leaves the", lambda: K().vae_tile_blend(t, out, 6, 7, 2, 6, **kw)),
        ("leaves the", lambda: K().vae_tile_blend(t, out, -1, 6, 2, 6, **kw)),
        ("leaves the", lambda: K().vae_tile_blend(t, out, 6, 6, 2, 7, **kw)),
        ("upleft comes with both", lambda: K().vae_tile_blend(t, out, 6, 6, 2, 6, up=u, upleft=ul, c=3)),
        ("upleft comes with both", lambda: K().vae_tile_blend(t, out, 6, 6, 2, 6, left=l, upleft=ul, c=3)),
        ("upleft comes with both", lambda: K().vae_tile_blend(t, out, 6, 6, 2, 6, upleft=ul, c=3)),
    ]
    for match, call in bad:
        with pytest.raises(HipLibraryError, match=match):
            call()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


def test_reduced_vae_tiled_decode_vs_oracle(dev, small_pair):
    """latents (2, 4, 6, 8), tiles of 4 latents every 3: a 2 x 3 grid with remainders of 3 and 2 latents; E = 8 px, limit 24 px.
    Tolerance: the untiled decoder's (tests/test_vae_gpu.py, rel 1e-2) -- a convex blend of tiles cannot enlarge it."""
    ov, hv = small_pair
    z = h(torch.randn(2, 4, 6, 8, generator=torch.Generator().manual_seed(11)))
    hv.enable_tiling()
    try:
        got = hv.decode(z.to(dev)).sample
    finally:
        hv.disable_tiling()
    with torch.no_grad():
        ref = R.tiled_decode(ov, z)
    assert got.shape == ref.shape == (2, 3, 48, 64) and got.dtype == torch.float32
    err, scale = compare(got, ref, rel=1e-2, name="tiled VAE decoder (reduced)")
    print(f"tiled VAE decode (reduced): max abs err {err:.3e} (max|ref| {scale:.3e})")


def test_reduced_vae_tiled_encode_vs_oracle(dev, small_pair):
    """(2, 3, 40, 72) px, tiles of 32 px every 24: a 2 x 3 grid with remainders of 16 and 24 px; E = 1 latent, limit 3.
    Tolerance: the untiled encoder moments' (rel 4.5e-3)."""
    ov, hv = small_pair
    img = h(torch.rand(2, 3, 40, 72, generator=torch.Generator().manual_seed(12)) * 2 - 1)
    hv.enable_tiling()
    try:
        got = hv.encode(img.to(dev)).latent_dist.parameters
    finally:
        hv.disable_tiling()
    with torch.no_grad():
        ref = R.tiled_encode(ov, img)
    assert got.shape == ref.shape == (2, 8, 5, 9) and got.dtype == torch.float32
    err, scale = compare(got, ref, rel=4.5e-3, name="tiled VAE encoder moments (reduced)")
    print(f"tiled VAE encode (reduced): max abs err {err:.3e} (max|ref| {scale:.3e})")


def test_sd_width_tiled_decode_vs_oracle(dev):
    """SD-1.5 width, sample_size 64: latents (1, 4, 12, 8) are a 2 x 1 grid of 8- and 6-latent tiles; E = 16 px, limit 48 px."""
    host_threads()
    ov, hv = _pair(SD_VAE, dev, seed=64)
    z = h(torch.randn(1, 4, 12, 8, generator=torch.Generator().manual_seed(13)))
    hv.enable_tiling()
    got = hv.decode(z.to(dev)).sample
    with torch.no_grad():
        ref = R.tiled_decode(ov, z)
    assert got.shape == ref.shape == (1, 3, 96, 64)
    err, scale = compare(got, ref, rel=1e-2, name="tiled VAE decoder (SD-1.5 width)")
    print(f"tiled VAE decode (SD-1.5 width): max abs err {err:.3e} (max|ref| {scale:.3e})")


def test_switch(dev, small_pair):
    _, hv = small_pair
    never = hip_model_random(SMALL_VAE, dev, seed=31, cls=pkg().AutoencoderKL)        # the same weights, tiling never enabled
    g = torch.Generator().manual_seed(14)
    z_small, z_large = h(torch.randn(2, 4, 4, 4, generator=g)).to(dev), h(torch.randn(2, 4, 6, 8, generator=g)).to(dev)
    x_small, x_large = (h(torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(dev),
                        h(torch.rand(2, 3, 40, 72, generator=g) * 2 - 1).to(dev))
    dec = lambda m, z: m.decode(z).sample
    enc = lambda m, x: m.encode(x).latent_dist.parameters
    off = [dec(hv, z_small), enc(hv, x_small), dec(hv, z_large), enc(hv, x_large)]
    hv.enable_tiling()
    try:
        assert hv.use_tiling
        on = [dec(hv, z_small), enc(hv, x_small), dec(hv, z_large), enc(hv, x_large)]
    finally:
        hv.disable_tiling()
    # an input that fits one tile takes the existing path, bit for bit
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    # a large one is really tiled: every tile has its own GroupNorm statistics and attention, so the result differs
    for a, b in ((on[2], off[2]), (on[3], off[3])):
        assert a.shape == b.shape and (a - b).abs().max().item() > 1e-3
    # ... and switching it off again is the VAE that never had it on
    assert torch.equal(dec(hv, z_large), dec(never, z_large)) and torch.equal(enc(hv, x_large), enc(never, x_large))
    assert torch.equal(dec(hv, z_large), off[2]) and torch.equal(enc(hv, x_large), off[3])


def test_pipeline_with_vae_tiling(dev, small_pair):
    """the reduced models of test_vae_gpu's end-to-end test at 64 x 48 px with a VAE of sample_size 32: the frames (8 x 6 latents: a
    3 x 2 grid) and the condition image (64 x 48 px: 3 x 2) are both tiled."""
    import PIL.Image
    from oracle.vae import DiagonalGaussianDistribution as OracleDist
    from tests.parity import hip_unet_from_oracle, oracle_small_unet
    p = pkg()
    ov, hv = small_pair
    hu = hip_unet_from_oracle(oracle_small_unet(), dev)
    pipe = p.I2VAdapterPipeline(vae=hv, unet=hu)
    g = torch.Generator().manual_seed(3)
    image = PIL.Image.fromarray((torch.rand(80, 72, 3, generator=g) * 255).to(torch.uint8).numpy())
    pe, ne = h(torch.randn(1, 7, 64, generator=g)), h(torch.randn(1, 7, 64, generator=g))
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image=image, height=64, width=48, num_frames=4,
              num_inference_steps=4, guidance_scale=7.5, frame_similarity_sample_ratio=0.3)
    gens = lambda: dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                        prior_noise_generator=torch.Generator().manual_seed(7))
    sf = hv.config["scaling_factor"]
    untiled = pipe(output_type="pt", **kw, **gens()).frames
    assert untiled.shape == (1, 4, 3, 64, 48)
    pipe.enable_vae_tiling()
    try:
        assert hv.use_tiling
        lat = pipe(output_type="latent", **kw, **gens()).frames
        vid = pipe(output_type="pt", **kw, **gens()).frames
        assert lat.shape == (1, 4, 4, 8, 6) and vid.shape == (1, 4, 3, 64, 48) and torch.isfinite(vid).all()
        assert torch.equal(vid[0], hv.decode((1 / sf * lat)[0]).sample)                 # (use_tiling is on: the tiled decode)
        with torch.no_grad():
            ref = R.tiled_decode(ov, lat[0].cpu() / sf)
        compare(vid[0], ref, rel=1e-2, name="pipeline decode_latents with VAE tiling vs tiled oracle VAE")
        assert (vid - untiled).abs().max().item() > 1e-3                                # the switch reached the VAE
        pipe.enable_vae_slicing()
        sliced = pipe(output_type="pt", **kw, **gens()).frames
        pipe.disable_vae_slicing()
        assert torch.equal(sliced, vid)
        # the condition image goes through tiled_encode.  sample = mean + exp(logvar / 2) eps on the same eps: its error is the
        # moments' (bound 4.5e-3 of max|moments|) times 1 + |eps| std / 2 <~ 3, against a max|sample| ~ 3x the moments': the same rel
        pre = pipe.image_processor.preprocess(image, height=64, width=48)
        got = pipe.encode_condition_image(image, 64, 48, generator=torch.Generator().manual_seed(5))
        with torch.no_grad():
            ref_lat = OracleDist(R.tiled_encode(ov, pre.float())).sample(torch.Generator().manual_seed(5)) * sf
        assert got.shape == ref_lat.shape == (1, 4, 8, 6)
        compare(got, ref_lat, rel=4.5e-3, name="pipeline condition-image latents with VAE tiling vs tiled oracle VAE")
    finally:
        pipe.disable_vae_tiling()
    assert not hv.use_tiling
    assert torch.equal(pipe(output_type="pt", **kw, **gens()).frames, untiled)
