"""Tiled-VAE reference for the tests (the oracle AutoencoderKL has no tiling): diffusers 0.24's `blend_v` / `blend_h` / `tiled_decode` /
`tiled_encode` restated literally -- Python loops over rows and columns, IN-PLACE blends in raster order, crop, torch.cat -- in the
dtype of what they are given (fp32 for the oracle VAE, fp64 for the kernel tests), over any pair of callables or over an oracle
`AutoencoderKL`; a stitcher of the same loops for a grid of already-made raw tiles; and the closed four-tile form that
i2v_vae_tile_blend implements (include/i2v_hip.h), in fp64 torch, which never modifies a tile."""
import torch


def geometry(tile_in, tile_out, f=0.25):
    """(overlap in input elements, blend extent E and limit in output elements), as diffusers computes them"""
    extent = int(tile_out * f)
    return int(tile_in * (1 - f)), extent, tile_out - extent


def blend_v(a, b, blend_extent):
    """in place on b: its first e = min(a.H, b.H, E) rows cross-fade from a's last e rows; returns b"""
    blend_extent = min(a.shape[2], b.shape[2], blend_extent)
    for y in range(blend_extent):
        b[:, :, y, :] = a[:, :, -blend_extent + y, :] * (1 - y / blend_extent) + b[:, :, y, :] * (y / blend_extent)
    return b


def blend_h(a, b, blend_extent):
    blend_extent = min(a.shape[3], b.shape[3], blend_extent)
    for x in range(blend_extent):
        b[:, :, :, x] = a[:, :, :, -blend_extent + x] * (1 - x / blend_extent) + b[:, :, :, x] * (x / blend_extent)
    return b


def stitch(rows, blend_extent, limit):
    """rows[i][j]: the raw tiles [N, C, h, w] of a grid.  The literal second half of tiled_decode / tiled_encode, on clones (the
    caller's tiles stay raw): blend every tile with the ALREADY BLENDED tile above and to the left, crop, concatenate."""
    rows = [[t.clone() for t in row] for row in rows]
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = blend_v(rows[i - 1][j], tile, blend_extent)
            if j > 0:
                tile = blend_h(row[j - 1], tile, blend_extent)
            result_row.append(tile[:, :, :limit, :limit])
        result_rows.append(torch.cat(result_row, dim=3))
    return torch.cat(result_rows, dim=2)


def tiled(x, fn, tile, overlap, blend_extent, limit):
    """the literal loop: fn on x[:, :, i : i + tile, j : j + tile] for i, j in range(0, size, overlap), then `stitch`"""
    rows = []
    for i in range(0, x.shape[2], overlap):
        rows.append([fn(x[:, :, i: i + tile, j: j + tile]) for j in range(0, x.shape[3], overlap)])
    return stitch(rows, blend_extent, limit)


def vae_geometry(vae):
    ts = vae.config["sample_size"]
    return ts, int(ts / (2 ** (len(vae.config["block_out_channels"]) - 1)))


def tiled_decode(vae, z, f=0.25):
    """oracle AutoencoderKL, tiled as diffusers 0.24 does: z (N, 4, h, w) -> (N, 3, 8h, 8w)"""
    ts, tl = vae_geometry(vae)
    overlap, extent, limit = geometry(tl, ts, f)
    return tiled(z, lambda t: vae.decoder(vae.post_quant_conv(t)), tl, overlap, extent, limit)


def tiled_encode(vae, x, f=0.25):
    """-> the stitched moments (N, 8, H / 8, W / 8): mean | logvar before the clamp, what DiagonalGaussianDistribution receives"""
    ts, tl = vae_geometry(vae)
    overlap, extent, limit = geometry(ts, tl, f)
    return tiled(x, lambda t: vae.quant_conv(vae.encoder(t)), ts, overlap, extent, limit)


def random_grid(heights, widths, n=1, c=3, seed=0, dtype=torch.float64):
    """raw N(0, 1) tiles [N, C, h, w] of a grid with the given tile heights and widths"""
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, c, h, w, generator=g, dtype=torch.float64).to(dtype) for w in widths] for h in heights]


def closed_form_tile(T, U, L, UL, blend_extent, limit):
    """the crop of one tile from at most four RAW tiles [N, C, h, w] (None = no neighbour), fp64, as the kernel evaluates it"""
    lerp = lambda a, b, w: a * (1 - w) + b * w
    T = T.double()
    th, tw = T.shape[2:]
    ev = min(U.shape[2], th, blend_extent) if U is not None else 0
    eh = min(L.shape[3], tw, blend_extent) if L is not None else 0
    v = T.clone()
    wy = (torch.arange(ev, dtype=torch.float64) / max(ev, 1)).view(1, 1, ev, 1)
    wx = (torch.arange(eh, dtype=torch.float64) / max(eh, 1)).view(1, 1, 1, eh)
    if ev:
        FU = U.double()[:, :, U.shape[2] - ev:, :].clone()
        if eh and UL is not None:
            FU[:, :, :, :eh] = lerp(UL.double()[:, :, UL.shape[2] - ev:, UL.shape[3] - eh:], FU[:, :, :, :eh], wx)
        v[:, :, :ev] = lerp(FU, T[:, :, :ev], wy)
    if eh:
        FL = L.double()[:, :, :, L.shape[3] - eh:].clone()
        if ev and UL is not None:
            FL[:, :, :ev] = lerp(UL.double()[:, :, UL.shape[2] - ev:, UL.shape[3] - eh:], FL[:, :, :ev], wy)
        v[:, :, :, :eh] = lerp(FL, v[:, :, :, :eh], wx)
    return v[:, :, :limit, :limit]


def closed_form_stitch(rows, blend_extent, limit):
    """the grid through `closed_form_tile`: every tile from raw neighbours, in any order"""
    out_rows = []
    for i, row in enumerate(rows):
        out_rows.append(torch.cat([closed_form_tile(t, rows[i - 1][j] if i else None, row[j - 1] if j else None,
                                                    rows[i - 1][j - 1] if i and j else None, blend_extent, limit)
                                   for j, t in enumerate(row)], dim=3))
    return torch.cat(out_rows, dim=2)
