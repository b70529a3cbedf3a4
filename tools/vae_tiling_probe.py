"""Tiled VAE measurement, on one MI355X, everything inside ONE call of this script:

  (a) decode of latents (1, 4, 96, 96) -- 768 x 768 px, BASELINE config 5's frame -- at SD-1.5 width with random weights, tiled
      (`enable_tiling`: a 2 x 2 grid of 64- and 48-latent tiles) and untiled in one process: torch.cuda.max_memory_allocated of each
      and the median of a few timed decodes of each after warm-up, alternating.
  (b) `i2v_vae_tile_blend` at that geometry (fp32 sources, c = ld = 3, tiles of 512 / 384 px, E = 128, limit = 384: the four launches
      that stitch one 768 x 768 frame) next to the plain copy of the same output, `i2v_tokens_to_nchw` of a [1, 768, 768, 3] fp32
      image: time per frame from device events around replays of a captured graph of back-to-back launches, and bytes/s from the
      bytes the shapes say are moved.

One GPU process at a time: each step is a child process under its own time limit, and the first one that fails ends the script (nothing
more is started on the GPU after a failure).  usage (GPU box, repository root):   python tools/vae_tiling_probe.py --out FILE.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATENT = 96                      # 768 px
STEP_LIMIT_S = {"decode": 420, "blend": 180}


def _median_ms(fn, torch, rounds, inner):
    """median over `rounds` windows of `inner` back-to-back calls, device events around each window: ms per call"""
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return statistics.median(out), min(out), max(out)


def worker_decode(args):
    sys.path.insert(0, ROOT)
    import torch
    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    dev = torch.device("cuda:0")
    vae = pkg.AutoencoderKL()
    init_random_weights_(vae, seed=3)
    vae = vae.to(device=dev, dtype=torch.float16).eval()
    z = torch.randn(1, 4, LATENT, LATENT, generator=torch.Generator().manual_seed(1)).to(dev)
    res = {"latents": list(z.shape), "tile_latent_min_size": vae.tile_latent_min_size, "tile_sample_min_size": vae.tile_sample_min_size}
    modes = {"untiled": False, "tiled": True}
    for name, on in modes.items():                      # warm-up of every shape of both paths, and the peak of each on its own
        vae.enable_tiling(on)
        vae.decode(z)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        img = vae.decode(z).sample
        torch.cuda.synchronize()
        res[name] = {"max_memory_allocated_bytes": torch.cuda.max_memory_allocated(), "allocated_before_bytes": base,
                     "output": list(img.shape)}
        del img
    times = {k: [] for k in modes}
    for _ in range(args.rounds):                        # alternating: both see the same clock and neighbours
        for name, on in modes.items():
            vae.enable_tiling(on)
            med, _, _ = _median_ms(lambda: vae.decode(z), torch, 1, args.decodes)
            times[name].append(med)
    for name in modes:
        res[name].update(decode_ms_median=statistics.median(times[name]), decode_ms_min=min(times[name]),
                         decode_ms_max=max(times[name]), timed_decodes=args.rounds * args.decodes)
    vae.enable_tiling(True)
    a = vae.decode(z).sample
    vae.disable_tiling()
    b = vae.decode(z).sample
    res["max_abs_difference_tiled_vs_untiled"] = (a - b).abs().max().item()
    res["max_abs_untiled"] = b.abs().max().item()
    print(json.dumps(res))


def blend_bytes(heights, widths, extent, limit, c, ld, elt):
    """bytes one stitched frame needs: per tile, its crop from the tile, the blend zones from the neighbours, the crop written in fp32"""
    rd = wr = 0
    for i, th in enumerate(heights):
        for j, tw in enumerate(widths):
            ch, cw = min(th, limit), min(tw, limit)
            ev = min(heights[i - 1], th, extent) if i else 0
            eh = min(widths[j - 1], tw, extent) if j else 0
            rd += (ch * cw + ev * cw + ch * eh + ev * eh) * ld * elt
            wr += ch * cw * c * 4
    return rd, wr


def worker_blend(args):
    sys.path.insert(0, ROOT)
    import torch
    import i2v_adapter_unofficial_amd as pkg
    K = pkg.kernels
    dev = torch.device("cuda:0")
    heights = widths = (512, 384)
    extent, limit, c = 128, 384, 3
    g = torch.Generator().manual_seed(2)
    grid = [[torch.randn(1, th, tw, c, generator=g).to(dev) for tw in widths] for th in heights]
    side = sum(min(v, limit) for v in heights)
    out = torch.empty(1, c, side, side, device=dev)
    whole = torch.randn(1, side, side, c, generator=g).to(dev)

    def stitch():
        oy = 0
        for i, th in enumerate(heights):
            ox = 0
            for j, tw in enumerate(widths):
                K.vae_tile_blend(grid[i][j], out, oy, ox, extent, limit, up=grid[i - 1][j] if i else None,
                                 left=grid[i][j - 1] if j else None, upleft=grid[i - 1][j - 1] if i and j else None)
                ox += min(tw, limit)
            oy += min(th, limit)

    copy = lambda: K.tokens_to_nchw(whole, dtype=torch.float32)
    graphs = {}
    for name, fn in (("blend", stitch), ("copy", copy)):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        # the launches are a few microseconds each, less than a host call: replay them from a captured graph (one linear chain of
        # `launches` frames), so that the events time the device and not the enqueue
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(args.launches):
                fn()
        graphs[name].replay()
    torch.cuda.synchronize()
    t = {"blend": [], "copy": []}
    for _ in range(args.rounds):
        for name in ("blend", "copy"):
            t[name].append(_median_ms(graphs[name].replay, torch, 1, 5)[0] / args.launches)
    rd, wr = blend_bytes(heights, widths, extent, limit, c, c, 4)
    crd = cwr = side * side * c * 4
    res = {"geometry": {"tiles_px": list(heights), "blend_extent": extent, "limit": limit, "c": c, "ld": c, "source": "fp32",
                        "output": [1, c, side, side]}}
    for name, (r, w, launches) in (("blend", (rd, wr, len(heights) * len(widths))), ("copy", (crd, cwr, 1))):
        med = statistics.median(t[name])
        res[name] = {"launches_per_frame": launches, "ms_per_frame_median": med, "ms_per_frame_min": min(t[name]),
                     "ms_per_frame_max": max(t[name]), "bytes_read": r, "bytes_written": w, "gb_per_s": (r + w) / (med * 1e-3) / 1e9}
    res["copy"]["kernel"] = "i2v_tokens_to_nchw [1, 768, 768, 3] fp32 -> NCHW fp32"
    res["blend"]["kernel"] = "i2v_vae_tile_blend x 4 (one 768 x 768 frame)"
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "vae_tiling_probe.json"))
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per variant")
    ap.add_argument("--decodes", type=int, default=3, help="decodes per window")
    ap.add_argument("--launches", type=int, default=200, help="stitched frames per window of the kernel measurement")
    ap.add_argument("--worker", choices=["decode", "blend"])
    args = ap.parse_args()
    if args.worker:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("vae_tiling_probe: needs a GPU (a measurement does not fall back)")
        with torch.no_grad():
            {"decode": worker_decode, "blend": worker_blend}[args.worker](args)
        return 0
    result = {}
    for step in ("decode", "blend"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]), sys.executable, os.path.abspath(__file__), "--worker", step,
               "--rounds", str(args.rounds), "--decodes", str(args.decodes), "--launches", str(args.launches)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            print(f"vae_tiling_probe: step {step} ended with status {r.returncode}; nothing more is run\n{r.stdout[-2000:]}\n"
                  f"{r.stderr[-4000:]}", file=sys.stderr)
            return 1
        result[step] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{step}: {json.dumps(result[step])}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
