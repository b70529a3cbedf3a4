"""What FreeInit costs on the GPU, in one process:

  (a) mix:     `kernels.freeinit_mix` (five direct-DFT launches) against the same arithmetic written with torch.fft on the device (fftn of
               two tensors, fftshift, mask and 1 - mask, add, ifftshift, ifftn, .real: rocFFT plus elementwise launches and complex
               temporaries), at (1, 16, 4, 64, 64) and (1, 32, 4, 96, 96); device events around `--reps` calls, median of `--windows`
               windows after a warm-up, the two forms alternating; and their largest difference;
  (b) sample:  the wall time of a whole `pipe(...)` call on bench.py's default problem (SD-1.5 width, 16 frames, 512 x 512, CFG on,
               latents out) on a cached graph: a plain call, 3 FreeInit rounds (against 3 x the plain call) and 3 rounds with
               use_fast_sampling (every round re-captures: its cost is in the figure);
  (c) the one condition: a mix must cost less than one replayed denoising step at the same shape.

Run once on the GPU:  python tools/freeinit_probe.py --out profiles/freeinit_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "freeinit_probe.json"))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--reps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=21)
    ap.add_argument("--no-sample", action="store_true", help="only the mix (a)")
    args = ap.parse_args()

    import torch

    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.free_init import free_init_filter

    K = pkg.kernels
    dev = torch.device("cuda:0")
    a999 = float(pkg.DDIMScheduler().alphas_cumprod[999])
    sa, sb = a999 ** 0.5, (1 - a999) ** 0.5
    dims = (1, 3, 4)

    def torch_mix(lat, noise, zr, lpf):
        z_t = sa * lat + sb * noise
        m = lpf[None, :, None]
        xf = torch.fft.fftshift(torch.fft.fftn(z_t, dim=dims), dim=dims)
        nf = torch.fft.fftshift(torch.fft.fftn(zr, dim=dims), dim=dims)
        return torch.fft.ifftn(torch.fft.ifftshift(xf * m + nf * (1 - m), dim=dims), dim=dims).real

    def window(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / args.reps          # us per call

    result = {"mix": {"what": f"us per call, device events around {args.reps} calls, median / min of {args.windows} windows after warm-up, "
                              "hip = kernels.freeinit_mix, torch = torch.fft on the device", "rows": []}}
    for shape in ((1, 16, 4, 64, 64), (1, 32, 4, 96, 96)):
        g = torch.Generator().manual_seed(1)
        lat, noise, zr = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
        lpf = free_init_filter((shape[1], shape[3], shape[4]), device=dev)
        hip, ref = (lambda: K.freeinit_mix(lat, noise, zr, lpf, sa, sb)), (lambda: torch_mix(lat, noise, zr, lpf))
        diff = (hip() - ref()).abs().max().item()
        for _ in range(3):
            window(hip), window(ref)
        t_hip, t_ref = [], []
        for _ in range(args.windows):
            t_hip.append(window(hip))
            t_ref.append(window(ref))
        row = dict(shape=list(shape), hip_us_median=round(statistics.median(t_hip), 2), hip_us_min=round(min(t_hip), 2),
                   torch_us_median=round(statistics.median(t_ref), 2), torch_us_min=round(min(t_ref), 2),
                   torch_over_hip=round(statistics.median(t_ref) / statistics.median(t_hip), 3), max_abs_diff=diff)
        result["mix"]["rows"].append(row)
        print(json.dumps(row), flush=True)

    if not args.no_sample:
        import bench
        unet = bench.build_hip_model(dev, seed=1234)
        pipe = pkg.I2VAdapterPipeline(unet=unet)
        d = bench.sample_inputs(0, args.frames, args.size // 8, ip=False)
        gens = lambda: dict(generator=torch.Generator().manual_seed(1), prior_mask_generator=torch.Generator().manual_seed(2),
                            prior_noise_generator=torch.Generator().manual_seed(3))
        call = dict(prompt_embeds=d["pe"].half(), negative_prompt_embeds=d["ne"].half(), condition_image_latents=d["cond"],
                    num_frames=args.frames, blur_sigma=0.8, output_type="latent", num_inference_steps=args.steps, guidance_scale=7.5)

        def sample_ms(label, repeats=3):
            pipe(**call, **gens())                     # warm: captures (fast sampling re-captures every round of every call anyway)
            out = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                frames = pipe(**call, **gens()).frames
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
                assert bool(torch.isfinite(frames).all())
            row = dict(config=label, steps=args.steps, wall_ms=[round(v, 2) for v in out], wall_ms_median=round(statistics.median(out), 2))
            print(json.dumps(row), flush=True)
            return row

        rows = [sample_ms("plain")]
        graph, gst = next(iter(pipe._graph_cache.values()))
        step = []
        for _ in range(5):
            gst["step_idx"].zero_()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(10):
                graph.replay()
            e.record()
            torch.cuda.synchronize()
            step.append(s.elapsed_time(e) / 10)
        pipe.enable_free_init(num_iters=3)
        rows.append(sample_ms("free_init x3"))
        pipe.enable_free_init(num_iters=3, use_fast_sampling=True)
        rows.append(sample_ms("free_init x3, use_fast_sampling (re-captures included)"))
        pipe.disable_free_init()
        plain = rows[0]["wall_ms_median"]
        for row in rows:
            row["over_plain"] = round(row["wall_ms_median"] / plain, 3)
        mix_ms = result["mix"]["rows"][0]["hip_us_median"] / 1e3
        result["sample"] = {"what": "wall ms of one pipe(...) call, latents out (prior, tables, steps, mixes; no VAE), second and later "
                                    "calls of each configuration", "rows": rows,
                            "three_plain_calls_ms": round(3 * plain, 2)}
        result["condition"] = dict(what="one mix against one replayed denoising step at 16 frames x 512 x 512 (the mix's shape "
                                        "(1, 16, 4, 64, 64))", step_ms_median=round(statistics.median(step), 3), mix_ms=round(mix_ms, 4),
                                   mix_over_step=round(mix_ms / statistics.median(step), 5), holds=bool(mix_ms < statistics.median(step)))
        print(json.dumps(result["condition"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
