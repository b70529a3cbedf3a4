"""Hires-fix measurement, on one MI355X, in ONE process:

  (a) the `i2v_resize_renoise_f32` launch at the largest real case -- 16 frames x 4 channels = 64 planes of 64 x 64 latents to 96 x 96
      and to 128 x 128, with the re-noise fused in -- against `K.axpby` on the output shape (the launch the fusion saves: it reads and
      writes the same output bytes) and against the unfused pair resize + axpby, alternating windows.  The launch moves at most 9.4 MB:
      the times are launch latency and cache behaviour, not bandwidth;
  (b) a hires sample at bench.py's synthetic SD-1.5-width UNet, latents in and latents out -- `--steps` steps at `--size`^2, then
      int(steps * 0.6) steps at 1.5 x the size -- against `--steps` direct steps at the target size, alternating, each after one
      warm-up sample that captures its graphs.

usage (GPU box, repository root):   timeout -k 10 900 python tools/hires_probe.py --out profiles/hires_probe.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/hires_probe.json")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--strength", type=float, default=0.6)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50, help="launches per window")
    ap.add_argument("--samples", type=int, default=3, help="timed samples per arm of (b)")
    ap.add_argument("--no-sample", action="store_true", help="(a) only")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.hires_fix import device_tables

    assert torch.cuda.is_available(), "the probe measures the GPU: there is nothing to time without one"
    dev, K = torch.device("cuda:0"), pkg.kernels

    def window(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / reps                 # us per call

    def alternate(fns):
        for fn in fns.values():
            window(fn, 3)
        t = {k: [] for k in fns}
        for _ in range(args.windows):
            for k, fn in fns.items():
                t[k].append(window(fn, args.reps))
        return {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1)) for k, v in t.items()}

    result = {"what": f"device events around {args.reps} calls, {args.windows} alternating windows after warm-up; us per call",
              "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        # ---------------------------------------------------------------- (a) the kernel
        g = torch.Generator(device=dev).manual_seed(1)
        planes, h = args.frames * 4, args.size // 8
        src = torch.randn((1, args.frames, 4, h, h), generator=g, device=dev)
        result["kernel"] = {}
        for target in (h * 3 // 2, h * 2):
            tables = device_tables(h, h, target, target, "bicubic-antialiased", dev)
            noise = torch.randn((1, args.frames, 4, target, target), generator=g, device=dev)
            y = torch.randn_like(noise)
            out_bytes = noise.numel() * 4
            t = alternate({"resize_renoise_fused": lambda: K.resize_renoise(src, tables, noise, 0.6, 0.8),
                           "resize_only": lambda: K.resize_renoise(src, tables),
                           "axpby_output_shape": lambda: K.axpby(y, noise, 1.0, 1e-3),
                           "resize_then_axpby": lambda: K.axpby(K.resize_renoise(src, tables), noise, 0.6, 0.8)})
            result["kernel"][f"{h}->{target}"] = dict(planes=planes, fused_bytes_moved=src.numel() * 4 + 2 * out_bytes,
                                                       axpby_bytes_moved=3 * out_bytes, **t)
            del noise, y

        # ---------------------------------------------------------------- (b) the sample
        if not args.no_sample:
            unet = bench.build_hip_model(dev, seed=1234)
            pipe = pkg.I2VAdapterPipeline(unet=unet)
            big = 8 * round(args.size * 1.5 / 8)
            s = bench.sample_inputs(0, args.frames, h, False)
            kw = dict(prompt_embeds=s["pe"], negative_prompt_embeds=s["ne"], num_frames=args.frames, num_inference_steps=args.steps,
                      guidance_scale=7.5, output_type="latent")
            gens = lambda: dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                                prior_noise_generator=torch.Generator().manual_seed(7))
            cond_big = pipe.upscale_latents(s["cond"][:, None], big, big, upscaler="bicubic-antialiased")[:, 0].cpu()

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            def hires():
                pipe.enable_hires_fix(scale=1.5, strength=args.strength)
                try:
                    return pipe(**kw, condition_image_latents=s["cond"], **gens()).frames
                finally:
                    pipe.disable_hires_fix()

            def direct():
                # (its own pipeline object: one graph per pipeline, so the arms do not evict each other's captures)
                return direct_pipe(**kw, condition_image_latents=cond_big, **gens()).frames

            direct_pipe = pkg.I2VAdapterPipeline(unet=unet)
            first = dict(hires_ms=round(timed(hires), 1), direct_ms=round(timed(direct), 1))          # (captures included)
            t = {"hires": [], "direct": []}
            for _ in range(args.samples):
                t["hires"].append(timed(hires))
                t["direct"].append(timed(direct))
            second_steps = int(args.steps * args.strength)
            result["sample"] = dict(
                what=f"{args.frames} frames, CFG, latents in and out (no VAE): hires = {args.steps} steps at {args.size}^2 + {second_steps} "
                     f"steps at {big}^2; direct = {args.steps} steps at {big}^2; wall ms per sample, alternating, graphs replayed",
                first_sample_with_captures=first, graphs_kept_by_the_hires_pipeline=len(pipe._graph_cache),
                **{k: dict(median_ms=round(statistics.median(v), 1), min_ms=round(min(v), 1), max_ms=round(max(v), 1)) for k, v in t.items()},
                hires_over_direct=round(statistics.median(t["hires"]) / statistics.median(t["direct"]), 4))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
