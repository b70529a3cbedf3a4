"""What LCM sampling costs and buys on bench.py's default problem (SD-1.5 width, 16 frames, 512 x 512, CFG on), in one process:

  (a) step:    the replayed hipGraph step with LCMScheduler (i2v_lcm_cfg_step: one more fp32 tensor read, the step's noise row)
               against DDIMScheduler (i2v_ddim_cfg_step), captured and timed alternately (DDIM, LCM, DDIM, LCM) so that clock drift
               shows as a difference between the two rounds of one scheduler;
  (b) sample:  the wall time of a whole `pipe(...)` call, latents out, on a cached graph (the second call of each configuration):
               4, 6 and 8 LCM steps at guidance 1.5 against 25 DDIM steps at guidance 7.5.  The LCM calls include drawing the noise
               table on the host generator and copying it to the device.

Run once on the GPU:  python tools/lcm_probe.py --out profiles/lcm_probe.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "lcm_probe.json"))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--replays", type=int, default=10, help="graph replays per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()

    import torch

    import bench
    import i2v_adapter_unofficial_amd as pkg

    dev = torch.device("cuda:0")
    unet = bench.build_hip_model(dev, seed=1234)
    pipe = pkg.I2VAdapterPipeline(unet=unet)
    d = bench.sample_inputs(0, args.frames, args.size // 8, ip=False)
    gens = lambda: dict(generator=torch.Generator().manual_seed(1), prior_mask_generator=torch.Generator().manual_seed(2),
                        prior_noise_generator=torch.Generator().manual_seed(3))
    call = dict(prompt_embeds=d["pe"].half(), negative_prompt_embeds=d["ne"].half(), condition_image_latents=d["cond"],
                num_frames=args.frames, blur_sigma=0.8, output_type="latent")
    schedulers = {"ddim": lambda: pkg.DDIMScheduler(), "lcm": lambda: pkg.LCMScheduler()}

    def step_windows(kind, n_steps, guidance):
        """capture the step of `kind` (a whole sample through the pipeline), then time windows of replays of that graph"""
        pipe.scheduler = schedulers[kind]()
        pipe(**call, num_inference_steps=n_steps, guidance_scale=guidance, **gens())
        graph, gst = next(iter(pipe._graph_cache.values()))
        saved = gst["latents"].clone()
        out = []
        for _ in range(args.windows):
            gst["latents"].copy_(saved)
            gst["step_idx"].zero_()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.replays):
                graph.replay()
            e.record()
            torch.cuda.synchronize()
            out.append(s.elapsed_time(e) / args.replays)
        return out

    result = {"problem": dict(frames=args.frames, size=args.size, cfg_copies=2, replays_per_window=args.replays, windows=args.windows),
              "step_ms": {"what": "ms per replayed step, every window; the same graph as the pipeline replays; 8-step schedules, guidance 7.5",
                          "rounds": []}}
    for r in range(args.rounds):
        row = {}
        for kind in ("ddim", "lcm"):
            w = step_windows(kind, 8, 7.5)
            row[kind] = dict(windows=[round(v, 4) for v in w], median=round(statistics.median(w), 4), min=round(min(w), 4))
        row["lcm_over_ddim_median"] = round(row["lcm"]["median"] / row["ddim"]["median"], 5)
        result["step_ms"]["rounds"].append(row)
        print(json.dumps(row), flush=True)

    def sample_ms(kind, n_steps, guidance, repeats=3):
        pipe.scheduler = schedulers[kind]()
        pipe(**call, num_inference_steps=n_steps, guidance_scale=guidance, **gens())          # captures
        out = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frames = pipe(**call, num_inference_steps=n_steps, guidance_scale=guidance, **gens()).frames
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
            assert bool(torch.isfinite(frames).all())
        return dict(scheduler=kind, steps=n_steps, guidance=guidance, wall_ms=[round(v, 2) for v in out],
                    wall_ms_median=round(statistics.median(out), 2))

    rows = [sample_ms("ddim", 25, 7.5)] + [sample_ms("lcm", n, 1.5) for n in (4, 6, 8)]
    base = rows[0]["wall_ms_median"]
    for row in rows:
        row["speedup_over_ddim25"] = round(base / row["wall_ms_median"], 3)
        print(json.dumps(row), flush=True)
    result["sample"] = {"what": "wall ms of one pipe(...) call on a cached graph, latents out (prior, tables, steps; no VAE)", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
