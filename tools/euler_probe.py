"""What the Euler samplers cost next to DDIM, in one process:

  (a) kernels: `i2v_sigma_prep` and `i2v_euler_cfg_step` (Euler: no noise table; ancestral: with one) at 16 frames of 64 x 64 latents
               with CFG, against `i2v_ddim_prep`, `i2v_ddim_cfg_step` and `i2v_lcm_cfg_step` on the same operands and against a
               device-to-device copy of as many bytes as the Euler step moves, each timed with device events over windows of back-to-back
               launches (a step wrapper launches the update and the one-thread counter bump: two launches per call);
  (b) step:    the replayed hipGraph step on bench.py's default problem (SD-1.5 width, 16 frames, 512 x 512, CFG on) under
               EulerDiscreteScheduler, EulerAncestralDiscreteScheduler and DDIMScheduler, captured and timed alternately (DDIM, Euler,
               Euler a, DDIM, ...) so that clock drift shows as a difference between the rounds of one scheduler.  Every window is kept:
               the spread is the result, not only the median.

Run once on the GPU:  python tools/euler_probe.py --out profiles/euler_probe.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SD15 = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "euler_probe.json"))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--replays", type=int, default=10, help="graph replays per timed window")
    ap.add_argument("--launches", type=int, default=200, help="kernel launches per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip_step", action="store_true", help="part (a) only (no UNet is built)")
    args = ap.parse_args()

    import torch

    import i2v_adapter_unofficial_amd as pkg

    K = pkg.kernels
    dev = torch.device("cuda:0")
    summary = lambda w: dict(windows=[round(v, 4) for v in w], median=round(statistics.median(w), 4), min=round(min(w), 4),
                             max=round(max(w), 4))

    def windows_of(fn, per_window, reset=None):
        for _ in range(20):             # warm-up: code objects loaded, clocks up
            fn()
        out = []
        for _ in range(args.windows):
            if reset is not None:       # (the steps' updates compound: a fresh operand per window keeps it finite)
                reset()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(per_window):
                fn()
            e.record()
            torch.cuda.synchronize()
            out.append(s.elapsed_time(e) / per_window)
        return out

    # ---- (a) the kernels alone
    b, f, c, hw, c_pad, copies, n_steps = 1, args.frames, 4, 64, 8, 2, 25
    g = torch.Generator().manual_seed(1)
    lat = torch.randn(b, f, c, hw, hw, generator=g).to(dev)
    cond = torch.randn(b, c, hw, hw, generator=g).to(dev)
    tok = torch.randn(copies * b * f, hw, hw, c_pad, generator=g).half().to(dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    tables = {}
    for name, cls in (("euler", pkg.EulerDiscreteScheduler), ("euler_ancestral", pkg.EulerAncestralDiscreteScheduler),
                      ("ddim", pkg.DDIMScheduler), ("lcm", pkg.LCMScheduler)):
        s = cls(**SD15)
        s.set_timesteps(n_steps)
        tables[name] = (s, s.step_coefficients(s.timesteps).to(dev))
    anc_noise = tables["euler_ancestral"][0].step_noise(tables["euler_ancestral"][0].timesteps, tuple(lat.shape), g, dev)
    lcm_noise = tables["lcm"][0].step_noise(tables["lcm"][0].timesteps, tuple(lat.shape), g, dev)
    step_bytes = 2 * lat.numel() * 4 + copies * b * f * hw * hw * c * 2         # latents in and out, eps of both CFG halves (fp16)
    prep_bytes = lat.numel() * 4 + tok.numel() * 2                              # latents in, the padded fp16 model input out
    src_step, dst_step = (torch.empty(step_bytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    src_prep, dst_prep = (torch.empty(prep_bytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    kernels = {
        "ddim_prep": lambda: K.ddim_prep(lat, cond, c_pad, copies),
        "sigma_prep": lambda: K.sigma_prep(lat, cond, tables["euler"][1], idx, c_pad, copies),
        "copy_of_prep_bytes": lambda: dst_prep.copy_(src_prep),
        "ddim_cfg_step": lambda: K.ddim_cfg_step(lat, tok, tables["ddim"][1], idx, 7.5, copies),
        "lcm_cfg_step": lambda: K.lcm_cfg_step(lat, lcm_noise, tok, tables["lcm"][1], idx, 7.5, copies),
        "euler_cfg_step": lambda: K.euler_cfg_step(lat, None, tok, tables["euler"][1], idx, 7.5, copies),
        "euler_ancestral_cfg_step": lambda: K.euler_cfg_step(lat, anc_noise, tok, tables["euler_ancestral"][1], idx, 7.5, copies),
        "copy_of_step_bytes": lambda: dst_step.copy_(src_step),
    }
    result = {"kernels_us": {"what": "microseconds per call, every window; device events around back-to-back calls on one stream "
                                     "(launch-to-launch time, not kernel time); prep calls include the output allocation",
                             "problem": dict(batch=b, frames=f, channels=c, latent=hw, c_pad=c_pad, cfg_copies=copies, noise_pred="fp16",
                                             calls_per_window=args.launches, windows=args.windows, step_bytes=step_bytes,
                                             prep_bytes=prep_bytes),
                             "rounds": []}}
    with torch.no_grad():
        for r in range(args.rounds):
            row = {}
            for name, fn in kernels.items():
                if name == "euler_cfg_step":
                    # the wrapper's table check reads the device outside capture: time the launches as the captured step issues them
                    graph = torch.cuda.CUDAGraph()
                    fn()
                    torch.cuda.synchronize()
                    with torch.cuda.graph(graph):
                        fn()
                    row[name + "_captured"] = summary([1e3 * v for v in windows_of(graph.replay, args.launches, lat.normal_)])
                row[name] = summary([1e3 * v for v in windows_of(fn, args.launches, lat.normal_)])
            result["kernels_us"]["rounds"].append(row)
            print(json.dumps(row), flush=True)

    # ---- (b) the replayed step
    if not args.skip_step:
        import bench
        unet = bench.build_hip_model(dev, seed=1234)
        pipe = pkg.I2VAdapterPipeline(unet=unet)
        d = bench.sample_inputs(0, args.frames, args.size // 8, ip=False)
        gens = lambda: dict(generator=torch.Generator().manual_seed(1), prior_mask_generator=torch.Generator().manual_seed(2),
                            prior_noise_generator=torch.Generator().manual_seed(3))
        call = dict(prompt_embeds=d["pe"].half(), negative_prompt_embeds=d["ne"].half(), condition_image_latents=d["cond"],
                    num_frames=args.frames, blur_sigma=0.8, output_type="latent")
        schedulers = {"ddim": pkg.DDIMScheduler, "euler": lambda: pkg.EulerDiscreteScheduler(**SD15),
                      "euler_ancestral": lambda: pkg.EulerAncestralDiscreteScheduler(**SD15)}

        def step_windows(kind):
            """capture the step of `kind` (a whole sample through the pipeline), then time windows of replays of that graph"""
            pipe.scheduler = schedulers[kind]()
            frames = pipe(**call, num_inference_steps=8, guidance_scale=7.5, **gens()).frames
            assert bool(torch.isfinite(frames).all())
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

        result["step_ms"] = {"what": "ms per replayed step, every window; the same graph as the pipeline replays; 8-step schedules, "
                                     "guidance 7.5",
                             "problem": dict(frames=args.frames, size=args.size, cfg_copies=2, replays_per_window=args.replays,
                                             windows=args.windows),
                             "rounds": []}
        for r in range(args.rounds):
            row = {kind: summary(step_windows(kind)) for kind in ("ddim", "euler", "euler_ancestral")}
            for kind in ("euler", "euler_ancestral"):
                row[kind + "_over_ddim_median"] = round(row[kind]["median"] / row["ddim"]["median"], 5)
            result["step_ms"]["rounds"].append(row)
            print(json.dumps(row), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
