"""Video-to-video measurement at bench.py's flagship workload (16 frames x 512 x 512, CFG), on one MI355X, in ONE process:

  (a) the `i2v_masked_renoise_f32` launch of one step (the fp32 latents of the 16 frames, one mask plane per frame) against
      `i2v_copy3d_f16` moving the same number of bytes, alternating windows.  The launch moves 4.5 MB (1 MiB per fp32 tensor): the times
      are launch latency, not bandwidth;
  (b) `pipe.encode_video` of the 16 source frames (once per sample), with an SD-width AutoencoderKL of random weights, in one batch
      and frame by frame (`enable_vae_slicing`);
  (c) the replayed step -- one captured graph each -- with a mask and without, and a second capture of the step without as a control
      (what two captures of one step differ by), alternating windows, repeated `--repeats` times to show the spread.

usage (GPU box, repository root):   timeout -k 10 900 python tools/video2video_probe.py --out profiles/video2video_probe.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/video2video_probe.json")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="launches / replays per window")
    ap.add_argument("--repeats", type=int, default=3, help="repetitions of the step comparison")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_

    assert torch.cuda.is_available(), "the probe measures the GPU: there is nothing to time without one"
    dev, K, f16 = torch.device("cuda:0"), pkg.kernels, torch.float16
    frames, h_lat = args.frames, args.size // 8

    def window(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / reps                 # us per call

    def alternate(fns, reps=None):
        for fn in fns.values():
            window(fn, 3)
        t = {k: [] for k in fns}
        for _ in range(args.windows):
            for k, fn in fns.items():
                t[k].append(window(fn, reps or args.reps))
        return {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1)) for k, v in t.items()}

    result = {"what": f"{frames} frames x {args.size}^2, CFG; device events around {args.reps} calls, {args.windows} alternating windows "
                      "after warm-up; us per call",
              "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        # ---------------------------------------------------------------- (a) the blend
        g = torch.Generator(device=dev).manual_seed(1)
        shape = (1, frames, 4, h_lat, h_lat)
        lat, src, noise = (torch.randn(shape, generator=g, device=dev) for _ in range(3))
        mask = (torch.rand((1, frames, 1, h_lat, h_lat), generator=g, device=dev) < 0.5).float()
        table = torch.tensor([[1.0, 0.0], [0.8, 0.6]], device=dev)
        idx = torch.ones(1, dtype=torch.int32, device=dev)
        blend_bytes = 4 * (4 * lat.numel() + mask.numel())    # three reads and one write over the latents, the mask once per pixel
        rows = (blend_bytes // 4) // 1280                     # copy3d moves 2 bytes in + 2 bytes out per value
        a, b = torch.randn((1, rows, 1280), generator=g, device=dev).to(f16), torch.empty((1, rows, 1280), dtype=f16, device=dev)
        t = alternate({"masked_renoise": lambda: K.masked_renoise(lat, src, noise, mask, table, idx), "copy3d_same_bytes": lambda: K.copy3d(a, b)})
        result["blend"] = dict(latents=list(shape), bytes_moved=blend_bytes, copy_bytes_moved=rows * 1280 * 4, **t)
        del a, b

        # ---------------------------------------------------------------- (b) the once-per-sample encode
        vae = pkg.AutoencoderKL()
        init_random_weights_(vae, seed=3)
        vae = vae.to(device=dev, dtype=f16).eval()
        unet = bench.build_hip_model(dev, seed=1234)
        pipe = pkg.I2VAdapterPipeline(vae=vae, unet=unet)
        video = torch.rand((frames, 3, args.size, args.size), generator=torch.Generator().manual_seed(2))
        gen = torch.Generator().manual_seed(3)
        enc = {"encode_video": lambda: pipe.encode_video(video, args.size, args.size, gen)}
        result["encode_video"] = dict(frames=frames, **alternate(enc, reps=2)["encode_video"])
        pipe.enable_vae_slicing()
        result["encode_video_sliced"] = dict(frames=frames, **alternate(enc, reps=2)["encode_video"])
        del vae, pipe

        # ---------------------------------------------------------------- (c) the step
        sch = pkg.DDIMScheduler()
        sch.set_timesteps(25)
        ts = sch.timesteps
        s = bench.sample_inputs(0, frames, h_lat, False)
        pipe = pkg.I2VAdapterPipeline(unet=unet, scheduler=sch)

        def captured(with_mask):
            st = dict(latents=s["lat"].to(dev).float().contiguous(), cond=s["cond"].to(dev).float().contiguous(), copies=2, num_frames=frames,
                      guidance=7.5, t_table=ts.float().to(dev), coef=sch.step_coefficients(ts).to(dev),
                      step_idx=torch.zeros(1, dtype=torch.int32, device=dev), ctx_text=torch.cat([s["ne"], s["pe"]]).to(dev, f16), ctx_ip=None)
            if with_mask:
                st.update(v2v_mask=mask, v2v_source=src, v2v_noise=noise, v2v_coef=pipe.renoise_table(ts).to(dev))
            pipe._project_once(st)
            pipe._step(st)                                    # warm-up outside capture
            st["step_idx"].zero_()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                pipe._step(st)
            return graph, st
        plain, _st0 = captured(False)
        masked, _st1 = captured(True)
        control, _st2 = captured(False)                       # a second capture of the SAME step: what two graphs differ by on their own
        runs = []
        for _ in range(args.repeats):
            t = alternate({"step": plain.replay, "step_with_mask": masked.replay, "step_control": control.replay})
            p, m, c = (t[k]["median_us"] for k in ("step", "step_with_mask", "step_control"))
            runs.append(dict(t, mask_added_us=round(m - p, 1), mask_ratio=round(m / p, 4), control_added_us=round(c - p, 1)))
        added, ctl = [r["mask_added_us"] for r in runs], [r["control_added_us"] for r in runs]
        result["step"] = dict(runs=runs, mask_added_us_min=min(added), mask_added_us_max=max(added), control_added_us_min=min(ctl),
                              control_added_us_max=max(ctl))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
