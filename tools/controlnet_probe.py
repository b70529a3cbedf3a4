"""ControlNet measurement at bench.py's flagship workload (16 frames x 512 x 512, CFG), on one MI355X, in ONE process:

  (a) `i2v_add_residuals_f16` on the 12 skip tensors of that step in one launch (+ the mid tensor in a second, as the UNet issues
      them) against `i2v_copy3d_f16` moving the same number of bytes, alternating windows;
  (b) `ControlNetModel.embed_condition` for the 16 control frames (once per sample);
  (c) the replayed step -- one captured graph each -- with and without a ControlNet, alternating windows of replays.

The ControlNet is `ControlNetModel.from_unet` of the benchmark's UNet with random zero convolutions (the launches do not depend on
the values).  usage (GPU box, repository root):   python tools/controlnet_probe.py --out profiles/controlnet_probe.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/controlnet_probe.json")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="launches / replays per window")
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

    def alternate(fns):
        for fn in fns.values():
            window(fn, 3)
        t = {k: [] for k in fns}
        for _ in range(args.windows):
            for k, fn in fns.items():
                t[k].append(window(fn, args.reps))
        return {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1)) for k, v in t.items()}

    result = {"what": f"{frames} frames x {args.size}^2, CFG (batch of {2 * frames} images); device events around {args.reps} calls, "
                      f"{args.windows} alternating windows after warm-up; us per call",
              "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        # ---------------------------------------------------------------- (a) the add
        n, ch = 2 * frames, (320, 640, 1280, 1280)
        shapes = [(n, h_lat, h_lat, ch[0])]
        for i, c in enumerate(ch):
            hw = h_lat >> i
            shapes += [(n, hw, hw, c)] * 2
            if i < 3:
                shapes.append((n, hw // 2, hw // 2, c))
        mid_shape = (n, h_lat >> 3, h_lat >> 3, ch[-1])
        g = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda s: torch.randn(s, generator=g, device=dev, dtype=torch.float32).to(f16)
        skips, ress, mid, mid_res = [rnd(s) for s in shapes], [rnd(s) for s in shapes], rnd(mid_shape), rnd(mid_shape)
        outs, mid_out = [torch.empty_like(t) for t in skips], torch.empty_like(mid)
        table, idx = torch.tensor([0.0, 1.0], device=dev), torch.ones(1, dtype=torch.int32, device=dev)
        elems = sum(t.numel() for t in skips) + mid.numel()
        # copy3d moves 2 bytes in + 2 bytes out per value, the add 4 in + 2 out: 1.5 x the values for the same bytes
        rows = (elems * 3 // 2) // 1280
        src, dst = rnd((1, rows, 1280)), torch.empty((1, rows, 1280), dtype=f16, device=dev)

        def add():
            K.add_residuals(skips, ress, scale=(table, idx), out=outs)
            K.add_residuals([mid], [mid_res], scale=(table, idx), out=[mid_out])
        t = alternate({"add_residuals": add, "copy3d": lambda: K.copy3d(src, dst)})
        gbytes = elems * 6 / 1e9
        result["add_residuals"] = dict(tensors=len(shapes) + 1, values=elems, bytes_moved=elems * 6, launches=2, **{
            k: dict(v, tb_per_s=round(gbytes / v["median_us"] * 1e3, 2)) for k, v in t.items()})
        del skips, ress, outs, src, dst

        # ---------------------------------------------------------------- the models
        unet = bench.build_hip_model(dev, seed=1234)
        cn = pkg.ControlNetModel.from_unet(unet)
        init_random_weights_(cn.controlnet_down_blocks, seed=5)
        init_random_weights_(cn.controlnet_mid_block, seed=6)
        init_random_weights_(cn.controlnet_cond_embedding, seed=7)

        # ---------------------------------------------------------------- (b) the embedding
        control = torch.rand((frames, 3, args.size, args.size), generator=g, device=dev).to(f16)
        result["embed_condition"] = dict(frames=frames, **alternate({"embed": lambda: cn.embed_condition(control)})["embed"])

        # ---------------------------------------------------------------- (c) the step
        sch = pkg.DDIMScheduler()
        sch.set_timesteps(25)
        ts = sch.timesteps
        s = bench.sample_inputs(0, frames, h_lat, False)

        def captured(pipe, with_cn):
            st = dict(latents=s["lat"].to(dev).float().contiguous(), cond=s["cond"].to(dev).float().contiguous(), copies=2, num_frames=frames,
                      guidance=7.5, t_table=ts.float().to(dev), coef=sch.step_coefficients(ts).to(dev),
                      step_idx=torch.zeros(1, dtype=torch.int32, device=dev), ctx_text=torch.cat([s["ne"], s["pe"]]).to(dev, f16), ctx_ip=None)
            if with_cn:
                st["cn_cond"] = K.duplicate_batch(cn.embed_condition(control))
                st["cn_scale"] = torch.ones(len(ts), dtype=torch.float32, device=dev)
            pipe._project_once(st)
            pipe._step(st)                                    # warm-up outside capture
            st["step_idx"].zero_()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                pipe._step(st)
            return graph, st
        plain, _st0 = captured(pkg.I2VAdapterPipeline(unet=unet), False)
        ctrl, _st1 = captured(pkg.I2VAdapterPipeline(unet=unet, controlnet=cn), True)
        t = alternate({"step": plain.replay, "step_with_controlnet": ctrl.replay})
        a, b = t["step"]["median_us"], t["step_with_controlnet"]["median_us"]
        result["step"] = dict(t, added_us=round(b - a, 1), ratio=round(b / a, 4))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
