"""T2I-Adapter measurement at bench.py's flagship workload (16 frames x 512 x 512, CFG), on one MI355X, in ONE process:

  (a) the four `i2v_add_broadcast_residual_f16` launches of one step (the UNet's four down levels, full CFG batch, ONE copy of the
      features) against `i2v_copy3d_f16` moving the same number of bytes, against `i2v_add_residuals_f16` on a ControlNet's 12 + 1
      tensors and against that kernel on the same four tensors (four launches, the features repeated), alternating windows;
  (b) `T2IAdapter.embed` for the 16 control frames (once per sample);
  (c) the replayed step -- one captured graph each -- with an adapter, with a ControlNet and with neither, alternating windows.

The adapter has the default (SD-1.5) width with random weights and the ControlNet is `ControlNetModel.from_unet` of the benchmark's
UNet with random zero convolutions (the launches do not depend on the values).
usage (GPU box, repository root):   timeout -k 10 900 python tools/t2i_adapter_probe.py --out profiles/t2i_adapter_probe.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/t2i_adapter_probe.json")
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
        # ---------------------------------------------------------------- (a) the adds
        n, ch = 2 * frames, (320, 640, 1280, 1280)
        g = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda s: torch.randn(s, generator=g, device=dev, dtype=torch.float32).to(f16)
        levels = [(h_lat >> i, h_lat >> i, c) for i, c in enumerate(ch)]
        xs, feats = [rnd((n,) + lv) for lv in levels], [rnd((frames,) + lv) for lv in levels]
        outs = [torch.empty_like(t) for t in xs]
        table, idx = torch.tensor([0.0, 1.0], device=dev), torch.ones(1, dtype=torch.int32, device=dev)
        x_vals, f_vals = sum(t.numel() for t in xs), sum(t.numel() for t in feats)
        add_bytes = 4 * x_vals + 2 * f_vals                   # x in, out; one copy of the features in
        # the ControlNet's add on the same step: 12 skip tensors + the mid tensor, 2 values in + 1 out each
        cn_shapes = [(n, h_lat, h_lat, ch[0])]
        for i, c in enumerate(ch):
            hw = h_lat >> i
            cn_shapes += [(n, hw, hw, c)] * 2 + ([(n, hw // 2, hw // 2, c)] if i < 3 else [])
        cn_shapes.append((n, h_lat >> 3, h_lat >> 3, ch[-1]))
        skips, ress = [rnd(s) for s in cn_shapes], [rnd(s) for s in cn_shapes]
        cn_outs = [torch.empty_like(t) for t in skips]
        cn_bytes = 6 * sum(t.numel() for t in skips)
        rows = (add_bytes // 4) // 1280                       # copy3d moves 2 bytes in + 2 bytes out per value
        src, dst = rnd((1, rows, 1280)), torch.empty((1, rows, 1280), dtype=f16, device=dev)

        def adds():
            for x, ft, o in zip(xs, feats, outs):
                K.add_broadcast_residual(x, ft, scale=(table, idx), out=o)

        def cn_add():
            K.add_residuals(skips[:-1], ress[:-1], scale=(table, idx), out=cn_outs[:-1])
            K.add_residuals(skips[-1:], ress[-1:], scale=(table, idx), out=cn_outs[-1:])
        # like for like: the existing kernel on the same four tensors as four launches, the features repeated for the second CFG half
        reps2 = [torch.cat([ft, ft]) for ft in feats]

        def same_four():
            for x, ft, o in zip(xs, reps2, outs):
                K.add_residuals([x], [ft], scale=(table, idx), out=[o])
        t = alternate({"add_broadcast_residual_x4": adds, "copy3d_same_bytes": lambda: K.copy3d(src, dst), "add_residuals_controlnet": cn_add,
                       "add_residuals_same_four_x4": same_four})
        nbytes = {"add_broadcast_residual_x4": add_bytes, "copy3d_same_bytes": rows * 1280 * 4, "add_residuals_controlnet": cn_bytes,
                  "add_residuals_same_four_x4": 6 * x_vals}
        result["adds"] = dict(levels=[list(lv) for lv in levels], x_values=x_vals, feature_values=f_vals, launches=4, **{
            k: dict(v, bytes_moved=nbytes[k], tb_per_s=round(nbytes[k] / 1e9 / v["median_us"] * 1e3, 2)) for k, v in t.items()})
        del xs, outs, skips, ress, cn_outs, src, dst, reps2

        # ---------------------------------------------------------------- the models
        unet = bench.build_hip_model(dev, seed=1234)
        cn = pkg.ControlNetModel.from_unet(unet)
        init_random_weights_(cn.controlnet_down_blocks, seed=5)
        init_random_weights_(cn.controlnet_mid_block, seed=6)
        init_random_weights_(cn.controlnet_cond_embedding, seed=7)
        with torch.device("meta"):
            ad = pkg.T2IAdapter()
        ad = init_random_weights_(ad.to_empty(device=dev).half(), seed=8).eval()

        # ---------------------------------------------------------------- (b) the once-per-sample network
        control = torch.rand((frames, 3, args.size, args.size), generator=g, device=dev).to(f16)
        result["embed"] = dict(frames=frames, parameters=sum(q.numel() for q in ad.parameters()),
                               **alternate({"embed": lambda: ad.embed(control)})["embed"])

        # ---------------------------------------------------------------- (c) the step
        sch = pkg.DDIMScheduler()
        sch.set_timesteps(25)
        ts = sch.timesteps
        s = bench.sample_inputs(0, frames, h_lat, False)

        def captured(pipe, with_cn=False, with_adapter=False):
            st = dict(latents=s["lat"].to(dev).float().contiguous(), cond=s["cond"].to(dev).float().contiguous(), copies=2, num_frames=frames,
                      guidance=7.5, t_table=ts.float().to(dev), coef=sch.step_coefficients(ts).to(dev),
                      step_idx=torch.zeros(1, dtype=torch.int32, device=dev), ctx_text=torch.cat([s["ne"], s["pe"]]).to(dev, f16), ctx_ip=None)
            if with_cn:
                st["cn_cond"] = K.duplicate_batch(cn.embed_condition(control))
                st["cn_scale"] = torch.ones(len(ts), dtype=torch.float32, device=dev)
            if with_adapter:
                st["t2i_feats"] = ad.embed(control)
                st["t2i_scale"] = torch.ones(len(ts), dtype=torch.float32, device=dev)
            pipe._project_once(st)
            pipe._step(st)                                    # warm-up outside capture
            st["step_idx"].zero_()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                pipe._step(st)
            return graph, st
        plain, _st0 = captured(pkg.I2VAdapterPipeline(unet=unet))
        adapt, _st1 = captured(pkg.I2VAdapterPipeline(unet=unet, t2i_adapter=ad), with_adapter=True)
        ctrl, _st2 = captured(pkg.I2VAdapterPipeline(unet=unet, controlnet=cn), with_cn=True)
        t = alternate({"step": plain.replay, "step_with_adapter": adapt.replay, "step_with_controlnet": ctrl.replay})
        a, b, c = (t[k]["median_us"] for k in ("step", "step_with_adapter", "step_with_controlnet"))
        result["step"] = dict(t, adapter_added_us=round(b - a, 1), adapter_ratio=round(b / a, 4), controlnet_added_us=round(c - a, 1),
                              controlnet_ratio=round(c / a, 4))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
