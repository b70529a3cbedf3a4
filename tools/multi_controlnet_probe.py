"""Multi-ControlNet measurement ("Several ControlNets") at bench.py's flagship workload (16 frames x 512 x 512, CFG), on
one MI355X, in ONE process, alternating windows:

  (a) for N = 2, 3, 4: `i2v_add_multi_residuals_f16` on the 12 skip tensors in one launch (+ the mid tensor in a second, as the UNet
      issues them) against N times the pair of `i2v_add_residuals_f16` launches that N single nets would need, and against
      `i2v_copy3d_f16` moving the bytes of the fused launch ((N + 2) x 2 bytes per value);
  (b) the replayed step -- one captured graph each -- with 0, 1 and 2 ControlNets.

The byte model gives the fused launch (N + 2) / 3 N of the N launches' time; the measured ratio is written next to it.
The ControlNets are `ControlNetModel.from_unet` of the benchmark's UNet with random zero convolutions (the launches do not depend on
the values).  usage (GPU box, repository root):   python tools/multi_controlnet_probe.py --out profiles/multi_controlnet_probe.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/multi_controlnet_probe.json")
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
        shapes.append((n, h_lat >> 3, h_lat >> 3, ch[-1]))    # the mid tensor, added in a launch of its own
        g = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda s: torch.randn(s, generator=g, device=dev, dtype=torch.float32).to(f16)
        skips, outs = [rnd(s) for s in shapes], [torch.empty(s, dtype=f16, device=dev) for s in shapes]
        sets = [[rnd(s) for s in shapes] for _ in range(4)]
        idx = torch.ones(1, dtype=torch.int32, device=dev)
        elems = sum(t.numel() for t in skips)
        result["add"] = dict(tensors=len(shapes), values=elems)
        for nets in (2, 3, 4):
            table = torch.tensor([[0.0, 1.0 - 0.25 * k] for k in range(nets)], device=dev)
            rows = [table[k].contiguous() for k in range(nets)]
            rows_copy = (elems * (nets + 2) // 2) // 1280       # copy3d: 2 bytes in + 2 out per value
            src, dst = rnd((1, rows_copy, 1280)), torch.empty((1, rows_copy, 1280), dtype=f16, device=dev)

            def fused():
                K.add_multi_residuals(skips[:-1], [s[:-1] for s in sets[:nets]], scale=(table, idx), out=outs[:-1])
                K.add_multi_residuals(skips[-1:], [s[-1:] for s in sets[:nets]], scale=(table, idx), out=outs[-1:])

            def chained():                                    # what N single nets cost: the first out of place, the rest in place
                for k in range(nets):
                    src_k = skips if k == 0 else outs
                    K.add_residuals(src_k[:-1], sets[k][:-1], scale=(rows[k], idx), out=outs[:-1])
                    K.add_residuals(src_k[-1:], sets[k][-1:], scale=(rows[k], idx), out=outs[-1:])
            t = alternate({"fused": fused, "n_launches": chained, "copy3d_same_bytes": lambda: K.copy3d(src, dst)})
            fused_bytes, chained_bytes = elems * 2 * (nets + 2), elems * 6 * nets
            t["fused"]["tb_per_s"] = round(fused_bytes / t["fused"]["median_us"] / 1e6, 2)
            t["n_launches"]["tb_per_s"] = round(chained_bytes / t["n_launches"]["median_us"] / 1e6, 2)
            t["copy3d_same_bytes"]["tb_per_s"] = round(fused_bytes / t["copy3d_same_bytes"]["median_us"] / 1e6, 2)
            result["add"][f"nets_{nets}"] = dict(t, fused_bytes=fused_bytes, n_launches_bytes=chained_bytes,
                                                 byte_model_ratio=round((nets + 2) / (3 * nets), 4),
                                                 measured_ratio=round(t["fused"]["median_us"] / t["n_launches"]["median_us"], 4))
            del src, dst
        del skips, outs, sets

        # ---------------------------------------------------------------- (b) the step with 0, 1 and 2 nets
        unet = bench.build_hip_model(dev, seed=1234)

        def net(seed):
            cn = pkg.ControlNetModel.from_unet(unet)
            init_random_weights_(cn.controlnet_down_blocks, seed=seed)
            init_random_weights_(cn.controlnet_mid_block, seed=seed + 1)
            init_random_weights_(cn.controlnet_cond_embedding, seed=seed + 2)
            return cn
        nets = [net(5), net(15)]
        control = torch.rand((frames, 3, args.size, args.size), generator=g, device=dev).to(f16)
        sch = pkg.DDIMScheduler()
        sch.set_timesteps(25)
        ts = sch.timesteps
        s = bench.sample_inputs(0, frames, h_lat, False)

        def captured(pipe, n_nets):
            st = dict(latents=s["lat"].to(dev).float().contiguous(), cond=s["cond"].to(dev).float().contiguous(), copies=2, num_frames=frames,
                      guidance=7.5, t_table=ts.float().to(dev), coef=sch.step_coefficients(ts).to(dev),
                      step_idx=torch.zeros(1, dtype=torch.int32, device=dev), ctx_text=torch.cat([s["ne"], s["pe"]]).to(dev, f16), ctx_ip=None)
            if n_nets == 1:
                st["cn_cond"] = K.duplicate_batch(nets[0].embed_condition(control))
                st["cn_scale"] = torch.ones(len(ts), dtype=torch.float32, device=dev)
            elif n_nets > 1:
                st["cn_cond"] = tuple(K.duplicate_batch(cn.embed_condition(control)) for cn in nets[:n_nets])
                st["cn_scale"] = torch.ones(n_nets, len(ts), dtype=torch.float32, device=dev)
            pipe._project_once(st)
            pipe._step(st)                                    # warm-up outside capture
            st["step_idx"].zero_()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                pipe._step(st)
            return graph, st
        g0, _s0 = captured(pkg.I2VAdapterPipeline(unet=unet), 0)
        g1, _s1 = captured(pkg.I2VAdapterPipeline(unet=unet, controlnet=nets[0]), 1)
        g2, _s2 = captured(pkg.I2VAdapterPipeline(unet=unet, controlnet=pkg.MultiControlNetModel(nets)), 2)
        t = alternate({"step": g0.replay, "step_with_1_net": g1.replay, "step_with_2_nets": g2.replay})
        a, b, c = (t[k]["median_us"] for k in ("step", "step_with_1_net", "step_with_2_nets"))
        result["step"] = dict(t, first_net_adds_us=round(b - a, 1), second_net_adds_us=round(c - b, 1), ratio_2_nets=round(c / a, 4))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
