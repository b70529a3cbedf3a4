"""What FreeNoise costs on the GPU, in one process:

  (a) kernels: `kernels.freenoise_gather` / `kernels.freenoise_blend` at the three widths of the SD-1.5 motion modules (64 frames,
               L = 16, S = 4, CFG batch of a 512 x 512 clip) against a plain device copy (`Tensor.copy_`) of as many bytes as the
               kernel reads and writes; device events around `--reps` calls, median of `--windows` windows after a warm-up, the two
               forms alternating; effective GB/s = (bytes read + bytes written) / time;
  (b) step:    one replayed denoising step (the captured hipGraph) on bench.py's model at 512 x 512 with CFG: 32 frames without
               FreeNoise, 32 frames with FreeNoise (L = 16, S = 4), 64 frames with FreeNoise -- and the row expansion
               windows * L / F of the attention sub-blocks for each.

Run once on the GPU:  python tools/freenoise_probe.py --out profiles/freenoise_probe.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "freenoise_probe.json"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--no-step", action="store_true", help="only the kernels (a)")
    args = ap.parse_args()

    import torch

    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd import free_noise

    K = pkg.kernels
    dev = torch.device("cuda:0")
    L, S = args.length, args.stride
    st = free_noise.FreeNoiseSettings(L, S, "pyramid", "shuffle_context")

    def window(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / args.reps          # us per call

    def ab(fn, ref):
        for _ in range(2):
            window(fn), window(ref)
        a, b = [], []
        for _ in range(args.windows):
            a.append(window(fn))
            b.append(window(ref))
        return statistics.median(a), statistics.median(b)

    result = {"kernels": {"what": f"us per call, device events around {args.reps} calls, median of {args.windows} windows after warm-up; copy = "
                                  "Tensor.copy_ of (bytes read + bytes written) / 2 bytes; GB/s = (read + written) / time", "rows": []}}
    F = 64
    lat = args.size // 8
    for c, hw in ((320, lat * lat), (640, lat * lat // 4), (1280, lat * lat // 16)):
        n_pixels = 2 * hw
        starts, idx, coef = free_noise.tables(F, st, dev)
        W = starts.numel()
        t = torch.randn(n_pixels * F, c, device=dev, dtype=torch.float16)
        tw = K.freenoise_gather(t, starts, n_pixels=n_pixels, frames=F, length=L)
        out = K.freenoise_blend(tw, idx, coef, n_pixels=n_pixels, windows=W, length=L)
        live = int((coef != 0).sum().item())                 # source rows read per pixel by the blend
        for name, fn, rd, wr in (
                ("gather", lambda: K.freenoise_gather(t, starts, n_pixels=n_pixels, frames=F, length=L), tw.numel() * 2, tw.numel() * 2),
                ("blend", lambda: K.freenoise_blend(tw, idx, coef, n_pixels=n_pixels, windows=W, length=L), n_pixels * live * c * 2,
                 out.numel() * 2)):
            half = (rd + wr) // 2
            a, b = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
            t_k, t_c = ab(fn, lambda: b.copy_(a))
            row = dict(kernel=name, c=c, n_pixels=n_pixels, frames=F, windows=W, length=L, read_mb=round(rd / 2 ** 20, 1),
                       written_mb=round(wr / 2 ** 20, 1), us=round(t_k, 1), gbps=round((rd + wr) / t_k / 1e3, 1), copy_us=round(t_c, 1),
                       copy_gbps=round((rd + wr) / t_c / 1e3, 1), over_copy=round(t_k / t_c, 3))
            result["kernels"]["rows"].append(row)
            print(json.dumps(row), flush=True)
        del t, tw, out

    if not args.no_step:
        import bench
        unet = bench.build_hip_model(dev, seed=1234)
        pipe = pkg.I2VAdapterPipeline(unet=unet)
        gens = lambda: dict(generator=torch.Generator().manual_seed(1), prior_mask_generator=torch.Generator().manual_seed(2),
                            prior_noise_generator=torch.Generator().manual_seed(3))
        rows = []
        for frames, on in ((32, False), (32, True), (64, True)):
            if on:
                pipe.enable_free_noise(context_length=L, context_stride=S)
            else:
                pipe.disable_free_noise()
            d = bench.sample_inputs(0, frames, lat, ip=False)
            frames_out = pipe(prompt_embeds=d["pe"].half(), negative_prompt_embeds=d["ne"].half(), condition_image_latents=d["cond"],
                              num_frames=frames, blur_sigma=0.8, output_type="latent", num_inference_steps=2, guidance_scale=7.5,
                              **gens()).frames
            assert bool(torch.isfinite(frames_out).all())
            graph, gst = next(iter(pipe._graph_cache.values()))
            step = []
            for _ in range(5):
                gst["step_idx"].zero_()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(2):
                    graph.replay()
                e.record()
                torch.cuda.synchronize()
                step.append(s.elapsed_time(e) / 2)
            W = len(free_noise.windows(frames, L, S)) if on else 1
            row = dict(frames=frames, free_noise=on, windows=W, attention_row_expansion=round(W * L / frames, 3) if on else 1.0,
                       step_ms=[round(v, 2) for v in step], step_ms_median=round(statistics.median(step), 2),
                       step_ms_per_frame=round(statistics.median(step) / frames, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
        pipe.disable_free_noise()
        result["step"] = {"what": f"ms of one replayed denoising step (hipGraph), SD-1.5 width, {args.size} x {args.size}, CFG on; FreeNoise "
                                  f"L = {L}, S = {S}, pyramid", "rows": rows,
                          "free_noise_over_plain_at_32_frames": round(rows[1]["step_ms_median"] / rows[0]["step_ms_median"], 4)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
