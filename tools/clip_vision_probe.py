"""What an image prompt costs on the GPU, in one process:

  (a) encode:  one and two 224-px images through the 32-layer ViT-H/14 tower (IP-Adapter's image encoder) on the HIP kernels
               (`CLIPVisionModelWithProjection.forward`, seeded weights), against the same tower evaluated by torch's own fp16 ops on
               the same GPU (tests/clip_vision_reference.py moved to the device -- a yardstick, not product code).  Device events on
               the stream around `--reps` forwards, median of `--windows` windows after a warm-up, the two forms alternating.  The HIP
               forward's launches are counted from the kernel wrappers, and its host time per forward (a host clock around the enqueue,
               no synchronise inside) is reported beside the device time: where the two agree the forward is launch-latency bound.
  (b) step:    one replayed denoising step (the captured hipGraph) of bench.py's default configuration (16 frames, 512 x 512, CFG) in
               the same process, and the image prompt's share of a 25-step sample.

Run once on the GPU:  python tools/clip_vision_probe.py --out profiles/clip_vision_probe.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "clip_vision_probe.json"))
    ap.add_argument("--reps", type=int, default=10, help="forwards per timed window")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--no-step", action="store_true", help="only the encode (a)")
    args = ap.parse_args()

    import torch

    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.clip_vision import CLIPVisionModelWithProjection, init_clip_vision_weights_
    from tests.clip_vision_reference import ClipVisionReference, pixel_like

    assert torch.cuda.is_available(), "the probe measures the GPU: there is nothing to time without one"
    dev = torch.device("cuda:0")
    with torch.device("meta"):
        model = CLIPVisionModelWithProjection()
    model = init_clip_vision_weights_(model.to_empty(device=dev).half(), seed=0, qk_gain=3.0).eval()
    cfg = dict(model.config)
    ref = ClipVisionReference({k: v.detach() for k, v in model.state_dict().items()}, cfg)
    K = pkg.kernels
    names = ("gemm", "layernorm", "clip_patchify", "clip_vision_embed", "clip_vision_attention", "quick_gelu")

    def window(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        for _ in range(args.reps):
            fn()
        e.record()
        host = (time.perf_counter() - t0) * 1e6 / args.reps
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / args.reps, host      # us per forward: device events, host enqueue

    result = {"what": f"us per forward of B x 257 tokens through 32 layers of width 1280; device events around {args.reps} forwards, median "
                      f"of {args.windows} windows after warm-up, forms alternating; host_enqueue_us = host clock around the same loop "
                      "before the synchronise"}
    for batch in (1, 2):
        px = pixel_like(batch, 224, seed=batch).to(dev, torch.float16)
        hip = lambda: model(px)
        eager = lambda: ref(px)
        a, b = hip().image_embeds.float(), eager()[0].float()
        agree = ((a - b).abs().max() / b.abs().max()).item()
        launches = {}
        saved = {n: getattr(K, n) for n in names}

        def counting(name, fn):
            def w(*a, **kw):
                if not kw.get("query_ln_support"):
                    launches[name] = launches.get(name, 0) + 1
                return fn(*a, **kw)
            return w
        for n, fn in saved.items():
            setattr(K, n, counting(n, fn))
        hip()
        for n, fn in saved.items():
            setattr(K, n, fn)
        for _ in range(2):
            window(hip), window(eager)
        th, te, hh, he = [], [], [], []
        for _ in range(args.windows):
            d, h = window(hip)
            th.append(d), hh.append(h)
            d, h = window(eager)
            te.append(d), he.append(h)
        result[f"encode_{batch}"] = {
            "images": batch, "hip_us": round(statistics.median(th), 1), "hip_us_min_max": [round(min(th), 1), round(max(th), 1)],
            "hip_host_enqueue_us": round(statistics.median(hh), 1),
            "torch_fp16_us": round(statistics.median(te), 1), "torch_fp16_us_min_max": [round(min(te), 1), round(max(te), 1)],
            "torch_fp16_host_enqueue_us": round(statistics.median(he), 1),
            "hip_over_torch": round(statistics.median(th) / statistics.median(te), 3),
            "hip_launches": launches, "hip_launches_total": sum(launches.values()),
            "hip_us_per_launch": round(statistics.median(th) / max(1, sum(launches.values())), 2),
            "max_rel_difference_hip_vs_torch_fp16": agree}
        print(json.dumps(result[f"encode_{batch}"]), flush=True)

    if not args.no_step:
        import bench
        unet = bench.build_hip_model(dev, seed=1234)
        pipe = pkg.I2VAdapterPipeline(unet=unet)
        d = bench.sample_inputs(0, 16, 64, ip=False)
        out = pipe(prompt_embeds=d["pe"].half(), negative_prompt_embeds=d["ne"].half(), condition_image_latents=d["cond"], num_frames=16,
                   blur_sigma=0.8, output_type="latent", num_inference_steps=2, guidance_scale=7.5,
                   generator=torch.Generator().manual_seed(1), prior_mask_generator=torch.Generator().manual_seed(2),
                   prior_noise_generator=torch.Generator().manual_seed(3)).frames
        assert bool(torch.isfinite(out).all())
        graph, gst = next(iter(pipe._graph_cache.values()))
        step = []
        for _ in range(7):
            gst["step_idx"].zero_()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(2):
                graph.replay()
            e.record()
            torch.cuda.synchronize()
            step.append(s.elapsed_time(e) / 2)
        step_ms = statistics.median(step)
        enc_ms = result["encode_1"]["hip_us"] / 1e3
        result["step"] = {"what": "one replayed denoising step of bench.py's default configuration (16 frames, 512 x 512, CFG), same process",
                          "step_ms": [round(v, 2) for v in step], "step_ms_median": round(step_ms, 2),
                          "image_over_step": round(enc_ms / step_ms, 4), "image_over_25_steps": round(enc_ms / (25 * step_ms), 5)}
        print(json.dumps(result["step"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
