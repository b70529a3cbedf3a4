"""Prompt travel measurement on one MI355X, in ONE process, SD-1.5 width with random weights (the launches do not depend
on the values):

  (a) `i2v_interp_rows_f16` making the per-frame contexts of a CFG batch (2 F rows of 77 x 768 from 4 keyframe rows, linspace weights)
      against `i2v_copy3d_f16` moving the same number of bytes, alternating windows, at 16 and 128 frames;
  (b) the once-per-sample cost for 2 and 4 keyframes at 16 and 64 frames: `encode_prompt_travel` (tokenise, the text encoder on the K
      keyframe texts + the negative prompt, one interpolation launch; host wall time around a device sync) and the pipeline's
      `_project_once` into the captured step's buffers (K / V^T of every context for the 16 cross-attention layers, the fused kernel's
      fragments, the time table), next to the same two numbers for one prompt;
  (c) the replayed step -- one captured graph each -- with per-frame contexts against the same pipeline with one prompt, alternating
      windows, at 16 f x 512^2 and at 64 f x 512^2 with FreeNoise (windows of 16, stride 4), and the peak device memory of a whole call of
      each kind, started from the same allocator state.

usage (GPU box, repository root):   timeout -k 10 900 python tools/prompt_travel_probe.py --out profiles/prompt_travel_probe.json"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/prompt_travel_probe.json")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="kernel launches per window")
    ap.add_argument("--step-reps", type=int, default=3, help="step replays per window")
    ap.add_argument("--long-frames", type=int, default=64, help="the FreeNoise clip of (b) and (c); 0 skips it")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd import prompt_travel as PT
    from i2v_adapter_unofficial_amd.clip_text import CLIPTextModel, init_clip_weights_
    from tests.clip_text_reference import StubTokenizer

    assert torch.cuda.is_available(), "the probe measures the GPU: there is nothing to time without one"
    dev, K, f16 = torch.device("cuda:0"), pkg.kernels, torch.float16
    lat = args.size // 8

    def window(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / reps                 # us per call

    def alternate(fns, reps):
        for fn in fns.values():
            window(fn, 2)
        t = {k: [] for k in fns}
        for _ in range(args.windows):
            for k, fn in fns.items():
                t[k].append(window(fn, reps))
        return {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1)) for k, v in t.items()}

    result = {"what": f"SD-1.5 width, {args.size}^2, CFG; device events around the calls of a window, {args.windows} alternating windows after "
                      "warm-up", "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        # ---------------------------------------------------------------- (a) the kernel
        rows_a = []
        g = torch.Generator(device=dev).manual_seed(1)
        for frames in (16, 128):
            src = torch.randn((8, 77, 768), generator=g, device=dev, dtype=torch.float32).to(f16)
            keys = [0, frames // 3, 2 * frames // 3, frames - 1]
            lo, hi, w, _ = PT.batch_tables([keys, keys], frames)                 # the two CFG halves: 2 F output rows
            lo_d, hi_d, w_d = (torch.as_tensor(t).to(dev) for t in (lo, hi, w))
            out = torch.empty((2 * frames, 77, 768), dtype=f16, device=dev)
            e = 77 * 768
            lib = pkg._lib.load()
            ptr = lambda t: pkg._lib.C.c_void_p(t.data_ptr())
            stream = lambda: pkg._lib.C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def launch():                                                        # the C entry alone: the tables are on the device already
                assert lib.i2v_interp_rows_f16(ptr(src), e, 8, ptr(lo_d), ptr(hi_d), ptr(w_d), ptr(out), e, 2 * frames, e, stream()) == 0
            interp = int((w != 0).sum())
            nbytes = (2 * interp + (2 * frames - interp) + 2 * frames) * e * 2   # rows read (two where 0 < w < 1, else one) + rows written
            half = nbytes // 4 // 768
            a, b = torch.empty((1, half, 768), dtype=f16, device=dev), torch.empty((1, half, 768), dtype=f16, device=dev)
            t = alternate({"interp_rows": launch, "interp_rows_wrapper": lambda: K.interp_rows(src, lo, hi, w, out=out),
                           "copy3d_same_bytes": lambda: K.copy3d(a, b)}, args.reps)
            row = dict(frames=frames, out_rows=2 * frames, interpolated_rows=interp, row_values=e, bytes_moved=nbytes,
                       **{k: dict(v, gb_per_s=round(nbytes / v["median_us"] / 1e3, 1)) for k, v in t.items()},
                       interp_over_copy=round(t["interp_rows"]["median_us"] / t["copy3d_same_bytes"]["median_us"], 3))
            rows_a.append(row)
            print(json.dumps(row), flush=True)
            del src, out, a, b
        result["interp_rows"] = {"what": "us per launch; interp_rows: the C entry with device tables; interp_rows_wrapper: kernels.interp_rows "
                                         "(host tables checked and uploaded per call)", "rows": rows_a}

        # ---------------------------------------------------------------- the models
        unet = bench.build_hip_model(dev, seed=1234)
        with torch.device("meta"):
            te = CLIPTextModel()
        te = init_clip_weights_(te.to_empty(device=dev).half(), seed=0, qk_gain=3.0).eval()
        pipe = pkg.I2VAdapterPipeline(unet=unet, text_encoder=te, tokenizer=StubTokenizer(77, dict(te.config)["vocab_size"]))
        texts = ["a red fox runs through a forest", "snow begins to fall on the trees", "night, the fox sleeps under the moon",
                 "dawn over a frozen lake"]

        def travel(n_keys, frames):
            keys = [round(i * (frames - 1) / (n_keys - 1)) for i in range(n_keys)]
            return {k: texts[i] for i, k in enumerate(keys)}

        def wall_ms(fn, n=5):
            fn()
            ts = []
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return round(statistics.median(ts), 3)
        gens = lambda: dict(generator=torch.Generator().manual_seed(1), prior_mask_generator=torch.Generator().manual_seed(2),
                            prior_noise_generator=torch.Generator().manual_seed(3))
        once, steps = [], []
        for frames in (16, args.long_frames):
            if not frames:
                continue
            free_noise = frames > 32
            if free_noise:
                pipe.enable_free_noise(context_length=16, context_stride=4)
            d = bench.sample_inputs(0, frames, lat, ip=False)
            kw = dict(condition_image_latents=d["cond"], num_frames=frames, blur_sigma=0.8, output_type="latent", num_inference_steps=2,
                      guidance_scale=7.5)
            graphs, peaks = {}, {}

            def sample(prompt):
                out = pipe(prompt=prompt, negative_prompt="blurry", **kw, **gens()).frames
                assert bool(torch.isfinite(out).all())
            for name, prompt in (("one_prompt", texts[0]), ("travel_2_keyframes", travel(2, frames)), ("travel_4_keyframes", travel(4, frames))):
                if isinstance(prompt, str):
                    enc = wall_ms(lambda: pipe.encode_prompt(prompt, dev, 1, True, negative_prompt="blurry"))
                else:
                    enc = wall_ms(lambda: pipe.encode_prompt_travel(prompt, frames, dev, 1, True, negative_prompt="blurry"))
                sample(prompt)
                graph, gst = next(iter(pipe._graph_cache.values()))
                proj = wall_ms(lambda: pipe._project_once(gst, into=True))
                kv_bytes = sum(t.numel() * 2 for kv in gst["ctx_proj"].kv.values() for t in kv if t is not None)
                row = dict(frames=frames, free_noise=free_noise, prompt=name, contexts=int(gst["ctx_text"].shape[0]), encode_ms=enc,
                           project_once_ms=proj, kv_bytes=kv_bytes, kv_gib=round(kv_bytes / 2 ** 30, 4))
                once.append(row)
                print(json.dumps(row), flush=True)
                if name != "travel_2_keyframes":
                    graphs[name] = (graph, gst)              # (kept alive: the next call's capture clears the cache, not this graph)

            def replay(name):
                graph, gst = graphs[name]

                def fn():
                    gst["step_idx"].zero_()
                    graph.replay()
                return fn
            t = alternate({k: replay(k) for k in graphs}, args.step_reps)
            a, b = t["one_prompt"]["median_us"], t["travel_4_keyframes"]["median_us"]
            # peak memory of a whole call, each from the same state: no captured step alive, the allocator's cache released, weights packed
            del graphs, graph, gst
            for name, prompt in (("one_prompt", texts[0]), ("travel_4_keyframes", travel(4, frames))):
                pipe._graph_cache.clear()
                pipe._graph = None
                gc.collect()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                sample(prompt)
                torch.cuda.synchronize()
                peaks[name] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)
                peaks[name + "_before"] = round(base / 2 ** 30, 3)
            row = dict(frames=frames, free_noise=free_noise, step_us=t, travel_added_us=round(b - a, 1), travel_ratio=round(b / a, 4),
                       peak_gib_one_prompt=peaks["one_prompt"], peak_gib_travel=peaks["travel_4_keyframes"],
                       allocated_gib_before_the_call=peaks["one_prompt_before"])
            steps.append(row)
            print(json.dumps(row), flush=True)
            pipe._graph_cache.clear()
            pipe._graph = None
            if free_noise:
                pipe.disable_free_noise()
        result["once_per_sample"] = {"what": "encode_ms: encode_prompt / encode_prompt_travel, host wall time around a device sync (median of 5); "
                                             "project_once_ms: _project_once into the captured step's buffers, the same way; kv_bytes: K / V^T of "
                                             "all contexts over the 16 cross-attention layers", "rows": once}
        result["step"] = {"what": "us of one replayed denoising step (hipGraph), one prompt against per-frame contexts, same process", "rows": steps}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
