"""Weighted and long prompts, measured on one MI355X, in ONE process, SD-1.5 width with random weights (the launches do not
depend on the values):

  (a) `i2v_weight_embeds_f16` at P = 2 and P = 32 prompts of 77, 154 and 231 tokens x 768 against `i2v_copy3d_f16` moving the same
      bytes (one read and one write of every value; the kernel's second read of the source comes from L2), alternating windows;
  (b) the once-per-sample cost of `encode_weighted_prompt` against `encode_prompt` (tokenise, the text encoder, the weighting launch,
      the read of the ratios; host wall time around a device sync) for a short prompt and for prompts of two and three chunks;
  (c) the replayed step -- one captured graph each -- at 16 f x 512^2 with CFG for contexts of 77, 154 and 231 rows, alternating
      windows: the price of a long prompt, whose contexts leave the fused text cross-attention for i2v_attention_f16.

usage (GPU box, repository root):   timeout -k 10 900 python tools/prompt_weighting_probe.py --out profiles/prompt_weighting_probe.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/prompt_weighting_probe.json")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="kernel launches per window")
    ap.add_argument("--step-reps", type=int, default=3, help="step replays per window")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench
    import i2v_adapter_unofficial_amd as pkg
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

    result = {"what": f"SD-1.5 width, {args.size}^2, {args.frames} frames, CFG; device events around the calls of a window, {args.windows} "
                      "alternating windows after warm-up", "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        # ---------------------------------------------------------------- (a) the kernel
        rows_a = []
        g = torch.Generator(device=dev).manual_seed(1)
        lib = pkg._lib.load()
        ptr = lambda t: pkg._lib.C.c_void_p(t.data_ptr())
        stream = lambda: pkg._lib.C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for p in (2, 32):
            for tokens in (77, 154, 231):
                src = (torch.randn((p, tokens, 768), generator=g, device=dev, dtype=torch.float32) + 0.5).to(f16)
                w = (1.0 + 0.3 * torch.randn((p, tokens), generator=g, device=dev, dtype=torch.float32)).clamp(0.2, 2.0)
                out, ratio = torch.empty_like(src), torch.empty(p, dtype=torch.float32, device=dev)

                def launch(restore=1):                              # the C entry alone
                    assert lib.i2v_weight_embeds_f16(ptr(src), ptr(w), ptr(out), ptr(ratio), p, tokens, 768, 768, 768, restore, stream()) == 0
                a, b = torch.empty((1, p * tokens, 768), dtype=f16, device=dev), torch.empty((1, p * tokens, 768), dtype=f16, device=dev)
                t = alternate({"weight_embeds": launch, "weight_embeds_no_restore": lambda: launch(0),
                               "copy3d_same_bytes": lambda: K.copy3d(a, b)}, args.reps)
                nbytes = 2 * p * tokens * 768 * 2
                row = dict(prompts=p, tokens=tokens, bytes_moved=nbytes,
                           **{k: dict(v, gb_per_s=round(nbytes / v["median_us"] / 1e3, 1)) for k, v in t.items()},
                           weight_over_copy=round(t["weight_embeds"]["median_us"] / t["copy3d_same_bytes"]["median_us"], 3))
                rows_a.append(row)
                print(json.dumps(row), flush=True)
                del src, out, a, b
        result["weight_embeds"] = {"what": "us per launch of the C entry (one workgroup of 1024 lanes per prompt, both passes) against "
                                           "i2v_copy3d_f16 of the same rows", "rows": rows_a}

        # ---------------------------------------------------------------- the models
        unet = bench.build_hip_model(dev, seed=1234)
        with torch.device("meta"):
            te = CLIPTextModel()
        te = init_clip_weights_(te.to_empty(device=dev).half(), seed=0, qk_gain=3.0).eval()
        # the character tokenizer of the tests: a prompt of n characters is n tokens
        pipe = pkg.I2VAdapterPipeline(unet=unet, text_encoder=te, tokenizer=StubTokenizer(77, dict(te.config)["vocab_size"]))
        base = "a red fox runs through a forest while snow begins to fall on the trees and the night comes, "
        prompts = {77: "a (red:1.3) fox runs through a [forest]", 154: "(" + (base * 2)[:120] + ":1.2)", 231: "(" + (base * 3)[:200] + ":1.2)"}

        def wall_ms(fn, n=7):
            fn()
            ts = []
            for _ in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return round(statistics.median(ts), 3)
        # ---------------------------------------------------------------- (b) once per sample
        once = []
        plain = wall_ms(lambda: pipe.encode_prompt("a red fox runs through a forest", dev, 1, True, negative_prompt="blurry"))
        once.append(dict(path="encode_prompt", context_rows=77, encode_ms=plain))
        pipe.enable_prompt_weighting(3)
        for rows, text in prompts.items():
            ms = wall_ms(lambda: pipe.encode_weighted_prompt(text, dev, 1, True, negative_prompt="(blurry:1.2)"))
            shape = tuple(pipe.encode_weighted_prompt(text, dev, 1, True, negative_prompt="(blurry:1.2)")[0].shape)
            assert shape[1] == rows, (shape, rows)
            once.append(dict(path="encode_weighted_prompt", context_rows=rows, encode_ms=ms, over_encode_prompt=round(ms / plain, 3)))
        for row in once:
            print(json.dumps(row), flush=True)
        result["once_per_sample"] = {"what": "host wall time around a device sync, median of 7: prompt + negative prompt -> embeddings "
                                             "(12-layer text encoder at SD-1.5's size, random weights)", "rows": once}

        # ---------------------------------------------------------------- (c) the replayed step
        gens = lambda: dict(generator=torch.Generator().manual_seed(1), prior_mask_generator=torch.Generator().manual_seed(2),
                            prior_noise_generator=torch.Generator().manual_seed(3))
        d = bench.sample_inputs(0, args.frames, lat, ip=False)
        kw = dict(condition_image_latents=d["cond"], num_frames=args.frames, blur_sigma=0.8, output_type="latent", num_inference_steps=2,
                  guidance_scale=7.5)
        graphs = {}
        for rows, text in prompts.items():
            out = pipe(prompt=text, negative_prompt="(blurry:1.2)", **kw, **gens()).frames
            assert bool(torch.isfinite(out).all())
            graph, gst = next(iter(pipe._graph_cache.values()))
            assert int(gst["ctx_text"].shape[1]) == rows, (tuple(gst["ctx_text"].shape), rows)
            graphs[f"context_{rows}"] = (graph, gst)          # (kept alive: the next call's capture clears the cache, not this graph)

        def replay(name):
            graph, gst = graphs[name]

            def fn():
                gst["step_idx"].zero_()
                graph.replay()
            return fn
        t = alternate({k: replay(k) for k in graphs}, args.step_reps)
        a = t["context_77"]["median_us"]
        result["step"] = {"what": "us of one replayed denoising step (hipGraph) per context length, same process; 77 rows take the fused "
                                  "text cross-attention at the top level, longer contexts i2v_attention_f16",
                          "step_us": t, "ratio_154_over_77": round(t["context_154"]["median_us"] / a, 4),
                          "ratio_231_over_77": round(t["context_231"]["median_us"] / a, 4)}
        print(json.dumps(result["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
