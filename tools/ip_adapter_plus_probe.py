"""What IP-Adapter Plus costs on the GPU, in one process:

  (a) resampler:  blocks.Resampler at the SD-1.5 Plus geometry (1280 -> 768, 12 heads, depth 4, 16 queries) on B = 2 images of 257
                  tokens -- what one CFG sample projects -- against the same forward by torch's own fp16 ops on the same GPU (a
                  yardstick, not product code).  Device events around `--reps` forwards, median of `--windows` windows after a warm-up,
                  the two forms alternating; the host clock around the enqueue beside it.  Per-launch times: device events around each
                  single launch of one forward (they include the launch's own latency), median over the windows, summed per entry.
  (b) attention:  i2v_perceiver_attention_f16 alone at (B, n_q, len_a, len_b) = (2, 16, 257, 16), 12 heads, events around `--reps` launches.
  (c) step:       one replayed denoising step (the captured hipGraph) of bench.py's default configuration (16 frames, 512 x 512, CFG)
                  with the Plus adapter (16 image tokens), with the plain adapter (4) and without an adapter: three models in one
                  process, the three graphs replayed in turn, median of 7 rounds of 2 steps each.

Run once on the GPU:  python tools/ip_adapter_plus_probe.py --out profiles/ip_adapter_plus_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMETRY = dict(embed_dims=1280, hidden=768, heads=12, depth=4, num_queries=16)
NAMES = ("gemm", "layernorm", "perceiver_attention")


def torch_fp16_forward(m, x):
    """blocks.Resampler's forward by torch's fp16 ops on the module's own weights (tests/ip_adapter_plus_reference.py on the device)"""
    import torch
    import torch.nn.functional as F
    b, heads, d = x.shape[0], m.heads, m.dim_head
    ln = lambda t, n: F.layer_norm(t, n.weight.shape, n.weight, n.bias, n.eps)
    sp = lambda t: t.view(b, -1, heads, d).transpose(1, 2)
    lat = m.latents.repeat(b, 1, 1)
    x = m.proj_in(x)
    for ln0, ln1, attn, ff in m.layers:
        nl = ln(lat, ln1)
        kv_in = torch.cat([ln(x, ln0), nl], dim=-2)
        w = torch.softmax(sp(attn.to_q(nl)) @ sp(attn.to_k(kv_in)).transpose(-1, -2) * d ** -0.5, dim=-1)
        o = (w @ sp(attn.to_v(kv_in))).transpose(1, 2).reshape(b, -1, heads * d)
        lat = attn.to_out[0](o) + lat
        lat = ff[1].net[2](F.gelu(ff[1].net[0].proj(ln(lat, ff[0])))) + lat
    return ln(m.proj_out(lat), m.norm_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "ip_adapter_plus_probe.json"))
    ap.add_argument("--reps", type=int, default=20, help="forwards per timed window")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--no-step", action="store_true", help="only (a) and (b)")
    args = ap.parse_args()

    import torch

    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.unet_motion_cross_frame_attn import convert_ip_adapter_plus_image_proj
    from tests.ip_adapter_plus_reference import plus_state_dict

    assert torch.cuda.is_available(), "the probe measures the GPU: there is nothing to time without one"
    dev = torch.device("cuda:0")
    K = pkg.kernels

    def window(fn, reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        host = (time.perf_counter() - t0) * 1e6 / reps
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / reps, host            # us per call: device events, host enqueue

    class FakeUNet:
        config = {"cross_attention_dim": 768}
        attn_processor_names = staticmethod(lambda: [])
        named_modules = staticmethod(lambda: [])

    kwargs, conv = convert_ip_adapter_plus_image_proj(plus_state_dict(FakeUNet(), seed=3, qk_gain=1.5, **GEOMETRY)["image_proj"])
    m = pkg.blocks.Resampler(**kwargs)
    m.load_state_dict(conv)
    m = m.half().to(dev).eval()
    batch, tokens = 2, 257
    x = torch.randn(batch, tokens, GEOMETRY["embed_dims"], generator=torch.Generator().manual_seed(1)).to(dev, torch.float16)
    result = {"what": f"(a) us per Resampler forward at {GEOMETRY}, B = {batch} x {tokens} tokens: device events around {args.reps} forwards, "
                      f"median of {args.windows} windows after warm-up, forms alternating; (b) the attention launch alone; (c) one replayed step"}
    with torch.no_grad():
        hip, eager = (lambda: m(x)), (lambda: torch_fp16_forward(m, x))
        a, b = hip().float(), eager().float()
        agree = ((a - b).abs().max() / b.abs().max()).item()
        # launches of one forward, and device events around each of them
        saved = {n: getattr(K, n) for n in NAMES}
        marks = []

        def timing(name, fn):
            def w(*a, **kw):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                out = fn(*a, **kw)
                e.record()
                marks.append((name, s, e))
                return out
            return w
        per_launch = {}
        hip()
        for _ in range(args.windows):
            marks.clear()
            for n, fn in saved.items():
                setattr(K, n, timing(n, fn))
            try:
                hip()
            finally:
                for n, fn in saved.items():
                    setattr(K, n, fn)
            torch.cuda.synchronize()
            for i, (name, s, e) in enumerate(marks):
                per_launch.setdefault((i, name), []).append(s.elapsed_time(e) * 1e3)
        launches, by_entry = {}, {}
        for (i, name), v in sorted(per_launch.items()):
            launches[name] = launches.get(name, 0) + 1
            by_entry[name] = by_entry.get(name, 0.0) + statistics.median(v)
        for _ in range(2):
            window(hip, args.reps), window(eager, args.reps)
        th, te, hh, he = [], [], [], []
        for _ in range(args.windows):
            d, h = window(hip, args.reps)
            th.append(d), hh.append(h)
            d, h = window(eager, args.reps)
            te.append(d), he.append(h)
        result["resampler"] = {
            "hip_us": round(statistics.median(th), 1), "hip_us_min_max": [round(min(th), 1), round(max(th), 1)],
            "hip_host_enqueue_us": round(statistics.median(hh), 1),
            "torch_fp16_us": round(statistics.median(te), 1), "torch_fp16_us_min_max": [round(min(te), 1), round(max(te), 1)],
            "torch_fp16_host_enqueue_us": round(statistics.median(he), 1),
            "hip_over_torch": round(statistics.median(th) / statistics.median(te), 3),
            "hip_launches": launches, "hip_launches_total": sum(launches.values()),
            "single_launch_us_summed_per_entry": {k: round(v, 1) for k, v in by_entry.items()},
            "single_launch_us_each": [[name, round(statistics.median(v), 1)] for (i, name), v in sorted(per_launch.items())],
            "max_rel_difference_hip_vs_torch_fp16": agree}
        print(json.dumps(result["resampler"]), flush=True)

        # (b) the attention alone
        heads, nq, hid = GEOMETRY["heads"], GEOMETRY["num_queries"], GEOMETRY["heads"] * 64
        g = torch.Generator().manual_seed(2)
        qkv = torch.randn(batch * nq, 3 * hid, generator=g).to(dev, torch.float16)
        kv = torch.randn(batch * tokens, 2 * hid, generator=g).to(dev, torch.float16)
        out = torch.empty(batch * nq, hid, dtype=torch.float16, device=dev)
        att = lambda: K.perceiver_attention(qkv, kv, qkv, batch=batch, n_q=nq, len_a=tokens, len_b=nq, heads=heads, out=out)
        for _ in range(2):
            window(att, 5 * args.reps)
        ta = [window(att, 5 * args.reps)[0] for _ in range(args.windows)]
        kv_bytes = batch * (tokens + nq) * 2 * hid * 2
        result["perceiver_attention"] = {
            "shape": dict(batch=batch, n_q=nq, len_a=tokens, len_b=nq, heads=heads, head_dim=64), "workgroups": batch * heads,
            "us": round(statistics.median(ta), 2), "us_min_max": [round(min(ta), 2), round(max(ta), 2)],
            "what": f"events around {5 * args.reps} back-to-back launches: launch rate, not kernel time; k | v read once = {kv_bytes} bytes"}
        print(json.dumps(result["perceiver_attention"]), flush=True)

    if not args.no_step:
        import bench
        pipes = {}
        for name in ("plus_16_tokens", "plain_4_tokens", "no_adapter"):
            unet = bench.build_hip_model(dev, seed=1234)
            extra = {}
            gi = torch.Generator().manual_seed(9)
            if name == "plus_16_tokens":
                unet._load_ip_adapter_weights(plus_state_dict(unet, seed=3, **GEOMETRY), num_image_tokens=tokens)
                extra = dict(image_embeds=torch.randn(1, tokens, 1280, generator=gi).half(),
                             negative_image_embeds=torch.randn(1, tokens, 1280, generator=gi).half())
            elif name == "plain_4_tokens":
                unet._load_ip_adapter_weights(bench.synthetic_ip_state_dict(unet))
                extra = dict(image_embeds=torch.randn(1, 1024, generator=gi).half())
            pipe = pkg.I2VAdapterPipeline(unet=unet)
            d = bench.sample_inputs(0, 16, 64, ip=False)
            out = pipe(prompt_embeds=d["pe"].half(), negative_prompt_embeds=d["ne"].half(), condition_image_latents=d["cond"], num_frames=16,
                       blur_sigma=0.8, output_type="latent", num_inference_steps=2, guidance_scale=7.5,
                       generator=torch.Generator().manual_seed(1), prior_mask_generator=torch.Generator().manual_seed(2),
                       prior_noise_generator=torch.Generator().manual_seed(3), **extra).frames
            assert bool(torch.isfinite(out).all())
            pipes[name] = (pipe,) + next(iter(pipe._graph_cache.values()))
        times = {n: [] for n in pipes}
        for rnd in range(8):
            for name, (_, graph, gst) in pipes.items():
                gst["step_idx"].zero_()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(2):
                    graph.replay()
                e.record()
                torch.cuda.synchronize()
                if rnd:                                          # round 0 warms every graph up
                    times[name].append(s.elapsed_time(e) / 2)
        med = {n: statistics.median(v) for n, v in times.items()}
        res_ms = result["resampler"]["hip_us"] / 1e3
        result["step"] = {"what": "ms per replayed denoising step of bench.py's default configuration (16 frames, 512 x 512, CFG): three models in "
                                  "one process, graphs replayed in turn, 7 rounds of 2 steps",
                          "step_ms": {n: [round(x, 2) for x in v] for n, v in times.items()},
                          "step_ms_median": {n: round(v, 2) for n, v in med.items()},
                          "plus_over_plain": round(med["plus_16_tokens"] / med["plain_4_tokens"], 4),
                          "plus_over_no_adapter": round(med["plus_16_tokens"] / med["no_adapter"], 4),
                          "plain_over_no_adapter": round(med["plain_4_tokens"] / med["no_adapter"], 4),
                          "resampler_over_step": round(res_ms / med["plus_16_tokens"], 4),
                          "resampler_over_25_steps": round(res_ms / (25 * med["plus_16_tokens"]), 5)}
        print(json.dumps(result["step"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
