"""AutoencoderTiny measurement, on one MI355X, everything inside ONE call of this script:

  (a) layer:  i2v_conv3x3_c64_f16 (convolution + bias + ReLU in one launch) against the existing route -- `kernels.conv3x3` with the
              same weights and bias, then a separate elementwise pass over the same bytes (`i2v_silu_f16` stands in for the ReLU pass
              the library does not have) -- at 16 x {64^2, 128^2, 256^2, 512^2} pixels of 64 channels.  Time per layer from device
              events around replays of a captured graph of back-to-back launches, alternating the two; the achieved TB/s and TFLOP/s
              from the bytes and operations the shape needs (input read once, output written once, the weights once; 2 x 576 x 64
              per pixel) and the fraction of the roofline max(bytes / 8.0 TB/s, FLOP / 2.5 PFLOP/s) (spec peaks), naming the bound.
  (b) vae:    AutoencoderTiny.decode against AutoencoderKL.decode for 16 frames at 512^2 (the whole batch, and frame by frame as
              `enable_vae_slicing` runs it), and `encode` of one 512^2 image, random weights, alternating, medians.
  (c) sample: a 4-step LCM sample (guidance 1.5) of 16 frames at 512^2 end to end -- condition image in, frames out -- with each VAE:
              wall time of `pipe(...)` on a cached graph, alternating.

One GPU process at a time: each step is a child process under its own time limit, and the first one that fails ends the script (nothing
more is started on the GPU after a failure).  usage (GPU box, repository root):   python tools/taesd_probe.py --out FILE.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = {"layer": 240, "vae": 300, "sample": 420}
HBM_PEAK, MFMA_PEAK = 8.0e12, 2.5e15          # spec: bytes/s, fp16 FLOP/s dense


def _window_ms(fn, torch, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _alternate(fns, torch, rounds, inner):
    """{name: [ms per call, one per round]}: the variants take turns inside every round, so all see the same clock and neighbours"""
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_window_ms(fn, torch, inner))
    return t


def _stats(v):
    return dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v))


def worker_layer(args):
    import torch
    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.blocks import pack_conv3x3
    K, dev = pkg.kernels, torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    w = (torch.rand(64, 64, 3, 3, generator=g) * 2 - 1) * (3.0 / 576) ** 0.5
    wc, wg, bias = K.pack_conv_c64(w.to(dev)), pack_conv3x3(w.to(dev)), (torch.rand(64, generator=g) - 0.5).half().to(dev)
    res = {"peaks": dict(hbm_bytes_per_s=HBM_PEAK, fp16_mfma_flop_per_s=MFMA_PEAK), "sizes": []}
    for side in (64, 128, 256, 512):
        x = torch.randn(16, side, side, 64, generator=g).half().to(dev)
        out = torch.empty_like(x)
        new = lambda: K.conv3x3_c64(x, wc, bias, relu_mid=True, out=out)
        old_conv = lambda: K.conv3x3(x, wg, bias)
        old = lambda: K.silu(K.conv3x3(x, wg, bias))
        route = None
        graphs = {}
        for name, fn in (("c64", new), ("conv3x3", old_conv), ("conv3x3_then_pass", old)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            if name == "conv3x3":
                route = K.last_gemm_route()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(args.launches):
                    fn()
            graphs[name].replay()
        torch.cuda.synchronize()
        t = _alternate({k: gr.replay for k, gr in graphs.items()}, torch, args.rounds, 3)
        pixels = 16 * side * side
        flop, byts = 2.0 * 576 * 64 * pixels, pixels * 64 * 2 * 2 + 64 * 576 * 2
        floor_s = max(byts / HBM_PEAK, flop / MFMA_PEAK)
        row = {"pixels": [16, side, side], "flop": flop, "bytes": byts, "launches_per_window": args.launches,
               "roofline_bound": "hbm" if byts / HBM_PEAK >= flop / MFMA_PEAK else "mfma", "roofline_ms": floor_s * 1e3,
               "conv3x3_route": route}
        for k, v in t.items():
            ms = [m / args.launches for m in v]
            med = statistics.median(ms)
            row[k] = dict(_stats(ms), tb_per_s=byts / (med * 1e-3) / 1e12, tflop_per_s=flop / (med * 1e-3) / 1e12,
                          fraction_of_roofline=floor_s / (med * 1e-3))
        row["c64_over_conv3x3_then_pass"] = row["c64"]["ms_median"] / row["conv3x3_then_pass"]["ms_median"]
        row["c64_over_conv3x3"] = row["c64"]["ms_median"] / row["conv3x3"]["ms_median"]
        # (same weights, same input: the two routes' results before the activation differ by summation order only)
        a, b = K.conv3x3_c64(x, wc, bias), K.conv3x3(x, wg, bias)
        row["max_abs_difference_pre_activation"] = (a.float() - b.float()).abs().max().item()
        res["sizes"].append(row)
        del graphs, x, out
    print(json.dumps(res))


def _vaes(torch, pkg, dev):
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    kl, tiny = pkg.AutoencoderKL(), pkg.AutoencoderTiny()
    init_random_weights_(kl, seed=3)
    init_random_weights_(tiny, seed=4)
    return kl.to(device=dev, dtype=torch.float16).eval(), tiny.to(device=dev, dtype=torch.float16).eval()


def worker_vae(args):
    import torch
    import i2v_adapter_unofficial_amd as pkg
    dev = torch.device("cuda:0")
    kl, tiny = _vaes(torch, pkg, dev)
    g = torch.Generator().manual_seed(2)
    z = torch.randn(16, 4, 64, 64, generator=g).to(dev)
    img = (torch.rand(1, 3, 512, 512, generator=g) * 2 - 1).to(dev)
    sliced = lambda v: [v.decode(z[i: i + 1]).sample for i in range(16)]
    fns = {"tiny_decode_batch16": lambda: tiny.decode(z), "kl_decode_batch16": lambda: kl.decode(z),
           "tiny_decode_sliced16": lambda: sliced(tiny), "kl_decode_sliced16": lambda: sliced(kl),
           "tiny_encode_1": lambda: tiny.encode(img), "kl_encode_1": lambda: kl.encode(img)}
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    t = _alternate(fns, torch, args.rounds, 2)
    res = {"latents": list(z.shape), "image": list(img.shape), "what": "ms per call (16 frames for the decodes, one image for the encodes)"}
    for k, v in t.items():
        res[k] = _stats(v)
    res["kl_over_tiny_decode_batch16"] = res["kl_decode_batch16"]["ms_median"] / res["tiny_decode_batch16"]["ms_median"]
    res["kl_over_tiny_decode_sliced16"] = res["kl_decode_sliced16"]["ms_median"] / res["tiny_decode_sliced16"]["ms_median"]
    res["kl_decode_ms_per_frame_512"] = res["kl_decode_sliced16"]["ms_median"] / 16
    res["tiny_decode_ms_per_frame_512"] = res["tiny_decode_sliced16"]["ms_median"] / 16
    print(json.dumps(res))


def worker_sample(args):
    sys.path.insert(0, ROOT)
    import PIL.Image
    import torch
    import bench
    import i2v_adapter_unofficial_amd as pkg
    dev = torch.device("cuda:0")
    kl, tiny = _vaes(torch, pkg, dev)
    unet = bench.build_hip_model(dev, seed=1234)
    d = bench.sample_inputs(0, 16, 64, ip=False)
    image = PIL.Image.fromarray((torch.rand(512, 512, 3, generator=torch.Generator().manual_seed(9)) * 255).to(torch.uint8).numpy())
    gens = lambda: dict(generator=torch.Generator().manual_seed(1), prior_mask_generator=torch.Generator().manual_seed(2),
                        prior_noise_generator=torch.Generator().manual_seed(3))
    call = dict(prompt_embeds=d["pe"].half(), negative_prompt_embeds=d["ne"].half(), condition_image=image, height=512, width=512,
                num_frames=16, blur_sigma=0.8, num_inference_steps=4, guidance_scale=1.5, output_type="pt")
    pipe = pkg.I2VAdapterPipeline(vae=kl, unet=unet, scheduler=pkg.LCMScheduler())       # (the VAE is outside the captured step: swapped per call)
    pipes = {"kl": kl, "tiny": tiny, "latent_only": tiny}
    for vae in (kl, tiny):
        pipe.vae = vae
        pipe(**call, **gens())                             # captures the step (once), warms every VAE shape
    t = {k: [] for k in pipes}
    for _ in range(args.rounds):
        for name, vae in pipes.items():
            pipe.vae = vae
            kw = dict(call, output_type="latent") if name == "latent_only" else call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frames = pipe(**kw, **gens()).frames
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3)
            assert bool(torch.isfinite(frames).all())
    res = {"what": "wall ms of one pipe(...) call on a cached graph: condition image in, 16 frames of 512 x 512 out (latent_only: "
                   "latents out, the tiny VAE's encode in front), LCMScheduler, 4 steps, guidance 1.5"}
    for k, v in t.items():
        res[k] = _stats(v)
    res["kl_over_tiny"] = res["kl"]["ms_median"] / res["tiny"]["ms_median"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "taesd_probe.json"))
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per variant")
    ap.add_argument("--launches", type=int, default=20, help="layers per captured graph of the kernel measurement")
    ap.add_argument("--steps", default="layer,vae,sample")
    ap.add_argument("--worker", choices=sorted(STEP_LIMIT_S))
    args = ap.parse_args()
    if args.worker:
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("taesd_probe: needs a GPU (a measurement does not fall back)")
        with torch.no_grad():
            {"layer": worker_layer, "vae": worker_vae, "sample": worker_sample}[args.worker](args)
        return 0
    result = {}
    for step in args.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]), sys.executable, os.path.abspath(__file__), "--worker", step,
               "--rounds", str(args.rounds), "--launches", str(args.launches)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            print(f"taesd_probe: step {step} ended with status {r.returncode}; nothing more is run\n{r.stdout[-2000:]}\n"
                  f"{r.stderr[-4000:]}", file=sys.stderr)
            return 1
        result[step] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{step}: {json.dumps(result[step])}", flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
