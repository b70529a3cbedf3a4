"""LoRA measurement, on one MI355X, everything inside ONE call of this script:

  (a) kernel:  `i2v_lora_merge` of one fp16 weight next to the device-to-device `copy_` of the same weight (the floor: it moves the same
      base-in / dst-out bytes) and next to the same merge through torch (`torch.addmm` in fp32 over fp32 copies of the operands, then
      `.half()`), for the SD-1.5 shapes 320x320, 1280x1280, 1280x768, 2560x320 (GEGLU), 320x2880 and 1280x11520 (convs) at ranks 4,
      16, 64, 128 and 1 and 2 adapters: time per call from device events around replays of a captured graph of back-to-back launches,
      alternating the three, and GB/s from the bytes the shapes say are moved (base + dst + the factors once).  The buffers (59 MB at
      most) stay in the 256 MiB Infinity Cache across replays: cache-resident rates, comparable with each other, not HBM rates.
  (b) sync:    the whole `_sync_lora()` of the SD-1.5-width UNet (random weights) for an attention-only rank-16 LoRA and an all-layers
      rank-64 one: launches (`i2v_lora_merge` calls) and wall time (host clock around the call, ending in a device synchronise).
  (c) bench:   `bench.py --gpus 1 --steps K --warmup W --no-cpu-baseline` on this tree with no LoRA, on this tree with a rank-16
      attention LoRA merged into the model bench.py builds (same kernels, other weights), and -- with --parent-tree DIR, a built
      checkout of the parent commit -- on that tree.  The three are reported, not gated.

One GPU process at a time: each step is a child process under its own time limit, and the first one that fails ends the script (nothing
more is started on the GPU after a failure).  usage (GPU box, repository root):   python tools/lora_probe.py --out FILE.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(320, 320), (1280, 1280), (1280, 768), (2560, 320), (320, 2880), (1280, 11520)]
RANKS = [4, 16, 64, 128]
STEP_LIMIT_S = {"kernel": 420, "sync": 300, "bench_plain": 240, "bench_lora": 240, "bench_parent": 240}


def _ms(fn, torch, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def worker_kernel(args):
    sys.path.insert(0, ROOT)
    import torch
    import i2v_adapter_unofficial_amd as pkg
    K = pkg.kernels
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    rows = []
    for n_out, n_in in SHAPES:
        base = (torch.randn(n_out, n_in, generator=g) * 0.05).half().to(dev)
        dst = torch.empty_like(base)
        base32 = base.float()
        for rank in RANKS:
            for n_ad in (1, 2):
                ads = [((torch.randn(rank, n_in, generator=g) / rank ** 0.5).half().to(dev),
                        (torch.randn(n_out, rank, generator=g) * 0.02).half().to(dev), 0.75 - 0.5 * j) for j in range(n_ad)]
                ads32 = [(d.float(), u.float(), s) for d, u, s in ads]

                def merge():
                    K.lora_merge(dst, base, ads)

                def copy():
                    dst.copy_(base)

                def addmm():
                    acc = base32
                    for d, u, s in ads32:
                        acc = torch.addmm(acc, u, d, alpha=s)
                    return acc.half()
                fns = {"merge": merge, "copy": copy, "torch_addmm_f32": addmm}
                # a launch is a few microseconds, less than a host call: replay a captured chain of them, so the events time the device
                launches = max(8, min(args.launches, int(2e9 / (n_out * n_in * 4))))
                graphs = {}
                for name, fn in fns.items():
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    graphs[name] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graphs[name]):
                        for _ in range(launches):
                            fn()
                    graphs[name].replay()
                torch.cuda.synchronize()
                t = {k: [] for k in fns}
                for _ in range(args.rounds):                      # alternating: all see the same clock and neighbours
                    for name in fns:
                        t[name].append(_ms(graphs[name].replay, torch, 2) / launches * 1e3)
                wbytes = 2 * n_out * n_in * 2
                fbytes = sum(2 * rank * (n_in + n_out) for _ in ads)
                row = {"out": n_out, "in": n_in, "rank": rank, "adapters": n_ad, "launches_per_replay": launches,
                       "weight_bytes_in_plus_out": wbytes, "factor_bytes": fbytes, "flop": 2 * n_out * n_in * rank * n_ad}
                for name in fns:
                    us = statistics.median(t[name])
                    row[name + "_us"] = round(us, 3)
                    row[name + "_us_min"] = round(min(t[name]), 3)
                row["merge_gb_per_s"] = round((wbytes + fbytes) / (row["merge_us"] * 1e-6) / 1e9, 1)
                row["copy_gb_per_s"] = round(wbytes / (row["copy_us"] * 1e-6) / 1e9, 1)
                row["merge_over_copy"] = round(row["merge_us"] / row["copy_us"], 2)
                rows.append(row)
                del graphs
    print(json.dumps({"what": "us per call, median over alternating graph replays; GB/s from the shapes' bytes (fp16 base in + dst out, "
                              "+ the factors once for the merge).  Every working set (59 MB at most) fits the 256 MiB Infinity Cache "
                              "and is replayed over the same buffers: these are cache-resident rates, comparable with each other, "
                              "not HBM rates", "rows": rows}))


def _sd15_unet(torch, seed=1234):
    sys.path.insert(0, ROOT)
    import bench
    return bench.build_hip_model(torch.device("cuda:0"), seed=seed)


def _random_lora_state_dict(torch, unet, rank, attention_only, seed):
    """diffusers-spelled random LoRA for the model's Linear / conv weights (alpha-free), fp16"""
    from i2v_adapter_unofficial_amd.lora import lora_target_shapes
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for path, shape in lora_target_shapes(unet).items():
        if attention_only and not path.endswith((".to_q", ".to_k", ".to_v", ".to_out.0")):
            continue
        n_in = 1
        for s in shape[1:]:
            n_in *= s
        sd[f"{path}.lora.down.weight"] = (torch.randn(rank, n_in, generator=g) / rank ** 0.5 * 0.1).half()
        sd[f"{path}.lora.up.weight"] = (torch.randn(shape[0], rank, generator=g) * 0.02).half()
    return sd


def worker_sync(args):
    import torch
    unet = _sd15_unet(torch)
    import i2v_adapter_unofficial_amd as pkg
    K = pkg.kernels
    res = {}
    for name, rank, attn in (("attention_only_rank16", 16, True), ("all_layers_rank64", 64, False)):
        sd = _random_lora_state_dict(torch, unet, rank, attn, seed=rank)
        rep = unet.load_lora(sd, adapter_name=name)
        calls = []
        real = K.lora_merge
        K.lora_merge = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        times = []
        try:
            for i in range(args.rounds + 1):
                unet.set_lora_scale(1.0 - 0.01 * i)                      # a changed scale: every targeted weight is merged again
                calls.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                unet._sync_lora()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
        finally:
            K.lora_merge = real
        wbytes = sum(2 * dict(unet.named_modules())[p].weight.numel() * 2 for p in unet._lora_state()["stash"])
        res[name] = {"modules": rep["modules"], "launches": len(calls), "wall_ms_first": round(times[0], 3),
                     "wall_ms_median_after": round(statistics.median(times[1:]), 3), "wall_ms_min": round(min(times[1:]), 3),
                     "weight_bytes_in_plus_out": wbytes}
        t0 = time.perf_counter()
        unet.unload_lora()
        torch.cuda.synchronize()
        res[name]["unload_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    print(json.dumps(res))


def worker_bench_lora(args):
    """bench.py, unchanged, over a model with a LoRA merged: its model builder is wrapped, nothing else"""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    build = bench.build_hip_model

    def build_with_lora(dev, seed=None):
        m = build(dev, seed=seed)
        if seed is not None:
            m.load_lora(_random_lora_state_dict(torch, m, 16, True, seed=16), adapter_name="probe")
            m._sync_lora()
        return m
    bench.build_hip_model = build_with_lora
    sys.argv = ["bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--no-cpu-baseline"]
    return bench.main()


def _bench_fields(line):
    d = json.loads(line)
    return {k: d.get(k) for k in ("metric", "value", "unit", "ms_per_step", "window_ms_per_step", "steps", "warmup")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "lora_probe.json"))
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per variant")
    ap.add_argument("--launches", type=int, default=100, help="launches per captured chain of the kernel measurement (fewer for large weights)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: its bench.py is run too")
    ap.add_argument("--skip", default="", help="comma-separated steps to leave out")
    ap.add_argument("--worker", choices=["kernel", "sync", "bench_lora"])
    args = ap.parse_args()
    if args.worker:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("lora_probe: needs a GPU (a measurement does not fall back)")
        if args.worker == "bench_lora":
            return worker_bench_lora(args) or 0
        with torch.no_grad():
            {"kernel": worker_kernel, "sync": worker_sync}[args.worker](args)
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--rounds", str(args.rounds), "--launches", str(args.launches), "--steps",
          str(args.steps), "--warmup", str(args.warmup)]
    bench = ["bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--no-cpu-baseline"]
    steps = [("kernel", me + ["--worker", "kernel"], ROOT), ("sync", me + ["--worker", "sync"], ROOT),
             ("bench_plain", [sys.executable] + bench, ROOT), ("bench_lora", me + ["--worker", "bench_lora"], ROOT)]
    if args.parent_tree:
        steps.insert(2, ("bench_parent", [sys.executable] + bench, os.path.abspath(args.parent_tree)))
    result = {}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for step, cmd, cwd in steps:
        if step in args.skip.split(","):
            continue
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S[step])] + cmd, capture_output=True, text=True, cwd=cwd)
        if r.returncode != 0:
            print(f"lora_probe: step {step} ended with status {r.returncode}; nothing more is run\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}",
                  file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1]
        result[step] = _bench_fields(line) if step.startswith("bench") else json.loads(line)
        print(f"{step}: {json.dumps(result[step])[:3000]}", flush=True)
        with open(args.out, "w") as f:                                # (after every step: a later failure keeps what was measured)
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
