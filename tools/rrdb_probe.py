"""RRDBNet measurement, on one MI355X, everything inside ONE call of this script:

  (a) dense:   i2v_conv3x3_dense_f16 at every cin (64 .. 160 -> 32 in place, 192 -> 64 with the residual stage) at 16 x 512^2 and
               16 x 64^2 pixels against the route the parent commit has for the same layer: the copy that builds a contiguous tensor of
               the first cin channels (the concatenation) plus `K.conv3x3` on it.  The two take turns inside every round (same clock,
               same neighbours); the parent route's two parts are also timed apart.
  (b) up2:     i2v_conv3x3_c64_up2_prelu_f16 (16 x 512^2 -> 1024^2) against a mover that writes the upsampled tensor plus the plain
               PReLU launch on it, alternating.
  (c) network: RRDBNet.forward for num_block 6 and 23 on 16 frames of 512^2 -> 2048^2 (random weights), ms per call and TFLOP/s on the
               body's count (2 x 9 x 26624 x 3 FLOP per pixel and RRDB: 33.07 MFLOP per pixel at 23 blocks) and on the whole network's.

One GPU process at a time: each step is a child process under its own time limit, and the first one that fails ends the script (nothing
more is started on the GPU after a failure).  usage (GPU box, repository root):
    python tools/rrdb_probe.py --out profiles/rrdb_probe.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = {"dense": 300, "up2": 120, "network": 300}
RRDB_FLOP = 2 * 9 * (32 * (64 + 96 + 128 + 160) + 64 * 192) * 3                 # per pixel and RRDB
TAIL_FLOP = 2 * 9 * 64 * 64 * (2 + 4 + 16 + 16) + 2 * 9 * 64 * 3 * 16 + 2 * 9 * 3 * 64       # per input pixel: first, body, up1, up2, hr, last


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


def worker_dense(args):
    import torch
    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.blocks import pack_conv3x3
    K, dev = pkg.kernels, torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    res = {"what": "ms per layer; parent = copy of the first cin channels to a contiguous tensor + K.conv3x3 on it", "sizes": []}
    for side, inner in ((512, 3), (64, 20)):
        n = 16
        buf = torch.randn(n, side, side, 192, generator=g).half().to(dev)
        nxt = torch.empty((n, side, side, 64), dtype=torch.float16, device=dev)
        row = {"pixels": [n, side, side], "calls_per_window": inner, "cin": {}}
        for cin in K.DENSE_CIN:
            cout = 64 if cin == 192 else 32
            w = (torch.rand(cout, cin, 3, 3, generator=g) * 2 - 1) * (3.0 / (9 * cin)) ** 0.5
            bias = (torch.rand(cout, generator=g) - 0.5).half().to(dev)
            wd, wg = K.pack_conv_dense(w.to(dev)), pack_conv3x3(w.to(dev))
            cat = torch.empty((n, side, side, cin), dtype=torch.float16, device=dev)
            own = buf[..., :64]
            if cout == 32:
                dense = lambda: K.conv3x3_dense(buf, cin, wd, bias, out=buf[..., cin: cin + 32], slope=0.2)
            else:
                dense = lambda: K.conv3x3_dense(buf, cin, wd, bias, out=nxt, slope=1.0, s1=0.2, r1=own)
            copy = lambda: cat.copy_(buf[..., :cin])
            conv = lambda: K.conv3x3(cat, wg, bias)
            fns = {"dense": dense, "parent_copy_plus_conv": lambda: (copy(), conv()), "parent_copy": copy, "parent_conv": conv}
            for fn in fns.values():
                fn()
                fn()
            torch.cuda.synchronize()
            route = None
            conv()
            route = K.last_gemm_route()
            t = _alternate(fns, torch, args.rounds, inner)
            e = {k: _stats(v) for k, v in t.items()}
            e["parent_conv_route_family"] = route["family"]
            e["dense_tflops"] = 2 * 9 * cin * cout * n * side * side / (e["dense"]["ms_median"] * 1e-3) / 1e12
            e["dense_over_parent"] = e["dense"]["ms_median"] / e["parent_copy_plus_conv"]["ms_median"]
            e["dense_over_parent_conv_alone"] = e["dense"]["ms_median"] / e["parent_conv"]["ms_median"]
            row["cin"][str(cin)] = e
            del cat
        res["sizes"].append(row)
        del buf, nxt
    print(json.dumps(res))


def worker_up2(args):
    import torch
    import i2v_adapter_unofficial_amd as pkg
    K, dev = pkg.kernels, torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    n, side = 16, 512
    x = torch.randn(n, side, side, 64, generator=g).half().to(dev)
    w = (torch.rand(64, 64, 3, 3, generator=g) * 2 - 1) * (3.0 / 576) ** 0.5
    wc, bias = K.pack_conv_c64(w.to(dev)), (torch.rand(64, generator=g) - 0.5).half().to(dev)
    slope = torch.full((64,), 0.2, device=dev)
    up = torch.empty((n, 2 * side, 2 * side, 64), dtype=torch.float16, device=dev)
    out = torch.empty_like(up)
    mover = lambda: up.view(n, side, 2, side, 2, 64).copy_(x.view(n, side, 1, side, 1, 64).expand(n, side, 2, side, 2, 64))
    plain = lambda: K.conv3x3_c64(up, wc, bias, slope=slope, out=out)
    fns = {"up2": lambda: K.conv3x3_c64_up2(x, wc, bias, slope, out=out), "mover_plus_plain": lambda: (mover(), plain()), "mover": mover,
           "plain": plain}
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    fns["up2"]()
    a = out.clone()
    fns["mover_plus_plain"]()
    res = {"source": [n, side, side, 64], "bit_equal": bool(torch.equal(a, out))}
    t = _alternate(fns, torch, args.rounds, 3)
    for k, v in t.items():
        res[k] = _stats(v)
    res["up2_over_mover_plus_plain"] = res["up2"]["ms_median"] / res["mover_plus_plain"]["ms_median"]
    res["up2_over_plain"] = res["up2"]["ms_median"] / res["plain"]["ms_median"]
    res["up2_tflops"] = 2 * 9 * 64 * 64 * n * 4 * side * side / (res["up2"]["ms_median"] * 1e-3) / 1e12
    print(json.dumps(res))


def worker_network(args):
    import torch
    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    frames = (torch.rand(16, 3, 512, 512, generator=g) * 2 - 1).to(dev)
    pixels = 16 * 512 * 512
    res = {"frames": list(frames.shape), "what": "ms per forward: prep + conv_first + 15 dense launches per RRDB + the six tail launches"}
    for nb in (6, 23):
        m = pkg.RRDBNet(num_block=nb)
        init_random_weights_(m, seed=nb)
        m = m.to(dev).eval()
        fn = lambda: m(frames)
        fn()
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t = _alternate({"forward": fn}, torch, args.rounds, 1)["forward"]
        e = _stats(t)
        s = e["ms_median"] * 1e-3
        e["body_tflops"] = RRDB_FLOP * nb * pixels / s / 1e12
        e["network_tflops"] = (RRDB_FLOP * nb + TAIL_FLOP) * pixels / s / 1e12
        e["body_mflop_per_pixel"] = RRDB_FLOP * nb / 1e6
        e["peak_allocated_gb"] = torch.cuda.max_memory_allocated() / 1e9
        res[f"num_block_{nb}"] = e
        del m
    print(json.dumps(res))


WORKERS = {"dense": worker_dense, "up2": worker_up2, "network": worker_network}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "rrdb_probe.json"))
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per variant")
    ap.add_argument("--steps", default="dense,up2,network")
    ap.add_argument("--worker", choices=sorted(STEP_LIMIT_S))
    args = ap.parse_args()
    if args.worker:
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("rrdb_probe: needs a GPU (a measurement does not fall back)")
        with torch.no_grad():
            WORKERS[args.worker](args)
        return 0
    result = {}
    for step in args.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]), sys.executable, os.path.abspath(__file__), "--worker", step,
               "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            print(f"rrdb_probe: step {step} ended with status {r.returncode}; nothing more is run\n{r.stdout[-2000:]}\n"
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
