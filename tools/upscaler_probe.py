"""Upscaler measurement, on one MI355X, everything inside ONE call of this script:

  (a) layer:   i2v_conv3x3_c64_prelu_f16 against i2v_conv3x3_c64_f16 (ReLU) at 16 x 512^2 and 16 x 64^2 pixels -- and, with
               --parent_lib, against the ReLU launch of a library built from the parent commit, loaded beside this one: the three take
               turns inside every round (same clock, same neighbours).  Time per layer from device events around replays of a captured
               graph of back-to-back launches.
  (b) exit:    i2v_pixel_shuffle_add_f32 (s = 4, 16 x 512^2 in, 16 x 3 x 2048^2 fp32 out) against i2v_copy3d_f16 moving the same
               number of bytes (read + written), alternating; the achieved TB/s of both.
  (c) network: SRVGGNetCompact.forward for num_conv 16 and 32 at s = 4 on 16 frames of 512^2 (random weights), ms per call, and
               the sum of its parts from (a) and (b).
  (d) taesd:   AutoencoderTiny.decode of 16 latents of 64^2 with this library's i2v_conv3x3_c64_f16 / i2v_taesd_prep_f16 and, with
               --parent_lib, with the parent's, alternating (the two entry points are swapped on the loaded handle; every other kernel
               of the decode is the same code in both builds).

One GPU process at a time: each step is a child process under its own time limit, and the first one that fails ends the script (nothing
more is started on the GPU after a failure).  usage (GPU box, repository root):
    python tools/upscaler_probe.py --out profiles/upscaler_probe.json [--parent_lib PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = {"layer": 240, "exit": 120, "network": 240, "taesd": 240}


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


def _parent(args, lib):
    """the parent commit's library beside this one: its two c64 entry points bound with this build's signatures (the struct is unchanged)"""
    if not args.parent_lib:
        return None
    h = C.CDLL(os.path.abspath(args.parent_lib))
    for name in ("i2v_conv3x3_c64_f16", "i2v_taesd_prep_f16"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = lib.SIGNATURES[name]
    return h


def worker_layer(args):
    import torch
    import i2v_adapter_unofficial_amd as pkg
    K, lib, dev = pkg.kernels, pkg._lib, torch.device("cuda:0")
    parent = _parent(args, lib)
    g = torch.Generator().manual_seed(1)
    w = (torch.rand(64, 64, 3, 3, generator=g) * 2 - 1) * (3.0 / 576) ** 0.5
    wc, bias = K.pack_conv_c64(w.to(dev)), (torch.rand(64, generator=g) - 0.5).half().to(dev)
    slope = (torch.rand(64, generator=g) * 1.6 - 0.3).to(dev)
    res = {"parent_lib": bool(parent), "abi_parent": parent.i2v_abi_version() if parent else None, "sizes": []}
    for side in (512, 64):
        x = torch.randn(16, side, side, 64, generator=g).half().to(dev)
        out = torch.empty_like(x)
        fns = {"prelu": lambda: K.conv3x3_c64(x, wc, bias, slope=slope, out=out),
               "relu": lambda: K.conv3x3_c64(x, wc, bias, relu_mid=True, out=out)}
        if parent:
            p = lib.ConvC64Params()
            p.x, p.ldx, p.w, p.bias, p.out, p.ldo = x.data_ptr(), 64, wc.data_ptr(), bias.data_ptr(), out.data_ptr(), 64
            p.n_img, p.height, p.width, p.cin, p.cout, p.relu_mid = 16, side, side, 64, 64, 1

            def relu_parent():
                if parent.i2v_conv3x3_c64_f16(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0:
                    raise RuntimeError("the parent library refused the launch")
            fns["relu_parent"] = relu_parent
        graphs = {}
        for name, fn in fns.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(args.launches):
                    fn()
            graphs[name].replay()
        torch.cuda.synchronize()
        t = _alternate({k: gr.replay for k, gr in graphs.items()}, torch, args.rounds, 3)
        row = {"pixels": [16, side, side], "launches_per_window": args.launches}
        for k, v in t.items():
            row[k] = _stats([m / args.launches for m in v])
        row["prelu_over_relu"] = row["prelu"]["ms_median"] / row["relu"]["ms_median"]
        if parent:
            row["relu_over_relu_parent"] = row["relu"]["ms_median"] / row["relu_parent"]["ms_median"]
            row["prelu_over_relu_parent"] = row["prelu"]["ms_median"] / row["relu_parent"]["ms_median"]
            fns["relu"]()
            a = out.clone()
            fns["relu_parent"]()
            row["relu_bit_equal_to_parent"] = bool(torch.equal(a, out))
        res["sizes"].append(row)
        del graphs, x, out
    print(json.dumps(res))


def worker_exit(args):
    import torch
    import i2v_adapter_unofficial_amd as pkg
    K, dev = pkg.kernels, torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    n, side, s = 16, 512, 4
    y = (torch.randn(n, side, side, 64, generator=g) * 0.1).half().to(dev)
    src = (torch.rand(n, 3, side, side, generator=g) * 2 - 1).to(dev)
    out = torch.empty((n, 3, s * side, s * side), dtype=torch.float32, device=dev)
    # bytes the exit must move: 3 s^2 fp16 of every pixel of y, the source once, the output once
    moved = n * side * side * (3 * s * s * 2 + 3 * 4) + out.numel() * 4
    # a copy of the same traffic: rows of 64 fp16, moved / 2 bytes in and as many out
    rows = moved // 2 // 128 // 16
    a = torch.randn(16, rows, 64, generator=g).half().to(dev)
    b = torch.empty_like(a)
    fns = {"exit": lambda: K.pixel_shuffle_add(y, src, s, unit_in=True, clamp=True, signed_out=True, out=out),
           "copy3d_same_bytes": lambda: K.copy3d(a, b)}
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    t = _alternate(fns, torch, args.rounds, 5)
    res = {"frames": [n, 3, side, side], "s": s, "bytes_needed": moved, "bytes_of_the_y_buffer": y.numel() * 2}
    for k, v in t.items():
        res[k] = dict(_stats(v), tb_per_s=moved / (statistics.median(v) * 1e-3) / 1e12)
    res["exit_over_copy"] = res["exit"]["ms_median"] / res["copy3d_same_bytes"]["ms_median"]
    print(json.dumps(res))


def worker_network(args):
    import torch
    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    frames = (torch.rand(16, 3, 512, 512, generator=g) * 2 - 1).to(dev)
    nets = {}
    for nc in (16, 32):
        m = pkg.SRVGGNetCompact(num_conv=nc, upscale=4)
        init_random_weights_(m, seed=nc)
        nets[f"num_conv_{nc}"] = m.to(dev).eval()
    fns = {k: (lambda m=m: m(frames)) for k, m in nets.items()}
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    t = _alternate(fns, torch, args.rounds, 2)
    res = {"frames": list(frames.shape), "s": 4, "what": "ms per forward: prep + (1 + num_conv) PReLU launches + exit convolution + exit"}
    for k, v in t.items():
        res[k] = _stats(v)
    print(json.dumps(res))


def worker_taesd(args):
    import torch
    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    lib, dev = pkg._lib, torch.device("cuda:0")
    h = lib.load()
    parent = _parent(args, lib)
    tiny = pkg.AutoencoderTiny()
    init_random_weights_(tiny, seed=4)
    tiny = tiny.to(device=dev, dtype=torch.float16).eval()
    z = torch.randn(16, 4, 64, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    names = ("i2v_conv3x3_c64_f16", "i2v_taesd_prep_f16")
    own = {n: getattr(h, n) for n in names}

    def decode_with(fnset):
        def run():
            for n in names:
                setattr(h, n, fnset[n])
            try:
                return tiny.decode(z).sample
            finally:
                for n in names:
                    setattr(h, n, own[n])
        return run
    fns = {"this_build": decode_with(own)}
    if parent:
        fns["parent_c64"] = decode_with({n: getattr(parent, n) for n in names})
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    t = _alternate(fns, torch, args.rounds, 2)
    res = {"latents": list(z.shape), "parent_lib": bool(parent), "what": "ms per AutoencoderTiny.decode of 16 frames at 512^2"}
    for k, v in t.items():
        res[k] = _stats(v)
    if parent:
        res["this_over_parent"] = res["this_build"]["ms_median"] / res["parent_c64"]["ms_median"]
        res["bit_equal_to_parent"] = bool(torch.equal(fns["this_build"](), fns["parent_c64"]()))
    print(json.dumps(res))


WORKERS = {"layer": worker_layer, "exit": worker_exit, "network": worker_network, "taesd": worker_taesd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "upscaler_probe.json"))
    ap.add_argument("--parent_lib", default=None, help="libi2v_hip.so built from the parent commit, for the same-box comparisons")
    ap.add_argument("--rounds", type=int, default=7, help="alternating windows per variant")
    ap.add_argument("--launches", type=int, default=20, help="layers per captured graph of the kernel measurement")
    ap.add_argument("--steps", default="layer,exit,network,taesd")
    ap.add_argument("--worker", choices=sorted(STEP_LIMIT_S))
    args = ap.parse_args()
    if args.worker:
        sys.path.insert(0, ROOT)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("upscaler_probe: needs a GPU (a measurement does not fall back)")
        with torch.no_grad():
            WORKERS[args.worker](args)
        return 0
    result = {}
    for step in args.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]), sys.executable, os.path.abspath(__file__), "--worker", step,
               "--rounds", str(args.rounds), "--launches", str(args.launches)]
        if args.parent_lib:
            cmd += ["--parent_lib", args.parent_lib]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            print(f"upscaler_probe: step {step} ended with status {r.returncode}; nothing more is run\n{r.stdout[-2000:]}\n"
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
