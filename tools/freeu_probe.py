"""FreeU measurement: what the switch costs when it is off and when it is on, at bench.py's flagship workload
(16 frames x 512 x 512, CFG, one captured step per replay), on one MI355X, everything inside ONE call of this script.

  (a) FreeU off, this tree against an earlier tree (--parent DIR: a built checkout of the parent commit, e.g. `git worktree add
      .ab_old/parent HEAD~1` + `python __graft_entry__.py` there): `python bench.py --dump-outputs` in both, alternating; the
      latents of the last timed step must be equal bit for bit, and the step's launch list (entry point, every scalar argument,
      every parameter struct with its pointers blanked) must be the same list.
  (b) FreeU on against off in one process, alternating windows of graph replays: added ms per step; then the same step under
      `rocprofv3 --kernel-trace --stats`, in a run of its own, for the per-launch time of the six i2v_freeu_f16 launches.

Every GPU step is a child process under its own `timeout`; the first one that fails ends the script (nothing more is started on the
GPU after a failure).  usage (GPU box, repository root):   python tools/freeu_probe.py --parent .ab_old/parent --out DIR
The modes below --worker are the children."""
import argparse
import glob
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREEU = dict(s1=0.9, s2=0.2, b1=1.2, b2=1.4)


# ------------------------------------------------------------------------------------------------------------- children
def _state(tree, frames, size):
    """bench.py's flagship state in `tree` (its bench.py, its package): (pkg, pipe, st, load)"""
    sys.path.insert(0, tree)
    import torch
    import bench
    import i2v_adapter_unofficial_amd as pkg
    dev = torch.device("cuda:0")
    model = bench.build_hip_model(dev, seed=1234)
    pipe = pkg.I2VAdapterPipeline(unet=model)
    sch = pipe.scheduler
    sch.set_timesteps(25)
    ts = sch.timesteps
    h_lat = size // 8
    s = bench.sample_inputs(0, frames, h_lat, False)
    st = dict(latents=torch.empty(1, frames, 4, h_lat, h_lat, device=dev), cond=torch.empty(1, 4, h_lat, h_lat, device=dev), copies=2,
              num_frames=frames, guidance=7.5, t_table=ts.float().to(dev), coef=sch.step_coefficients(ts).to(dev),
              step_idx=torch.zeros(1, dtype=torch.int32, device=dev),
              ctx_text=torch.empty(2, 77, 768, dtype=torch.float16, device=dev), ctx_ip=None)

    def load():
        st["latents"].copy_(s["lat"])
        st["cond"].copy_(s["cond"])
        st["ctx_text"].copy_(torch.cat([s["ne"], s["pe"]]).half())
        st["ctx_proj"] = model.project_context(st["ctx_text"], None, out=st.get("ctx_proj"))
        st["temb_table"] = model.project_time_table(st["t_table"], out=st.get("temb_table"))
        st["step_idx"].zero_()
    return pkg, pipe, st, load


def worker_launches(args):
    """the launch list of one step, FreeU off (works in a tree from before FreeU too): JSON {count, sha256, per entry point}"""
    import ctypes as C  # noqa: F401
    import torch
    pkg, pipe, st, load = _state(os.path.abspath(args.tree), args.frames, args.size)
    H, L = pkg.handle, pkg._lib
    with torch.no_grad():
        load()
        pipe._step(st)                       # packs weights
        load()
        torch.cuda.synchronize()
        rec = H._RecordingLib(L.load())
        saved, L._lib = L._lib, rec
        try:
            pipe._step(st)
        finally:
            L._lib = saved
        torch.cuda.synchronize()
    names = getattr(H, "ENTRY_NAMES", None) or {i: n for n, i in H.ENTRY_IDS.items()}      # (a tree from before ENTRY_NAMES)
    hsh, per = hashlib.sha256(), {}
    for entry, sbytes, slots, ptrs in rec.ops:
        blk = bytearray(sbytes) + bytearray(-len(sbytes) % 8)
        for v in slots:
            blk += v
        for off, _v, _what in ptrs:          # addresses differ from run to run: blank them, keep which arguments are set
            blk[off: off + 8] = b"\xff" * 8
        hsh.update(names[entry].encode() + bytes(blk))
        per[names[entry]] = per.get(names[entry], 0) + 1
    print(json.dumps(dict(launches=len(rec.ops), sha256=hsh.hexdigest(), per_entry=per)))


def worker_onoff(args):
    """FreeU off / on captured steps in one process, alternating windows"""
    import torch
    pkg, pipe, st, load = _state(ROOT, args.frames, args.size)
    unet = pipe.unet
    graphs = {}
    with torch.no_grad():
        load()
        for mode in ("off", "on"):
            if mode == "on":
                unet.enable_freeu(**FREEU)
            s2 = dict(st)                                  # its own latents and step counter; the per-sample buffers are read only
            s2["latents"], s2["step_idx"] = st["latents"].clone(), st["step_idx"].clone()
            pipe._step(s2)                                 # eager warm-up
            s2["latents"].copy_(st["latents"])
            s2["step_idx"].zero_()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                pipe._step(s2)
            graphs[mode] = (g, s2)
        unet.disable_freeu()
        times = {"off": [], "on": []}
        for r in range(args.rounds + 1):
            for mode in ("off", "on"):
                g, s2 = graphs[mode]
                s2["latents"].copy_(st["latents"])
                s2["step_idx"].zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    g.replay()
                torch.cuda.synchronize()
                if r:                              # (round 0 warms up)
                    times[mode].append((time.perf_counter() - t0) / args.steps * 1e3)
        finite = all(bool(torch.isfinite(graphs[m][1]["latents"]).all()) for m in graphs)
        differ = not torch.equal(graphs["on"][1]["latents"], graphs["off"][1]["latents"])
    print(json.dumps(dict(off_ms=times["off"], on_ms=times["on"], finite=finite, outputs_differ=differ)))


def worker_trace(args):
    """the FreeU-on step replayed --steps times: the child of the rocprofv3 run"""
    import torch
    pkg, pipe, st, load = _state(ROOT, args.frames, args.size)
    pipe.unet.enable_freeu(**FREEU)
    with torch.no_grad():
        load()
        pipe._step(st)
        load()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pipe._step(st)
        for _ in range(args.steps):
            g.replay()
        torch.cuda.synchronize()
    print(json.dumps(dict(finite=bool(torch.isfinite(st["latents"]).all()))))


# ------------------------------------------------------------------------------------------------------------- the driver
class StepFailed(RuntimeError):
    pass


def run(cmd, cwd, limit, log):
    """one GPU step under its own time limit; a failure ends the script"""
    full = ["timeout", "-k", "10", str(limit)] + cmd
    log.write(f"$ (cd {os.path.relpath(cwd, ROOT)} && {' '.join(full)})\n")
    log.flush()
    res = subprocess.run(full, cwd=cwd, capture_output=True, text=True)
    if res.returncode != 0:
        log.write(res.stdout[-2000:] + "\n" + res.stderr[-4000:] + f"\nexit status {res.returncode}\n")
        raise StepFailed(f"{' '.join(cmd)} in {cwd}: exit status {res.returncode} (nothing more is started on the GPU)")
    return res.stdout


def last_json(text):
    return json.loads([ln for ln in text.strip().splitlines() if ln.startswith("{")][-1])


def driver(args):
    import numpy as np
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    py = sys.executable
    me = os.path.abspath(__file__)
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))
    with open(os.path.join(out, "freeu_probe.log"), "w") as log:
        say("# FreeU (DESIGN 4.8): one MI355X, every run inside ONE call of tools/freeu_probe.py, alternating.")
        say(f"# workload: bench.py's flagship step, {args.frames} frames x {args.size} x {args.size}, CFG (B = 2), one graph replay per step")
        parent = os.path.abspath(args.parent) if args.parent else None
        if parent:
            say()
            say(f"(a) FreeU off: the parent commit's tree against this tree, `python bench.py --steps {args.steps} --warmup 3 --dump-outputs`")
            ms = {"parent": [], "this": []}
            say(f"{'pair':6s}{'parent ms':>12s}{'this ms':>12s}{'this - parent':>16s}")
            for r in range(args.pairs):
                for name, tree in (("parent", parent), ("this", ROOT)):
                    d = os.path.join(out, f"dump_{name}")
                    o = run([py, "bench.py", "--steps", str(args.steps), "--warmup", "3", "--dump-outputs", d], tree, 600, log)
                    ms[name].append(last_json(o)["ms_per_step"])
                say(f"{r + 1:<6d}{ms['parent'][-1]:12.3f}{ms['this'][-1]:12.3f}{ms['this'][-1] - ms['parent'][-1]:16.3f}")
            sp = lambda v: max(v) - min(v)
            diff = statistics.mean(ms["this"]) - statistics.mean(ms["parent"])
            say(f"mean difference {diff:+.3f} ms; spread between same-tree runs: parent {sp(ms['parent']):.3f} ms, this {sp(ms['this']):.3f} ms")
            a, b = (np.load(os.path.join(out, f"dump_{n}", "latents.npy")) for n in ("parent", "this"))
            same = a.shape == b.shape and a.tobytes() == b.tobytes()
            say(f"bench.py --dump-outputs latents ({a.size} values), this tree against the parent: {'equal bit for bit' if same else 'DIFFERENT'}")
            ll = {}
            for name, tree in (("parent", parent), ("this", ROOT)):
                ll[name] = last_json(run([py, me, "--worker", "launches", "--tree", tree, "--frames", str(args.frames),
                                          "--size", str(args.size)], ROOT, 420, log))
            same_l = ll["parent"]["sha256"] == ll["this"]["sha256"] and ll["parent"]["launches"] == ll["this"]["launches"]
            say(f"launch list of one step, FreeU off: parent {ll['parent']['launches']} launches, this {ll['this']['launches']}; entry points, "
                f"scalar arguments and parameter structs (pointers blanked) {'are the same list' if same_l else 'DIFFER'}")
            say(f"  sha256 parent {ll['parent']['sha256'][:16]}..., this {ll['this']['sha256'][:16]}...; per entry point: "
                + ", ".join(f"{k.replace('i2v_', '')} {v}" for k, v in sorted(ll["this"]["per_entry"].items())))
            if not (same and same_l):
                raise StepFailed("FreeU off does not reproduce the parent")
        say()
        say(f"(b) FreeU on (s1 0.9, s2 0.2, b1 1.2, b2 1.4) against off, one process, alternating windows of {args.steps} graph replays")
        oo = last_json(run([py, me, "--worker", "onoff", "--frames", str(args.frames), "--size", str(args.size), "--steps", str(args.steps),
                            "--rounds", str(args.rounds)], ROOT, 600, log))
        say(f"{'window':8s}{'off ms':>10s}{'on ms':>10s}{'added ms':>10s}")
        for i, (x, y) in enumerate(zip(oo["off_ms"], oo["on_ms"])):
            say(f"{i + 1:<8d}{x:10.3f}{y:10.3f}{y - x:10.3f}")
        off, on = statistics.median(oo["off_ms"]), statistics.median(oo["on_ms"])
        say(f"median off {off:.3f} ms, on {on:.3f} ms: FreeU adds {on - off:+.3f} ms per step ({(on - off) / off * 100:+.2f} %); spread of the "
            f"off windows {max(oo['off_ms']) - min(oo['off_ms']):.3f} ms, of the on windows {max(oo['on_ms']) - min(oo['on_ms']):.3f} ms; "
            f"outputs finite: {oo['finite']}, on differs from off: {oo['outputs_differ']}")
        prof = os.path.join(out, "freeu_prof")
        run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--", py, me, "--worker", "trace", "--frames",
             str(args.frames), "--size", str(args.size), "--steps", "10"], ROOT, 900, log)
        import csv
        f = glob.glob(prof + "/**/*kernel_stats.csv", recursive=True)[0]
        rows = list(csv.DictReader(open(f)))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        say()
        say("rocprofv3 --kernel-trace --stats of the FreeU-on step (a run of its own: 1 eager step + capture + 10 replays):")
        for r in rows:
            if "freeu" in r["Name"]:
                say(f"  {r['Name'][:90]}: {r['Calls']} launches, {float(r['AverageNs']) / 1e3:.2f} us average "
                    f"(min {float(r['MinNs']) / 1e3:.2f}, max {float(r['MaxNs']) / 1e3:.2f}), {float(r['TotalDurationNs']) / 1e6:.3f} ms = "
                    f"{float(r['TotalDurationNs']) / tot * 100:.3f} % of all kernel time; six per step = "
                    f"{6 * float(r['AverageNs']) / 1e6:.4f} ms")
        kt = glob.glob(prof + "/**/*kernel_trace.csv", recursive=True)
        if kt:
            per = {}
            for r in csv.DictReader(open(kt[0])):
                if "freeu" in r["Kernel_Name"]:
                    key = (r["Grid_Size_X"] if "Grid_Size_X" in r else r.get("Grid_Size", "?"))
                    per.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            for key, v in sorted(per.items(), key=lambda kv: int(kv[0]) if kv[0].isdigit() else 0):
                say(f"    grid {key:>8s} threads: {len(v):3d} launches, median {statistics.median(v):6.2f} us")
    with open(os.path.join(out, "freeu_ab.txt"), "w") as fo:
        fo.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["launches", "onoff", "trace"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit (measurement (a)); without it only (b) runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "freeu_probe"))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=2)
    args = ap.parse_args()
    if args.worker:
        return {"launches": worker_launches, "onoff": worker_onoff, "trace": worker_trace}[args.worker](args)
    try:
        driver(args)
    except StepFailed as e:
        print(f"freeu_probe: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
