#!/usr/bin/env python
"""Headline benchmark: denoising steps/sec @ 16 f x 512 x 512, SD-1.5 + motion-adapter + I2V-Adapter, fp16.

  python bench.py --gpus N --steps K --warmup W            BASELINE configs[1] (default), one sample per GPU
  python bench.py --ip                                      configs[2]: + IP-Adapter image-prompt branch
  python bench.py --pairs 64 [--batch B]                    configs[3]: 64 (image, prompt) pairs sharded over the ranks,
                                                            B samples per graph replay, K steps per pair
  python bench.py --frames 32 --size 768                    configs[4]: 32 f x 768 x 768
  N > 1: either `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py
  --gpus N ...` (one rank per GPU, RANK / LOCAL_RANK / WORLD_SIZE from the environment), or plain `python bench.py --gpus N`,
  which starts that launcher as a child process before anything touches the GPU and relays rank 0's JSON line.

One *step* = one iteration of the reference loop pipe:666-697 for one (image, prompt) sample: frame-0 overwrite,
CFG duplicate (B = 2), UNet forward, CFG combine, DDIM update -- replayed as one hipGraph.  Inputs are synthetic
(SURVEY 8d): random-init weights of the SD-1.5 + AnimateDiff + I2V-Adapter architecture (seed 1234, torch's default
Linear / Conv law drawn on the GPU, adapter to_out ~ N(0, 0.02^2)), resident in HBM before the timed region.  Samples
are independent: they shard over ranks with no per-step collective; rank 0 draws the weights and broadcasts them once
as one flat buffer over RCCL.

A plain run sets up, warms up, times exactly K steps (one window) and prints ONE JSON line (rank 0) with the contract
fields (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`, ...); `--dump-outputs DIR` then also writes
the latents the last timed step produced as DIR/latents.npy (float32).  With `--full` the line carries in addition
  "roofline":     live HIP-event timing of the dominant kernel class over one instrumented eager step,
  "cpu_baseline": the CPU oracle (fp32, unfused torch graph = the reference's op graph) timed on the host cores on ONE
                  CFG UNet forward of this same workload (rank 0, N = 1 only), and `parity`: the HIP forward compared
                  with that oracle forward on the same weights and inputs,
  "stream_modes": the other residual-stream mode timed and checked beside the timed one,
and the timed window is repeated (`--windows`, 5 by default) with the median window reported.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic work per step, SURVEY.md Appendix B (2*MAC, B = 2 CFG, K/V of adapter & text counted once per clip)
FLOPS_PER_STEP = {(16, 512, False): 40.199e12, (16, 512, True): 40.205e12, (8, 256, False): 4.299e12,
                  (32, 768, False): 225.074e12}
MFMA_PEAK_TFLOPS = 2500.0   # dense fp16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBPS = 8000.0
# max-abs error of the HIP CFG forward against the fp32 CPU oracle above which the run is a FAILURE (exit code 3):
# tests/test_full_width_gpu.py FWD_ABS_TOL
PARITY_ABS_TOL = 4.0e-3
# ... and its RMS error: the maximum over 524 288 outputs is an extreme-value statistic that wanders +- 15 % between equivalent
# rounding patterns, the RMS is stable to 1 % (3.6 - 3.7e-4 on the config-2 forward since round 3) -- the gate that catches a real
# numerical regression
PARITY_RMS_TOL = 4.5e-4
# --dump-outputs writes at most this many bytes in all (a fixed, seeded sample of an output above it)
DUMP_MAX_BYTES = 64 << 20

SD15 = dict(sample_size=64, in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280),
            layers_per_block=2, cross_attention_dim=768, num_attention_heads=8, norm_num_groups=32,
            motion_num_attention_heads=8, motion_max_seq_length=32)


def build_hip_model(dev, seed=None):
    """SD-1.5-width model materialised on the GPU in fp16; `seed` draws the synthetic weights there."""
    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    with torch.device("meta"):
        m = pkg.UNetMotionCrossFrameAttnModel(**SD15)
    m = m.to_empty(device=dev).half()
    if seed is not None:
        init_random_weights_(m, seed=seed)
    return m.eval()


def synthetic_ip_state_dict(model, seed=7, clip_dim=1024):
    """ip-adapter_sd15.bin layout with synthetic values; key ids 1, 3, ... in attn_processors order."""
    g = torch.Generator().manual_seed(seed)
    cross = model.config["cross_attention_dim"]
    r = lambda *shape, s: torch.randn(*shape, generator=g) * s
    sd = {"image_proj": {"proj.weight": r(4 * cross, clip_dim, s=clip_dim ** -0.5), "proj.bias": r(4 * cross, s=0.1),
                         "norm.weight": 1 + r(cross, s=0.1), "norm.bias": r(cross, s=0.1)}, "ip_adapter": {}}
    mods = dict(model.named_modules())
    names = [n for n in model.attn_processor_names() if n.endswith("attn2.processor") and "motion_modules" not in n]
    for i, n in enumerate(names):
        a = mods[n[: -len(".processor")]]
        sd["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"] = r(a.inner_dim, cross, s=cross ** -0.5)
        sd["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"] = r(a.inner_dim, cross, s=cross ** -0.5)
    return sd


def sample_inputs(index, frames, h_lat, ip):
    """synthetic (condition latents, prompt embeds, negative embeds, initial latents[, image embeds]) of pair `index`."""
    s = 1000 * index
    rn = lambda seed, *shape: torch.randn(*shape, generator=torch.Generator().manual_seed(s + seed))
    d = dict(cond=rn(1, 1, 4, h_lat, h_lat), pe=rn(2, 1, 77, 768), ne=rn(3, 1, 77, 768),
             lat=rn(5, 1, frames, 4, h_lat, h_lat))
    if ip:
        d["ie"] = rn(4, 1, 1024)
    return d


def host_threads(cap=32):
    """threads for the CPU oracle: the cores this process may run on, no more than OMP_NUM_THREADS when that is set
    (os.cpu_count() counts the whole host, and a pool sized by it oversubscribes a CPU quota), at most `cap`."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:
        n = min(n, int(omp))
    return max(1, min(cap, n))


def dump_outputs(out_dir, arrays, seed=0):
    """`--dump-outputs DIR`: each array as DIR/<name>.npy in float32.  Above DUMP_MAX_BYTES in all, every array is
    replaced by the same fixed, seeded sample of its flattened elements (same shape and seed -> same positions)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.numel() * 4 for a in arrays.values())
    for name, a in arrays.items():
        a = a.detach().float().cpu()
        if total > DUMP_MAX_BYTES:
            n = max(1, a.numel() * DUMP_MAX_BYTES // total)
            idx = torch.randperm(a.numel(), generator=torch.Generator().manual_seed(seed))[:n].sort().values
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a.numpy())


def cpu_baseline_and_parity(model, ip_sd, frames, h_lat, dev, n_forwards=3):
    """`n_forwards` CFG UNet forwards (B = 2) of this workload through the CPU oracle on the host cores, with the HIP
    model's weights; the MEDIAN time is the baseline, and the forward is compared with the HIP forward of the
    same inputs."""
    from oracle import blocks as oblocks
    from oracle.unet_motion_cross_frame_attn import UNetMotionCrossFrameAttnModel as OracleUNet
    import torch.nn.functional as F
    with torch.device("meta"):
        ou = OracleUNet(**SD15)
    ou = ou.to_empty(device="cpu").float()
    ou.load_state_dict({k: v.detach().float().cpu() for k, v in model.state_dict().items()
                        if "_ip." not in k and not k.startswith("encoder_hid_proj")})
    if ip_sd is not None:
        ou._load_ip_adapter_weights({a: {k: v.half().float() for k, v in d.items()} for a, d in ip_sd.items()})
    ou.eval()
    # the reference's attention op is F.scaled_dot_product_attention (AttnProcessor2_0); the oracle's explicit-softmax
    # form would materialise 2 x 17 GB of scores at the 64 x 64 level
    orig = oblocks.Attention._sdpa
    oblocks.Attention._sdpa = lambda self, q, k, v: F.scaled_dot_product_attention(q, k, v, scale=self.scale)
    g = torch.Generator().manual_seed(11)
    # the batch the timed step runs: the SAME latents twice (pipe:672 `torch.cat([latents] * 2)`) against the negative and
    # the positive prompt; the HIP forward takes the same route as the timed step (prefix shared between the halves or not)
    lat = torch.randn(1, frames, 4, h_lat, h_lat, generator=g).half().float()
    x = torch.cat([lat, lat])
    ctx = torch.randn(2, 77, 768, generator=g).half().float()
    added = None
    added_d = None
    if ip_sd is not None:
        ie = torch.randn(2, 1024, generator=g).half().float()
        added, added_d = {"image_embeds": ie}, {"image_embeds": ie.to(dev)}
    t = torch.tensor([481, 481])
    cores = host_threads()
    torch.set_num_threads(cores)
    try:
        with torch.no_grad():
            times = []
            for _ in range(max(1, n_forwards)):
                t0 = time.time()
                ref = ou(x, t, True, ctx, added_cond_kwargs=added).sample
                times.append(time.time() - t0)
            dt = sorted(times)[len(times) // 2]
            from i2v_adapter_unofficial_amd import blocks as hblocks, pipeline_i2v_adapter as pl
            fwd = lambda: model(x.to(dev), t.to(dev), True, ctx.to(dev), added_cond_kwargs=added_d,
                                cross_attention_kwargs={"cfg_shared_prefix": pl.CFG_SHARED}).sample.float().cpu()
            got = fwd()
            # the same forward in the OTHER residual-stream mode (blocks.set_precise_stream), against the same oracle forward
            prev = hblocks.set_precise_stream(not hblocks.precise_stream())
            try:
                got_other = fwd()
            finally:
                hblocks.set_precise_stream(prev)
    finally:
        oblocks.Attention._sdpa = orig
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    base = {"value": 1.0 / dt, "unit": "denoising steps/sec", "cores": cores, "kind": "port",
            "sample": (f"median of {len(times)} fp32 CFG UNet forwards (B = 2) of the CPU oracle at {frames}f x "
                       f"{h_lat * 8}x{h_lat * 8}: {dt:.1f} s ({', '.join(f'{v:.1f}' for v in times)}) on {cores} threads of a "
                       f"{os.cpu_count()}-thread host (torch {torch.__version__}); a step is that forward plus "
                       "negligible elementwise work")}
    # the maximum over 524 288 outputs is an extreme-value statistic: equivalent rounding patterns (e.g. another GELU form)
    # move it by +- 15 % (1.9 .. 2.3e-3) while the RMS stays put -- both are reported
    parity = {"max_abs_err": err, "max_abs_ref": scale, "rel": err / max(scale, 1e-30),
              "rms_err": (got - ref).pow(2).mean().sqrt().item(), "rms_ref": ref.pow(2).mean().sqrt().item(),
              "what": ("HIP UNet forward of the CFG batch [latents ; latents] x [negative ; positive prompt], routed as the "
                       "timed step routes it, vs the fp32 CPU oracle forward timed above (same weights, same inputs)")}
    mode = lambda on: "precise" if on else "default"
    d_o = got_other - ref
    parity["stream_mode"] = mode(hblocks.precise_stream())
    parity["other_stream_mode"] = {"stream_mode": mode(not hblocks.precise_stream()), "max_abs_err": d_o.abs().max().item(),
                                   "rms_err": d_o.pow(2).mean().sqrt().item()}
    return base, parity


def write_shape_table(prof, path, what):
    """where the step's time sits per (kernel wrapper, problem shape, fused extras); algorithmic TFLOP/s and GB/s."""
    rows = sorted(prof.by_shape().items(), key=lambda kv: -kv[1]["ms"])
    total = sum(d["ms"] for _, d in rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(f"# one instrumented eager step ({what}): {total:.2f} ms in {sum(d['calls'] for _, d in rows)} launches\n")
        f.write(f"{'launch':58s} {'n':>4s} {'ms':>8s} {'%':>6s} {'us/launch':>10s} {'TFLOP/s':>8s} {'GB/s':>7s}\n")
        for name, d in rows:
            f.write(f"{name:58s} {d['calls']:4d} {d['ms']:8.3f} {100 * d['ms'] / total:6.2f} "
                    f"{1e3 * d['ms'] / d['calls']:10.1f} {d['tflops']:8.1f} {d['gbps']:7.0f}\n")


def plan_groups(n_pairs_total, rank, world, batch):
    """this rank's (image, prompt) pair indices, `batch` per graph replay: static block partition of the pairs over the
    ranks (sharding.shard_range), no per-step collective."""
    from i2v_adapter_unofficial_amd.sharding import shard_range
    if n_pairs_total % (world * batch) != 0:
        raise SystemExit(f"--pairs {n_pairs_total} must be a multiple of ranks x batch = {world * batch}")
    lo, hi = shard_range(n_pairs_total, rank, world)
    idx = list(range(lo, hi))
    return [idx[i: i + batch] for i in range(0, len(idx), batch)]


def latent_parity(args, model, dev):
    """`--latent-parity N`: N DDIM steps of this workload (config 2 by default) through the HIP pipeline (hipGraph replay, the
    route the timed step runs) and through the CPU oracle's pipeline (pipe:629-700 restated, fp32) on the same weights, seeds
    and condition latents; prints ONE JSON line with the max-abs / rms difference of the final LATENTS -- the quantity
    north_star's tolerance is worded on.  ~1 minute of host time per step at 16 f x 512^2: kept out of the default run."""
    import torch.nn.functional as F
    import i2v_adapter_unofficial_amd as pkg
    from oracle import blocks as oblocks
    from oracle.pipeline_i2v_adapter import I2VAdapterPipeline as OraclePipeline
    from oracle.unet_motion_cross_frame_attn import UNetMotionCrossFrameAttnModel as OracleUNet
    n_steps, frames, h_lat = args.latent_parity, args.frames, args.size // 8
    with torch.device("meta"):
        ou = OracleUNet(**SD15)
    ou = ou.to_empty(device="cpu").float()
    ou.load_state_dict({k: v.detach().float().cpu() for k, v in model.state_dict().items()})
    ou.eval()
    oblocks.Attention._sdpa = lambda self, q, k, v: F.scaled_dot_product_attention(q, k, v, scale=self.scale)
    cores = host_threads()
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(21)
    h16 = lambda t: t.half().float()
    pe, ne = h16(torch.randn(1, 77, 768, generator=g)), h16(torch.randn(1, 77, 768, generator=g))
    cond = torch.randn(1, 4, h_lat, h_lat, generator=g)
    total = 25
    kw = dict(num_frames=frames, num_inference_steps=total, guidance_scale=7.5, blur_sigma=1.0,
              frame_similarity_sample_ratio=(n_steps + 0.5) / total)          # get_timesteps: the LAST n_steps of the schedule
    gens = lambda: dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                        prior_noise_generator=torch.Generator().manual_seed(7))
    pipe = pkg.I2VAdapterPipeline(unet=model)
    with torch.no_grad():
        got = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, **kw, **gens()).frames
        got = got.float().cpu()
        t0 = time.time()
        ref = OraclePipeline(ou)(pe, ne, cond, **kw, **gens()).frames
        dt = time.time() - t0
    d = got - ref
    out = {"what": f"final latents after {n_steps} DDIM steps (CFG 7.5), {frames}f x {args.size}x{args.size}: HIP pipeline "
                   "(hipGraph) vs the fp32 CPU oracle pipeline, same weights / seeds / condition latents",
           "steps": n_steps, "max_abs_err": d.abs().max().item(), "rms_err": d.pow(2).mean().sqrt().item(),
           "max_ref": ref.abs().max().item(), "rms_ref": ref.pow(2).mean().sqrt().item(),
           "frame0_equals_condition": bool(torch.equal(got[:, 0], cond)), "oracle_seconds": dt, "oracle_threads": cores}
    print(json.dumps(out), flush=True)
    return out


def _profile_files(kind):
    """profiles/r<N>_<kind>.json, newest round first."""
    import re
    out = []
    for name in os.listdir(os.path.join(ROOT, "profiles")):
        m = re.fullmatch(rf"r(\d+)_{kind}\.json", name)
        if m:
            out.append((int(m.group(1)), name))
    return [n for _, n in sorted(out, reverse=True)]


def dominant_kernel(by_shape):
    """The dominant KERNEL of the step (a kernel, not a class of them) from the newest committed rocprofv3 --kernel-trace --stats
    summary that was taken on exactly this library's kernel sources (profiles/r*_kernel_stats.txt, `# library_source_stamp`): name,
    calls, average duration, and -- for the flash-attention kernels, whose launches the instrumented step can attribute by head
    width -- algorithmic FLOP per launch (average over the launches of that head width in one step) and the fraction of the dense
    fp16 MFMA peak.  Returns a dict (with `reason` instead when no summary matches)."""
    import re
    stamp, seen = source_stamp(), []
    names = sorted((n for n in os.listdir(os.path.join(ROOT, "profiles")) if re.fullmatch(r"r(\d+)_kernel_stats\.txt", n)),
                   key=lambda n: -int(re.match(r"r(\d+)", n).group(1)))
    for name in names:
        lines = open(os.path.join(ROOT, "profiles", name)).read().splitlines()
        st = next((ln.split()[2] for ln in lines if ln.startswith("# library_source_stamp")), None)
        seen.append(f"{name}: {st}")
        if st != stamp:
            continue
        rows = []
        for ln in lines:
            m = re.match(r"(.+?)\s+(\d+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s*$", ln)
            if m and not ln.startswith("#") and "spin_kernel" not in m.group(1):
                rows.append((m.group(1).strip(), int(m.group(2)), float(m.group(3)), float(m.group(4)), float(m.group(5))))
        if not rows:
            continue
        kname, calls, total_ms, avg_us, pct = max(rows, key=lambda r: r[2])
        out = {"name": kname, "calls": calls, "avg_us": avg_us, "pct_of_kernel_time": pct,
               "source": f"profiles/{name} (rocprofv3 --kernel-trace --stats, same kernel sources)"}
        m = re.match(r".*attn_kernel<\s*\d+,\s*(\d+),", kname)
        if m and by_shape:
            dpad = int(m.group(1))           # head_dim padded to a multiple of 16
            sel = [d for n, d in by_shape.items() if n.startswith("attention ") and
                   (int(re.search(r" d(\d+)", n).group(1)) + 15) // 16 * 16 == dpad]
            n_calls = sum(d["calls"] for d in sel)
            if n_calls:
                fl = sum(d["flops"] for d in sel) / n_calls
                live_us = sum(d["ms"] for d in sel) * 1e3 / n_calls       # HIP events of THIS run's instrumented eager step
                out.update(flops_per_launch=fl, achieved_tflops=fl / (avg_us * 1e-6) / 1e12,
                           frac=fl / (avg_us * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS,
                           live_avg_us=live_us, live_launches=n_calls, live_achieved_tflops=fl / (live_us * 1e-6) / 1e12,
                           live_frac=fl / (live_us * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS,
                           flops_note="algorithmic 4 Lq Lk C per image, averaged over this head width's launches of one step; `avg_us` is "
                                      "rocprofv3's average over the committed profile's graph replays, `live_avg_us` HIP events around the "
                                      "same launches of this run's eager step (a few per cent slower: cold caches between eager launches)")
        return out
    return {"reason": f"no profiles/r*_kernel_stats.txt was taken on this library's kernel sources ({stamp}); found {seen}"}


def run_windows(groups, steps, n_windows, n_tab, load_group, run_step, reset_step_index, sync, world, device):
    """The timed region, `n_windows` times: exactly `steps` steps for every group of this rank between barrier + sync on
    both sides, elapsed = MAX over ranks (an all-reduce of one double OUTSIDE the timed bracket).  Returns the list of
    window times (identical on every rank)."""
    import torch.distributed as dist
    windows = []
    for _ in range(max(1, n_windows)):
        load_group(groups[0])
        sync()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        for gi, grp in enumerate(groups):
            if gi:
                load_group(grp)
            for done in range(steps):
                if done % n_tab == 0 and done:
                    reset_step_index()      # wrap the timestep table (the kernels also clamp the index)
                run_step()
        sync()
        if world > 1:
            dist.barrier()
        w_elapsed = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([w_elapsed], dtype=torch.float64, device=device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            w_elapsed = float(tt.item())
        windows.append(w_elapsed)
    return windows


def dry_run(args, rank, world):
    """the N-rank plumbing of main() on CPU (gloo): everything but the kernels and RCCL."""
    import torch.distributed as dist
    from i2v_adapter_unofficial_amd.i2v_adapter import I2VAdapterModule
    from i2v_adapter_unofficial_amd.sharding import broadcast_model_weights
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(1234 + rank)                        # different weights per rank until the broadcast
    model = I2VAdapterModule(2, (32, 64, 64), 4)
    nbytes = broadcast_model_weights(model, src=0) if world > 1 else 0
    checksum = float(sum(p.detach().double().sum() for p in model.parameters()))
    B = args.batch
    n_pairs_total = args.pairs if args.pairs > 0 else world * B
    groups = plan_groups(n_pairs_total, rank, world, B)
    done = {}

    def run_step():
        for i in current["grp"]:
            done[i] = done.get(i, 0) + 1
    current = {"grp": None}
    windows = run_windows(groups, args.steps, 1, 25, lambda grp: current.update(grp=grp), run_step, lambda: None,
                          lambda: None, world, torch.device("cpu"))
    if world > 1:
        sums = [None] * world
        dist.all_gather_object(sums, (checksum, sorted(done.items())))
    else:
        sums = [(checksum, sorted(done.items()))]
    if rank == 0:
        covered = sorted(i for _, d in sums for i, _ in d)
        print(json.dumps({"dry_run": True, "n_gpus": world, "steps": args.steps, "pairs": n_pairs_total, "batch": B,
                          "ranks_in_group": dist.get_world_size() if world > 1 else 1, "broadcast_bytes": nbytes,
                          "weights_equal_on_all_ranks": len({c for c, _ in sums}) == 1,
                          "pairs_covered_once": covered == list(range(n_pairs_total)),
                          "steps_per_pair": sorted({n for _, d in sums for _, n in d}),
                          "window_s": windows[0]}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def launch_ranks(n_gpus):
    """`python bench.py --gpus N` without a launcher: start `python -m torch.distributed.run --nproc-per-node N bench.py
    ...` as a CHILD process (this process has not touched the GPU and never execs), relay its output -- rank 0's JSON line
    on stdout -- and return its exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:                       # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def train_bench(args, model, ip, rank, world, dev):
    """`--train`: the reference's training step (src/train_image_to_video.py:839-884) for the adapter parameters, one clip
    per rank per step (data parallel: the gradient bucket is summed with ONE RCCL all-reduce per step), W + K steps timed
    as the inference bench times its steps.  Prints one JSON line with the contract's fields; the metric is NOT BASELINE's."""
    import torch.distributed as dist
    from i2v_adapter_unofficial_amd.training import AdapterOptimizer, UNetAdapterTrainer
    F, lat = args.frames, args.size // 8
    g = torch.Generator().manual_seed(100 + rank)                   # every rank trains on its own clip
    x = torch.randn(1, F, 4, lat, lat, generator=g).half().to(dev)
    noise = torch.randn(1, F, 4, lat, lat, generator=g).to(dev)
    ctx = torch.randn(1, 77, 768, generator=g).half().to(dev)
    added = {"image_embeds": torch.randn(1, 1024, generator=g).half().to(dev)} if ip else None
    t = torch.tensor([481], device=dev)
    umm = bool(args.update_motion_modules)
    trainer, opt = UNetAdapterTrainer(model, update_motion_modules=umm), AdapterOptimizer(model, lr=1e-5, update_motion_modules=umm)

    def step():
        trainer.forward(x, t, ctx, added_cond_kwargs=added)
        loss, grads = trainer.backward(noise, loss_scale=2.0 ** 12)
        opt.step(grads)
        return loss
    for _ in range(max(1, args.warmup)):
        loss0 = step()
    sync = torch.cuda.synchronize
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    sync()
    el = torch.tensor([time.perf_counter() - t0], device=dev)
    if world > 1:
        dist.barrier()
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = el.item()
    if rank == 0:
        n_train = opt.master.numel()
        print(json.dumps({
            "metric": f"adapter training steps/sec @ {F}fx{args.size}x{args.size} SD1.5+I2V-Adapter (one clip per GPU per step)",
            "value": world * args.steps / elapsed, "unit": "clip-steps/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "ranks_in_rccl_group": (dist.get_world_size() if world > 1 else 1), "vs_baseline": None, "dtype": "f16",
            "data": "synthetic",
            "config": {"workload": ("adapter training step of src/train_image_to_video.py:839-884 (forward, MSE without the "
                                    "first frame, backward through the frozen UNet, all-reduce of the adapter gradients, "
                                    f"clip + AdamW), SD-1.5 width, {F}f x {args.size}x{args.size}, IP {'on' if ip else 'off'}, one clip "
                                    "per rank; NOT the BASELINE metric"),
                       "update_motion_modules": umm,
                       "trainable_parameters": n_train, "allreduce_bytes_per_step": 4 * n_train if world > 1 else 0,
                       "loss_first": float(loss0), "loss_last": float(loss), "finite": bool(torch.isfinite(loss).item())},
            "roofline": None, "cpu_baseline": None}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def source_stamp():
    """hash of the kernel sources the running library was built from (csrc/*.hip, *.h, include/i2v_hip.h): recorded next
    to PMC traffic figures so that a figure measured on another binary is never attached to this one"""
    import hashlib
    csrc = os.path.join(ROOT, "i2v-adapter-unofficial_amd", "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    files.append(os.path.join(ROOT, "include", "i2v_hip.h"))
    hsh = hashlib.sha256()
    for f in files:
        hsh.update(os.path.basename(f).encode())
        hsh.update(open(f, "rb").read())
    return hsh.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ip", action="store_true", help="IP-Adapter image-prompt branch on (BASELINE configs[2])")
    ap.add_argument("--pairs", type=int, default=0, help="total (image, prompt) pairs sharded over the ranks (configs[3])")
    ap.add_argument("--batch", type=int, default=1, help="samples per graph replay")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--shapes", default="", help="write the per-shape time table of the instrumented step here")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--latent-parity", type=int, default=0,
                    help="N > 0: compare the final latents of N DDIM steps with the CPU oracle's pipeline and exit")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: repeated timed windows, the instrumented eager step "
                         "(roofline, kernel classes, --shapes), the other residual-stream mode, the CPU-oracle baseline "
                         "and the parity gate (exit code 3 on failure)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (the latents) as DIR/<name>.npy")
    ap.add_argument("--windows", type=int, default=None,
                    help="the K-step timed window is repeated this many times (each bracketed by barrier + synchronize); "
                         "the line reports the MEDIAN window, and min / max as `window_ms_per_step` (default 1, 5 with --full)")
    ap.add_argument("--cpu-forwards", type=int, default=3, help="oracle forwards timed for cpu_baseline (median)")
    ap.add_argument("--train", action="store_true",
                    help="time the ADAPTER TRAINING STEP instead (SURVEY 8 f4: forward + backward + one all-reduce of the "
                         "adapter gradients + clip + AdamW; one clip per rank per step) -- not the BASELINE metric")
    ap.add_argument("--update-motion-modules", action="store_true",
                    help="with --train: the 21 motion modules train too (train_image_to_video.py:452, 669)")
    ap.add_argument("--parity-only", action="store_true",
                    help="no timing: ONE CFG UNet forward of this workload (--frames / --size / --ip) through the HIP model and "
                         "through the CPU oracle on the same weights and inputs, one JSON line with the errors (builder-run: "
                         "minutes of host time at 32 f x 768^2; profiles/r5_parity_configs.jsonl)")
    ap.add_argument("--precise", action="store_true",
                    help="time the step with the PRECISE residual stream (fp16 hi + lo pairs between the modules, DESIGN 2.1; "
                         "blocks.set_precise_stream); without it the default single-GPU run times the default stream, and with "
                         "--full adds the precise mode's ms_per_step and parity beside it (`stream_modes`)")
    ap.add_argument("--dry-run", action="store_true",
                    help="rehearse the multi-rank plumbing on a box WITHOUT GPUs: launcher, rendezvous, gloo group, flat "
                         "weight broadcast, pair sharding, timed loop with a stub step, MAX all-reduce, JSON line "
                         "(marked \"dry_run\": true; not a measurement)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.windows is None:
        args.windows = 5 if args.full else 1
    if args.shapes and not args.full:
        ap.error("--shapes needs --full (it comes from the instrumented eager step)")
    if args.dump_outputs and (args.train or args.latent_parity or args.parity_only or args.dry_run):
        ap.error("--dump-outputs applies to the timed inference step only")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus))       # bare `python bench.py --gpus N`: one child launcher, N ranks
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with python -m torch.distributed.run "
                         f"--nproc-per-node {args.gpus} bench.py --gpus {args.gpus} (or plain `python bench.py --gpus N`)")
    if args.dry_run:
        return dry_run(args, rank, world)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    import i2v_adapter_unofficial_amd as pkg
    from i2v_adapter_unofficial_amd import blocks as hblocks
    from i2v_adapter_unofficial_amd.profiling import KernelProfile
    if args.precise:
        hblocks.set_precise_stream(True)
    from i2v_adapter_unofficial_amd.sharding import broadcast_model_weights

    # ---- weights: rank 0 draws them on its GPU, one flat RCCL broadcast to the other ranks
    t_start = time.time()
    model = build_hip_model(dev, seed=1234 if rank == 0 else None)
    ip = args.ip or args.pairs > 0                     # configs[3] = 64 pairs "each as configs[2]" 
    ip_sd = None
    if ip:
        ip_sd = synthetic_ip_state_dict(model)
        model._load_ip_adapter_weights(ip_sd)          # same seed on every rank; covered by the broadcast anyway
    if world > 1:
        nbytes = broadcast_model_weights(model, src=0)
        if rank == 0:
            print(f"# broadcast {nbytes / 1e9:.2f} GB of weights over RCCL", file=sys.stderr)
    t_built = time.time()
    if args.train:
        return train_bench(args, model, ip, rank, world, dev)
    if args.latent_parity > 0:
        latent_parity(args, model, dev)
        return 0
    if args.parity_only:
        import threading
        done = threading.Event()

        def heartbeat():          # (the box kills a command that is silent for minutes)
            t0 = time.time()
            while not done.wait(45):
                print(f"# oracle forward running: {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
        threading.Thread(target=heartbeat, daemon=True).start()
        base, parity = cpu_baseline_and_parity(model, ip_sd, args.frames, args.size // 8, dev, n_forwards=1)
        done.set()
        parity["tolerance"], parity["rms_tolerance"] = PARITY_ABS_TOL, PARITY_RMS_TOL
        parity["parity_ok"] = bool(parity["max_abs_err"] <= PARITY_ABS_TOL and parity["rms_err"] <= PARITY_RMS_TOL)
        print(json.dumps({"parity_only": True, "workload": f"{args.frames}f x {args.size}x{args.size}, CFG batch (B = 2), IP "
                          f"{'on' if ip else 'off'}, SD-1.5 width", "parity": parity, "cpu_oracle": base,
                          "library_source_stamp": source_stamp()}), flush=True)
        return 0 if parity["parity_ok"] else 3

    # ---- this rank's samples (static block partition, no per-step collective)
    F, h_lat, B = args.frames, args.size // 8, args.batch
    n_pairs_total = args.pairs if args.pairs > 0 else world * B
    groups = [[sample_inputs(i, F, h_lat, ip) for i in grp] for grp in plan_groups(n_pairs_total, rank, world, B)]

    pipe = pkg.I2VAdapterPipeline(unet=model)
    sch = pipe.scheduler
    sch.set_timesteps(25)
    timesteps = sch.timesteps
    n_tab = len(timesteps)
    st = dict(latents=torch.empty(B, F, 4, h_lat, h_lat, device=dev), cond=torch.empty(B, 4, h_lat, h_lat, device=dev),
              copies=2, num_frames=F, guidance=7.5, t_table=timesteps.float().to(dev),
              coef=sch.step_coefficients(timesteps).to(dev), step_idx=torch.zeros(1, dtype=torch.int32, device=dev),
              ctx_text=torch.empty(2 * B, 77, 768, dtype=torch.float16, device=dev),
              ctx_ip=torch.empty(2 * B, 4, 768, dtype=torch.float16, device=dev) if ip else None)

    def load_group(grp):
        """this group's inputs into the static buffers the captured graph reads (async copies on the stream)."""
        st["latents"].copy_(torch.cat([s["lat"] for s in grp]), non_blocking=True)
        st["cond"].copy_(torch.cat([s["cond"] for s in grp]), non_blocking=True)
        st["ctx_text"].copy_(torch.cat([s["ne"] for s in grp] + [s["pe"] for s in grp]).half(), non_blocking=True)
        if ip:
            ie = torch.cat([torch.zeros_like(s["ie"]) for s in grp] + [s["ie"] for s in grp])      # pipe:343, 621-622
            st["ctx_ip"].copy_(model._project_image_embeds({"image_embeds": ie.to(dev)}))
        # per-sample work outside the step: K / V^T of the context for the 16 cross-attention layers, written into the
        # buffers the captured graph reads
        st["ctx_proj"] = model.project_context(st["ctx_text"], st["ctx_ip"], out=st.get("ctx_proj"))
        # ... and the time-embedding chain of every timestep of the schedule (a function of t alone): the step selects its row
        st["temb_table"] = model.project_time_table(st["t_table"], out=st.get("temb_table"))
        st["step_idx"].zero_()

    with torch.no_grad():
        load_group(groups[0])
        pipe._step(st)                      # eager warm-up: packs the kernel-layout weights, sizes the allocator
        load_group(groups[0])
        torch.cuda.synchronize()
        graph = None
        if not args.no_graph:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                pipe._step(st)
            load_group(groups[0])

        def run_step():
            if graph is not None:
                graph.replay()
            else:
                pipe._step(st)

        for i in range(args.warmup):
            if i % n_tab == 0 and i:
                st["step_idx"].zero_()
            run_step()
        # ---- timed region: exactly K steps per group between barrier + synchronize on both sides.  The window is
        #      repeated (a 20-step window is ~1 s of GPU time: box noise is +-5 %, and the driver's utilisation sampler
        #      cannot see it); every window is timed the same way, MAX over ranks, and the MEDIAN window is reported.
        windows = run_windows(groups, args.steps, args.windows, n_tab, load_group, run_step,
                              lambda: st["step_idx"].zero_(), torch.cuda.synchronize, world, dev)
        elapsed = sorted(windows)[len(windows) // 2]
        finite = bool(torch.isfinite(st["latents"]).all().item())
        # ---- what the last timed step computed, before anything below advances the same buffers
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, {"latents": st["latents"]})

        # ---- live per-kernel-class roofline (rank 0, --full): one instrumented eager step behind a GPU backlog so that
        #      the event pairs bracket back-to-back kernels, not host launch gaps
        roof, classes = None, None
        if rank == 0 and args.full:
            load_group(groups[0])
            torch.cuda._sleep(int(2.0e8))   # ~0.1 s device-side spin (not one of our kernels): the host runs ahead
            # (single-stream for this one step: the event pairs must bracket one kernel each.  The timed replays above are
            #  single-stream too by default -- the two-stream form of the small levels' chains, streams.py, is an
            #  off-by-default experiment (I2V_STREAMS=1); `disabled()` only matters when it is switched on)
            from i2v_adapter_unofficial_amd import streams
            with KernelProfile() as prof, streams.disabled():
                pipe._step(st)
            classes = prof.summary()
            if args.shapes:
                write_shape_table(prof, args.shapes, f"frames {F}, {args.size}x{args.size}, ip {ip}, batch {B}")
            dom = max(classes, key=lambda c: classes[c]["ms"])
            d = classes[dom]
            if d["flops"] > 0:
                roof = {"bound": "mfma", "kernel": dom, "achieved": d["tflops"], "peak": MFMA_PEAK_TFLOPS,
                        "unit": "TFLOP/s", "frac": d["tflops"] / MFMA_PEAK_TFLOPS, "traffic": None,
                        "launches": d["calls"], "avg_launch_us": d["ms"] * 1e3 / d["calls"],
                        "flops_per_launch": d["flops"] / d["calls"]}
            else:
                roof = {"bound": "hbm", "kernel": dom, "achieved": d["gbps"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": d["gbps"] / HBM_PEAK_GBPS, "traffic": None, "launches": d["calls"],
                        "avg_launch_us": d["ms"] * 1e3 / d["calls"], "bytes_per_launch": d["bytes"] / d["calls"]}
            roof["class_note"] = "`kernel` is a CLASS of launches timed live; the single dominant kernel is `dominant_kernel`"
            roof["dominant_kernel"] = dominant_kernel(prof.by_shape())
            # HBM-side bytes per launch of that class: PMC counters cannot be read from inside the process, so this is
            # the committed result of the separate rocprofv3 --pmc passes over this same command
            # (tools/pmc_traffic.sh -> profiles/r2_traffic.json), valid for the default workload only
            # the NEWEST profiles/r*_traffic.json measured on exactly this library's kernel sources (a kernel edit
            # invalidates older files instead of silently dropping `traffic`: the reason is reported)
            if (F, args.size, ip, B) == (16, 512, False, 1):
                tfile, seen = None, []
                for name in _profile_files("traffic"):
                    with open(os.path.join(ROOT, "profiles", name)) as f:
                        tj = json.load(f)
                    seen.append(f"{name}: {tj.get('source_stamp')}")
                    if tj.get("source_stamp") == source_stamp() and dom in tj.get("classes", {}):
                        tfile = (name, tj)
                        break
                if tfile is not None:
                    roof["traffic"] = tfile[1]["classes"][dom]["bytes_per_launch"]
                    roof["traffic_source"] = (f"profiles/{tfile[0]} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this "
                                              "command, same kernel sources)")
                else:
                    roof["traffic_source"] = (f"no profiles/r*_traffic.json was measured on this library's kernel sources "
                                              f"({source_stamp()}); found {seen}: not attached")
            # fractions of the ceilings MEASURED on this chip (tools/ceilings.hip -> profiles/r*_ceilings.json, newest),
            # next to the vendor peaks the `frac` above uses
            for name in _profile_files("ceilings"):
                with open(os.path.join(ROOT, "profiles", name)) as f:
                    cj = json.load(f)
                pm = cj.get("mfma_f16_tflops") if roof["bound"] == "mfma" else cj.get("hbm_copy_gbps")
                if pm:
                    roof["peak_measured"] = pm
                    roof["frac_of_measured"] = roof["achieved"] / pm
                    roof["peak_measured_source"] = f"profiles/{name} (MFMA-saturating loop / stream copy, this pool)"
                    break

        # ---- the OTHER residual-stream mode, timed the same way over two windows (--full single-GPU run only): the line
        #      carries ms_per_step and parity of both modes
        other_mode = None
        if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not args.no_graph:
            prev = hblocks.set_precise_stream(not hblocks.precise_stream())
            try:
                load_group(groups[0])
                pipe._step(st)
                load_group(groups[0])
                torch.cuda.synchronize()
                graph2 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph2):
                    pipe._step(st)
                load_group(groups[0])
                for _ in range(args.warmup):
                    graph2.replay()
                w2 = run_windows(groups, args.steps, 2, n_tab, load_group, graph2.replay, lambda: st["step_idx"].zero_(),
                                 torch.cuda.synchronize, world, dev)
                other_mode = {"stream_mode": "precise" if hblocks.precise_stream() else "default",
                              "ms_per_step": min(w2) / (len(groups) * args.steps) * 1e3,
                              "finite": bool(torch.isfinite(st["latents"]).all().item())}
                graph2 = None
            finally:
                hblocks.set_precise_stream(prev)

    used_graph = graph is not None
    graph = None
    t_gpu_done = time.time()
    cpu_base, parity = None, None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu_base, parity = cpu_baseline_and_parity(model, ip_sd, F, h_lat, dev, n_forwards=args.cpu_forwards)
        parity["tolerance"], parity["rms_tolerance"] = PARITY_ABS_TOL, PARITY_RMS_TOL
        parity["parity_ok"] = bool(parity["max_abs_err"] <= PARITY_ABS_TOL and parity["rms_err"] <= PARITY_RMS_TOL)
        if not parity["parity_ok"]:
            print(f"# PARITY FAILURE: {parity}", file=sys.stderr)
    if rank == 0:
        print(f"# timings: build {t_built - t_start:.1f}s, gpu {t_gpu_done - t_built:.1f}s, cpu baseline "
              f"{time.time() - t_gpu_done:.1f}s", file=sys.stderr)

    if rank == 0:
        sample_steps = n_pairs_total * args.steps       # every sample of the job advances K steps
        ms = elapsed / (len(groups) * args.steps) * 1e3  # one graph replay (B samples' step on one GPU)
        value = sample_steps / elapsed
        step_flops = FLOPS_PER_STEP.get((F, args.size, ip))
        # FLOPs the step EXECUTES (sum over the instrumented step's launches): below the algorithmic count when the
        # prompt-independent prefix is computed once for both CFG halves -- rates are quoted on the executed count
        from i2v_adapter_unofficial_amd import pipeline_i2v_adapter as pl
        exec_flops = sum(c["flops"] for c in classes.values()) / B if (classes and not args.pairs) else None
        rate_flops = exec_flops if exec_flops else step_flops
        cfg_name = ("configs[3]: batch of pairs, data-parallel" if args.pairs else
                    "configs[4]" if (F, args.size) == (32, 768) else
                    "configs[0] shape" if (F, args.size) == (8, 256) else
                    "configs[2]" if ip and (F, args.size) == (16, 512) else
                    "configs[1]" if (F, args.size) == (16, 512) else "no BASELINE config")
        # both residual-stream modes side by side: ms_per_step (this line's `ms_per_step` is the timed mode's median window; the other
        # mode's is the faster of two windows) and the forward's error against the oracle
        this_mode = "precise" if hblocks.precise_stream() else "default"
        stream_modes = {this_mode: {"ms_per_step": ms, "timed": f"median of {len(windows)} windows"}}
        if parity is not None:
            stream_modes[this_mode].update(max_abs_err=parity["max_abs_err"], rms_err=parity["rms_err"])
        if other_mode is not None:
            om = {"ms_per_step": other_mode["ms_per_step"], "timed": "faster of 2 windows", "finite": other_mode["finite"]}
            if parity is not None:
                om.update(max_abs_err=parity["other_stream_mode"]["max_abs_err"], rms_err=parity["other_stream_mode"]["rms_err"])
            stream_modes[other_mode["stream_mode"]] = om
        out = {
            "metric": ("denoising steps/sec @ 16fx512x512 SD1.5+I2V-Adapter" if (F, args.size) == (16, 512) else
                       f"denoising steps/sec @ {F}fx{args.size}x{args.size} SD1.5+I2V-Adapter"), "value": value,
            "unit": "denoising steps/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms, "window_ms_per_step": {"n": len(windows), "median": ms,
                                                      "min": min(windows) / (len(groups) * args.steps) * 1e3,
                                                      "max": max(windows) / (len(groups) * args.steps) * 1e3},
            "higher_is_better": True, "scaling": "weak" if not args.pairs else "strong", "full": bool(args.full),
            "ranks_in_rccl_group": (dist.get_world_size() if world > 1 else 1),
            "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": f"SD-v1.5 + motion-adapter-v1-5-2 + I2V-Adapter topology, {F}f x {args.size}x{args.size}, "
                                   f"CFG 7.5 (B=2 per sample), DDIM 25-step table, fp16, IP {'on' if ip else 'off'}, "
                                   f"{n_pairs_total} sample(s) over {world} GPU(s), {B} per graph replay (BASELINE {cfg_name}); "
                                   "hoisted out of the timed step, computed once per sample as the product pipeline does "
                                   "(pipeline_i2v_adapter.py _run_steps): the context K / V^T of the 16 cross-attention layers "
                                   "and the time-embedding chain of every timestep of the schedule (the step copies its row)",
                       "hoisted_per_sample": ["context K / V^T projections of the 16 cross-attention layers (prompt + image tokens)",
                                              "time_proj -> time_embedding -> silu -> 22 time_emb_proj for all timesteps of the schedule"],
                       "samples_total": n_pairs_total, "samples_per_replay": B, "graph": used_graph, "finite": finite,
                       "unet_forwards_per_cfg_half_per_sec": 2 * value,
                       "cfg_shared_prefix": bool(pl.CFG_SHARED), "residual_stream": this_mode,
                       "step_tflops": None if step_flops is None else step_flops / 1e12,
                       "executed_tflops_per_step": None if exec_flops is None else exec_flops / 1e12,
                       "achieved_tflops_per_gpu": None if rate_flops is None else
                       rate_flops * sample_steps / elapsed / world / 1e12},
            "roofline": roof,
            "cpu_baseline": cpu_base,
            "parity": parity,
            "stream_modes": stream_modes,
            "kernel_classes": {k: {kk: (round(vv, 3) if isinstance(vv, float) else vv) for kk, vv in v.items()}
                               for k, v in (classes or {}).items()},
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()
    if parity is not None and not parity["parity_ok"]:
        raise SystemExit(3)          # a numerically broken build must not look like a benchmark record (rc != 0)


if __name__ == "__main__":
    main()
