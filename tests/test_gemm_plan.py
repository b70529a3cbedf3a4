"""The dispatch plan of the 8-wave GEMM / conv kernel (csrc/gemm_big.hip), seen through the four host queries that read it:
i2v_gemm_workspace_bytes, i2v_gemm_ln_supported, i2v_gemm_batch_supported, i2v_gemm_gn_partial_rows.  Each problem of a
deterministic sweep is asked twice, without a workspace and with the workspace the row names attached, and the answers are
compared with tests/golden/gemm_plan_answers.txt, recorded from the library as it was BEFORE the planner was gathered
into one function (`python tests/test_gemm_plan.py --record` with I2V_LIB_PATH naming that library rewrites the table).
The queries are pure host arithmetic (pointers are only tested for null and alignment): no GPU, no launch."""
import ctypes as C
import itertools
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_answers.txt")
SHAPES = os.path.join(ROOT, "profiles", "r6_step_shapes.txt")
BASE = 0x7F0000000000          # fake, well-aligned addresses: one 4 GiB window per operand
PTRS = ("a", "w", "c", "residual", "rowvec", "ln_wsum", "c_lo", "residual_lo", "workspace", "gn_partial", "a2", "bias")
EPI = {"none": 0, "gelu": 1, "geglu": 2}
STORE = {"rm": 0, "perm": 1, "vt": 2, "vt_t": 3}


def _ptr(name, skew=0):
    return BASE + (PTRS.index(name) << 32) + skew


def problem(lib, M, N, K, conv_hw=0, **o):
    """one i2v_gemm_params; `o` names what differs from a plain row-major fp16 GEMM (see the sweep below)"""
    p = lib.GemmParams()
    p.a, p.w, p.c = _ptr("a"), _ptr("w"), _ptr("c", o.get("c_skew", 0))
    p.M, p.N, p.K, p.lda, p.ldw = M, N, K, K, K
    p.epilogue, p.store_mode = EPI[o.get("epi", "none")], STORE[o.get("store", "rm")]
    p.ldc = o.get("ldc", N // 2 if p.epilogue == 2 else N)
    p.out_scale = o.get("out_scale", 1.0)
    p.frames, p.hw = 16, max(M // 32, 1)
    p.vt_len = p.vt_ld = o.get("vt_len", 64)
    if conv_hw:
        side = int(round(conv_hw ** 0.5))
        stride, up = o.get("stride", 1), o.get("up", 0)
        p.a_mode, p.cin, p.lda = lib.I2V_A_CONV3X3, K // 9, K // 9
        p.n_img, p.out_h, p.out_w, p.stride, p.upsample = M // conv_hw, side, side, stride, up
        p.in_h = p.in_w = side // 2 if up else side * stride
        p.conv_kblock = o.get("kblock", 64 if p.cin % 64 == 0 else 0)
        p.gn_groups = o.get("gn", 0)
    if o.get("res"):
        p.residual, p.ldr = _ptr("residual", o.get("res_skew", 0)), o.get("ldr", N)
    if o.get("lo"):
        p.c_lo = _ptr("c_lo", o.get("lo_skew", 0))
        if o.get("res"):
            p.residual_lo = _ptr("residual_lo")
    if o.get("rowvec"):       # "block": one vector per rows_per_vec rows; an int: periodic with that period
        p.rowvec, p.ld_rowvec = _ptr("rowvec", o.get("rv_skew", 0)), o.get("ld_rowvec", N)
        if o["rowvec"] == "block":
            p.rows_per_vec = o.get("rows_per_vec", conv_hw or 1024)
        else:
            p.rowvec_period = o["rowvec"]
    if o.get("ln"):
        p.ln_wsum, p.ln_eps = _ptr("ln_wsum"), 1e-5
    if o.get("a2"):           # dual-source A, split at k_split = a2
        p.a2, p.k_split, p.lda, p.lda2 = _ptr("a2"), o["a2"], o["a2"], K - o["a2"]
    if o.get("wstack"):
        p.rows_per_w, p.w_batch_stride = o["wstack"], N * K
    if o.get("a_perm"):
        p.a_perm_frames, p.a_perm_hw = o["a_perm"]
    p.c_is_f32 = o.get("f32", 0)
    return p


def step_shapes():
    """every gemm / conv3x3 row of the recorded step, as (M, N, K, conv_hw, options)"""
    out = []
    for line in open(SHAPES):
        m = re.match(r"(gemm|conv3x3) (\d+)x(\d+)x(\d+)((?: [+\w]+)*?)\s+\d+\s+[\d.]+\s", line)
        if not m:
            continue
        M, N, K = int(m.group(2)), int(m.group(3)), int(m.group(4))
        flags, o, hw = m.group(5).split(), {}, 0
        if m.group(1) == "conv3x3":
            hw = M // 32 if int(round((M // 32) ** 0.5)) ** 2 == M // 32 else M // 16
            o["gn"] = 32
        for f in flags:
            if f == "+res": o["res"] = 1
            elif f == "+ln": o["ln"] = 1
            elif f == "geglu": o["epi"] = "geglu"
            elif f in ("st1", "st2", "st3"): o["store"] = ("perm", "vt", "vt_t")[int(f[2]) - 1]
            elif f == "up": o["up"] = 1
            elif f == "s2": o["stride"] = 2
            elif f.startswith("wstack"): o["wstack"] = M // int(f[6:])
            elif f == "perm": o["a_perm"] = (16, M // 32)
            elif f in ("+gn", "stats"): pass
            else: raise ValueError(f"unknown flag {f!r} in {line!r}")
        if o.get("store") == "vt_t":
            o["vt_len"] = M // 32
        out.append((M, N, K, hw, o))
    return out


def sweep():
    """(M, N, K, conv_hw, options, workspace kind) of every row, in table order.  Workspace kinds for the second ask:
    full = the reported size, small = half of it, skew = the reported size at an address that is not 16-byte aligned."""
    rows = []

    def add(M, N, K, hw=0, ws="full", **o):
        rows.append((M, N, K, hw, o, ws))

    for M, N, K, hw, o in step_shapes():
        add(M, N, K, hw, **o)
        if not o.get("ln") and o.get("epi") != "geglu" and o.get("store", "rm") in ("rm", "perm"):
            add(M, N, K, hw, lo=1, **o)
    # plain GEMMs: M one round / several / ragged; N multiples of 320, of 128 / 256 only, neither; K with and without K % 64 == 0,
    # below / above 128, 10 / 40 / 64 K tiles
    Ms, Ns = (256, 1280, 2048, 8192, 32768, 131072, 131072 + 64), (4, 128, 256, 320, 512, 640, 1280, 10240)
    core = ({}, {"res": 1}, {"ln": 1}, {"ln": 1, "epi": "geglu"}, {"res": 1, "lo": 1})
    for M, N, K, o in itertools.product(Ms, Ns, (64, 72, 320, 640, 2560, 4096, 5120), core):
        add(M, N, K, **o)
    extras = ({"epi": "geglu"}, {"epi": "gelu"}, {"lo": 1}, {"rowvec": "block"}, {"rowvec": 16}, {"rowvec": 12}, {"rowvec": "block", "res": 1},
              {"store": "perm"}, {"store": "perm", "lo": 1}, {"store": "perm", "ln": 1}, {"store": "vt"}, {"store": "vt_t"},
              {"store": "vt_t", "ln": 1}, {"store": "vt_t", "ln": 1, "rowvec": 16}, {"store": "vt_t", "ln": 1, "rowvec": 4},
              {"store": "vt_t", "ln": 1, "vt_len": 12}, {"ln": 1, "rowvec": 16}, {"ln": 1, "rowvec": 12}, {"ln": 1, "epi": "geglu", "rowvec": "block"},
              {"ln": 1, "res": 1}, {"f32": 1}, {"out_scale": 0.5}, {"a2": 320}, {"a2": 328}, {"a2": 320, "ln": 1},
              {"wstack": 256}, {"wstack": 128}, {"a_perm": (16, 64)}, {"a_perm": (12, 64)}, {"a_perm": (16, 100)},
              # pointers and leading dimensions that break the 16-byte rule of the row-contiguous epilogue, then the 8-byte one
              {"c_skew": 8}, {"c_skew": 4}, {"ldc": "N+4"}, {"ldc": "N+2"}, {"res": 1, "res_skew": 8}, {"res": 1, "res_skew": 4},
              {"res": 1, "ldr": "N+4"}, {"res": 1, "ldr": "N+2"}, {"lo": 1, "lo_skew": 8}, {"lo": 1, "lo_skew": 4},
              {"rowvec": "block", "rv_skew": 8}, {"rowvec": "block", "ld_rowvec": "N+4"}, {"rowvec": "block", "ld_rowvec": "N+2"})
    for M, N, K, o in itertools.product((2048, 8192, 131072), (320, 512, 1280), (640, 5120), extras):
        o = {k: (N + int(v[2:]) if isinstance(v, str) and v.startswith("N+") else v) for k, v in o.items()}
        add(M, N, K, **o)
    # 3x3 convolutions of the four UNet levels and the VAE's channel counts
    levels = ((2048, 64), (8192, 256), (32768, 1024), (131072, 4096))
    for (M, hw), N, cin, res, gn in itertools.product(levels, (4, 128, 256, 320, 640, 1280), (8, 64, 320, 640, 1280, 2560), (0, 1), (0, 32)):
        add(M, N, 9 * cin, hw, res=res, gn=gn)
    conv_extras = ({"gn": 32, "out_scale": 0.5}, {"gn": 32, "rowvec": "block"}, {"gn": 32, "rowvec": "block", "rows_per_vec": 100},
                   {"gn": 32, "rowvec": 16}, {"gn": 7}, {"gn": 32, "kblock": 0}, {"gn": 32, "lo": 1}, {"gn": 32, "res": 1, "lo": 1},
                   {"gn": 32, "f32": 1}, {"gn": 32, "epi": "gelu"}, {"gn": 32, "c_skew": 8}, {"gn": 1})
    for (M, hw), N, cin, o in itertools.product(levels, (256, 320, 1280), (320, 1280), conv_extras):
        add(M, N, 9 * cin, hw, **o)
    # a workspace that is too small / misaligned: the problems above that report one
    for M, N, K, hw, o, _ in [r for r in rows if r[4].get("epi", "none") == "none" and r[1] % 320 == 0 and r[2] >= 2560 and r[0] <= 8192][::3]:
        add(M, N, K, hw, ws="small", **o)
        add(M, N, K, hw, ws="skew", **o)
    return rows


def label(row):
    M, N, K, hw, o, ws = row
    return " ".join([f"{'conv' if hw else 'gemm'} {M}x{N}x{K}"] + ([f"hw={hw}"] if hw else []) +
                    [f"{k}={v}" for k, v in sorted(o.items()) if v] + ([f"ws={ws}"] if ws != "full" else []))


def ask(lib, h, row):
    """(workspace_bytes, ln_supported, batch_supported, gn_partial_rows) without a workspace, then with the row's"""
    M, N, K, hw, o, ws = row
    p = problem(lib, M, N, K, hw, **o)
    q = lambda: (h.i2v_gemm_workspace_bytes(C.byref(p)), h.i2v_gemm_ln_supported(C.byref(p)), h.i2v_gemm_batch_supported(C.byref(p)),
                 h.i2v_gemm_gn_partial_rows(C.byref(p)))
    before = q()
    if before[0] > 0:
        p.workspace, p.workspace_bytes = _ptr("workspace", 8 if ws == "skew" else 0), before[0] // 2 if ws == "small" else before[0]
    return before + q()


def table(lib):
    """the table's lines: a digest of the sweep's labels (so that a changed sweep is told apart from a changed answer), then per row
    `workspace_bytes ln batch gn_rows ln batch gn_rows` (without, with the workspace; the size itself must not depend on it)"""
    import hashlib
    h, rows = lib.load(), sweep()
    lines = [f"{len(rows)} {hashlib.sha1(chr(10).join(label(r) for r in rows).encode()).hexdigest()}"]
    for r in rows:
        a = ask(lib, h, r)
        assert a[4] == a[0], f"{label(r)}: the reported workspace size depends on the workspace attached"
        lines.append(" ".join(str(v) for v in a[:4] + a[5:]))
    return lines


def recorded():
    return [line.rstrip("\n") for line in open(GOLDEN)]


@pytest.fixture(scope="module")
def lib():
    import i2v_adapter_unofficial_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return pkg._lib


def test_recorded_table_exercises_every_answer():
    """the table cannot pass vacuously: every answer takes every value it can in at least 10 rows, and attaching the
    workspace changes at least one answer"""
    rows = [tuple(int(v) for v in line.split()) for line in recorded()[1:]]
    assert len(rows) >= 2000
    for col in (0, 1, 2, 4, 5):      # workspace_bytes, ln_supported, batch_supported (without / with the workspace)
        assert sum(r[col] > 0 for r in rows) >= 10 and sum(r[col] == 0 for r in rows) >= 10, col
    for col in (3, 6):               # gn_partial_rows
        for rows_per_block in (0, 128, 256):
            assert sum(r[col] == rows_per_block for r in rows) >= 10, (col, rows_per_block)
        assert all(r[col] in (0, 128, 256) for r in rows)
    assert sum(r[1:4] != r[4:] for r in rows) >= 1


def test_step_shapes_are_in_the_sweep():
    shapes = step_shapes()
    assert sum(1 for line in open(SHAPES) if line.startswith(("gemm ", "conv3x3 "))) == len(shapes) >= 70
    labels = {label(r) for r in sweep()}
    assert all(label((M, N, K, hw, o, "full")) in labels for M, N, K, hw, o in shapes)


def test_answers_match_the_recorded_table(lib):
    want, got, rows = recorded(), table(lib), sweep()
    assert got[0] == want[0], "the sweep changed: the table no longer describes it"
    bad = [f"{label(r)}: {g}   (recorded: {w})" for r, g, w in zip(rows, got[1:], want[1:]) if g != w]
    assert not bad and len(got) == len(want), f"{len(bad)} of {len(rows)} problems answer differently:\n" + "\n".join(bad[:20])


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: I2V_LIB_PATH=<library to record from> python tests/test_gemm_plan.py --record")
    sys.path.insert(0, ROOT)
    import i2v_adapter_unofficial_amd as pkg
    lines = table(pkg._lib)
    open(GOLDEN, "w").write("\n".join(lines) + "\n")
    print(f"{len(lines) - 1} rows from {pkg._lib.LIB_PATH} -> {GOLDEN}")
