"""Which kernel instantiation every temporal-attention problem of tests/tattn_route_cases.py takes (i2v_temporal_attention_route: host
arithmetic, no GPU), that every instantiation of the launch table (i2v_tattn_kernel_exists) is the route of at least one case, that
the production shapes keep their routes, and that the checker the GPU test uses (tests/tattn_bounds.py) has teeth: on every case a
torch emulation of the kernels' arithmetic and plain fp32 SDPA pass the bound, and each of six slightly wrong evaluations misses it."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import tattn_bounds as B
from tests import tattn_route_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# instantiations that exist and that no case can take, one line of reason each
UNREACHABLE = {}


@pytest.fixture(scope="module")
def lib():
    import i2v_adapter_unofficial_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return pkg._lib


def test_abi_version_20_exports_the_route_queries(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 20
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for sym in ("i2v_temporal_attention_route", "i2v_temporal_attention_last_route", "i2v_tattn_kernel_exists"):
        assert hasattr(h, sym) and sym in lib.SIGNATURES and re.search(rf"\b{sym}\(", src), sym
    assert (lib.I2V_TATTN_LDS_FORM, lib.I2V_TATTN_REG_FORM) == (G.LDS_FORM, G.REG_FORM) == (0, 1)
    r = lib.TAttnRoute()
    assert h.i2v_temporal_attention_route(None, C.byref(r)) == -1 and h.i2v_temporal_attention_route(C.byref(lib.TAttnParams()), None) == -1
    assert h.i2v_tattn_kernel_exists(None) == 0
    # the query refuses what the launch refuses, with the launch's words
    p = G.fake_params(lib, G.CASES[0])
    p.vt_ld = 4
    assert h.i2v_temporal_attention_route(C.byref(p), C.byref(r)) == -1 and b"vt_ld must be a multiple of 8" in h.i2v_last_error()
    p = G.fake_params(lib, G.CASES[0])
    p.head_dim = 168
    assert h.i2v_temporal_attention_route(C.byref(p), C.byref(r)) == -1 and b"head_dim (168)" in h.i2v_last_error()
    # before this thread's first launch the last route is an error, not stale data; after one (GPU tests earlier in the same
    # process) it names a kernel of the table
    assert h.i2v_temporal_attention_last_route(None) == -1
    if h.i2v_temporal_attention_last_route(C.byref(r)) == -1:
        assert b"no i2v_temporal_attention_f16 yet" in h.i2v_last_error()
    else:
        assert h.i2v_tattn_kernel_exists(C.byref(r)) == 1


def _key(r):
    """the instantiation a route names: the template arguments of its kernel (the grid is a run-time argument)"""
    return (r["form"], r["dqk"], r["dpv"], r["pf"], r["nqt"])


def existing_instantiations(lib):
    """the whole space of template arguments (and what lies just outside it), asked through the existence query"""
    h, found = lib.load(), set()
    sizes = (0, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 192)
    for form, dqk, dpv, pf, nqt in itertools.product((-1, 0, 1, 2), sizes, sizes, range(0, 6), range(0, 4)):
        r = lib.TAttnRoute(form=form, dqk=dqk, dpv=dpv, pf=pf, nqt=nqt, blocks=1)
        if h.i2v_tattn_kernel_exists(C.byref(r)):
            found.add(_key(r.as_dict()))
    return found


@pytest.mark.parametrize("env_name", list(G.ENVS))
def test_every_case_takes_its_expected_route(lib, env_name):
    """asked in a child that carries the environment's switch (it is read once per process); the child loads the library and calls
    host queries only"""
    env = {k: v for k, v in os.environ.items() if k not in G.SWITCHES}
    env.update(dict(G.ENVS[env_name]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tattn_route_cases.py"), "--routes", env_name], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    cases = G.cases_of(env_name)
    assert len(cases) >= 5 and sorted(got) == sorted(c["name"] for c in cases)
    bad = [f"{c['name']}: {got[c['name']]}, expected {c['route']}" for c in cases if got[c["name"]] != c["route"]]
    assert not bad, f"{len(bad)} of {len(cases)} cases take another kernel than the table says:\n" + "\n".join(bad)


def test_every_instantiation_has_a_case_in_the_default_environment(lib):
    exist = existing_instantiations(lib)
    expected = {(G.LDS_FORM, dqk, dpv, pf, 0) for dqk, dpv in G.CLASSES for pf in (1, 2, 3, 4)} | \
               {(G.REG_FORM, dqk, dpv, 0, nqt) for dqk, dpv in G.CLASSES for nqt in (1, 2)}
    assert len(expected) == 48 and exist == expected, sorted(exist ^ expected)
    covered = {_key(c["route"]) for c in G.cases_of("default")}
    assert covered <= exist, f"the table expects kernels that do not exist: {sorted(covered - exist)}"
    assert all(k in exist for k in UNREACHABLE), "UNREACHABLE lists what does not exist"
    uncovered = sorted(exist - covered - set(UNREACHABLE))
    assert not uncovered, f"{len(uncovered)} instantiations are no case's route:\n" + "\n".join(map(str, uncovered))


def test_the_table_covers_the_tails_the_kernels_have():
    """frame tails per form, head-dim tails and class sizes, head counts, one pixel, the prefetch and grid-stride thresholds, wide
    V^T rows, q / k slices, the output layouts, the input families"""
    d = G.cases_of("default")
    lds = [c for c in d if c["route"]["form"] == G.LDS_FORM]
    reg = {n: [c for c in d if c["route"]["nqt"] == n] for n in (1, 2)}
    assert {c["frames"] for c in lds} >= {1, 2, 7, 8, 9, 15, 16} and {c["frames"] for c in reg[1]} >= {1, 2, 7, 8, 9, 15, 16}
    assert {c["frames"] for c in reg[2]} >= {17, 24, 25, 31, 32}
    assert {c["head_dim"] for c in d} >= {8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 120, 128, 136, 152, 160}
    assert {c["heads"] for c in lds} >= {1, 2, 3, 5, 9} and {c["heads"] for c in reg[1] + reg[2]} >= {1, 2, 3, 5, 9}
    assert any(c["n_pixels"] == 1 for c in lds) and any(c["n_pixels"] == 1 for c in reg[1] + reg[2])
    assert any(c["n_pixels"] == 2048 + 5 for c in lds)
    for n in (1, 2):          # the grid-stride loop with a ragged last pass
        assert any(c["route"]["blocks"] == 2048 and 8192 < c["n_pixels"] * c["heads"] < 8192 + 64 and c["n_pixels"] * c["heads"] % 4 for c in reg[n])
    for group in (lds, reg[1], reg[2]):
        assert any(c["vt_ld"] > G.pad8(c["frames"]) for c in group)
        assert any(c["q_ld"] for c in group) and any(c["o"] == "wide" for c in group) and any(c["inputs"] == "spike" for c in group)
    C_ = lambda c: c["heads"] * c["head_dim"]
    assert any(c["q_ld"] == 2 * C_(c) for c in d) and any(c["q_ld"] == 3 * C_(c) for c in d)
    assert {c["o"] for c in reg[1] + reg[2]} >= {"odd", "oddbase"} and not any(c["o"] in ("odd", "oddbase") for c in lds)
    assert any(c["inputs"] == "large" for c in lds) and any(c["inputs"] == "large" for c in reg[1]) and any(c["inputs"] == "large" for c in reg[2])
    # the chunk overflow: LDS-sized shapes with more chunks than PF = 4 moves run on the register kernel
    by = {c["name"]: c for c in d}
    for name, chunks in (("reg1-c48-chunks1280", 1280), ("reg1-c128-chunks1152", 1152)):
        c = by[name]
        assert C_(c) // 8 * c["vt_ld"] == chunks > 1024 and 2 * (48 * (C_(c) + 8) + C_(c) * (c["vt_ld"] + 8)) <= 65536 and c["route"]["form"] == G.REG_FORM
    off = G.cases_of("lds0")
    assert len(off) >= 5 and all(c["route"]["form"] == G.REG_FORM and c["frames"] <= 16 for c in off)
    assert any((c["frames"], c["heads"], c["head_dim"]) == (16, 8, 40) for c in off)


# the un-fused motion modules' shapes of the benchmark configurations (B = 2 for CFG, 8 heads, q | k one [rows, 2 C] matrix,
# vt_ld = pad8(frames)): (config, n_pixels, frames, head_dim) -> the route they take at the commit before the route queries
PRODUCTION = [
    ("8 f x 256^2, 32^2 level", 2048, 8, 40, G.L(64, 48, 2, 2048)),
    ("8 f x 256^2, 16^2 level", 512, 8, 80, G.R(96, 80, 1, 1024)),
    ("8 f x 256^2, 8^2 level", 128, 8, 160, G.R(160, 160, 1, 256)),
    ("8 f x 256^2, 4^2 level", 32, 8, 160, G.R(160, 160, 1, 64)),
    ("16 f x 512^2, 64^2 level", 8192, 16, 40, G.L(64, 48, 3, 2048)),
    ("16 f x 512^2, 32^2 level", 2048, 16, 80, G.R(96, 80, 1, 2048)),
    ("16 f x 512^2, 16^2 level", 512, 16, 160, G.R(160, 160, 1, 1024)),
    ("16 f x 512^2, 8^2 level", 128, 16, 160, G.R(160, 160, 1, 256)),
    ("32 f x 768^2, 96^2 level", 18432, 32, 40, G.R(64, 48, 2, 2048)),
    ("32 f x 768^2, 48^2 level", 4608, 32, 80, G.R(96, 80, 2, 2048)),
    ("32 f x 768^2, 24^2 level", 1152, 32, 160, G.R(160, 160, 2, 2048)),
    ("32 f x 768^2, 12^2 level", 288, 32, 160, G.R(160, 160, 2, 576)),
]


def test_production_shapes_keep_their_routes(lib):
    for what, n_pixels, frames, d, route in PRODUCTION:
        c = dict(n_pixels=n_pixels, frames=frames, heads=8, head_dim=d, vt_ld=G.pad8(frames), q_ld=16 * d, k_ld=16 * d, o="own")
        assert G.ask_route(lib, c) == route, what


def test_no_shape_with_the_narrowest_vt_changes_route(lib):
    """vt_ld = pad8(frames) is what the model passes: there an LDS-sized pixel has at most 896 chunks, so the chunk limit of the LDS
    form sends nothing elsewhere (the largest C within 64 KiB at each vt_ld, asked from the library)"""
    for frames, d in itertools.product((8, 16), (8, 16, 40, 64)):
        lds_heads = [h for h in range(1, 80) if 2 * (48 * (h * d + 8) + h * d * (frames + 8)) <= 65536]
        c = dict(n_pixels=4, frames=frames, heads=lds_heads[-1], head_dim=d, vt_ld=frames, q_ld=None, k_ld=None, o="own")
        r = G.ask_route(lib, c)
        assert r["form"] == G.LDS_FORM and r["pf"] == -(-(lds_heads[-1] * d // 8 * frames) // 256) <= 4, (frames, d, r)
        c["heads"] += 1
        assert G.ask_route(lib, c)["form"] == G.REG_FORM


# ------------------------------------------------------------------------------------------------------------------- the checker
def mutants(c):
    """name -> keyword arguments of tattn_bounds.emulate for every mutant that applies to the case.
    The two bf16 roundings inject a relative 2^-8 at most: they show where the bound is a small multiple of the fp16 roundings, the
    `unit` family (the logit term of `large` / `spike` rows, which scales with sum |q||k|, exceeds them; a spike row's P is one-hot
    and exact in either format).  A single key's P is 1.0 in either format and at any scale.  The admitted slot has logit 0 (a zero K
    row): in the `large` family nearly every row's maximum lies tens of log2 units above it and the slot's weight vanishes."""
    F, d = c["frames"], c["head_dim"]
    m = {}
    if c["inputs"] == "unit":
        m["the output rounded through bf16"] = dict(out_bf16=True)
        if F >= 2:
            m["P rounded through bf16"] = dict(p_bf16=True)
    if F >= 2:
        m["the last frame's key dropped"] = dict(drop_last=True)
    if F < 32 and c["inputs"] != "large":
        m["key slot `frames` admitted with V = 0"] = dict(extra_slot=True)
    if B.class_of(d)[0] != d and F >= 2:
        m["scale = DQK^-0.5"] = dict(scale_dqk=True)
    if c["heads"] > 1:
        m["head h reads head h + 1's V"] = dict(next_head_v=True)
    return m


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_the_checker_has_teeth(c):
    """the bound is a condition on any evaluation in fp32 with P and the result rounded to fp16, so the emulation of the kernels'
    arithmetic and plain fp32 SDPA on the same inputs must pass it; and it is tight enough that each slightly wrong evaluation
    misses it.  No case is exempt from a mutant that applies to it."""
    t, _, _, _ = B.reference(c)
    args = (t["q"], t["k"], t["v"], c["heads"])
    assert B.check(c, B.emulate(*args)) is None, "the emulation of the kernels' arithmetic misses the bound: it is derived wrongly"
    assert B.check(c, B.sdpa_fp32(*args)) is None, "torch fp32 SDPA misses the bound: it is derived wrongly"
    for name, kw in mutants(c).items():
        msg = B.check(c, B.emulate(*args, **kw))
        assert msg is not None and ("miss the bound" in msg or "non-finite" in msg), f"the checker accepts the mutant `{name}`: {msg}"


def test_every_mutant_is_applied_somewhere_in_every_form():
    for group in ([c for c in G.CASES if c["route"]["form"] == G.LDS_FORM], [c for c in G.CASES if c["route"]["nqt"] == 1],
                  [c for c in G.CASES if c["route"]["nqt"] == 2]):
        names = set().union(*(mutants(c) for c in group))
        assert len(names) == 6, names
