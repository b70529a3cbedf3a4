"""Which kernel instantiation every GEMM / conv problem of tests/gemm_route_cases.py takes (i2v_gemm_route: host arithmetic, no
GPU), that every instantiation of the launch tables (i2v_gemm_kernel_exists) is the route of at least one case, and that the checker
the GPU test uses (tests/gemm_bounds.py) has teeth: on every case a plain torch fp32 evaluation passes the bound and each of five
slightly wrong evaluations misses it."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import gemm_bounds as B
from tests import gemm_route_cases as G

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


def test_abi_version_19_exports_the_route_queries(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 19
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for sym in ("i2v_gemm_route", "i2v_gemm_last_route", "i2v_gemm_kernel_exists"):
        assert hasattr(h, sym) and sym in lib.SIGNATURES and re.search(rf"\b{sym}\(", src), sym
    r = lib.GemmRoute()
    assert h.i2v_gemm_route(None, C.byref(r)) == -1 and h.i2v_gemm_route(C.byref(lib.GemmParams()), None) == -1
    assert h.i2v_gemm_kernel_exists(None) == 0
    # no launch on this thread yet (nothing in this process launches): the last route is an error, not stale data
    assert h.i2v_gemm_last_route(C.byref(r)) == -1 and b"no i2v_gemm_f16 yet" in h.i2v_last_error()


def _key(r):
    """the instantiation a route names: the template arguments of its kernel (split plan and vec4 are run-time arguments; so are the
    generic kernel's epilogue and store)"""
    if r["family"] == G.GENERIC:
        return ("generic", r["a_mode"], r["generic_tile"])
    if r["family"] == G.THIN:
        return ("conv_thin",)
    return (G.FAMILY[r["family"]], r["a_mode"], r["rows"], r["cols"], r["stages"], r["persistent"], r["extra"], r["epilogue"], r["store_mode"])


def existing_instantiations(lib):
    """the whole space of template arguments, asked through the existence query"""
    h, found = lib.load(), set()
    space = itertools.product(range(5), (0, 1), (0, 64, 128, 256), (0, 64, 128, 256, 320), (0, 2, 3, 4), (0, 1), (0, 1, 2, 4, 8, 3, 6),
                              (0, 1, 2), (0, 1, 2, 3), (-1, 0, 1, 2, 3))
    for fam, am, rows, cols, st, pers, ex, epi, store, gt in space:
        r = lib.GemmRoute(family=fam, a_mode=am, rows=rows, cols=cols, stages=st, persistent=pers, extra=ex, epilogue=epi, store_mode=store,
                          generic_tile=gt)
        if h.i2v_gemm_kernel_exists(C.byref(r)):
            found.add(_key(r.as_dict()))
    return found


@pytest.mark.parametrize("env_name", list(G.ENVS))
def test_every_case_takes_its_expected_route(lib, env_name):
    """asked in a child that carries the environment's switches (they are read once per process); the child loads the library and
    calls host queries only"""
    env = {k: v for k, v in os.environ.items() if k not in G.SWITCHES}
    env.update(dict(G.ENVS[env_name]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gemm_route_cases.py"), "--routes", env_name], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    cases = G.cases_of(env_name)
    assert len(cases) >= 5 and sorted(got) == sorted(c["name"] for c in cases)
    bad = [f"{c['name']}: {got[c['name']]}, expected {G.expected_route(lib, c)}" for c in cases if got[c["name"]] != G.expected_route(lib, c)]
    assert not bad, f"{len(bad)} of {len(cases)} cases take another kernel than the table says:\n" + "\n".join(bad)


def test_every_instantiation_has_a_case(lib):
    exist = existing_instantiations(lib)
    # 70 of the 8-wave kernel (22 + 18 plain and persistent tile, 16 conv tile, 10 deep, 4 split-K), 8 generic, the thin convolution
    assert len(exist) == 79, sorted(exist)
    covered = {_key(G.expected_route(lib, c)) for c in G.CASES}
    assert covered <= exist | set(), f"the table expects kernels that do not exist: {sorted(covered - exist)}"
    assert all(k in exist for k in UNREACHABLE), "UNREACHABLE lists what does not exist"
    uncovered = sorted(exist - covered - set(UNREACHABLE))
    assert not uncovered, f"{len(uncovered)} instantiations are no case's route:\n" + "\n".join(map(str, uncovered))


def test_every_generic_kernel_has_both_epilogues(lib):
    hit = {(_key(G.expected_route(lib, c)), c["route"]["vec4"]) for c in G.CASES if c["route"]["family"] == G.GENERIC}
    for a_mode, tile, vec4 in itertools.product((0, 1), range(4), (0, 1)):
        assert ((("generic", a_mode, tile)), vec4) in hit, f"generic kernel tile {tile}, a_mode {a_mode} has no case with vec4 = {vec4}"


def test_conv_weight_unpacking_inverts_the_library_packer():
    from i2v_adapter_unofficial_amd.blocks import pack_conv3x3
    for cin in (8, 64, 128):
        w = torch.randn(5, cin, 3, 3).half()
        assert torch.equal(B.unpack_conv(pack_conv3x3(w), cin).reshape(5, cin, 3, 3), w)
        assert torch.equal(B.pack_conv(w.reshape(5, cin, 9), cin), pack_conv3x3(w))


def _rounded(c, v, bf16=False):
    """(result, low half or None) as a kernel would store the fp32 values v"""
    o = G.canon(c)
    if bf16:
        hi = v.bfloat16().float()
        hi = hi if o["f32"] else hi.half()
    else:
        hi = v if o["f32"] else v.half()
    return hi, ((v - hi.float()).half() if o["lo"] else None)


def mutants(c):
    """name -> keyword arguments of gemm_bounds.evaluate for every mutant that applies to the case's form"""
    o, K = G.canon(c), G.canon(c)["K"]
    m = {"one K index dropped in the last K tile": dict(drop=(K - 3,)),
         "the last two rows swapped": dict(swap_rows=True),
         "rounded through bf16": dict(bf16=True)}
    if o["bias"]:
        m["bias shifted by one column"] = dict(bias_shift=True)
    if c["route"]["splits"]:
        end = min(2 * c["route"]["kps"] * 64, K)          # the second split's K range, shortened by 8
        m["one split's K range shortened by 8"] = dict(drop=tuple(range(end - 8, end)))
    return m


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_the_checker_has_teeth(c):
    """the bound is a condition on any fp32-accumulating evaluation, so plain torch fp32 on the same inputs, rounded to fp16, must pass
    it; and it is tight enough that each slightly wrong evaluation misses it.  No case is exempt from a mutant of its form."""
    t, _, _ = B.reference(c)
    v = B.evaluate(c, t, torch.float32)
    assert B.check(c, *_rounded(c, v)) is None, "torch fp32 misses the bound: it is derived wrongly"
    for name, kw in mutants(c).items():
        bf16 = kw.pop("bf16", False)
        vm = B.evaluate(c, t, torch.float32, **kw) if kw else v
        msg = B.check(c, *_rounded(c, vm, bf16))
        assert msg is not None and "miss the bound" in msg, f"the checker accepts the mutant `{name}`: {msg}"
