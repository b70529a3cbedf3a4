"""CPU checks of tests/attn_bwd_reference.py: the float64 reference against torch autograd; the kernels the LIBRARY takes for every
case (i2v_attention_bwd_route: host arithmetic, no GPU) against the forms, classes and partition counts written down here by hand;
that the launch table (i2v_attn_bwd_kernel_exists) holds exactly the 47 instantiations and that each is the route of a GPU case; the
coverage the case tables of tests/test_attention_bwd_edges_gpu.py are meant to give; and the reachability of the bound asserted
there: an emulation of the kernels' roundings stays within HALF of it on exactly the inputs the GPU tests use."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import attn_bwd_reference as R
from tests.parity import GRAD_REL_TOL

FWD_REL_TOL = 3e-3      # the forward output's bound in the GPU tests (tests/test_training_gpu.py)


@pytest.mark.parametrize("d,lq,lk,group,heads", [(8, 37, 45, 1, 2), (24, 70, 33, 3, 2), (40, 5, 131, 2, 3)])
def test_reference_equals_autograd(d, lq, lk, group, heads):
    bkv = 2
    q, k, v, do = (t.double() for t in R.make_inputs(d, lq, lk, group, heads, bkv))
    ref = R.reference(q, k, v, do, heads, group)
    q.requires_grad_(), k.requires_grad_(), v.requires_grad_()
    sp = lambda t: t.view(t.shape[0], t.shape[1], heads, d).transpose(1, 2)
    kk, vv = sp(k).repeat_interleave(group, dim=0), sp(v).repeat_interleave(group, dim=0)
    o = torch.nn.functional.scaled_dot_product_attention(sp(q), kk, vv).transpose(1, 2).reshape(q.shape)
    o.backward(do)
    for name, got, want in (("o", ref.o, o.detach()), ("dq", ref.dq, q.grad), ("dk", ref.dk, k.grad), ("dv", ref.dv, v.grad)):
        assert got.dtype == torch.float64 and got.shape == want.shape
        assert (got - want).abs().max().item() <= 1e-10 * want.abs().max().item(), name
    logits = torch.einsum("bhqd,bhkd->bhqk", sp(q), kk).detach() * d ** -0.5
    assert torch.allclose(ref.lse2, torch.logsumexp(logits, -1) * R.LOG2E, rtol=1e-12, atol=0)


INTENDED = {   # (d, lq, lk) -> (ks, dt, dq_form, dkv_form, lse_form), written down by hand from the rule of csrc/attention_bwd.hip
    (8, 70, 77): (1, 2, "dq1", "dkv1", "lse"),
    (16, 45, 515): (1, 2, "dq1", "dkv2", "lse"),
    (24, 603, 40): (1, 2, "dq2", "dkv1", "lse"),
    (32, 40, 601): (1, 2, "dq1", "dkv2", "lse"),
    (32, 600, 601): (1, 2, "dq2_lds", "dkv2_lds64", "lse_lds"),
    (48, 100, 523): (2, 3, "dq1", "dkv2_lds32", "lse"),
    (56, 517, 600): (2, 4, "dq2_lds", "dkv2_lds64", "lse_lds"),
    (72, 130, 77): (3, 5, "dq1", "dkv1", "lse"),
    (88, 96, 643): (3, 6, "dq1", "dkv2_lds32", "lse"),
    (96, 600, 600): (3, 6, "dq2_lds", "dkv2_lds64", "lse_lds"),
    (104, 70, 130): (4, 8, "dq1", "dkv1", "lse"),
    (128, 517, 523): (4, 8, "dq1", "dkv1", "lse"),
    (136, 33, 65): (5, 10, "dq1", "dkv1", "lse"),
    (160, 600, 520): (5, 10, "dq1", "dkv1", "lse"),
    (40, 601, 77): (2, 3, "dq2_lds", "dkv1", "lse_lds"),
    (40, 520, 4): (2, 3, "dq2", "dkv1", "lse"),
    (40, 260, 1000): (2, 3, "dq1", "dkv2_lds64", "lse"),
    (40, 256, 256): (2, 3, "dq1", "dkv1", "lse"),
    (40, 600, 601): (2, 3, "dq2_lds", "dkv2_lds64", "lse_lds"),
    (96, 517, 523): (3, 6, "dq2_lds", "dkv2_lds64", "lse_lds"),
    # the (class, form) pairs added with the route queries
    (24, 67, 517): (1, 2, "dq1", "dkv2_lds32", "lse"),
    (40, 45, 517): (2, 3, "dq1", "dkv2", "lse"),
    (64, 517, 45): (2, 4, "dq2", "dkv1", "lse"),
    (56, 45, 517): (2, 4, "dq1", "dkv2", "lse"),
    (64, 67, 517): (2, 4, "dq1", "dkv2_lds32", "lse"),
    (80, 517, 45): (3, 5, "dq2", "dkv1", "lse"),
    (72, 517, 67): (3, 5, "dq2_lds", "dkv1", "lse_lds"),
    (80, 45, 517): (3, 5, "dq1", "dkv2", "lse"),
    (72, 67, 517): (3, 5, "dq1", "dkv2_lds32", "lse"),
    (80, 131, 517): (3, 5, "dq1", "dkv2_lds64", "lse"),
    (96, 517, 45): (3, 6, "dq2", "dkv1", "lse"),
    (88, 45, 517): (3, 6, "dq1", "dkv2", "lse"),
}
SHORT_CLASS = {40: (2, 3), 80: (3, 5), 160: (5, 10), 16: (1, 2)}
# what the environment switches (read by the library once per process) move R.ENV_CASES to
SWITCHED = {
    ("I2V_ATTN_BWD_LDS", "0"): [(2, 3, "dq2", "dkv2", "lse"), (3, 6, "dq2", "dkv2", "lse")],
    ("I2V_ATTN_BWD_QB", "32"): [(2, 3, "dq2_lds", "dkv2_lds32", "lse_lds"), (3, 6, "dq2_lds", "dkv2_lds32", "lse_lds")],
}
# (d, lq, lk, group) -> the kv_partitions of bkv = 1 and of bkv = 2 (heads 2): kernels.dkv_partitions as it answered at the commit
# before the rule moved into the library, written down once
PARTS = {
    (8, 70, 77, 1): (1, 1), (16, 45, 515, 1): (1, 1), (24, 603, 40, 1): (1, 1), (32, 40, 601, 2): (2, 2), (32, 600, 601, 1): (1, 1),
    (48, 100, 523, 1): (1, 1), (56, 517, 600, 1): (1, 1), (72, 130, 77, 2): (2, 2), (88, 96, 643, 4): (4, 4), (96, 600, 600, 1): (1, 1),
    (104, 70, 130, 1): (1, 1), (128, 517, 523, 2): (2, 2), (136, 33, 65, 1): (1, 1), (160, 600, 520, 1): (1, 1), (40, 601, 77, 2): (2, 2),
    (40, 520, 4, 2): (2, 2), (40, 260, 1000, 8): (8, 8), (40, 256, 256, 1): (1, 1), (40, 600, 601, 1): (1, 1), (96, 517, 523, 2): (2, 2),
    # the added cases have group 1: nothing to deal out
    (24, 67, 517, 1): (1, 1), (40, 45, 517, 1): (1, 1), (64, 517, 45, 1): (1, 1), (56, 45, 517, 1): (1, 1), (64, 67, 517, 1): (1, 1),
    (80, 517, 45, 1): (1, 1), (72, 517, 67, 1): (1, 1), (80, 45, 517, 1): (1, 1), (72, 67, 517, 1): (1, 1), (80, 131, 517, 1): (1, 1),
    (96, 517, 45, 1): (1, 1), (88, 45, 517, 1): (1, 1),
}
KS_DT = sorted(set(v[:2] for v in INTENDED.values()))        # the (ks, dt) the cases are meant to reach: all seven
# instantiations that exist and that no GPU case can take, one line of reason each
UNREACHABLE = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH_NAMES = sorted({k for k, _ in R.ENV_SWITCHES})


@pytest.fixture(scope="module")
def lib():
    import i2v_adapter_unofficial_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    if any(k in os.environ for k in SWITCH_NAMES):
        pytest.fail(f"run the route tests without {SWITCH_NAMES} set: the tables are those of the default environment")
    return pkg._lib


def forms(lib, d, lq, lk, group=1, need_dkv=True, heads=R.RAGGED_HEADS, bkv=R.RAGGED_BKV):
    """(ks, dt, dq_form, dkv_form, lse_form) as the LIBRARY answers (i2v_attention_bwd_route), forms by name"""
    return R.route_forms(R.ask_route(lib, d, lq, lk, group, bkv, need_dkv, heads))


def test_abi_version_32_exports_the_route_queries(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 32
    h = lib.load()
    for sym in ("i2v_attention_bwd_route", "i2v_attention_bwd_last_route", "i2v_attn_bwd_kernel_exists"):
        assert hasattr(h, sym) and sym in lib.SIGNATURES and re.search(rf"\b{sym}\(", src), sym
    for names, prefix in ((R.DQ_FORMS, "I2V_ATTN_BWD_"), (R.DKV_FORMS, "I2V_ATTN_BWD_"), (R.LSE_FORMS, "I2V_ATTN_")):
        for value, name in enumerate(names):
            assert getattr(lib, prefix + name.upper()) == value and re.search(rf"\b{prefix}{name.upper()} = {value}\b", src), name
    assert (lib.I2V_ATTN_BWD_KIND_DQ, lib.I2V_ATTN_BWD_KIND_DKV, lib.I2V_ATTN_BWD_KIND_LSE) == (R.KIND_DQ, R.KIND_DKV, R.KIND_LSE)
    r = lib.AttnBwdRoute()
    assert h.i2v_attention_bwd_route(2, 1, 2, 40, 64, 64, 1, None) == -1 and h.i2v_attn_bwd_kernel_exists(R.KIND_DQ, None) == 0
    # the query refuses what the launch refuses, with the launch's words
    for args, words in (((2, 1, 2, 168, 64, 64, 1), b"head_dim (168) must be a multiple of 8 and <= 160"),
                        ((2, 1, 2, 36, 64, 64, 1), b"head_dim (36) must be a multiple of 8 and <= 160"),
                        ((3, 2, 2, 40, 64, 64, 1), b"bad sizes"), ((2, 1, 2, 40, 0, 64, 1), b"bad sizes"),
                        ((2, 1, 65536, 40, 64, 64, 1), b"heads / batch_q exceed the grid limits")):
        assert h.i2v_attention_bwd_route(*args, C.byref(r)) == -1 and words in h.i2v_last_error(), args
    p = lib.AttnBwdParams()
    for name in ("q", "k", "v", "kt", "dout", "lse", "delta", "dq"):
        setattr(p, name, 0x7F0000000000)
    p.batch_q, p.kv_group, p.heads, p.head_dim, p.lq, p.lk = 2, 1, 2, 168, 64, 64
    assert h.i2v_attention_bwd_f16(C.byref(p), None) == -1 and b"head_dim (168) must be a multiple of 8 and <= 160" in h.i2v_last_error()
    # before this thread's first launch the last route is an error, not stale data; after one (GPU tests earlier in the same
    # process) it names kernels of the table
    assert h.i2v_attention_bwd_last_route(None) == -1
    if h.i2v_attention_bwd_last_route(C.byref(r)) == -1:
        assert b"no i2v_attention_bwd_f16 yet" in h.i2v_last_error()
    else:
        assert h.i2v_attn_bwd_kernel_exists(R.KIND_DQ, C.byref(r)) == 1


def test_the_library_takes_the_intended_form_for_every_case(lib):
    for case in R.RAGGED + R.STRIDED + R.SCALED + R.ENV_CASES:
        d, lq, lk, group = case[:4]
        assert forms(lib, d, lq, lk, group) == INTENDED[(d, lq, lk)], case
        if not case[4]:      # without dK / dV: the same dQ and log-sum-exp kernels, no sweep over the queries
            want = INTENDED[(d, lq, lk)]
            assert forms(lib, d, lq, lk, group, need_dkv=False) == want[:3] + (None,) + want[4:], case
    for heads, d, f in R.SHORT + [R.ONE_FRAME]:
        assert forms(lib, d, f, f, heads=heads, bkv=R.SHORT_PIXELS) == SHORT_CLASS[d] + ("dq1", "dkv1", "lse"), (d, f)
    assert all(c in R.RAGGED for c in R.STRIDED)
    assert sorted({forms(lib, *c[:3])[2] for c in R.STRIDED}) == ["dq1", "dq2", "dq2_lds"]
    # class boundaries and thresholds
    assert [forms(lib, d, 64, 64)[:2] for d in (32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 128, 136, 160)] == \
        [(1, 2), (2, 3), (2, 3), (2, 4), (2, 4), (3, 5), (3, 5), (3, 6), (3, 6), (4, 8), (4, 8), (5, 10), (5, 10)]
    assert forms(lib, 40, 511, 63)[2:] == ("dq1", "dkv1", "lse") and forms(lib, 40, 512, 63)[2:] == ("dq2", "dkv1", "lse")
    assert forms(lib, 40, 512, 64)[2:] == ("dq2_lds", "dkv1", "lse_lds") and forms(lib, 128, 512, 512)[2:] == ("dq1", "dkv1", "lse")
    assert [forms(lib, 40, lq, 512)[3] for lq in (63, 64, 127, 128)] == ["dkv2", "dkv2_lds32", "dkv2_lds32", "dkv2_lds64"]
    assert forms(lib, 104, 600, 600)[4] == "lse" and forms(lib, 96, 600, 600)[4] == "lse_lds"
    r = lib.AttnBwdRoute()
    assert lib.load().i2v_attention_bwd_route(2, 1, 2, 168, 64, 64, 1, C.byref(r)) == -1
    # the grids: 64 queries / keys per workgroup in the one-tile forms, 128 in the two-tile forms; none without the sweep
    for (lq, lk), (bq_, bk_) in (((511, 63), (8, 1)), ((512, 63), (4, 1)), ((513, 512), (5, 4)), ((64, 513), (1, 5)), ((65, 511), (2, 8))):
        got = R.ask_route(lib, 40, lq, lk, 1)
        assert (got["dq_blocks"], got["dkv_blocks"]) == (bq_, bk_), (lq, lk, got)
    assert R.ask_route(lib, 128, 513, 513, 1)["dq_blocks"] == 9 and R.ask_route(lib, 40, 513, 513, 1, need_dkv=False)["dkv_blocks"] == 0


@pytest.mark.parametrize("switch,value", R.ENV_SWITCHES)
def test_environment_switches_move_the_long_cases(lib, switch, value):
    """asked in a child that carries the switch (it is read once per process); the child loads the library and calls host queries only"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCH_NAMES}
    env[switch] = value
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_bwd_reference.py"), "--routes"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = [tuple(x) for x in json.loads(r.stdout.strip().splitlines()[-1])]
    assert R.ENV_CASES == [(40, 600, 601, 1, True), (96, 517, 523, 2, True)] and got == SWITCHED[(switch, value)]
    assert got != [INTENDED[c[:3]] for c in R.ENV_CASES], "the switch moves nothing"


def _parts(lib, case, bkv=R.RAGGED_BKV):
    d, lq, lk, group = case[:4]
    return R.ask_route(lib, d, lq, lk, group, bkv)["kv_partitions"]


def coverage_gaps(lib, table):
    """what the ragged table fails to cover, as a list of sentences (empty = complete); the routes are the library's"""
    gaps = []
    f = {c: forms(lib, *c[:4]) for c in table}
    dkv = [c for c in table if c[4]]                 # the cases that launch the dK / dV sweep
    ragged8_q, ragged8_k = (lambda c: c[1] % 8 != 0), (lambda c: c[2] % 8 != 0)
    for ks, dt in KS_DT:
        dmax = 16 * dt                               # the widest head of the class: dt 16-channel output tiles
        members = [c for c in table if f[c][:2] == (ks, dt)]
        if not members:
            gaps.append(f"class (KS {ks}, DT {dt}) has no case")
        if not any(c[0] < dmax for c in members):
            gaps.append(f"class (KS {ks}, DT {dt}) has no case with d below {dmax}")
        if not any(c in dkv for c in members):
            gaps.append(f"class (KS {ks}, DT {dt}) has no case with dK / dV")
    for form in ("dq1", "dq2", "dq2_lds"):
        members = [c for c in table if f[c][2] == form]
        if not any(ragged8_q(c) for c in members):
            gaps.append(f"{form} has no case with lq % 8 != 0")
        if not any(ragged8_k(c) for c in members):
            gaps.append(f"{form} has no case with lk % 8 != 0")
    for form in ("dkv1", "dkv2", "dkv2_lds32", "dkv2_lds64"):
        members = [c for c in dkv if f[c][3] == form]
        if not any(ragged8_q(c) for c in members):
            gaps.append(f"{form} has no case with lq % 8 != 0")
        if not any(ragged8_k(c) for c in members):
            gaps.append(f"{form} has no case with lk % 8 != 0")
    for form in ("lse", "lse_lds"):
        if not any(f[c][4] == form for c in table):
            gaps.append(f"{form} has no case")
    for ks in (1, 4):
        if not any(f[c][0] == ks and f[c][4] == "lse" for c in table):
            gaps.append(f"attn_lse_kernel<{ks}> has no case")
    if not any(f[c][0] == 1 and f[c][4] == "lse_lds" for c in table):
        gaps.append("attn_lse_lds_kernel<1> has no case")
    for form in ("dkv1", "dkv2_lds32", "dkv2_lds64"):
        if not any(f[c][3] == form and _parts(lib, c) > 1 and c[2] % 32 != 0 for c in dkv):
            gaps.append(f"{form} has no case with kv_partitions > 1 and a ragged lk")
    # a two-tiles-per-wave form whose last wave has a partly / a wholly masked second tile (32 rows per wave: rows % 32 in 17..31 / 1..16)
    for idx, form_idx, name in ((1, 2, "dq"), (2, 3, "dkv")):
        two = [c for c in (table if idx == 1 else dkv) if f[c][form_idx] not in ("dq1", "dkv1")]
        if not any(0 < c[idx] % 32 <= 16 for c in two):
            gaps.append(f"no two-tile {name} case with a wholly masked second tile")
        if not any(c[idx] % 32 > 16 for c in two):
            gaps.append(f"no two-tile {name} case with a partly masked second tile")
    return gaps


def test_tables_cover_every_class_form_and_tail(lib):
    assert KS_DT == [(1, 2), (2, 3), (2, 4), (3, 5), (3, 6), (4, 8), (5, 10)]
    assert coverage_gaps(lib, R.RAGGED) == []
    assert len(set(R.RAGGED)) == len(R.RAGGED)
    # the check has teeth: without its only case a form or class is reported (`also`: the cases added for the (class, form) pairs
    # that share the property leave with it)
    dkv2, dq2 = (lambda c: (c[1], c[2]) == (45, 517)), (lambda c: (c[1], c[2]) == (517, 45))
    none = lambda c: False
    for only, also, what in (((16, 45, 515, 1, True), dkv2, "dkv2 has no case with lq % 8 != 0"),
                             ((104, 70, 130, 1, True), none, "class (KS 4, DT 8) has no case with d below 128"),
                             ((32, 600, 601, 1, True), none, "attn_lse_lds_kernel<1> has no case"),
                             ((24, 603, 40, 1, True), dq2, "dq2 has no case with lq % 8 != 0"),
                             ((88, 96, 643, 4, True), none, "dkv2_lds32 has no case with kv_partitions > 1 and a ragged lk")):
        assert only in R.RAGGED
        assert what in coverage_gaps(lib, [c for c in R.RAGGED if c != only and not also(c)]), only
        assert what not in coverage_gaps(lib, [c for c in R.RAGGED if not also(c)]), only
    # the batch-independence check compares a two-entry call with a one-entry call: the same partition count in both
    for case in R.RAGGED:
        assert _parts(lib, case, bkv=2) == _parts(lib, case, bkv=1), case
    # short sequences as the issue lists them
    assert {(hh, d) for hh, d, _ in R.SHORT} == {(8, 40), (8, 80), (2, 160), (4, 16)}
    assert sorted(f for hh, d, f in R.SHORT if d == 40) == [2, 3, 5, 8, 12, 16, 24, 32]
    for d in (80, 160, 16):
        assert sorted(f for _, dd, f in R.SHORT if dd == d) == [3, 16, 24]


def test_partition_counts_are_those_of_the_table(lib):
    """the recommended kv_partitions (the rule lives in the library; kernels.dkv_partitions hands it on) against the numbers written
    down in PARTS"""
    import i2v_adapter_unofficial_amd as pkg
    cases = R.RAGGED + R.SCALED + R.ENV_CASES
    assert sorted(PARTS) == sorted({c[:4] for c in cases})
    for case in cases:
        d, lq, lk, group = case[:4]
        for i, bkv in enumerate((1, 2)):
            assert _parts(lib, case, bkv) == PARTS[case[:4]][i], (case, bkv)
            assert R.ask_route(lib, d, lq, lk, group, bkv, need_dkv=False)["kv_partitions"] == PARTS[case[:4]][i], (case, bkv)
            assert pkg.kernels.dkv_partitions(bkv * group, group, R.RAGGED_HEADS, d, lq, lk) == PARTS[case[:4]][i], (case, bkv)
    for heads, d, f in R.SHORT:
        assert R.ask_route(lib, d, f, f, 1, R.SHORT_PIXELS, heads=heads)["kv_partitions"] == 1
        assert pkg.kernels.dkv_partitions(R.SHORT_PIXELS, 1, heads, d, f, f) == 1


# ---------------------------------------------------------------------------------------------- the launch table
ONE_TILE = {R.KIND_DQ: ("dq1",), R.KIND_DKV: ("dkv1",)}
TWO_TILE = {R.KIND_DQ: ("dq2", "dq2_lds"), R.KIND_DKV: ("dkv2", "dkv2_lds32", "dkv2_lds64")}


def existing_instantiations(lib):
    """the whole space of template arguments (and what lies just outside it), asked through the existence query: a set of
    (kind, ks, dt, form name); the log-sum-exp kernels have no dt (0)"""
    h, found = lib.load(), set()
    for ks, dt, form in itertools.product(range(0, 8), range(0, 13), range(-1, 6)):
        r = lib.AttnBwdRoute(ks=ks, dt=dt, dq_form=form, dkv_form=form, lse_form=form, kv_partitions=1, dq_blocks=1, dkv_blocks=1)
        for kind, names in ((R.KIND_DQ, R.DQ_FORMS), (R.KIND_DKV, R.DKV_FORMS), (R.KIND_LSE, R.LSE_FORMS)):
            if h.i2v_attn_bwd_kernel_exists(kind, C.byref(r)):
                found.add((kind, ks, 0 if kind == R.KIND_LSE else dt, names[form]))
        assert not h.i2v_attn_bwd_kernel_exists(-1, C.byref(r)) and not h.i2v_attn_bwd_kernel_exists(3, C.byref(r))
    return found


def instantiations_of(route_forms):
    """the table entries a route (ks, dt, dq_form, dkv_form | None, lse_form) launches"""
    ks, dt, dq, dkv, lse = route_forms
    out = {(R.KIND_DQ, ks, dt, dq), (R.KIND_LSE, ks, 0, lse)}
    return out | ({(R.KIND_DKV, ks, dt, dkv)} if dkv is not None else set())


def test_the_table_holds_exactly_the_47_instantiations_and_every_one_has_a_gpu_case(lib):
    exist = existing_instantiations(lib)
    two = [c for c in KS_DT if c[1] <= 6]
    expected = {(kind, ks, dt, form) for kind in ONE_TILE for ks, dt in KS_DT for form in ONE_TILE[kind]} | \
               {(kind, ks, dt, form) for kind in TWO_TILE for ks, dt in two for form in TWO_TILE[kind]} | \
               {(R.KIND_LSE, ks, 0, "lse") for ks in (1, 2, 3, 4, 5)} | {(R.KIND_LSE, ks, 0, "lse_lds") for ks in (1, 2, 3)}
    assert len(two) == 5 and len(expected) == 47 and exist == expected, sorted(exist ^ expected)
    # what the GPU tests launch (tests/test_attention_bwd_edges_gpu.py): the ragged, scaled and short cases in the default
    # environment, the switched cases in their children
    covered = set()
    for d, lq, lk, group, need_dkv in R.RAGGED + R.SCALED:
        covered |= instantiations_of(forms(lib, d, lq, lk, group, need_dkv))
    for heads, d, f in R.SHORT + [R.ONE_FRAME]:
        covered |= instantiations_of(forms(lib, d, f, f, heads=heads, bkv=R.SHORT_PIXELS))
    for routes in SWITCHED.values():
        for rf in routes:
            covered |= instantiations_of(rf)
    assert covered <= exist, f"the cases expect kernels that do not exist: {sorted(covered - exist)}"
    assert all(k in exist for k in UNREACHABLE), "UNREACHABLE lists what does not exist"
    uncovered = sorted(exist - covered - set(UNREACHABLE))
    assert not uncovered, f"{len(uncovered)} instantiations are no GPU case's route:\n" + "\n".join(map(str, uncovered))
    # every route a valid size can take names entries of the table (a missing entry would be I2V_ERR_UNSUPPORTED at the launch)
    for d, lq, lk in itertools.product(range(8, 161, 8), (1, 63, 64, 127, 128, 511, 512), (1, 63, 64, 511, 512)):
        assert instantiations_of(forms(lib, d, lq, lk)) <= exist, (d, lq, lk)


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


def _emulation_errors(args, group, heads, need_dkv=True):
    (q, k, v, do), ref = R.case_data(*args)
    em = R.emulate(q, k, v, do, heads, group)
    errs = {"o": _rel(em.o, ref.o), "dq": _rel(em.dq, ref.dq)}
    if need_dkv:
        errs.update(dk=_rel(em.dk, ref.dk), dv=_rel(em.dv, ref.dv))
    return errs


def _assert_half_bound(errs, what):
    for name, e in errs.items():
        bound = FWD_REL_TOL if name == "o" else GRAD_REL_TOL
        assert e <= 0.5 * bound, f"{what}: emulated {name} is {e:.3e} of max|ref|, more than half the bound {bound:.1e}"


@pytest.mark.parametrize("case", R.RAGGED + R.ENV_CASES + [c for c in R.SCALED if c not in R.RAGGED], ids=R.case_id)
def test_bound_is_reachable_ragged(case):
    d, lq, lk, group, need_dkv = case
    _assert_half_bound(_emulation_errors((d, lq, lk, group), group, R.RAGGED_HEADS, need_dkv), case)


@pytest.mark.parametrize("case", R.SHORT, ids=R.case_id)
def test_bound_is_reachable_short(case):
    heads, d, f = case
    _assert_half_bound(_emulation_errors(R.short_case(heads, d, f), 1, heads), case)


@pytest.mark.parametrize("exp", R.SCALE_EXPONENTS)
@pytest.mark.parametrize("case", R.SCALED, ids=R.case_id)
def test_bound_is_reachable_scaled(case, exp):
    d, lq, lk, group, _ = case
    errs = _emulation_errors((d, lq, lk, group, R.RAGGED_HEADS, R.RAGGED_BKV, exp), group, R.RAGGED_HEADS)
    del errs["o"]
    _assert_half_bound(errs, (case, exp))


def test_one_frame_reference_and_emulation():
    """one key: P = 1, so dV = dO and the references of dQ, dK are zero; the emulation's dQ, dK (the fp32 difference between
    dO . V and rowsum(dO o O)) stay within half of the 1e-3 max|dV| the GPU test asserts"""
    heads, d, f = R.ONE_FRAME
    (q, k, v, do), ref = R.case_data(*R.short_case(heads, d, f))
    assert torch.equal(ref.dv, do.double()) and torch.equal(ref.o, v.double())
    assert ref.dq.abs().max().item() <= 1e-12 and ref.dk.abs().max().item() <= 1e-12      # (two float64 sums of the same terms)
    em = R.emulate(q, k, v, do, heads, 1)
    assert torch.equal(em.dv.half(), do)
    lim = 0.5 * 1e-3 * ref.dv.abs().max().item()
    assert em.dq.abs().max().item() <= lim and em.dk.abs().max().item() <= lim
