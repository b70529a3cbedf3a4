"""The flash-attention backward (csrc/attention_bwd.hip) at every kernel instantiation and tail: the HIP kernels against the
float64 reference of tests/attn_bwd_reference.py (explicit formulas, no autograd), on the case tables defined there.  After every
launch the library's own report of the kernels it took (kernels.last_attn_bwd_route()) must be the route written down by hand in
tests/test_attention_bwd_reference.py, which also shows on the CPU that the tables reach every instantiation of the launch table,
the lq / lk pads and the kv_partitions path, and that a kernel with the documented roundings sits within half of the bound.

Bounds: gradients GRAD_REL_TOL (2.5e-3) of the largest reference entry, forward output 3e-3, log2-sum-exp 1e-3: the project's own
(tests/parity.py, tests/test_training_gpu.py).  Measured on MI355X: profiles/attn_bwd_edges_errors.jsonl."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import attn_bwd_reference as R
from tests.parity import GRAD_REL_TOL, compare
from tests.test_attention_bwd_reference import INTENDED, PARTS, SHORT_CLASS, SWITCHED

pytestmark = pytest.mark.gpu
FWD_REL_TOL, LSE_REL_TOL = 3e-3, 1e-3


def K():
    import i2v_adapter_unofficial_amd as p
    return p.kernels


def _assert_route(want, parts, need_dkv=True):
    """the launch just made took the kernels the tables say: want = (ks, dt, dq_form, dkv_form, lse_form) by name, parts = the
    kv_partitions it ran with"""
    got = K().last_attn_bwd_route()
    want = tuple(want) if need_dkv else tuple(want[:3]) + (None,) + tuple(want[4:])
    parts = parts if need_dkv else 1
    assert R.route_forms(got) == want and got["kv_partitions"] == parts, \
        f"another kernel ran than the test is about: {R.route_forms(got)} x {got['kv_partitions']}, expected {want} x {parts}"


def _run(dev, inputs, *, heads, d, group, want, parts, need_dkv=True, embed=None):
    """forward (with its log-sum-exp), attention_lse, and the backward from both statistics, on fp16 [b, l, C] host operands.
    embed: a function that places a dense [rows, C] matrix on the device in the layout under test.
    want, parts: the route both backward launches must report (_assert_route)."""
    k_ = K()
    q, k, v, do = inputs
    (bq, lq, C), (bkv, lk, _) = q.shape, k.shape
    to = embed or (lambda t: t.to(dev))
    qd, kd, vd, dod = (to(t.reshape(-1, C)) for t in (q, k, v, do))
    kw = dict(batch_q=bq, lq=lq, lk=lk, heads=heads, head_dim=d, kv_group=group)
    od, lse_f = k_.attention(qd, kd, k_.transpose_tokens(vd, lk), return_lse=True, **kw)
    lse = k_.attention_lse(qd, kd, **kw)
    # the statistic the forward kernel itself writes (i2v_attn_params.lse): the same output bits, its own (fp16-scaled-Q) logits
    od_k, lse_k = k_.attention(qd, kd, k_.transpose_tokens(vd, lk), return_lse="fused", **kw)
    assert torch.equal(od, od_k)
    grads = k_.attention_bwd(qd, kd, vd, od, dod, need_dkv=need_dkv, **kw)                    # recomputes the log-sum-exp
    _assert_route(want, parts, need_dkv)
    grads_f = k_.attention_bwd(qd, kd, vd, od, dod, need_dkv=need_dkv, lse=lse_f, **kw)      # the one the forward wrote
    _assert_route(want, parts, need_dkv)
    return dict(o=od, lse=lse, lse_f=lse_f, lse_k=lse_k, grads=grads, grads_f=grads_f, dev=(qd, kd, vd, dod), kw=kw)


def _check(run, ref, tag, need_dkv=True, grads_only=False):
    bq, heads, lq = ref.lse2.shape
    C = ref.o.shape[-1]
    if not grads_only:
        compare(run["o"], ref.o.reshape(-1, C), rel=FWD_REL_TOL, name=f"{tag}: forward output")
        compare(run["lse"], ref.lse2, rel=LSE_REL_TOL, name=f"{tag}: attention_lse")
        compare(run["lse_f"], ref.lse2, rel=LSE_REL_TOL, name=f"{tag}: the forward's log-sum-exp")
        compare(run["lse_k"], ref.lse2, rel=LSE_REL_TOL, name=f"{tag}: the forward kernel's fused log-sum-exp")
    for key, how in (("grads", "recomputed lse"), ("grads_f", "forward's lse")):
        dq, dk, dv = run[key]
        compare(dq, ref.dq.reshape(-1, C), rel=GRAD_REL_TOL, name=f"{tag}: dQ ({how})")
        if need_dkv:
            compare(dk, ref.dk.reshape(-1, C), rel=GRAD_REL_TOL, name=f"{tag}: dK ({how})")
            compare(dv, ref.dv.reshape(-1, C), rel=GRAD_REL_TOL, name=f"{tag}: dV ({how})")
        else:
            assert dk is None and dv is None


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _tag(case):
    d, lq, lk = case[:3]
    return f"attn bwd d={d} lq={lq} lk={lk} group={case[3]} {'/'.join(INTENDED[(d, lq, lk)][2:])}"


def _want(case):
    """(forms, kv_partitions at bkv = 2) of a ragged / strided / scaled case, from the hand-written tables"""
    return dict(want=INTENDED[case[:3]], parts=PARTS[case[:4]][1])


@pytest.mark.parametrize("case", R.RAGGED, ids=R.case_id)
def test_ragged(dev, case):
    """every launch form and head-dim class with ragged lengths: values against the float64 reference, a second call bit-identical,
    and the first K / V entry's results bit-identical to a call on that entry alone (a missing tail mask reads the neighbouring
    batch entry's rows in one call and something else in the other)."""
    d, lq, lk, group, need_dkv = case
    heads, bkv = R.RAGGED_HEADS, R.RAGGED_BKV
    k_ = K()
    inputs, ref = R.case_data(d, lq, lk, group)
    run = _run(dev, inputs, heads=heads, d=d, group=group, need_dkv=need_dkv, **_want(case))
    _check(run, ref, _tag(case), need_dkv)
    qd, kd, vd, dod = run["dev"]
    again = k_.attention_bwd(qd, kd, vd, run["o"], dod, need_dkv=need_dkv, **run["kw"])
    _assert_route(INTENDED[case[:3]], PARTS[case[:4]][1], need_dkv)
    assert _same(run["grads"], again), "a second identical call differs"
    # batch independence, bit for bit: K / V entry 0 with its whole group of query batches
    assert k_.dkv_partitions(bkv * group, group, heads, d, lq, lk) == k_.dkv_partitions(group, group, heads, d, lq, lk)
    nq, nk = group * lq, lk
    one = k_.attention_bwd(qd[:nq].clone(), kd[:nk].clone(), vd[:nk].clone(), run["o"][:nq].clone(), dod[:nq].clone(),
                           need_dkv=need_dkv, **dict(run["kw"], batch_q=group))
    _assert_route(INTENDED[case[:3]], PARTS[case[:4]][0], need_dkv)
    dq, dk, dv = run["grads"]
    assert torch.equal(dq[:nq], one[0]), "dQ of batch entry 0 depends on the other entries"
    if need_dkv:
        assert torch.equal(dk[:nk], one[1]), "dK of batch entry 0 depends on the other entries"
        assert torch.equal(dv[:nk], one[2]), "dV of batch entry 0 depends on the other entries"


@pytest.mark.parametrize("case", R.SHORT, ids=R.case_id)
def test_short_sequences(dev, case):
    """a motion module's shape: batch = pixels, lq = lk = frames <= 32, most of a 32-row block masked"""
    heads, d, f = case
    inputs, ref = R.case_data(*R.short_case(heads, d, f))
    want = SHORT_CLASS[d] + ("dq1", "dkv1", "lse")
    run = _run(dev, inputs, heads=heads, d=d, group=1, want=want, parts=1)
    _check(run, ref, f"attn bwd short heads={heads} d={d} F={f}")
    qd, kd, vd, dod = run["dev"]
    assert _same(run["grads"], K().attention_bwd(qd, kd, vd, run["o"], dod, **run["kw"])), "a second identical call differs"
    _assert_route(want, 1)


def _one_frame(dev, key):
    heads, d, f = R.ONE_FRAME
    inputs, ref = R.case_data(*R.short_case(heads, d, f))
    run = _run(dev, inputs, heads=heads, d=d, group=1, want=SHORT_CLASS[d] + ("dq1", "dkv1", "lse"), parts=1)
    C = heads * d
    compare(run["o"], ref.o.reshape(-1, C), rel=FWD_REL_TOL, name="attn bwd one frame: forward output")
    lim = 1e-3 * ref.dv.abs().max().item()
    dq, dk, dv = run[key]
    compare(dq, ref.dq.reshape(-1, C), abs_tol=lim, name=f"attn bwd one frame: dQ ({key})")
    compare(dk, ref.dk.reshape(-1, C), abs_tol=lim, name=f"attn bwd one frame: dK ({key})")
    bad = dv.cpu() != inputs[3].reshape(-1, C)
    assert not bad.any(), f"dV is not dO in {int(bad.sum())} of {bad.numel()} entries"


def test_one_frame(dev):
    """one key per query: P = 1, so dV = fp16(dO) exactly and dQ = dK = 0 up to the fp32 difference between the MFMA's dO . V and
    rowdot_heads' delta (about d 2^-24 |dO| |V| ~ 1e-4 before the 1 / sqrt d scale): <= 1e-3 max|dV|.  With the log-sum-exp
    recomputed by attention_lse (measured: dV exact, max|dQ|, max|dK| 1.0e-6)."""
    _one_frame(dev, "grads")


def test_one_frame_with_the_forwards_log_sum_exp(dev):
    """The same with the log-sum-exp attention(return_lse=True) hands over, as the trainer runs it.  This test found that the
    statistic the forward KERNEL writes (return_lse="fused") does not serve: csrc/attention.hip scales Q by scale log2 e and rounds
    it to fp16 before Q K^T, so its statistic belongs to those rounded logits (off by up to 1.2e-3 here, attention_lse: 6e-7), the
    backward's P, recomputed from the unrounded Q, carried a factor 2^(-error) on whole rows, and dV differed from dO in 9519 of
    81920 entries by up to 1.95e-3.  return_lse=True now returns attention_lse's statistic; the kernel's stays as "fused"."""
    _one_frame(dev, "grads_f")


@pytest.mark.parametrize("case", R.STRIDED, ids=R.case_id)
def test_strided_operands(dev, case):
    """q, k, v, dO as column slices of wider matrices (the trainer's fused projections), the other columns poisoned: the same bits
    as the dense call"""
    d, lq, lk, group, _ = case
    heads = R.RAGGED_HEADS
    C = heads * d
    inputs, ref = R.case_data(d, lq, lk, group)

    def embed(t):
        buf = torch.full((t.shape[0], C + 16), 1e4, dtype=torch.float16, device=dev)
        buf[:, 8:8 + C] = t.to(dev)
        return buf[:, 8:8 + C]

    dense = _run(dev, inputs, heads=heads, d=d, group=group, **_want(case))
    strided = _run(dev, inputs, heads=heads, d=d, group=group, embed=embed, **_want(case))
    assert strided["dev"][0].stride(0) == C + 16 and not strided["dev"][0].is_contiguous()
    _check(strided, ref, _tag(case) + " strided", grads_only=True)
    assert torch.equal(dense["o"], strided["o"]) and torch.equal(dense["lse"], strided["lse"])
    assert _same(dense["grads"], strided["grads"]) and _same(dense["grads_f"], strided["grads_f"])


@pytest.mark.parametrize("exp", R.SCALE_EXPONENTS)
@pytest.mark.parametrize("case", R.SCALED, ids=R.case_id)
def test_gradient_scale(dev, case, exp):
    """dO scaled by 2^-6 and 2^6 (a loss scale): the same relative bound against the reference of the scaled dO"""
    d, lq, lk, group, _ = case
    heads = R.RAGGED_HEADS
    inputs, ref = R.case_data(d, lq, lk, group, heads, R.RAGGED_BKV, exp)
    run = _run(dev, inputs, heads=heads, d=d, group=group, **_want(case))
    _check(run, ref, _tag(case) + f" dO*2^{exp}", grads_only=True)


_CHILD = r"""
import json, sys, torch
sys.path.insert(0, %r)
from tests import attn_bwd_reference as R
import i2v_adapter_unofficial_amd as pkg
k_ = pkg.kernels; dev = torch.device("cuda:0")
for d, lq, lk, group, _ in R.ENV_CASES:
    heads, bkv = R.RAGGED_HEADS, R.RAGGED_BKV
    (q, k, v, do), ref = R.case_data(d, lq, lk, group)
    C = heads * d
    qd, kd, vd, dod = (t.reshape(-1, C).to(dev) for t in (q, k, v, do))
    kw = dict(batch_q=bkv * group, lq=lq, lk=lk, heads=heads, head_dim=d, kv_group=group)
    od = k_.attention(qd, kd, k_.transpose_tokens(vd, lk), **kw)
    got = k_.attention_bwd(qd, kd, vd, od, dod, **kw)
    rel = [(g.double().cpu() - r.reshape(-1, C)).abs().max().item() / r.abs().max().item() for g, r in zip(got, (ref.dq, ref.dk, ref.dv))]
    assert all(torch.isfinite(g).all() for g in got)
    route = k_.last_attn_bwd_route()
    print("ROUTE", json.dumps([list(R.route_forms(route)), route["kv_partitions"]]))
    print("REL", d, lq, lk, group, *rel)
print("OK")
"""


@pytest.mark.parametrize("switch,value", R.ENV_SWITCHES)
def test_environment_switches_in_child_process(dev, switch, value):
    """I2V_ATTN_BWD_LDS=0 (the L2-fed two-tile forms at long lengths) and I2V_ATTN_BWD_QB=32 (32 staged queries per barrier) are
    read once per process, hence the child: the same bound against the same reference, and the switch really moved the case:
    dq2 / dkv2 / lse under I2V_ATTN_BWD_LDS=0, dkv2_lds32 under I2V_ATTN_BWD_QB=32"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD % root], env=dict(os.environ, **{switch: value}), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    lines = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("REL ")]
    assert len(lines) == len(R.ENV_CASES)
    routes = [json.loads(ln[len("ROUTE "):]) for ln in r.stdout.splitlines() if ln.startswith("ROUTE ")]
    assert len(routes) == len(R.ENV_CASES)
    for (forms, parts), case, want in zip(routes, R.ENV_CASES, SWITCHED[(switch, value)]):
        assert tuple(forms) == want != INTENDED[case[:3]] and parts == PARTS[case[:4]][1], f"{switch}={value} {case}: ran {forms} x {parts}"
    moved = {"I2V_ATTN_BWD_LDS": ("dq2", "dkv2", "lse"), "I2V_ATTN_BWD_QB": ("dq2_lds", "dkv2_lds32", "lse_lds")}[switch]
    assert all(tuple(forms[2:]) == moved for forms, _ in routes)
    from tests.parity import log_error
    for (d, lq, lk, group, *rels), case in zip(lines, R.ENV_CASES):
        assert (int(d), int(lq), int(lk), int(group)) == case[:4]
        for name, rel in zip(("dQ", "dK", "dV"), rels):
            log_error(f"attn bwd d={d} lq={lq} lk={lk} group={group} {switch}={value}: {name}", float(rel), 1.0, GRAD_REL_TOL)
            assert float(rel) <= GRAD_REL_TOL, f"{switch}={value} {case}: {name} is {float(rel):.3e} of max|ref|"
