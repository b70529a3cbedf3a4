"""CPU checks of tests/attn_bwd_reference.py: the float64 reference against torch autograd, the launch mirror and the coverage the
case tables of tests/test_attention_bwd_edges_gpu.py are meant to give, and the reachability of the bound asserted there: an
emulation of the kernels' roundings stays within HALF of it on exactly the inputs the GPU tests use."""
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


INTENDED = {   # (d, lq, lk) -> (ks, dt, dq_form, dkv_form, lse_form), written down by hand from launch_bwd / i2v_attention_lse_f32
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
}
SHORT_CLASS = {40: (2, 3), 80: (3, 5), 160: (5, 10), 16: (1, 2)}


def test_forms_returns_the_intended_form_for_every_case():
    for case in R.RAGGED + R.STRIDED + R.SCALED + R.ENV_CASES:
        d, lq, lk = case[:3]
        assert R.forms(d, lq, lk) == INTENDED[(d, lq, lk)], case
    for heads, d, f in R.SHORT + [R.ONE_FRAME]:
        assert R.forms(d, f, f) == SHORT_CLASS[d] + ("dq1", "dkv1", "lse"), (d, f)
    assert all(c in R.RAGGED for c in R.STRIDED)
    assert sorted({R.forms(*c[:3])[2] for c in R.STRIDED}) == ["dq1", "dq2", "dq2_lds"]
    # the environment switches (read by the library once per process) move the long cases to the other forms
    assert R.forms(40, 600, 601, lds=False) == (2, 3, "dq2", "dkv2", "lse")
    assert R.forms(96, 517, 523, lds=False) == (3, 6, "dq2", "dkv2", "lse")
    assert R.forms(40, 600, 601, qb64=False) == (2, 3, "dq2_lds", "dkv2_lds32", "lse_lds")
    assert R.forms(96, 517, 523, qb64=False) == (3, 6, "dq2_lds", "dkv2_lds32", "lse_lds")
    # class boundaries and thresholds
    assert [R.forms(d, 64, 64)[:2] for d in (32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 128, 136, 160)] == \
        [(1, 2), (2, 3), (2, 3), (2, 4), (2, 4), (3, 5), (3, 5), (3, 6), (3, 6), (4, 8), (4, 8), (5, 10), (5, 10)]
    assert R.forms(40, 511, 63)[2:] == ("dq1", "dkv1", "lse") and R.forms(40, 512, 63)[2:] == ("dq2", "dkv1", "lse")
    assert R.forms(40, 512, 64)[2:] == ("dq2_lds", "dkv1", "lse_lds") and R.forms(128, 512, 512)[2:] == ("dq1", "dkv1", "lse")
    assert [R.forms(40, lq, 512)[3] for lq in (63, 64, 127, 128)] == ["dkv2", "dkv2_lds32", "dkv2_lds32", "dkv2_lds64"]
    assert R.forms(104, 600, 600)[4] == "lse" and R.forms(96, 600, 600)[4] == "lse_lds"
    with pytest.raises(ValueError):
        R.forms(168, 64, 64)


def _parts(case, bkv=R.RAGGED_BKV):
    d, lq, lk, group = case[:4]
    return R.dkv_partitions(bkv * group, group, R.RAGGED_HEADS, d, lq, lk)


def coverage_gaps(table):
    """what the ragged table fails to cover, as a list of sentences (empty = complete)"""
    gaps = []
    f = {c: R.forms(*c[:3]) for c in table}
    dkv = [c for c in table if c[4]]                 # the cases that launch the dK / dV sweep
    ragged8_q, ragged8_k = (lambda c: c[1] % 8 != 0), (lambda c: c[2] % 8 != 0)
    for dmax, ks, dt in R.CLASSES:
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
        if not any(f[c][3] == form and _parts(c) > 1 and c[2] % 32 != 0 for c in dkv):
            gaps.append(f"{form} has no case with kv_partitions > 1 and a ragged lk")
    # a two-tiles-per-wave form whose last wave has a partly / a wholly masked second tile (32 rows per wave: rows % 32 in 17..31 / 1..16)
    for idx, form_idx, name in ((1, 2, "dq"), (2, 3, "dkv")):
        two = [c for c in (table if idx == 1 else dkv) if f[c][form_idx] not in ("dq1", "dkv1")]
        if not any(0 < c[idx] % 32 <= 16 for c in two):
            gaps.append(f"no two-tile {name} case with a wholly masked second tile")
        if not any(c[idx] % 32 > 16 for c in two):
            gaps.append(f"no two-tile {name} case with a partly masked second tile")
    return gaps


def test_tables_cover_every_class_form_and_tail():
    assert coverage_gaps(R.RAGGED) == []
    assert len(set(R.RAGGED)) == len(R.RAGGED)
    # the check has teeth: without its only case a form or class is reported
    for only, what in (((16, 45, 515, 1, True), "dkv2 has no case with lq % 8 != 0"),
                       ((104, 70, 130, 1, True), "class (KS 4, DT 8) has no case with d below 128"),
                       ((32, 600, 601, 1, True), "attn_lse_lds_kernel<1> has no case"),
                       ((24, 603, 40, 1, True), "dq2 has no case with lq % 8 != 0"),
                       ((88, 96, 643, 4, True), "dkv2_lds32 has no case with kv_partitions > 1 and a ragged lk")):
        assert what in coverage_gaps([c for c in R.RAGGED if c != only]), only
    # the batch-independence check compares a two-entry call with a one-entry call: the same partition count in both
    for case in R.RAGGED:
        assert _parts(case, bkv=2) == _parts(case, bkv=1), case
    # short sequences as the issue lists them
    assert {(hh, d) for hh, d, _ in R.SHORT} == {(8, 40), (8, 80), (2, 160), (4, 16)}
    assert sorted(f for hh, d, f in R.SHORT if d == 40) == [2, 3, 5, 8, 12, 16, 24, 32]
    for d in (80, 160, 16):
        assert sorted(f for _, dd, f in R.SHORT if dd == d) == [3, 16, 24]


def test_partition_mirror_follows_the_package():
    pkg = pytest.importorskip("i2v_adapter_unofficial_amd")
    for case in R.RAGGED + R.SCALED + R.ENV_CASES:
        d, lq, lk, group = case[:4]
        for bkv in (1, 2):
            args = (bkv * group, group, R.RAGGED_HEADS, d, lq, lk)
            assert R.dkv_partitions(*args) == pkg.kernels.dkv_partitions(*args), case
    for heads, d, f in R.SHORT:
        assert pkg.kernels.dkv_partitions(R.SHORT_PIXELS, 1, heads, d, f, f) == 1


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
