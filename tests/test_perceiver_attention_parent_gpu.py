"""The Resampler's attention entry point, bit for bit against the library that had a kernel of its own for it; and the entry points
that now share one instantiation, against each other.

tests/golden/perceiver_attention_parent.json (tools/record_clip_attention.py --cases perceiver) holds, per case, the sha256 of the fp16
output of `kernels.perceiver_attention` as that library's csrc/perceiver_attention.hip computed it on MI355X.
csrc/short_attention.hip's one kernel fills LDS with the same K and V^T and does every query's arithmetic in the same order, so each
digest must still match: no tolerance.  The inputs are rebuilt from integers by the same numpy code the recorder used
(tests/perceiver_attention_cases.py)."""
import pytest
import torch

from tests.clip_attention_cases import qkv_values
from tests.perceiver_attention_cases import case_id, cases, load_golden, run_case

GOLDEN = load_golden()


def test_the_file_holds_every_case():
    """the recorded cases are the module's list: none dropped, none added, the parameters unchanged"""
    assert [{k: v for k, v in e.items() if k != "sha256"} for e in GOLDEN] == cases()
    assert all(len(e["sha256"]) == 64 for e in GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", GOLDEN, ids=case_id)
def test_output_is_the_parents_bit_for_bit(dev, entry):
    import i2v_adapter_unofficial_amd as pkg
    got = run_case(pkg.kernels, dev, entry)
    assert got == entry["sha256"], f"{case_id(entry)}: sha256 {got} differs from the recorded {entry['sha256']}"


@pytest.mark.gpu
@pytest.mark.parametrize("L", [17, 64])
def test_self_attention_through_either_entry_is_one_computation(dev, L):
    """the vision tower's entry and the Resampler's with q = source A = the packed buffer and no source B run the same
    instantiation <64, not causal> on the same operands: equal bit for bit"""
    import i2v_adapter_unofficial_amd as pkg
    B, heads, d = 2, 2, 64
    hidden = heads * d
    qkv = qkv_values(B * L, heads, d, 2, seed=L).to(dev)
    tower = pkg.kernels.clip_vision_attention(qkv, batch=B, length=L, heads=heads, head_dim=d)
    resampler = pkg.kernels.perceiver_attention(qkv, qkv, None, batch=B, n_q=L, len_a=L, len_b=0, heads=heads, head_dim=d, ka_off=hidden,
                                                va_off=2 * hidden)
    assert torch.isfinite(tower).all() and torch.equal(tower, resampler)
