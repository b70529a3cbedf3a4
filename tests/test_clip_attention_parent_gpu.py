"""Both CLIP attention entry points, bit for bit against the library that had one attention kernel per tower.

tests/golden/clip_attention_parent.json (tools/record_clip_attention.py) holds, per case, the sha256 of the fp16 output of
`kernels.clip_attention` / `kernels.clip_vision_attention` as that library computed it on MI355X.  csrc/short_attention.hip's one kernel
does every query's arithmetic in the same order -- the causal instantiation skips the key tiles right of the diagonal, which add an
exact + 0.f to the row sum -- so each digest must still match: no tolerance.  The inputs are rebuilt from integers by the same numpy
code the recorder used (tests/clip_attention_cases.py)."""
import pytest

from tests.clip_attention_cases import case_id, cases, load_golden, run_case

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
