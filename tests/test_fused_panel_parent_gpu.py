"""The three persistent kernels that LayerNorm a tile of rows into an LDS panel -- csrc/ln_qkv.hip, csrc/ff_fused.hip and
csrc/motion_attn.hip, 13 instantiations -- bit for bit against the library in which each carried a private copy of the panel code.

tests/golden/fused_panel_parent.json (tools/record_clip_attention.py --cases fused_panel) holds, per case, the sha256 of the entry
point's fp16 outputs as that library computed them on MI355X.  csrc/ln_panel.h's one definition fetches and normalises the same rows
with the same arithmetic and feeds every accumulator its MFMAs in the same order, so each digest must still match: no tolerance.
The inputs are rebuilt from integers by the same numpy code the recorder used (tests/fused_panel_cases.py)."""
import pytest

from tests.fused_panel_cases import case_id, cases, load_golden, run_case

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
