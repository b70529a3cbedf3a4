"""With no Plus adapter loaded nothing changed: the reduced UNet's forward without an adapter and with the plain IP-Adapter, bit for bit
against digests recorded from the library of the commit before IP-Adapter Plus (tests/golden/ip_adapter_plus_parent.json,
tools/record_ip_adapter_plus_parent.py; weights and inputs come from the CPU generator)."""
import pytest

from tests.ip_adapter_plus_unchanged_cases import CASES, digests, load_golden


def test_the_file_holds_every_case():
    golden = load_golden()
    assert tuple(golden) == CASES and all(len(v) == 64 for v in golden.values())


@pytest.mark.gpu
def test_forward_is_the_parents_bit_for_bit(dev):
    golden, got = load_golden(), digests(dev)
    for name in CASES:
        assert got[name] == golden[name], f"{name}: sha256 {got[name]} differs from the recorded {golden[name]}"
