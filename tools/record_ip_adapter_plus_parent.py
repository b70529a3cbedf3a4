"""Record tests/ip_adapter_plus_unchanged_cases.py's digests: the reduced UNet's forward without an adapter and with the plain
IP-Adapter, sha256 of the fp32 outputs.  tests/golden/ip_adapter_plus_parent.json is one such run on MI355X, taken on the commit BEFORE
IP-Adapter Plus (with this file and the cases module copied into that tree); tests/test_ip_adapter_plus_unchanged_gpu.py holds every
later library to it.

Run once on the GPU:  python tools/record_ip_adapter_plus_parent.py --out tests/golden/ip_adapter_plus_parent.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from tests.ip_adapter_plus_unchanged_cases import GOLDEN, digests

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the recorder runs the kernels: there is nothing to record without a GPU"
    dev = torch.device("cuda:0")
    got = digests(dev)
    assert got == digests(dev), "the forward is not deterministic"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    for k, v in got.items():
        print(k, v)


if __name__ == "__main__":
    main()
