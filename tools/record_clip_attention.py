"""Record what the two CLIP attention entry points compute, bit for bit: every case of tests/clip_attention_cases.py through
`kernels.clip_attention` / `kernels.clip_vision_attention`, the sha256 of each output's fp16 bytes written next to the case's
parameters.  tests/golden/clip_attention_parent.json is one such run, taken on the library BEFORE the two towers' attention kernels
were merged into csrc/clip_attention.hip; tests/test_clip_attention_parent_gpu.py holds every later library to it.

Run once on the GPU:  python tools/record_clip_attention.py --out tests/golden/clip_attention_parent.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    import i2v_adapter_unofficial_amd as pkg
    from tests.clip_attention_cases import GOLDEN, case_id, cases, run_case

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the recorder runs the kernels: there is nothing to record without a GPU"
    dev = torch.device("cuda:0")
    entries = []
    for c in cases():
        entries.append(dict(c, sha256=run_case(pkg.kernels, dev, c)))
        print(case_id(c), entries[-1]["sha256"], flush=True)
        assert entries[-1]["sha256"] == run_case(pkg.kernels, dev, c), "the kernel is not deterministic"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(entries, f, indent=1)
        f.write("\n")
    print("wrote", args.out, len(entries), "cases")


if __name__ == "__main__":
    main()
