"""Record what kernel entry points compute, bit for bit: every case of a cases module through its entry point, the sha256 of each
output's fp16 bytes written next to the case's parameters.

  --cases clip        tests/clip_attention_cases.py through `kernels.clip_attention` / `kernels.clip_vision_attention`.
                      tests/golden/clip_attention_parent.json is one such run, taken on the library BEFORE the two towers' attention
                      kernels were merged; tests/test_clip_attention_parent_gpu.py holds every later library to it.
  --cases perceiver   tests/perceiver_attention_cases.py through `kernels.perceiver_attention`.
                      tests/golden/perceiver_attention_parent.json is one such run, taken on the library BEFORE the Resampler's
                      attention kernel and the towers' were merged into csrc/short_attention.hip;
                      tests/test_perceiver_attention_parent_gpu.py holds every later library to it.
  --cases fused_panel tests/fused_panel_cases.py through `kernels.ln_qkv`, `kernels.ff_fused`, `kernels.motion_attn`,
                      `kernels.motion_attn_wide` and `kernels.cross_attn_fused`.  tests/golden/fused_panel_parent.json is one such
                      run, taken on the library BEFORE the three kernels' LayerNorm panel code moved into csrc/ln_panel.h;
                      tests/test_fused_panel_parent_gpu.py holds every later library to it.

Run once on the GPU (I2V_LIB_PATH selects the library to record):  python tools/record_clip_attention.py --cases perceiver
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {"clip": "tests.clip_attention_cases", "perceiver": "tests.perceiver_attention_cases", "fused_panel": "tests.fused_panel_cases"}


def main():
    import torch

    import i2v_adapter_unofficial_amd as pkg

    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", choices=tuple(CASES), default="clip")
    ap.add_argument("--out", default=None, help="default: the cases module's GOLDEN")
    args = ap.parse_args()
    mod = importlib.import_module(CASES[args.cases])
    out = args.out or mod.GOLDEN
    assert torch.cuda.is_available(), "the recorder runs the kernels: there is nothing to record without a GPU"
    dev = torch.device("cuda:0")
    entries = []
    for c in mod.cases():
        entries.append(dict(c, sha256=mod.run_case(pkg.kernels, dev, c)))
        print(mod.case_id(c), entries[-1]["sha256"], flush=True)
        assert entries[-1]["sha256"] == mod.run_case(pkg.kernels, dev, c), "the kernel is not deterministic"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(entries, f, indent=1)
        f.write("\n")
    print("wrote", out, len(entries), "cases")


if __name__ == "__main__":
    main()
