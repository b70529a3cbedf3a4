"""What the UNet computed before IP-Adapter Plus existed, for tests/test_ip_adapter_plus_unchanged_gpu.py: the reduced UNet's forward
without an adapter and with the plain IP-Adapter, weights and inputs drawn by the CPU generator (the same numbers on every machine),
the sha256 of each fp32 output.  tests/golden/ip_adapter_plus_parent.json (tools/record_ip_adapter_plus_parent.py) is this module's
`digests` run on MI355X on the commit before the feature; it uses nothing that commit did not have."""
import hashlib
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ip_adapter_plus_parent.json")
CASES = ("no adapter, cross-frame", "no adapter, no cross-frame", "plain adapter, cross-frame")


def _sha(t):
    return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def digests(dev):
    from tests.parity import hip_unet_from_oracle, oracle_small_unet, round_fp16_, small_ip_state_dict, small_unet_inputs
    ou = oracle_small_unet(ip=False)
    inp = small_unet_inputs()
    d = lambda t: t.to(dev)
    out = {}
    with torch.no_grad():
        hu = hip_unet_from_oracle(ou, dev)
        for name, cf in ((CASES[0], True), (CASES[1], False)):
            out[name] = _sha(hu(d(inp["sample"]), d(inp["timestep"]), cf, d(inp["ctx"])).sample)
        ipsd = {k: {kk: vv.half().float() for kk, vv in v.items()} for k, v in small_ip_state_dict(ou).items()}
        hu = hip_unet_from_oracle(ou, dev, ip_state_dict=ipsd)
        out[CASES[2]] = _sha(hu(d(inp["sample"]), d(inp["timestep"]), True, d(inp["ctx"]),
                                added_cond_kwargs={"image_embeds": d(inp["image_embeds"])}).sample)
    return out


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
