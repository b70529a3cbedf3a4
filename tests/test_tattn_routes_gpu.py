"""Every case of tests/tattn_route_cases.py through the real wrapper (kernels.temporal_attention: real pointers, strided q / k, V^T
tails of NaN, poisoned output buffers) on the GPU: the launch took the kernel instantiation the table says
(kernels.last_tattn_route()), every element obeys the derived bound of tests/tattn_bounds.py against the fp64 reference and is finite,
nothing outside the output view was written, and a second call on the same inputs gives the same bits.  The I2V_TATTN_LDS=0 cases
run in one child pytest process of this file (the switch is read once per process)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import tattn_bounds as B
from tests import tattn_route_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = G.current_env_name()          # which environment of the table this process runs under
CHILD_TIMEOUT = 300


def K():
    import i2v_adapter_unofficial_amd as pkg
    return pkg.kernels


@pytest.mark.parametrize("c", G.cases_of(ENV) if ENV else [], ids=lambda c: c["name"])
def test_case_takes_its_route_and_obeys_the_bound(dev, c):
    k = K()
    t = B.reference(c)[0]
    res = B.run(k, dev, c, t)
    assert res["route"] == c["route"], "another kernel ran than the table expects"
    assert bool(torch.isfinite(res["out"].float()).all()), "non-finite output (the V^T tails hold NaN: they must be masked)"
    msg = B.check(c, res["out"])
    assert msg is None, msg
    if c["o"] != "own":
        assert res["untouched"] is True, "memory outside the output view was written"
    again = B.run(k, dev, c, t)
    assert torch.equal(again["out"].view(torch.int16), res["out"].view(torch.int16)), "two calls on the same inputs differ"


def test_the_default_output_and_the_out_argument_agree(dev):
    """without `out=` the wrapper allocates [rows, C] itself: same kernel, same bits; an `out` whose row stride is no multiple of 4
    is refused before any launch"""
    k = K()
    c = next(x for x in G.cases_of(ENV or "default") if x["o"] == "own")
    t = B.reference(c)[0]
    a, b = B.run(k, dev, c, t), B.run(k, dev, c, t, with_out=False)
    assert a["route"] == b["route"] and torch.equal(a["out"].view(torch.int16), b["out"].view(torch.int16))
    rows, Cc = c["n_pixels"] * c["frames"], c["heads"] * c["head_dim"]
    q, kk = t["q"].reshape(rows, Cc).to(dev), t["k"].reshape(rows, Cc).to(dev)
    vt = torch.zeros((c["n_pixels"], Cc, c["vt_ld"]), dtype=torch.float16, device=dev)
    bad = torch.zeros((rows, Cc + 2), dtype=torch.float16, device=dev)
    with pytest.raises(ValueError, match="row stride"):
        k.temporal_attention(q, kk, vt, n_pixels=c["n_pixels"], frames=c["frames"], heads=c["heads"], head_dim=c["head_dim"], out=bad[:, :Cc])
    assert not bool(bad.any())


if ENV == "default":
    def test_cases_without_the_lds_form_in_a_child_process(dev):
        """I2V_TATTN_LDS=0: this file again in one child pytest process.  A child that fails, is killed by a signal or runs out of
        time fails the test, and nothing is started after it."""
        n = len(G.cases_of("lds0")) + 1
        assert n >= 6
        env = {k: v for k, v in os.environ.items() if k not in G.SWITCHES}
        env.update(dict(G.ENVS["lds0"]))
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_tattn_routes_gpu.py"), "-q", "-x", "-m", "gpu",
                            "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        assert r.returncode == 0 and f"{n} passed" in r.stdout, f"the child ended with {r.returncode}:\n" + r.stdout[-4000:] + r.stderr[-2000:]
