"""Every case of tests/attn_route_cases.py through the real wrapper (kernels.attention: real pointers, q / k as column slices, V^T tails
of NaN, poisoned output buffers, accumulate and the fused lse) on the GPU: the launch took the kernel instantiation, the grid and the
workgroup mapping the table says (kernels.last_attn_route()), every element is finite and obeys checks (a) and (b) of
tests/attn_bounds.py against the fp64 references, the fused lse obeys its bound, nothing outside the output view was written, and a
second call on the same inputs gives the same bits.  The cases of the three other environments run in one child pytest process of this
file each (the switches are read once per process)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import attn_bounds as B
from tests import attn_route_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = G.current_env_name()          # which environment of the table this process runs under
CHILD_TIMEOUT = 300


def K():
    import i2v_adapter_unofficial_amd as pkg
    return pkg.kernels


@pytest.mark.parametrize("c", G.cases_of(ENV) if ENV else [], ids=lambda c: c["name"])
def test_case_takes_its_route_and_obeys_the_bounds(dev, c):
    k = K()
    t = B.reference(c)[0]
    res = B.run(k, dev, c, t)
    assert res["route"] == c["route"], "another kernel, grid or mapping ran than the table expects"
    assert bool(torch.isfinite(res["out"].float()).all()), "non-finite output (the V^T tails hold NaN: they must be masked)"
    print(f"{c['name']}: error / bound {B.ratios(c, res['out'], res['lse'])}")
    msg = B.check(c, res["out"])
    assert msg is None, msg
    if c["form"] == "lse":
        msg = B.check_lse(c, res["lse"])
        assert msg is None, msg
    if c["o"] != "own":
        assert res["untouched"] is True, "memory outside the output view was written"
    again = B.run(k, dev, c, t)
    assert torch.equal(again["out"].view(torch.int16), res["out"].view(torch.int16)), "two calls on the same inputs differ"
    if c["form"] == "lse":
        assert torch.equal(again["lse"].view(torch.int32), res["lse"].view(torch.int32)), "two calls give another lse"


def test_the_process_runs_under_an_environment_of_the_table():
    """under other values of the switches no case of the table applies and the file would check nothing"""
    assert ENV is not None, f"{G.SWITCHES} are set to values that match none of {list(G.ENVS)}"


if ENV == "default":
    def test_cases_of_the_other_environments_in_child_processes(dev):
        """I2V_ATTN_KVT=128 with I2V_ATTN_QT=1 and 2, I2V_ATTN_WALK=0: this file again in one child pytest process each.  A child that
        fails, is killed by a signal or runs out of time fails the test, and nothing is started after it."""
        for name in ("kvt128-qt1", "kvt128-qt2", "walk0"):
            n = len(G.cases_of(name)) + 1
            assert n >= 3
            env = {k: v for k, v in os.environ.items() if k not in G.SWITCHES}
            env.update(dict(G.ENVS[name]))
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_attn_routes_gpu.py"), "-q", "-x", "-m", "gpu",
                                "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            assert r.returncode == 0 and f"{n} passed" in r.stdout, f"{name}: the child ended with {r.returncode}:\n" + r.stdout[-4000:] + r.stderr[-2000:]
