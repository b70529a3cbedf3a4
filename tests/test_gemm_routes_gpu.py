"""Every case of tests/gemm_route_cases.py through the real wrappers (kernels.gemm / conv3x3 / project_vt: real pointers, the real
split-K workspace) on the GPU: the launch took the kernel instantiation the table says (kernels.last_gemm_route()), the result obeys
the derived per-element bound of tests/gemm_bounds.py against the fp64 reference, and nothing outside the output view was written.
Cases under non-default switches run in two child pytest processes of this file (the switches are read once per process)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_bounds as B
from tests import gemm_route_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = G.current_env_name()          # which environment of the table this process runs under
CHILD_TIMEOUT = 600


def K():
    import i2v_adapter_unofficial_amd as pkg
    return pkg.kernels


@pytest.mark.parametrize("c", G.cases_of(ENV) if ENV else [], ids=lambda c: c["name"])
def test_case_takes_its_route_and_obeys_the_bound(dev, c):
    k = K()
    t, _, _ = B.reference(c)
    res = B.run(k, dev, c, t, attach_workspace=c["ws"])
    assert res["route"] == G.expected_route(k._lib, c), "another kernel ran than the table expects"
    msg = B.check(c, res["out"], res["lo"])
    assert msg is None, msg
    o = G.canon(c)
    if c["op"] == "gemm" and o["store"] in ("rm", "perm") and not o["lo"]:
        assert res["untouched"] is True, "memory outside the output view was written"
    if o["gn"]:
        _check_groupnorm_statistics(k, dev, c, o, res)


def _check_groupnorm_statistics(k, dev, c, o, res):
    """the GroupNorm partials of the convolution's epilogue, through the norm that consumes them, against fp64 GroupNorm of the
    convolution's own fp16 output (as test_groupnorm_statistics_from_the_conv_epilogue)"""
    cv, N, groups = o["conv"], o["N"], o["gn"]
    assert res["stats"] is not None, "an un-split 3x3 convolution of whole row tiles writes the partials"
    part, rows = res["stats"]
    assert rows == c["route"]["rows"] and tuple(part.shape) == (cv["n"], cv["oh"] * cv["ow"] // rows, groups, 2) and bool(torch.isfinite(part).all())
    g = torch.Generator().manual_seed(N)
    ga, be = (1 + 0.3 * torch.randn(N, generator=g)).half(), (0.3 * torch.randn(N, generator=g)).half()
    y = k.groupnorm(res["raw"], ga.to(dev), be.to(dev), groups, 1e-6, silu=True, stats=res["stats"]).cpu().double()
    ref = F.silu(F.group_norm(res["raw"].cpu().double().permute(0, 3, 1, 2), groups, ga.double(), be.double(), eps=1e-6)).permute(0, 2, 3, 1)
    err, tol = (y - ref).abs(), 2e-3 * ref.abs() + 2e-3 * ref.abs().max()
    assert bool((err <= tol).all()), f"GroupNorm from the convolution's partials: max err {float(err.max()):.3e}"


if ENV == "default":
    def test_cases_under_switches_in_child_processes(dev):
        """I2V_GEMM_PERSIST=1, then I2V_GEMM_DEEP=0 I2V_GEMM_SPLIT256=0 (each with the generic kernel's tile override its cases name):
        this file again in a child pytest process per environment, one after the other.  A child that fails, is killed by a signal
        or runs out of time fails the test, and nothing is started after it."""
        for name in ("persist", "deep0_split256_0"):
            n = len(G.cases_of(name))
            assert n >= 5
            env = {k: v for k, v in os.environ.items() if k not in G.SWITCHES}
            env.update(dict(G.ENVS[name]))
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gemm_routes_gpu.py"), "-q", "-x", "-m", "gpu",
                                "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            assert r.returncode == 0 and f"{n} passed" in r.stdout, f"child `{name}` ended with {r.returncode}:\n" + r.stdout[-4000:] + r.stderr[-2000:]
