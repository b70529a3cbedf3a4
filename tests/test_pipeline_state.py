"""The captured step's per-sample inputs on the host side (no GPU): `SAMPLE_INPUTS` is the one list behind the copy-in of a graph-cache
hit (`_copy_sample_inputs`) and behind the shape part of `_graph_key`; `_schedule_tables` makes the tables of a schedule for round 0 of
a call and for FreeInit's fast-sampling rounds.  The bits on the GPU are tests/test_pipeline_state_gpu.py's."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import controlnet_reference as CR  # noqa: E402
from tests.parity import SMALL_UNET  # noqa: E402

DECLARED = {"latents", "cond", "t_table", "coef", "ctx_text", "ctx_ip", "noise", "cn_cond", "cn_scale", "t2i_feats", "t2i_scale",
            "v2v_source", "v2v_noise", "v2v_mask", "v2v_coef"}


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def P():
    return pkg().pipeline_i2v_adapter


def _state(seed, steps=3):
    """a full fake state of CPU tensors of a few elements: every declared entry, t2i_feats a tuple, and the scalars of the key"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=g)
    st = dict(latents=r(1, 2, 4, 2, 2), cond=r(1, 4, 2, 2), t_table=r(steps), coef=r(steps, 4), ctx_text=r(2, 3, 4).half(),
              ctx_ip=r(2, 2, 4).half(), noise=r(steps, 1, 2, 4, 2, 2), cn_cond=r(4, 2, 2, 8).half(), cn_scale=r(steps),
              t2i_feats=(r(2, 2, 2, 8).half(), r(2, 1, 1, 16).half()), t2i_scale=r(steps), v2v_source=r(1, 2, 4, 2, 2),
              v2v_noise=r(1, 2, 4, 2, 2), v2v_mask=r(1, 2, 1, 2, 2), v2v_coef=r(steps, 2))
    assert set(st) == DECLARED
    st.update(copies=2, num_frames=2, guidance=7.5, step_idx=torch.full((1,), 2, dtype=torch.int32))
    return st


def _tensors(st):
    """(name, index or None, tensor) of every declared tensor of a state"""
    for name in sorted(DECLARED):
        v = st.get(name)
        if isinstance(v, tuple):
            yield from ((name, i, t) for i, t in enumerate(v))
        elif v is not None:
            yield name, None, v


def test_the_declaration_lists_the_fifteen_inputs_and_not_the_steps_history():
    assert isinstance(P().SAMPLE_INPUTS, tuple) and set(P().SAMPLE_INPUTS) == DECLARED and len(P().SAMPLE_INPUTS) == len(DECLARED)
    assert "x0_prev" not in P().SAMPLE_INPUTS and "step_idx" not in P().SAMPLE_INPUTS


def test_copy_in_copies_every_declared_entry_in_place():
    st, gst = _state(1), _state(2)
    gst["x0_prev"] = torch.ones(3)
    ptrs = {(n, i): t.data_ptr() for n, i, t in _tensors(gst)}
    step_ptr = gst["step_idx"].data_ptr()
    assert all(not torch.equal(a, b) for (_, _, a), (_, _, b) in zip(_tensors(st), _tensors(gst)))
    P()._copy_sample_inputs(gst, st)
    for (n, i, got), (_, _, want) in zip(_tensors(gst), _tensors(st)):
        assert torch.equal(got, want), (n, i)
        assert got.data_ptr() == ptrs[(n, i)] and got.data_ptr() != want.data_ptr(), (n, i)
    assert int(gst["step_idx"]) == 0 and gst["step_idx"].data_ptr() == step_ptr and int(st["step_idx"]) == 2
    assert torch.equal(gst["x0_prev"], torch.ones(3))


@pytest.mark.parametrize("absent", sorted(DECLARED - {"latents"}))
def test_copy_in_leaves_what_the_sample_does_not_hold(absent):
    st, gst = _state(1), _state(2)
    before = [t.clone() for n, _, t in _tensors(gst) if n == absent]
    if absent in ("noise", "ctx_ip"):
        st[absent] = None           # (an entry may be None as well as missing)
    else:
        del st[absent]
    P()._copy_sample_inputs(gst, st)
    assert all(torch.equal(a, b) for a, b in zip(before, [t for n, _, t in _tensors(gst) if n == absent]))
    assert all(torch.equal(got, dict(((n, i), t) for n, i, t in _tensors(st))[(n, i)]) for n, i, got in _tensors(gst) if n != absent)
    assert int(gst["step_idx"]) == 0


@pytest.fixture(scope="module")
def pipe():
    p = pkg()
    return p.I2VAdapterPipeline(unet=p.UNetMotionCrossFrameAttnModel(**SMALL_UNET), controlnet=p.ControlNetModel(**CR.small_config()))


def _grown(t):
    """the same tensor with one more row"""
    return torch.cat([t, t[:1]])


CASES = [(n, None) for n in sorted(DECLARED - {"t2i_feats"})] + [("t2i_feats", 0), ("t2i_feats", 1)]


@pytest.mark.parametrize("name,index", CASES)
def test_the_key_holds_the_shape_of_every_declared_entry(pipe, name, index):
    st = _state(1)
    key = pipe._graph_key(st)
    other = dict(st)
    if index is None:
        other[name] = _grown(st[name])
    else:
        other[name] = tuple(_grown(t) if i == index else t for i, t in enumerate(st[name]))
    assert pipe._graph_key(other) != key, f"a cache hit would copy {name} into a buffer of another shape"
    if name != "latents":           # (absent is not present: the step has other launches)
        assert pipe._graph_key({k: v for k, v in st.items() if k != name}) != key


def test_the_key_holds_dtypes_and_no_contents(pipe):
    st = _state(1)
    key = pipe._graph_key(st)
    assert pipe._graph_key(dict(st, v2v_mask=st["v2v_mask"].half())) != key
    assert pipe._graph_key(dict(st, t2i_feats=(st["t2i_feats"][0], st["t2i_feats"][1].float()))) != key
    other = _state(2)
    assert all(not torch.equal(a, b) for (_, _, a), (_, _, b) in zip(_tensors(st), _tensors(other)))
    assert pipe._graph_key(other) == key, "two samples of one shape do not share a captured step"
    assert pipe._graph_key(dict(other, step_idx=torch.zeros(1, dtype=torch.int32), x0_prev=torch.zeros(7))) == key
    hash(key)


def test_the_key_of_a_partial_state(pipe):
    """what the benchmark and the probes hold: no optional entry at all"""
    st = {k: v for k, v in _state(1).items() if k in ("latents", "t_table", "coef", "ctx_text", "copies", "num_frames", "guidance")}
    key = pipe._graph_key(st)
    assert key == pipe._graph_key(dict(st)) and key != pipe._graph_key(dict(st, guidance=1.5))
    assert key != pipe._graph_key(dict(st, coef=_grown(st["coef"])))


@pytest.mark.parametrize("kind", ["ddim", "dpmsolver++", "lcm"])
def test_schedule_tables_are_the_functions_called_directly(kind):
    p = pkg()
    from i2v_adapter_unofficial_amd.controlnet import controlnet_keep_table
    from i2v_adapter_unofficial_amd.t2i_adapter import adapter_scale_table
    sched = {"ddim": p.DDIMScheduler, "dpmsolver++": p.DPMSolverMultistepScheduler, "lcm": p.LCMScheduler}[kind]()
    pipe = p.I2VAdapterPipeline(unet=p.UNetMotionCrossFrameAttnModel(**SMALL_UNET), scheduler=sched)
    cn_args, t2i_args = (0.8, 0.0, 0.5), (0.6, 0.5)
    full = dict(latents=torch.zeros(1, 2, 4, 2, 2), cn_cond=torch.zeros(1), cn_args=cn_args, t2i_feats=(torch.zeros(1),), t2i_args=t2i_args,
                v2v_mask=torch.zeros(1))
    plain = dict(latents=torch.zeros(1, 2, 4, 2, 2), cn_args=cn_args, t2i_args=t2i_args)
    eta = 0.0
    for steps in (4, 7):
        sched.set_timesteps(steps)
        timesteps = sched.timesteps
        assert len(timesteps) == steps
        for st in (full, plain):
            pipe._schedule_tables(st, timesteps, eta)
            assert st["t_table"].dtype == torch.float32 and torch.equal(st["t_table"], timesteps.to(torch.float32))
            assert torch.equal(st["coef"], sched.step_coefficients(timesteps, eta)) and st["coef"].shape[0] == steps
        assert torch.equal(full["cn_scale"], torch.tensor(controlnet_keep_table(steps, *cn_args), dtype=torch.float32))
        assert torch.equal(full["t2i_scale"], torch.tensor(adapter_scale_table(steps, *t2i_args), dtype=torch.float32))
        assert torch.equal(full["v2v_coef"], pipe.renoise_table(timesteps)) and full["v2v_coef"].dtype == torch.float32
        assert [tuple(full[k].shape) for k in ("t_table", "cn_scale", "t2i_scale", "v2v_coef")] == [(steps,), (steps,), (steps,), (steps, 2)]
        # the windows are inside the schedule: the tables are not all one value
        assert len(set(full["cn_scale"].tolist())) == 2 and len(set(full["t2i_scale"].tolist())) == 2
        # a state without the features gets no table of theirs
        assert not {"cn_scale", "t2i_scale", "v2v_coef"} & set(plain)
    if kind == "ddim":
        pipe._schedule_tables(full, timesteps, 0.5)
        assert torch.equal(full["coef"], sched.step_coefficients(timesteps, 0.5)) and not torch.equal(full["coef"], plain["coef"])
