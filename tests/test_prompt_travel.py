"""Prompt travel on the host: the keyframe rules and their errors, the (lo, hi, w) tables of the interpolation launch against the
frame-by-frame restatement (tests/prompt_travel_reference.py), the callback path, the 4-D `prompt_embeds` checks, the per-frame oracle
UNet, the ABI of i2v_interp_rows_f16 with its host-side argument checks, the refusals, the driver's flag -- and the error bound the GPU
test holds the kernel to, shown here to pass a faithful fp32 evaluation and to reject two wrong ones.  No kernel is launched."""
import os
import re

import numpy as np
import pytest
import torch

from tests import prompt_travel_reference as R
from tests.parity import ROOT, SMALL_UNET

f16 = torch.float16


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def PT():
    from i2v_adapter_unofficial_amd import prompt_travel
    return prompt_travel


# ---------------------------------------------------------------------------------------------------------- the keyframe rules
def test_keyframes_are_sorted_and_checked():
    assert PT().check_keyframes({3: "b", 0: "a"}, 4) == R.keyframes({3: "b", 0: "a"}, 4) == [0, 3]
    assert PT().check_keyframes({0: "a"}, 1) == [0]
    assert PT().check_keyframes({0: "a", np.int64(2): "b"}, 3) == [0, 2]


@pytest.mark.parametrize("prompt,frames,key", [
    ({1: "a", 3: "b"}, 4, "1"),              # the first key is not 0
    ({-1: "a", 0: "b"}, 4, "-1"),            # a negative key sorts first
    ({0: "a", 4: "b"}, 4, "4"),              # the last key is not a frame
    ({0: "a", 9: "b", 2: "c"}, 8, "9"),
    ({0: "a", "2": "b"}, 4, "'2'"),          # a str key
    ({0: "a", 1.0: "b"}, 4, "1.0"),          # a float key
    ({0: "a", True: "b"}, 4, "True"),        # a bool is not a frame index
    ({0: "a", 2: None}, 4, "2"),             # a value that is not a str
    ({0: "a", 2: ["b"]}, 4, "2"),
])
def test_bad_keyframes_raise_value_error_naming_the_key(prompt, frames, key):
    for fn in (PT().check_keyframes, R.keyframes):
        with pytest.raises(ValueError, match=re.escape(key)):
            fn(prompt, frames)
    with pytest.raises(ValueError, match=re.escape(key)):
        PT().normalize_prompt(prompt, frames)
    with pytest.raises(ValueError, match=re.escape(key)):
        PT().normalize_prompt(["plain", prompt], frames)


def test_empty_dict_and_wrong_types_raise():
    with pytest.raises(ValueError, match="empty"):
        PT().check_keyframes({}, 4)
    with pytest.raises(ValueError, match="`prompt` has to be of type"):
        PT().normalize_prompt(7, 4)
    with pytest.raises(ValueError, match=r"`prompt\[1\]` has to be a `str` or a `dict`"):
        PT().normalize_prompt(["a", 7], 4)


def test_normalize_prompt_sends_single_key_dicts_down_the_plain_path():
    n = PT().normalize_prompt
    assert n("a", 4) == ("a", False) and n(None, 4) == (None, False)
    assert n({0: "a"}, 4) == ("a", False)                                    # today's str path: same launches, same bits
    assert n([{0: "a"}, "b"], 4) == (["a", "b"], False)
    d = {0: "a", 3: "b"}
    assert n(d, 4) == (d, True) and n(["x", d], 4) == (["x", d], True)
    assert PT().per_sample_keyframes("a", 2, 4) == [{0: "a"}, {0: "a"}]
    assert PT().per_sample_keyframes([d, "b"], 2, 4) == [d, {0: "b"}]
    with pytest.raises(ValueError, match="3 entries for a batch of 2"):
        PT().per_sample_keyframes(["a", "b", "c"], 2, 4)


# ---------------------------------------------------------------------------------------------------------- the tables
CASES = {
    "one keyframe": ([[0]], 5),
    "two keyframes": ([[0, 4]], 5),
    "three keyframes, shared boundary": ([[0, 3, 7]], 8),
    "last key below F - 1": ([[0, 2]], 6),
    "batch of two dicts with different keys": ([[0, 3], [0, 1, 5]], 6),
    "neighbouring keyframes": ([[0, 1, 2]], 3),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("repeats", [1, 2])
def test_tables_against_the_frame_by_frame_restatement(name, repeats):
    key_lists, frames = CASES[name]
    lo, hi, w, n_src = PT().batch_tables(key_lists, frames, repeats=repeats)
    rlo, rhi, rw = R.batch_frame_sources(key_lists, frames, repeats=repeats)
    assert n_src == sum(len(k) for k in key_lists)
    assert lo.dtype == hi.dtype == np.int32 and w.dtype == np.float32 and len(lo) == len(key_lists) * repeats * frames
    assert np.array_equal(w, rw)
    # where w == 0 only lo is read, so only lo must agree there (and hi must still be a valid row)
    assert np.array_equal(lo, rlo) and np.array_equal(hi[w != 0], rhi[w != 0])
    assert hi.min() >= 0 and hi.max() < n_src


def test_table_values():
    lo, hi, w = PT().travel_tables([0, 4], 5)
    assert lo.tolist() == [0, 0, 0, 0, 1] and hi[1:4].tolist() == [1, 1, 1] and w.tolist() == [0.0, 0.25, 0.5, 0.75, 0.0]
    lo, hi, w = PT().travel_tables([0, 3, 7], 8)                             # the shared boundary: frame 3 is keyframe 1 alone
    assert (lo[3], hi[3], w[3]) == (1, 1, 0.0) and (lo[7], hi[7], w[7]) == (2, 2, 0.0)
    assert w[1] == np.float32(np.linspace(0, 1, 4)[1]) and w[5] == np.float32(0.5)
    lo, hi, w = PT().travel_tables([0, 2], 6)                                # the last prompt is held
    assert lo[2:].tolist() == [1] * 4 and w[2:].tolist() == [0.0] * 4
    lo, hi, w = PT().travel_tables([0], 3, base=5)
    assert lo.tolist() == hi.tolist() == [5, 5, 5] and w.tolist() == [0.0] * 3


def test_interpolation_reference_and_callback():
    g = torch.Generator().manual_seed(0)
    e = torch.randn(3, 2, 8, generator=g)
    out = R.interpolate(e, [0, 2, 5], 7)
    assert torch.equal(out[0], e[0].double()) and torch.equal(out[2], e[1].double()) and torch.equal(out[5], e[2].double())
    assert torch.equal(out[6], e[2].double())                                # held
    assert torch.allclose(out[1], 0.5 * (e[0] + e[1]).double())
    calls = []

    def cb(s, t, a, b):
        calls.append((s, t))
        return torch.stack([a * (1 + i) for i in range(t - s + 1)])
    got = R.interpolate(e, [0, 2, 5], 7, callback=cb)
    assert calls == [(0, 2), (2, 5)]
    assert torch.equal(got[1], (2 * e[0]).double()) and torch.equal(got[2], e[1].double())      # the later segment's first row wins
    assert torch.equal(got[5], (4 * e[1]).double()) and torch.equal(got[6], e[2].double())


# ---------------------------------------------------------------------------------------------------------- the bound
def _fp32_eval(src, lo, hi, w, swap=False, shift=0):
    """the kernel's arithmetic on the host: fp32, one rounding to fp16 -- or a wrong evaluation (weights swapped; the neighbouring
    frame's weight)"""
    w = np.roll(np.asarray(w, dtype=np.float32), shift)
    rows = []
    for a, b, ww in zip(lo, hi, w):
        ww = torch.tensor(ww, dtype=torch.float32)
        if swap:
            ww = 1 - ww
        x, y = src[int(a)].float(), src[int(b)].float()
        rows.append(((1 - ww) * x + ww * y).half())
    return torch.stack(rows)


def test_the_bound_passes_fp32_arithmetic_and_rejects_wrong_weights():
    g = torch.Generator().manual_seed(3)
    src = (torch.randn(3, 7 * 48, generator=g) * 2).half()
    src[0, :8] = torch.tensor([0.0, 6e-8, -6e-8, 1e-5, 65504.0, -65504.0, 1.0, -1.0]).half()    # zeros, subnormals, the largest
    lo, hi, w = R.batch_frame_sources([[0, 4, 8]], 9)
    good = _fp32_eval(src, lo, hi, w)
    worst, ok = R.check_interp_rows(good, src, lo, hi, w)
    assert ok and worst <= 1.0, worst
    for wrong in (_fp32_eval(src, lo, hi, w, swap=True), _fp32_eval(src, lo, hi, w, shift=1)):
        worst, ok = R.check_interp_rows(wrong, src, lo, hi, w)
        assert not ok and worst > 10, worst
    # a NaN in the row that w == 0 / w == 1 does not read is no error; one that is read is
    nan_src = src.clone()
    nan_src[2] = float("nan")
    first = ([0, 0, 0], [2, 1, 1], [0.0, 0.5, 1.0])
    assert R.check_interp_rows(_fp32_eval(src, *first), nan_src, *first)[1]
    assert not R.check_interp_rows(_fp32_eval(nan_src, [0], [2], [0.5]), src, [0], [2], [0.5])[1]


# ---------------------------------------------------------------------------------------------------------- the pipeline's checks
def _cpu_pipe():
    p = pkg()
    return p.I2VAdapterPipeline(unet=p.UNetMotionCrossFrameAttnModel(**SMALL_UNET))


def _call(pipe, **kw):
    base = dict(condition_image_latents=torch.zeros(1, 4, 16, 16), num_frames=4, num_inference_steps=2, output_type="latent")
    return pipe(**{**base, **kw})


def test_bad_keyframe_dicts_raise_before_anything_is_encoded():
    pipe = _cpu_pipe()                        # no text encoder, no GPU: anything behind the check would raise something else
    for bad, key in (({1: "a"}, "1"), ({0: "a", 4: "b"}, "4"), ({0: "a", "x": "b"}, "'x'")):
        with pytest.raises(ValueError, match=re.escape(key)):
            _call(pipe, prompt=bad)
        with pytest.raises(ValueError, match="negative_prompt.*" + re.escape(key)):
            _call(pipe, prompt="a", negative_prompt=bad)
    with pytest.raises(ValueError, match="`text_encoder` and a `tokenizer`"):      # a valid dict goes on to the encoder
        _call(pipe, prompt={0: "a", 3: "b"})


def test_4d_prompt_embeds_shape_checks():
    pipe = _cpu_pipe()
    pe3, pe4 = torch.zeros(1, 7, 64), torch.zeros(1, 4, 7, 64)
    with pytest.raises(ValueError, match=r"`prompt_embeds` is \[B, F, L, D\].*F = 3 .*`num_frames` is 4"):
        _call(pipe, prompt_embeds=torch.zeros(1, 3, 7, 64), negative_prompt_embeds=pe3)
    with pytest.raises(ValueError, match=r"`negative_prompt_embeds` is \[B, F, L, D\].*F = 5"):
        _call(pipe, prompt_embeds=pe3, negative_prompt_embeds=torch.zeros(1, 5, 7, 64))
    # valid 4-D embeds, and 3-D ones as before, reach the no-CPU-path error
    for kw in (dict(prompt_embeds=pe4, negative_prompt_embeds=pe4), dict(prompt_embeds=pe3, negative_prompt_embeds=pe3)):
        with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
            _call(pipe, **kw)


def test_unet_forward_documents_per_frame_contexts():
    unet = pkg().UNetMotionCrossFrameAttnModel(**SMALL_UNET)
    assert "[B * F, L, D]" in unet.forward.__doc__


def test_per_frame_oracle_unet_equals_the_oracle_on_a_repeated_context():
    """the reference of the GPU tests: the oracle's UNet with only the context's per-frame repeat overridden.  Given the repeat as its
    input it is the oracle, bit for bit -- with and without the IP-Adapter's image tokens -- and another context per frame moves it."""
    from tests.parity import oracle_small_unet, small_unet_inputs
    inp = small_unet_inputs(b=1, f=2, hw=8)
    for ip in (False, True):
        ou = oracle_small_unet(ip=ip)
        pf, _ = R.oracle_small_unet_per_frame(ip=ip)
        if ip:
            pf.load_state_dict(ou.state_dict())
        added = {"image_embeds": inp["image_embeds"]} if ip else None
        with torch.no_grad():
            want = ou(inp["sample"], inp["timestep"], True, inp["ctx"], added_cond_kwargs=added).sample
            got = pf(inp["sample"], inp["timestep"], True, inp["ctx"].repeat_interleave(2, 0), added_cond_kwargs=added).sample
            other = pf(inp["sample"], inp["timestep"], True, torch.cat([inp["ctx"], -inp["ctx"]]), added_cond_kwargs=added).sample
        assert torch.equal(got, want)
        assert not torch.equal(other[:, 1], want[:, 1])
        assert (pf.encoder_hid_proj is not None) == ip                      # (the forward put the projection back)


# ---------------------------------------------------------------------------------------------------------- ABI
def test_abi_25_declares_exports_and_binds_interp_rows():
    lib = pkg()._lib
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 25
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    from i2v_adapter_unofficial_amd import handle as H
    name = "i2v_interp_rows_f16"
    assert re.search(rf"\bint {name}\(", src) and name in lib.SIGNATURES and hasattr(h, name)
    assert name not in H.ENTRY_IDS                              # the C handle's plan format is unchanged: it refuses per-frame contexts
    assert len(lib.SIGNATURES[name][1]) == 11
    assert callable(pkg().kernels.interp_rows)


def test_interp_rows_bad_arguments_are_refused_on_the_host():
    """I2V_ERR_INVALID_ARG before anything is launched: callable without a GPU (the pointers are never dereferenced)"""
    h = pkg()._lib.load()
    S, LO, HI, W, O = 1 << 40, 1 << 41, (1 << 41) + 4096, (1 << 41) + 8192, 1 << 42
    ok = dict(src=S, ld_src=336, n_src=3, lo=LO, hi=HI, w=W, out=O, ld_out=344, n_out=5, e=336)
    for kw, msg in ((dict(src=None), b"null"), (dict(lo=None), b"null"), (dict(hi=None), b"null"), (dict(w=None), b"null"),
                    (dict(out=None), b"null"), (dict(n_out=0), b"n_out 0"), (dict(n_src=0), b"n_src 0"), (dict(e=0), b"multiple of 8"),
                    (dict(e=332), b"multiple of 8"), (dict(ld_src=328), b"row strides"), (dict(ld_out=335), b"row strides"),
                    (dict(ld_out=340), b"row strides"), (dict(src=S + 8), b"16-byte"), (dict(out=O + 2), b"16-byte"),
                    (dict(lo=LO + 2), b"4-byte"), (dict(w=W + 1), b"4-byte"), (dict(out=S), b"overlaps"),
                    (dict(out=S + 2 * (2 * 336 + 328)), b"overlaps"), (dict(src=O + 2 * (4 * 344 + 328)), b"overlaps"),
                    (dict(n_out=1 << 30, e=64), b"too large")):
        args = tuple({**ok, **kw}.values())
        assert h.i2v_interp_rows_f16(*args, None) == -1, kw
        assert msg in h.i2v_last_error(), (kw, h.i2v_last_error())


def test_interp_rows_wrapper_refuses_host_tensors():
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        pkg().kernels.interp_rows(torch.zeros(2, 8, dtype=f16), [0], [1], [0.5])


# ---------------------------------------------------------------------------------------------------------- refusals, driver
def test_the_c_handle_and_the_trainer_refuse_per_frame_contexts():
    from i2v_adapter_unofficial_amd import handle, training
    pipe = _cpu_pipe()
    st = dict(latents=torch.zeros(1, 4, 4, 16, 16), copies=2, ctx_text=torch.zeros(2 * 4, 7, 64, dtype=f16), ctx_ip=None)
    for fn in (handle.record_step_plan, handle.record_prepare_plan):
        with pytest.raises(NotImplementedError, match=fn.__name__ + ".*per-frame text contexts"):
            fn(pipe, st)
    with pytest.raises(NotImplementedError, match="export_denoiser.*per-frame text contexts"):
        handle.export_denoiser(pipe, "unused", num_frames=4, latent_height=16, latent_width=16, per_frame_context=True)
    tr = training.UNetAdapterTrainer(pipe.unet)
    for ctx in (torch.zeros(1 * 4, 7, 64), torch.zeros(1, 4, 7, 64)):
        with pytest.raises(NotImplementedError, match="per-frame text contexts"):
            tr.forward(torch.zeros(1, 4, 4, 16, 16), 10, ctx)


def test_driver_flag_and_cell_format():
    parser = pkg().pipeline_i2v_adapter.build_parser()
    assert parser.parse_args(["--task_name", "t"]).prompt_travel_column is None
    a = parser.parse_args(["--task_name", "t", "--prompt_travel_column", "travel", "--negative_prompt", "blurry"])
    assert a.prompt_travel_column == "travel" and a.negative_prompt == "blurry"
    assert PT().parse_travel_cell('{"0": "a dog", "32": "a cat"}') == {0: "a dog", 32: "a cat"}
    for bad in ("not json", "[1, 2]", '{"x": "a"}'):
        with pytest.raises(ValueError, match="prompt travel"):
            PT().parse_travel_cell(bad)
