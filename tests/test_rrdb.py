"""RRDBNet (upscaler.RRDBNet, Real-ESRGAN x4plus) without a GPU: state-dict keys against the plain-torch restatement and the committed
key list, every load format, the inferred configuration and the refusals, `load_upscaler`'s dispatch, the dense kernel's weight
packing against a written-out index formula, the ABI of the new entry points and their host-side argument checks, and what the GPU
gates rely on -- the per-element bounds REJECT the wrong evaluations of every kernel case, and few outputs of the end-to-end cases
saturate."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

from tests import gemm_bounds as B
from tests import rrdb_reference as R
from tests import srvgg_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def U():
    return pkg().upscaler


# ------------------------------------------------------------------------------------------------------------- keys and files
def _golden():
    out, cur = {}, None
    for line in open(os.path.join(ROOT, "tests", "golden", "rrdb_keys.txt")).read().split():
        if line.startswith("[num_block="):
            cur = out.setdefault(int(line[len("[num_block="):-1]), [])
        else:
            cur.append(line)
    return out


@pytest.mark.parametrize("num_block", (6, 23))
def test_state_dict_keys_are_the_restatements_and_the_committed_list(num_block):
    with torch.device("meta"):
        keys = list(pkg().RRDBNet(num_block=num_block).state_dict().keys())
        ref = R.RRDBReference(num_block=num_block)
    assert keys == list(ref.state_dict().keys()) == _golden()[num_block] and len(keys) == 30 * num_block + 12
    shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert shapes["conv_first.weight"] == (64, 3, 3, 3) and shapes["conv_last.weight"] == (3, 64, 3, 3)
    for i, (cin, cout) in enumerate(((64, 32), (96, 32), (128, 32), (160, 32), (192, 64))):
        assert shapes[f"body.{num_block - 1}.rdb3.conv{i + 1}.weight"] == (cout, cin, 3, 3)


def test_every_load_format_and_the_round_trip(tmp_path):
    from safetensors.torch import save_file
    state = {k: v.clone() for k, v in R.seeded_reference(2, seed=3).state_dict().items()}
    N = pkg().RRDBNet
    torch.save({"params_ema": state, "params": {"junk": torch.zeros(1)}}, str(tmp_path / "ema.pth"))      # params_ema first
    torch.save({"params": state}, str(tmp_path / "params.pth"))
    torch.save(state, str(tmp_path / "bare.pt"))
    save_file({k: v.contiguous() for k, v in state.items()}, str(tmp_path / "m.safetensors"))
    for src in (str(tmp_path / "ema.pth"), str(tmp_path / "params.pth"), str(tmp_path / "bare.pt"), str(tmp_path / "m.safetensors"), state,
                {"params_ema": state}):
        for m in (N.from_pretrained(src), U().load_upscaler(src)):
            assert isinstance(m, N) and (m.num_block, m.upscale, m.training) == (2, 4, False)
            assert all(torch.equal(m.state_dict()[k], v) for k, v in state.items()) and list(m.state_dict()) == list(state)
    m.save_pretrained(str(tmp_path / "again" / "up.safetensors"))
    again = N.from_pretrained(str(tmp_path / "again" / "up.safetensors"))
    assert all(torch.equal(again.state_dict()[k], v) for k, v in state.items())
    with pytest.raises(ValueError, match="safetensors"):
        m.save_pretrained(str(tmp_path / "up.pth"))
    with pytest.raises(EnvironmentError):
        N.from_pretrained(str(tmp_path / "missing.pth"))


@pytest.mark.parametrize("num_block", (1, 6, 23))
def test_the_configuration_is_inferred_from_keys_and_shapes(num_block):
    with torch.device("meta"):
        state = R.RRDBReference(num_block=num_block).state_dict()
        assert U().infer_rrdb_config(state) == dict(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=num_block, num_grow_ch=32)
        assert U().is_rrdb_state_dict(state) and pkg().RRDBNet.from_pretrained(state).num_block == num_block


def _meta_state(**kw):
    """the state dict of an upstream-shaped network the HIP path may not implement, on the meta device"""
    cfg = dict(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=1, num_grow_ch=32)
    cfg.update(kw)
    nf, g = cfg["num_feat"], cfg["num_grow_ch"]
    st = {}

    def conv(name, cin, cout):
        st[f"{name}.weight"], st[f"{name}.bias"] = torch.empty((cout, cin, 3, 3), device="meta"), torch.empty((cout,), device="meta")

    conv("conv_first", cfg["num_in_ch"], nf)
    for i in range(cfg["num_block"]):
        for j in (1, 2, 3):
            for k in range(1, 6):
                conv(f"body.{i}.rdb{j}.conv{k}", nf + (k - 1) * g, g if k < 5 else nf)
    for name in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
        conv(name, nf, nf)
    conv("conv_last", nf, cfg["num_out_ch"])
    return st


def test_refusals_name_the_value():
    N = pkg().RRDBNet
    with torch.device("meta"):
        for kw, msg in ((dict(num_feat=32), "num_feat=32"), (dict(num_grow_ch=16), "num_grow_ch=16"), (dict(scale=2), "scale=2"),
                        (dict(scale=1), "scale=1"), (dict(num_in_ch=1), "num_in_ch=1"), (dict(num_out_ch=4), "num_out_ch=4")):
            with pytest.raises(NotImplementedError, match=msg):
                N(num_block=1, **kw)
        with pytest.raises(ValueError, match="num_block=0"):
            N(num_block=0)
    # ... and from a state dict, before anything is built or packed
    for kw, msg in ((dict(num_feat=32), "num_feat=32"), (dict(num_grow_ch=16), "num_grow_ch=16"), (dict(num_in_ch=12), "12 channels: a scale-2"),
                    (dict(num_in_ch=48), "48 channels: a scale-1"), (dict(num_in_ch=4), "num_in_ch=4"), (dict(num_out_ch=1), "num_out_ch=1")):
        for load in (N.from_pretrained, U().load_upscaler):
            with pytest.raises(NotImplementedError, match=msg):
                load(_meta_state(**kw))
    good = _meta_state()
    for extra in ("body.0.rdb1.conv6.weight", "conv_up3.weight", "body.0.weight", "upsampler.weight"):
        with pytest.raises(NotImplementedError, match=re.escape(f"unknown key `{extra}`")):
            N.from_pretrained({**good, extra: torch.zeros(64)})
    for missing in ("conv_hr.bias", "conv_body.weight"):
        with pytest.raises(NotImplementedError, match=re.escape(f"missing key `{missing}`")):
            N.from_pretrained({k: v for k, v in good.items() if k != missing})
    with pytest.raises(NotImplementedError, match="body indices"):
        N.from_pretrained({k.replace("body.0.", "body.1."): v for k, v in good.items()})
    with pytest.raises(RuntimeError, match="body.0.rdb2.conv3.bias"):                  # a key of a known name that is absent: strict loading
        N.from_pretrained({k: v for k, v in R.seeded_reference(1).state_dict().items() if k != "body.0.rdb2.conv3.bias"})
    for old in ("model.0.weight", "model.1.sub.0.RDB1.conv1.0.weight"):
        for load in (N.from_pretrained, U().load_upscaler):
            with pytest.raises(NotImplementedError, match="old ESRGAN architecture"):
                load({old: torch.zeros(64, 3, 3, 3)})
    with pytest.raises(pkg().HipLibraryError, match="no CPU fallback"):
        N(num_block=1)(torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        N(num_block=1)(torch.zeros(1, 4, 4, 4))


def test_load_upscaler_picks_the_class_by_keys():
    rr, sr = R.seeded_reference(1).state_dict(), S.seeded_reference(1, 2).state_dict()
    assert isinstance(U().load_upscaler(rr), pkg().RRDBNet) and isinstance(U().load_upscaler({"params": rr}), pkg().RRDBNet)
    m = U().load_upscaler(sr)
    assert isinstance(m, pkg().SRVGGNetCompact) and m.num_conv == 1 and m.upscale == 2
    with pytest.raises(ValueError, match="act_type='relu' with an RRDBNet"):
        U().load_upscaler(rr, act_type="relu")
    # an SRVGG dict with a stray RRDBNet key is still SRVGGNetCompact's to refuse, by that key
    with pytest.raises(NotImplementedError, match=re.escape("SRVGGNetCompact: unknown key `conv_first.weight`")):
        U().load_upscaler({**sr, "conv_first.weight": torch.zeros(64)})
    with pytest.raises(NotImplementedError, match=re.escape("SRVGGNetCompact: unknown key `conv_first.weight`")):
        pkg().SRVGGNetCompact.from_pretrained({**sr, "conv_first.weight": torch.zeros(64)})
    # ... and an RRDBNet dict with a stray SRVGG key likewise
    with pytest.raises(NotImplementedError, match="SRVGGNetCompact: unknown key"):
        U().load_upscaler({**rr, "body.0.weight": torch.zeros(64, 3, 3, 3)})


def test_the_pipeline_takes_an_rrdbnet_and_refuses_an_act_type():
    from i2v_adapter_unofficial_amd.pipeline_i2v_adapter import I2VAdapterPipeline
    pipe = I2VAdapterPipeline.__new__(I2VAdapterPipeline)
    pipe._upscaler = None
    with torch.device("meta"):
        m = pkg().RRDBNet(num_block=1)
    pipe.enable_upscaler(m, frames_per_batch=2)
    assert pipe.upscaler_enabled and pipe._upscaler == (m, 2)
    with pytest.raises(ValueError, match="act_type='relu' with an RRDBNet"):
        pipe.enable_upscaler(m, act_type="relu")
    with pytest.raises(ValueError, match="act_type='relu' with an RRDBNet"):
        pipe.enable_upscaler(R.seeded_reference(1).state_dict(), act_type="relu")
    with pytest.raises(ValueError, match="frames_per_batch"):
        pipe.enable_upscaler(m, frames_per_batch=0)
    pipe.enable_upscaler(R.seeded_reference(1).state_dict())
    assert isinstance(pipe._upscaler[0], pkg().RRDBNet)
    pipe.disable_upscaler()
    assert not pipe.upscaler_enabled


# ------------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("cout", (32, 64))
@pytest.mark.parametrize("cin", R.CINS)
def test_pack_conv_dense_is_the_written_out_index_formula(cin, cout):
    """packed[((((half (cin / 32) + chunk) 9 + tap) 2 + b) 64 + 16 g + l) 8 + j] = W[32 half + 8 (l >> 2) + 4 b + (l & 3)][32 chunk + 8 g + j][tap]"""
    g = torch.Generator().manual_seed(cin + cout)
    w = torch.randn((cout, cin, 3, 3), generator=g).half()
    packed = pkg().kernels.pack_conv_dense(w)
    assert packed.dtype == torch.float16 and packed.shape == (9 * cin * cout,)
    idx = torch.arange(9 * cin * cout)
    j, r = idx % 8, idx // 8
    l, r = r % 16, r // 16
    gg, r = r % 4, r // 4
    b, r = r % 2, r // 2
    tap, r = r % 9, r // 9
    chunk, half = r % (cin // 32), r // (cin // 32)
    want = w.reshape(cout, cin, 9)[32 * half + 8 * (l >> 2) + 4 * b + (l & 3), 32 * chunk + 8 * gg + j, tap]
    assert torch.equal(packed, want)
    for bad in ((48, cin, 3, 3), (cout, 80, 3, 3), (cout, cin, 1, 1)):
        with pytest.raises(ValueError, match="pack_conv_dense takes"):
            pkg().kernels.pack_conv_dense(torch.zeros(bad))


# ------------------------------------------------------------------------------------------------------------- the bounds reject
_DISTINCT = tuple(c for c in R.DENSE_CASES if c[3] == R.DENSE_STRIDES[0])          # (the stride does not enter the reference)


@functools.lru_cache(maxsize=None)
def _dense_ref(case):
    return R.dense_case_reference(case)


def test_dense_mutants_cover_the_list():
    seen = set()
    for case in _DISTINCT:
        seen |= set(R.dense_mutants_of(case))
    assert seen == set(R.DENSE_MUTANTS)


@pytest.mark.parametrize("case", _DISTINCT, ids=R.dense_case_id)
def test_the_dense_bound_rejects_every_wrong_evaluation(case):
    ref, tol = _dense_ref(case)
    # the right evaluation, rounded to fp16 as the kernel stores it, passes
    assert not bool((B.excess(ref.half(), ref, tol) > 0).any())
    for mutant in R.dense_mutants_of(case):
        bad, _ = R.dense_case_reference(case, mutant=mutant)
        ex = B.excess(bad.half(), ref, tol)
        assert bool((ex > 0).any()), f"{R.dense_case_id(case)}: the bound accepts `{mutant}` (largest excess {float(ex.max()):.3e})"


@pytest.mark.parametrize("case", [c for c in R.UP2_CASES if c[1] == 64], ids=R.up2_case_id)
def test_the_up2_bound_rejects_every_wrong_evaluation(case):
    x, w, b = R.up2_case_inputs(case)
    ref, tol = R.up2_layer_fp64(x, w, b)
    n, h, wd, _ = x.shape
    assert ref.shape == (n, 2 * h, 2 * wd, 64) and not bool((B.excess(ref.half(), ref, tol) > 0).any())
    # ... and is torch's nearest upsampling in front of the layer
    up = torch.nn.functional.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).half()
    pre, _ = S.layer_fp64(up.contiguous(), w, b, torch.full((64,), 0.2))
    assert torch.equal(pre, ref)
    for mutant in R.up2_mutants_of(case):
        bad, _ = R.up2_layer_fp64(x, w, b, mutant=mutant)
        assert bool((B.excess(bad.half(), ref, tol) > 0).any()), f"the bound accepts `{mutant}`"


@pytest.mark.parametrize("case", R.EXIT_CASES, ids=R.exit_case_id)
def test_the_exit_bound_rejects_the_misplaced_clamp(case):
    y = R.exit_case_inputs(case)
    ref, tol = R.exit_fp64(y, True, case[1])
    assert torch.equal(ref, R.leave_map(y.double()[..., :3].permute(0, 3, 1, 2), case[1]))
    for mutant in R.exit_mutants_of(case):
        bad, _ = R.exit_fp64(y, True, case[1], mutant=mutant)
        assert bool(((bad - ref).abs() > tol).any()), f"the bound accepts `{mutant}`"


@pytest.mark.parametrize("case", R.E2E_CASES, ids=str)
def test_few_outputs_of_the_end_to_end_cases_saturate(case):
    ref = R.seeded_reference(case[0])
    frac = R.saturated_fraction(ref, R.entry_map(R.e2e_frames(case)))
    print(f"{case}: {100 * frac:.2f} % of the fp32 reference's outputs lie outside (0, 1)")
    assert frac <= 0.10
    assert all(torch.equal(v, v.half().float()) for v in ref.state_dict().values())      # fp16 values: every evaluation reads the same


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_declares_exports_and_binds_the_new_entry_points():
    lib = pkg()._lib
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 34
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for name in ("i2v_conv3x3_dense_f16", "i2v_conv3x3_c64_up2_prelu_f16", "i2v_rgb_exit_f32"):
        assert re.search(rf"\bint {name}\(", src) and name in lib.SIGNATURES and hasattr(h, name)
    assert lib.SIGNATURES["i2v_conv3x3_dense_f16"][1] == [C.POINTER(lib.ConvDenseParams), C.c_void_p]
    assert lib.SIGNATURES["i2v_conv3x3_c64_up2_prelu_f16"][1] == lib.SIGNATURES["i2v_conv3x3_c64_prelu_f16"][1]
    # the struct as the header declares it: field names in order
    body = re.search(r"typedef struct i2v_conv_dense_params \{(.*?)\} i2v_conv_dense_params;", src, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [f[0] for f in lib.ConvDenseParams._fields_]
    assert pkg().RRDBNet is pkg().upscaler.RRDBNet
    assert pkg().kernels.DENSE_TILE == R.TILE and pkg().kernels.DENSE_CIN == R.CINS
    from i2v_adapter_unofficial_amd import handle as H
    assert not {"i2v_conv3x3_dense_f16", "i2v_conv3x3_c64_up2_prelu_f16", "i2v_rgb_exit_f32"} & set(H.ENTRY_IDS)      # in no recorded plan


def _dense_params(**kw):
    """a well-formed in-place `grow` launch at fake addresses (argument checks read no memory), with fields replaced"""
    lib = pkg()._lib
    p = lib.ConvDenseParams()
    base = 1 << 43
    p.x, p.ldx, p.w, p.bias = base, 192, 1 << 42, (1 << 42) + (1 << 20)
    p.out, p.ldo = base + 2 * 64, 192
    p.n_img, p.height, p.width, p.cin, p.cout = 2, 17, 17, 64, 32
    p.slope, p.s1, p.s2 = 0.2, 1.0, 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_bad_arguments_are_refused_on_the_host():
    """the refusals return I2V_ERR_INVALID_ARG before anything is launched: callable without a GPU"""
    lib = pkg()._lib
    h = lib.load()
    base, other = 1 << 43, 1 << 44

    def refused(match, **kw):
        rc = h.i2v_conv3x3_dense_f16(C.byref(_dense_params(**kw)), None)
        msg = h.i2v_last_error().decode()
        assert rc == -1 and re.search(match, msg), (rc, msg)

    refused("null pointer", x=None)
    refused("null pointer", out=None)
    refused("cin 80 must be 64, 96, 128, 160 or 192", cin=80)
    refused("cin 224", cin=224)
    refused("cout 48 must be 32 or 64", cout=48)
    refused("ldx 60 must be >= cin 64", ldx=60, out=other)
    refused("ldx 196 must be", ldx=196, out=other)
    refused("ldo 24 must be >= cout 32", ldo=24, out=other)
    refused("r1 pixel stride 20", r1=other, ldr1=20)
    refused("r2 pixel stride 33", r2=other, ldr2=33)
    refused("16-byte aligned", x=base + 8)
    refused("16-byte aligned", bias=(1 << 42) + 2)
    refused("n 0", n_img=0)
    refused("max_workgroups -1", max_workgroups=-1)
    # overlaps: out inside the channels that are read; out at another stride; out past the pixel's end; the weights; the residuals
    refused("out overlaps channels 0..63 of x", out=base)
    refused("out overlaps channels 0..63 of x", out=base + 2 * 48)
    refused("out overlaps channels 0..95 of x", cin=96)
    refused("out overlaps channels 0..63 of x", ldo=200)
    refused("out overlaps channels 0..63 of x", out=base + 2 * 176)                    # channels 176 .. 207: the next pixel's 0 .. 15
    refused("out overlaps the weights", w=base + 2 * 64 + 2 * 192)
    refused("out overlaps the weights", bias=base + 2 * 64 + 2 * 192 * 3)
    refused("out overlaps r1 without being it", r1=base + 2 * 64 + 16, ldr1=192)
    refused("out overlaps r1 without being it", r1=base + 2 * 64, ldr1=200)
    refused("out overlaps r2 without being it", r2=base + 2 * 64 - 16, ldr2=192)
    # the folded-upsample entry: an odd output size; the exit: a narrow pixel, an overlap
    p = lib.ConvC64Params()
    p.x, p.ldx, p.w, p.out, p.ldo = base, 64, 1 << 42, other, 64
    p.n_img, p.height, p.width, p.cin, p.cout = 1, 6, 7, 64, 64
    assert h.i2v_conv3x3_c64_up2_prelu_f16(C.byref(p), 1 << 41, None) == -1
    assert re.search("i2v_conv3x3_c64_up2_prelu_f16: output height 6 and width 7 must be even", h.i2v_last_error().decode())
    assert h.i2v_rgb_exit_f32(base, 2, other, 1, 4, 4, 1, 1, None) == -1
    assert re.search("ld 2 must be >= 3", h.i2v_last_error().decode())
    assert h.i2v_rgb_exit_f32(base, 3, base + 16, 1, 4, 4, 1, 1, None) == -1
    assert re.search("out overlaps y", h.i2v_last_error().decode())
    assert h.i2v_rgb_exit_f32(None, 3, other, 1, 4, 4, 1, 1, None) == -1
