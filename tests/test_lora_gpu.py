"""LoRA on the GPU: `i2v_lora_merge` against the fp64 merge (tests/lora_reference.py) at every code path of the kernel, an Attention
block and the reduced UNet carrying merged weights against the oracle with the same merge, the adapter state machine (set / delete /
scale / fuse / unload, bit-exact restores), the pipeline (graph == eager, re-capture on every LoRA change, the trajectory), a forward
plan recorded with a LoRA merged replayed through the model handle, and the training guard."""
import pytest
import torch

from tests.lora_reference import attention_paths, merge_reference, merged_oracle, random_lora, target_shapes, to_state_dict
from tests.parity import (REL_TOL_MODULE, REL_TOL_TRAJECTORY, REL_TOL_UNET, compare, hip_unet_from_oracle, oracle_small_unet,
                          round_fp16_, small_unet_inputs)

pytestmark = pytest.mark.gpu


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


def h16(t):
    return t.half().float()


# ---------------------------------------------------------------------------------------------------------- the kernel
def _one_ulp_ok(got, ref64, name):
    """the bound of tests/test_freeu_gpu.py::_one_ulp_ok: |out - ref| <= 2^-10 max(|ref|, 2^-14) elementwise, one fp16 ulp.  The kernel
    rounds once from fp32 (at most half an ulp), which leaves at least 2^-25 (half the bound's floor) for the fp32 arithmetic in front
    of it: exact fp16 x fp16 products summed in fp32 by the MFMA (one rounding per 32-deep chunk), one fp32 multiply-add by the scale
    per adapter and one add of base -- N = rank / 32 + 2 n + 1 roundings of at most 2^-25 M each, M the magnitude of the partial sums.
    `_problem` draws weight-scale data (base ~ N(0, 0.05^2) like SD-1.5's weights, low-rank updates of std 0.02 |scale| / sqrt(n)
    per adapter whatever the rank): where base and update cancel, M <= ~0.05 and N M < 1 for every case below, up to the largest rank; the
    8-adapter case (N = 26) sits at that limit in the worst case and a factor sqrt(N) below it for roundings of random sign."""
    got64 = got.double().cpu()
    assert torch.isfinite(got64).all(), f"{name}: non-finite values"
    err = (got64 - ref64).abs()
    bound = 2.0 ** -10 * torch.clamp(ref64.abs(), min=2.0 ** -14)
    worst = (err / bound).max().item()
    print(f"{name}: max |err| / (one fp16 ulp) = {worst:.3f}")
    assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} elements off by more than one fp16 ulp (worst {worst:.3f} ulp)"
    return worst


def _f32_ok(got, ref64, base, adapters, name):
    """|err| <= (R + n + 2) 2^-24 (|base| + sum_j |scale_j| (|up_j| @ |down_j|)) elementwise, R the total rank: every product and
    every partial sum rounded once in fp32, computed here from the inputs"""
    total_rank = sum(d.shape[0] for d, _, _ in adapters)
    mag = base.double().abs().reshape(base.shape[0], -1).clone()
    for d, u, s in adapters:
        mag += abs(s) * (u.double().abs() @ d.double().abs())
    bound = (total_rank + len(adapters) + 2) * 2.0 ** -24 * mag.reshape(base.shape)
    err = (got.double().cpu() - ref64).abs()
    worst = (err / bound.clamp(min=1e-300)).max().item()
    print(f"{name}: max |err| / bound = {worst:.3e}")
    assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} elements outside the fp32 bound (worst {worst:.3f} x)"


SCALES = (0.75, -0.5, 1.0, 0.625, -1.5, 0.125, 2.0, -0.25)          # (exact in fp32: the reference takes the same numbers)


def _problem(n_out, n_in, ranks, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(n_out, n_in, generator=g) * 0.05).to(dtype)
    adapters = []
    for j, r in enumerate(ranks):
        down = (torch.randn(r, n_in, generator=g) / r ** 0.5).half()
        up = (torch.randn(n_out, r, generator=g) * 0.02 / len(ranks) ** 0.5).half()
        adapters.append((down, up, SCALES[j]))
    return base, adapters


KERNEL_CASES = [
    # out, in, ranks
    (1, 1, (1,)),                      # degenerate
    (24, 40, (1,)),                    # small
    (320, 36, (4,)),                   # conv_in: in % 8 != 0, the element-wise form for fp16 (fp32: in % 4 == 0, vector)
    (17, 37, (3,)),                    # the element-wise form for fp32 too
    (33, 72, (5,)),                    # a rank that is no multiple of the MFMA's k, ragged out
    (64, 64, (5,)),
    (200, 328, (16,)),                 # 4 x 3 workgroups, ragged edges in both directions
    (128, 1152, (128,)),               # large rank: 4 k chunks
    (128, 1152, (256,)),               # the maximum rank
    (1280, 1280, (64,)),               # an SD-1.5 attention projection
    (200, 328, (4, 16)),               # two adapters of different ranks in one launch
    (72, 136, (1, 2, 3, 4, 5, 8, 16, 40)),      # the maximum number of adapters
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("n_out,n_in,ranks", KERNEL_CASES)
def test_kernel_against_the_fp64_merge(dev, n_out, n_in, ranks, dtype):
    K = pkg().kernels
    base, adapters = _problem(n_out, n_in, ranks, dtype, seed=n_out * 7 + n_in + sum(ranks))
    ref = merge_reference(base, adapters)
    bd = base.to(dev)
    dst = torch.full_like(bd, float("nan"))
    v0 = dst._version
    ret = K.lora_merge(dst, bd, [(d.to(dev), u.to(dev), s) for d, u, s in adapters])
    torch.cuda.synchronize()
    assert ret is dst and dst._version > v0, "the wrapper must bump dst's version (the packs and the graph key are keyed on it)"
    assert torch.equal(bd.cpu(), base), "base must not be modified"
    name = f"lora_merge {n_out}x{n_in} ranks={ranks} {dtype}"
    if dtype == torch.float16:
        _one_ulp_ok(dst, ref, name)
    else:
        _f32_ok(dst, ref, base, adapters, name)
    assert (dst.double().cpu() - base.double()).abs().max().item() > 1e-3 or n_out * n_in < 4, "the update must be visible"


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_kernel_unaligned_pointers_take_the_elementwise_form(dev, dtype):
    """in % 8 == 0 but base / dst / the factors start one element past a 16-byte boundary"""
    K = pkg().kernels
    n_out, n_in, r = 40, 64, 8
    base, adapters = _problem(n_out, n_in, (r,), dtype, seed=5)
    off = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)]).to(dev)[1:].view(t.shape)
    bd, dst = off(base), off(torch.zeros_like(base))
    assert bd.data_ptr() % 16 != 0 and bd.is_contiguous()
    guard = dst.storage_offset()
    K.lora_merge(dst, bd, [(off(d), off(u), s) for d, u, s in adapters])
    ref = merge_reference(base, adapters)
    if dtype == torch.float16:
        _one_ulp_ok(dst, ref, "lora_merge unaligned f16")
    else:
        _f32_ok(dst, ref, base, adapters, "lora_merge unaligned f32")
    assert guard == 1 and dst._base.reshape(-1)[0].item() == 0, "the element in front of dst must not be written"


def _special(dtype, n_out=40, n_in=72):
    base = torch.randn(n_out, n_in, generator=torch.Generator().manual_seed(2)).to(dtype)
    if dtype == torch.float16:
        bits = base.view(torch.int16)
        vals = (-32768, 1, 0x7C00, 0x7E01, 0x03FF)          # -0, the smallest and the largest subnormal, +inf, a NaN with a payload
    else:
        bits = base.view(torch.int32)
        vals = (-2147483648, 1, 0x7F800000, 0x7FC00123, 0x007FFFFF)
    for i, v in enumerate(vals):
        bits[:, 8 + i] = v
    return base, bits.clone()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_no_adapters_and_zero_scales_give_base_bit_for_bit(dev, dtype):
    K = pkg().kernels
    base, bits = _special(dtype)
    view = torch.int16 if dtype == torch.float16 else torch.int32
    bd = base.to(dev)
    g = torch.Generator().manual_seed(3)
    d1, u1 = torch.randn(4, 72, generator=g).half().to(dev), torch.randn(40, 4, generator=g).half().to(dev)
    d2, u2 = torch.randn(9, 72, generator=g).half().to(dev), torch.randn(40, 9, generator=g).half().to(dev)
    for adapters in ([], [(d1, u1, 0.0)], [(d1, u1, 0.0), (d2, u2, -0.0)]):
        dst = torch.zeros_like(bd)
        K.lora_merge(dst, bd, adapters)
        assert torch.equal(dst.cpu().view(view), bits), f"{len(adapters)} adapters at scale 0 must copy base's bits"
        assert torch.equal(bd.cpu().view(view), bits)


def test_wrapper_rejects_what_the_kernel_does_not_take(dev):
    p = pkg()
    K, E = p.kernels, p._lib.HipLibraryError
    z = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt, device=dev)
    base, dst = z(16, 24), z(16, 24)
    ok = (z(4, 24), z(16, 4), 1.0)
    K.lora_merge(dst, base, [ok])
    with pytest.raises(E, match="rank 257"):
        K.lora_merge(dst, base, [(z(257, 24), z(16, 257), 1.0)])
    with pytest.raises(E, match="at most 8"):
        K.lora_merge(dst, base, [ok] * 9)
    with pytest.raises(E, match="alias"):
        K.lora_merge(base, base, [ok])
    with pytest.raises(E, match="alias"):
        buf = z(17, 24)
        K.lora_merge(buf[1:], buf[:16], [ok])
    with pytest.raises(TypeError):
        K.lora_merge(dst, base.float(), [ok])
    with pytest.raises(TypeError):
        K.lora_merge(dst, base, [(z(4, 24, dt=torch.float32), z(16, 4), 1.0)])
    with pytest.raises(ValueError, match="contiguous"):
        K.lora_merge(dst, base, [(z(4, 48)[:, ::2], z(16, 4), 1.0)])
    with pytest.raises(ValueError, match="contiguous"):
        K.lora_merge(dst, z(16, 48)[:, :24], [ok])
    with pytest.raises(ValueError, match="do not fit"):
        K.lora_merge(dst, base, [(z(4, 25), z(16, 4), 1.0)])
    with pytest.raises(E):
        K.lora_merge(dst.cpu(), base, [ok])


# ---------------------------------------------------------------------------------------------------------- one Attention block
def test_attention_block_with_merged_projections(dev):
    """to_q / to_k / to_v / to_out.0 of a stand-alone Attention merged in place from clones of their values: the output matches the
    oracle block carrying half(merge_reference) weights, and the kernel-layout pack was rebuilt (the version bump reached it)"""
    from oracle.blocks import Attention as O
    torch.manual_seed(4)
    o = round_fp16_(O(64, cross_attention_dim=48, heads=4, dim_head=16)).eval()
    m = pkg().Attention(64, cross_attention_dim=48, heads=4, dim_head=16)
    m.load_state_dict(o.state_dict())
    m = m.to(device=dev, dtype=torch.float16).eval()
    g = torch.Generator().manual_seed(6)
    x, ctx = h16(torch.randn(3, 50, 64, generator=g)), h16(torch.randn(3, 9, 48, generator=g))
    with torch.no_grad():
        plain_ref = o(x, ctx)
        plain = m(x.half().to(dev), ctx.half().to(dev))
        pack0 = m.packed()
        wq0 = pack0["wq"]
        lora = random_lora(target_shapes(o), rank=4, seed=8, std=0.15, paths=["to_q", "to_k", "to_v", "to_out.0"])
        mods = dict(m.named_modules())
        for path, (d, u, _) in lora.items():
            w = mods[path].weight
            pkg().kernels.lora_merge(w, w.detach().clone(), [(d.to(dev), u.to(dev), 0.75)])
        sd = o.state_dict()
        for path, (d, u, _) in lora.items():
            sd[path + ".weight"] = merge_reference(sd[path + ".weight"], [(d, u, 0.75)]).half().float()
        o.load_state_dict(sd)
        ref = o(x, ctx)
        got = m(x.half().to(dev), ctx.half().to(dev))
    pack1 = m.packed()
    assert pack1 is not pack0 and pack1["wq"] is not wq0, "the pack must be rebuilt after a merge into its parameters"
    assert torch.equal(pack1["wq"], m.to_q.weight) and torch.equal(pack1["wo"], m.to_out[0].weight), "the pack holds the merged weights"
    _one_ulp_ok(m.to_q.weight, o.to_q.weight.double(), "Attention to_q merged in place")
    compare(plain, plain_ref, rel=REL_TOL_MODULE, name="Attention, no LoRA")
    _, scale = compare(got, ref, rel=REL_TOL_MODULE, name="Attention with merged LoRA")
    assert (ref - plain_ref).abs().max().item() > 10 * REL_TOL_MODULE * scale, "the LoRA must move the output past the gate"


# ---------------------------------------------------------------------------------------------------------- the reduced UNet
W_A, W_B = 0.7, -0.4


class _Small:
    """the reduced UNet pair, two rank-4 LoRAs on EVERY Linear and conv weight, and the oracle's outputs under the merges the tests
    use (each computed once, by the oracle carrying fp16-rounded merge_reference weights)"""

    def __init__(self, dev):
        self.dev = dev
        self.ou = oracle_small_unet()
        self.hu = hip_unet_from_oracle(self.ou, dev)
        self.shapes = target_shapes(self.ou)
        self.a = random_lora(self.shapes, rank=4, seed=101, std=0.05, alpha=2.0)        # kohya-style alpha: layer scale 2 / 4
        self.b = random_lora(self.shapes, rank=4, seed=202, std=0.07)
        self.inp = small_unet_inputs()
        self._refs = {}

    def ref(self, *loras):
        """oracle output with [(which, weight)] merged; () is the plain oracle"""
        if loras not in self._refs:
            pairs = [({"a": self.a, "b": self.b}[n], w) for n, w in loras]
            with torch.no_grad(), merged_oracle(self.ou, pairs) as m:
                self._refs[loras] = m(self.inp["sample"], self.inp["timestep"], True, self.inp["ctx"]).sample
        return self._refs[loras]

    def fwd(self, hu=None, **kw):
        hu = hu or self.hu
        with torch.no_grad():
            return hu(self.inp["sample"].to(self.dev), self.inp["timestep"].to(self.dev), True, self.inp["ctx"].to(self.dev), **kw).sample

    def load_both(self, hu=None):
        hu = hu or self.hu
        ra = hu.load_lora(to_state_dict(self.a, self.shapes, "kohya"), adapter_name="a")
        rb = hu.load_lora(to_state_dict(self.b, self.shapes, "diffusers", prefix="unet."), adapter_name="b")
        assert ra["modules"] == rb["modules"] == len(self.shapes) and ra["adapter_name"] == "a"
        hu.set_adapters(["a", "b"], [W_A, W_B])


@pytest.fixture(scope="module")
def small(dev):
    return _Small(dev)


def _params(hu):
    return {n: p.detach().clone() for n, p in hu.named_parameters()}


def _check_restored(hu, before):
    for n, p in hu.named_parameters():
        assert torch.equal(p, before[n]), f"{n} was not restored bit for bit"
    assert not hu.has_lora() and hu.lora_parameter_names() == []


def test_alpha_scales_the_oracle_as_documented(small):
    """(the helper's own convention: alpha / rank) so that the product and the reference cannot agree on a wrong one by construction"""
    path = next(iter(small.a))
    d, u, alpha = small.a[path]
    assert alpha == 2.0 and d.shape[0] == 4
    from tests.lora_reference import merged_state_dict
    w0 = small.ou.state_dict()[path + ".weight"]
    w1 = merged_state_dict(small.ou, [(small.a, 1.0)])[path + ".weight"]
    assert torch.equal(w1, merge_reference(w0, [(d, u, 0.5)]).half().float())


@pytest.mark.parametrize("precise", [False, True], ids=["stream", "precise_stream"])
def test_small_unet_with_a_lora_on_every_weight(small, precise):
    """two named adapters (weights 0.7 and -0.4, one with alpha) on every Linear and conv weight of the reduced UNet against the oracle
    with the same merge at REL_TOL_UNET; the LoRA moves the oracle's output by more than ten times the gate, so a cache that missed
    one changed weight cannot pass.  Unloading restores every parameter and the forward bit for bit."""
    from i2v_adapter_unofficial_amd import blocks
    hu = small.hu
    entry = blocks.set_precise_stream(precise)
    try:
        before, plain, keys = _params(hu), small.fwd(), set(hu.state_dict())
        small.load_both()
        try:
            assert hu.get_active_adapters() == ["a", "b"] and len(hu.lora_parameter_names()) == len(small.shapes)
            assert set(hu.state_dict()) == keys, "LoRA state must not change the state-dict keys"
            got = small.fwd()
            again = small.fwd()
        finally:
            hu.unload_lora()
        _check_restored(hu, before)
        after = small.fwd()
    finally:
        blocks.set_precise_stream(entry)
    ref, ref_plain = small.ref(("a", W_A), ("b", W_B)), small.ref()
    scale = ref.abs().max().item()
    moved = (ref - ref_plain).abs().max().item()
    print(f"LoRA moves the oracle by {moved:.3e}; gate {REL_TOL_UNET * scale:.3e}")
    assert moved >= 10 * REL_TOL_UNET * scale, "the test's LoRA is too weak to tell a missed weight"
    compare(plain, ref_plain, rel=REL_TOL_UNET, name="small UNet, before the LoRA")
    compare(got, ref, rel=REL_TOL_UNET, name=f"small UNet, LoRA on every weight, precise={precise}")
    assert torch.equal(again, got) and torch.equal(after, plain), "unloading must restore the forward bit for bit"


def test_set_adapters_scale_and_delete_follow_the_merged_oracle(small):
    hu = small.hu
    before = _params(hu)
    small.load_both()
    try:
        hu.set_adapters("a")                                                   # one adapter, weight 1
        assert hu.get_active_adapters() == ["a"]
        compare(small.fwd(), small.ref(("a", 1.0)), rel=REL_TOL_UNET, name="set_adapters('a')")
        half = small.fwd(cross_attention_kwargs={"scale": 0.5})                # the scale of one call ...
        compare(half, small.ref(("a", 0.5)), rel=REL_TOL_UNET, name="cross_attention_kwargs scale 0.5")
        compare(small.fwd(), small.ref(("a", 1.0)), rel=REL_TOL_UNET, name="... and the previous scale afterwards")
        hu.set_adapters(["a", "b"], [W_A, W_B])
        hu.delete_adapters("a")
        assert hu.get_active_adapters() == ["b"]
        compare(small.fwd(), small.ref(("b", W_B)), rel=REL_TOL_UNET, name="delete_adapters('a')")
        hu.delete_adapters("b")
        assert torch.equal(small.fwd(), small.fwd(hip_unet_from_oracle(small.ou, small.dev)))
    finally:
        hu.unload_lora()
    _check_restored(hu, before)


def test_partial_adapter_restores_the_weights_it_no_longer_touches(small):
    """an attention-only adapter beside an all-layers one: switching to it alone restores every other weight from its stash"""
    hu = small.hu
    before = _params(hu)
    attn = attention_paths(small.shapes)
    small.load_both()
    try:
        hu.delete_adapters("b")
        hu.load_lora(to_state_dict({p: small.b[p] for p in attn}, small.shapes, "peft"), adapter_name="attn_only")
        hu.set_adapters("attn_only", 1.0)
        hu._sync_lora()
        touched = {p + ".weight" for p in attn}
        for n, p in hu.named_parameters():
            assert torch.equal(p, before[n]) != (n in touched), n
        hu.delete_adapters("a")
        hu._sync_lora()
        assert sorted(hu.lora_parameter_names()) == sorted(touched), "stashes no loaded adapter needs are freed"
    finally:
        hu.unload_lora()
    _check_restored(hu, before)


def test_fuse_and_unfuse(small):
    hu = small.hu
    before, plain = _params(hu), small.fwd()
    small.load_both()
    try:
        hu.fuse_lora(0.5)
        assert hu.get_active_adapters() == [] and hu.has_lora()
        compare(small.fwd(), small.ref(("a", 0.5 * W_A), ("b", 0.5 * W_B)), rel=REL_TOL_UNET, name="fuse_lora(0.5)")
        with pytest.raises(ValueError, match="unfuse_lora"):
            hu.load_lora(to_state_dict(small.a, small.shapes, "kohya"))
        hu.unfuse_lora()
        _check_restored(hu, before)
        assert torch.equal(small.fwd(), plain)
    finally:
        hu.unload_lora()


def test_to_moves_the_stash_and_the_factors(small):
    """`.to(dtype)` with adapters loaded: the stashes follow the parameters' dtype, the factors stay fp16, the merge is redone in the
    new dtype, and casting back and unloading still restores the original fp16 values (fp16 -> fp32 -> fp16 is exact)"""
    hu = hip_unet_from_oracle(small.ou, small.dev)
    before = _params(hu)
    small.load_both(hu)
    try:
        hu = hu.float()
        st = hu._lora_state()
        assert all(t.dtype == torch.float32 for t in st["stash"].values())
        assert all(d.dtype == u.dtype == torch.float16 for held in st["adapters"].values() for d, u, _ in held.values())
        compare(small.fwd(hu), small.ref(("a", W_A), ("b", W_B)), rel=REL_TOL_UNET, name="LoRA merged into fp32 weights")
        hu = hu.half()
    finally:
        hu.unload_lora()
    _check_restored(hu, before)


def test_errors_on_the_device(small):
    hu = small.hu
    path = attention_paths(small.shapes)[0]
    n_out, n_in = small.shapes[path]
    with pytest.raises(ValueError, match="rank 300"):
        hu.load_lora({f"{path}.lora.down.weight": torch.zeros(300, n_in), f"{path}.lora.up.weight": torch.zeros(n_out, 300)})
    with pytest.raises(ValueError, match="no UNet keys"):
        hu.load_lora({"text_encoder.x.lora.down.weight": torch.zeros(2, 2)})
    assert not hu.has_lora()
    one = {f"{path}.lora.down.weight": torch.zeros(2, n_in), f"{path}.lora.up.weight": torch.zeros(n_out, 2)}
    try:
        names = [hu.load_lora(one)["adapter_name"] for _ in range(9)]
        assert names[:2] == ["default_0", "default_1"]
        with pytest.raises(ValueError, match="at most 8"):
            hu._sync_lora()
        with pytest.raises(ValueError, match="already loaded"):
            hu.load_lora(one, adapter_name="default_3")
    finally:
        hu.unload_lora()
    assert not hu.has_lora()


# ---------------------------------------------------------------------------------------------------------- the pipeline
def _pipe_problem(seed=31):
    g = torch.Generator().manual_seed(seed)
    return h16(torch.randn(1, 7, 64, generator=g)), h16(torch.randn(1, 7, 64, generator=g)), torch.randn(1, 4, 16, 16, generator=g)


def _gens():
    return dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                prior_noise_generator=torch.Generator().manual_seed(7))


PIPE_KW = dict(num_frames=4, num_inference_steps=4, guidance_scale=7.5, frame_similarity_sample_ratio=0.9)      # 3 steps


def test_pipeline_graph_eager_and_recapture(small):
    """graph replay == eager bit for bit with a LoRA loaded; loading, a changed scale and unloading each change the graph key and
    re-capture; a second call at the same scale reuses the captured graph"""
    hu = small.hu
    pe, ne, cond = _pipe_problem(seed=7)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, **PIPE_KW)
    pipe = pkg().I2VAdapterPipeline(unet=hu)
    key = lambda: next(iter(pipe._graph_cache))
    try:
        plain = pipe(**kw, **_gens()).frames
        k0, g0 = key(), pipe._graph
        pipe.load_lora_weights(to_state_dict(small.a, small.shapes, "kohya"), adapter_name="a")
        assert pipe.get_active_adapters() == ["a"]
        graph = pipe(**kw, **_gens()).frames
        k1, g1 = key(), pipe._graph
        assert k1 != k0 and g1 is not g0 and len(pipe._graph_cache) == 1 and not torch.equal(graph, plain), "a stale graph was replayed"
        seen = []
        eager = pipe(**kw, callback=lambda i, t, lat: seen.append(i), **_gens()).frames
        assert seen == [0, 1, 2] and torch.equal(eager, graph)
        again = pipe(**kw, **_gens()).frames
        assert key() == k1 and pipe._graph is g1 and torch.equal(again, graph), "the same LoRA state must reuse the graph"
        scaled = pipe(**kw, cross_attention_kwargs={"scale": 0.5, "cfg_shared_prefix": True, "other": 1}, **_gens()).frames
        k2, g2 = key(), pipe._graph
        assert k2 != k1 and g2 is not g1 and not torch.equal(scaled, graph) and not torch.equal(scaled, plain)
        scaled2 = pipe(**kw, cross_attention_kwargs={"scale": 0.5}, **_gens()).frames
        assert key() == k2 and pipe._graph is g2 and torch.equal(scaled2, scaled), "a second call at the same scale reuses the graph"
        assert hu._lora_state()["scale"] == 1.0, "the call's scale must not stick"
        back = pipe(**kw, **_gens()).frames
        assert torch.equal(back, graph) and key() != k2
        pipe.unload_lora_weights()
        off = pipe(**kw, **_gens()).frames
        assert torch.equal(off, plain) and pipe._graph is not g2
    finally:
        hu.unload_lora()


@pytest.mark.parametrize("use_graph", [False, True])
def test_pipeline_trajectory_against_the_merged_oracle(small, use_graph):
    from oracle.pipeline_i2v_adapter import I2VAdapterPipeline as OP
    hu = small.hu
    pe, ne, cond = _pipe_problem()
    if "traj" not in small._refs:
        with merged_oracle(small.ou, [(small.a, W_A), (small.b, W_B)]) as m:
            merged = OP(m)(pe, ne, cond, **PIPE_KW, **_gens()).frames
        small._refs["traj"] = (merged, OP(small.ou)(pe, ne, cond, **PIPE_KW, **_gens()).frames)
    ref, ref_plain = small._refs["traj"]
    pipe = pkg().I2VAdapterPipeline(unet=hu)
    small.load_both()
    try:
        got = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, condition_image_latents=cond, use_graph=use_graph, **PIPE_KW, **_gens()).frames
    finally:
        pipe.unload_lora_weights()
    assert got.shape == (1, 4, 4, 16, 16) and torch.equal(got[:, 0].cpu(), cond)
    err, scale = compare(got, ref, rel=REL_TOL_TRAJECTORY, name="3-step trajectory with a LoRA on every weight")
    moved = (ref - ref_plain).abs().max().item()
    print(f"LoRA trajectory use_graph={use_graph}: max abs latent err {err:.3e} (max|ref| {scale:.3e}); the LoRA moves the oracle by {moved:.3e}")
    assert moved > 10 * REL_TOL_TRAJECTORY * scale


# ---------------------------------------------------------------------------------------------------------- the model handle
def test_forward_plan_with_a_lora_through_the_c_abi(dev, monkeypatch, small):
    """a forward plan recorded with a LoRA merged reads the packs of the merged weights: replayed through i2v_unet_forward, with no
    kernels.py wrapper running, it equals the module forward bit for bit, also on other inputs, and differs from the plain forward"""
    p = pkg()
    H, K = p.handle, p.kernels
    hu = small.hu
    g = torch.Generator().manual_seed(5)

    def inputs(seed):
        g.manual_seed(seed)
        return dict(sample=torch.randn(2, 4, 4, 16, 16, generator=g).half().to(dev), t=torch.tensor([481.0, 37.0], device=dev),
                    ctx=torch.randn(2, 7, 64, generator=g).half().to(dev))

    def module(inp):
        with torch.no_grad():
            return hu(inp["sample"], inp["t"], True, inp["ctx"]).sample
    inp, inp2 = inputs(5), inputs(6)
    plain = module(inp)
    small.load_both()
    try:
        # recorded straight after the load: nothing has merged the LoRA yet, the recording itself must (its unrecorded first run)
        blob, weights = H.record_forward_plan(hu, inp["sample"], inp["t"], inp["ctx"])
        ref, ref2 = module(inp), module(inp2)
        hd = p.UNetHandle(hu)
        hd.plan(2, 4, 16, 16, ctx_len=7, has_ip=False)
        hd.set_plan(blob)
        hd.set_weights(weights)
        arena = torch.empty(hd.activation_bytes, dtype=torch.uint8, device=dev)
        hd.set_workspace(arena)
        out, out2 = torch.full_like(ref, float("nan")), torch.full_like(ref, float("nan"))

        def boom(*a, **k):
            raise AssertionError("a kernels.py wrapper ran during i2v_unet_forward")
        with monkeypatch.context() as m:
            for name in ("lora_merge", "gemm", "conv3x3", "attention", "groupnorm", "layernorm", "ff_fused", "motion_attn",
                         "cross_attn_fused", "ln_qkv", "temporal_attention", "nchw_to_tokens", "tokens_to_nchw", "timestep_embedding",
                         "silu", "copy3d"):
                m.setattr(K, name, boom)
            hd.forward(inp["sample"], inp["t"], inp["ctx"], None, out)
            hd.forward(inp2["sample"], inp2["t"], inp2["ctx"], None, out2)
            torch.cuda.synchronize()
        hd.close()
    finally:
        hu.unload_lora()
    assert torch.equal(out, ref), f"C-ABI forward differs from the module API: max |d| {(out.float() - ref.float()).abs().max().item():.3e}"
    assert torch.equal(out2, ref2) and not torch.equal(out, plain)
    assert torch.equal(module(inp), plain)


# ---------------------------------------------------------------------------------------------------------- training
def test_training_refuses_a_lora_on_trained_parameters(small):
    from i2v_adapter_unofficial_amd import training
    hu = small.hu
    pick = lambda frag: {p: small.a[p] for p in small.shapes if frag in p}
    try:
        frozen = [p for p in pick(".attn2.to_k") if ".motion_modules." not in p]
        assert frozen
        hu.load_lora(to_state_dict({p: small.a[p] for p in frozen}, small.shapes, "diffusers"), adapter_name="frozen")
        training.UNetAdapterTrainer(hu)                                        # a LoRA on frozen weights only: fine
        hu.load_lora(to_state_dict(pick(".motion_modules.0.proj_in"), small.shapes, "diffusers"), adapter_name="motion")
        training.UNetAdapterTrainer(hu)
        with pytest.raises(RuntimeError, match="LoRA state"):
            training.UNetAdapterTrainer(hu, update_motion_modules=True)
        with pytest.raises(RuntimeError, match="LoRA state"):
            training.AdapterOptimizer(hu, update_motion_modules=True)
        hu.load_lora(to_state_dict(pick(".i2v_adapter.to_q"), small.shapes, "diffusers"), adapter_name="adapter")
        with pytest.raises(RuntimeError, match="i2v_adapter.to_q.weight"):
            training.UNetAdapterTrainer(hu)
        with pytest.raises(RuntimeError, match="LoRA state"):
            training.AdapterOptimizer(hu)
    finally:
        hu.unload_lora()
    training.UNetAdapterTrainer(hu)
