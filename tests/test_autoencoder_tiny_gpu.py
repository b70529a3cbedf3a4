"""AutoencoderTiny on the GPU against tests/taesd_reference.py: seeded weights, images of 32 x 32 and 40 x 24, latents of 4 x 4 and
5 x 3.  Three gates and a pipeline run:

* binding, teacher-forced: every layer's HIP output against the fp64 layer applied to the HIP path's OWN fp16 input of that layer,
  with the derived per-element bound (tests/gemm_bounds.py: K 2^-23 S with the layer's K and operand sums) -- the layers that run on
  the existing kernels included;
* end to end: the yardstick is the largest error of the CPU fp16-storage variant against the fp32 restatement on the same input; the
  HIP model may miss the fp32 restatement by at most twice that (the accumulation order differs and the roundings of ~40 layers add
  roughly in quadrature; a wrong tap or a lost ReLU is orders of magnitude above);
* batch independence: the decode of a batch is its frames' decodes, bit for bit.
"""
import PIL.Image
import pytest
import torch

from tests import gemm_bounds as B
from tests import taesd_reference as R

pytestmark = pytest.mark.gpu


def pkg():
    import i2v_adapter_unofficial_amd as p
    return p


@pytest.fixture(scope="module")
def pair(dev):
    ref = R.seeded_reference(0)
    hv = pkg().AutoencoderTiny()
    hv.load_state_dict(ref.state_dict())
    return ref, hv.to(dev).eval()


def _inputs():
    g = torch.Generator().manual_seed(11)
    return {"encode": [torch.rand((2, 3, 32, 32), generator=g) * 2 - 1, torch.rand((1, 3, 40, 24), generator=g) * 2 - 1],
            "decode": [torch.randn((2, 4, 4, 4), generator=g) * 1.5, torch.randn((1, 4, 5, 3), generator=g) * 1.5]}


def _folded_fp64(x, wf):
    """the up-sampling convolution as the kernel reads it: four 2 x 2 convolutions of x [N, H, W, 64] with the FOLDED fp16 weights
    wf [4, Cout, 4 * 64] (blocks.pack_upconv_fold; k = 64 t + ci, t = 2 ty + tx), in fp64, and the bound's operand sums"""
    n, h, w, c = x.shape
    xp = torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1))
    out = torch.zeros((n, 2 * h, 2 * w, wf.shape[1]), dtype=torch.float64)
    S = torch.zeros_like(out)
    wd = wf.double().view(4, wf.shape[1], 4, c)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    win = xp[:, py + ty: py + ty + h, px + tx: px + tx + w]          # source pixel (i + py - 1 + ty, j + px - 1 + tx)
                    wt = wd[2 * py + px, :, 2 * ty + tx]
                    out[:, py::2, px::2] += torch.einsum("nhwc,oc->nhwo", win, wt)
                    S[:, py::2, px::2] += torch.einsum("nhwc,oc->nhwo", win.abs(), wt.abs())
    return out, 4 * c * R.U23 * S


@pytest.mark.parametrize("which", ("encode", "decode"))
def test_every_layer_binds_teacher_forced(dev, pair, which):
    ref, hv = pair
    k = pkg().kernels
    plan = {op[1]: op for op in hv.packed()[which + "r"]}
    for t in _inputs()[which]:
        hv._trace = []
        try:
            getattr(hv, which)(t.to(dev))
        finally:
            trace, hv._trace = hv._trace, None
        kinds = [e[1] for e in trace]
        assert kinds.count("block") == 30 and kinds.count("c64") == 1 and kinds.count("exit") == 1 and kinds.count("prep") == 1
        assert kinds.count("down" if which == "encode" else "up") == 3
        for name, kind, x, y, res in trace:
            if kind == "prep":
                continue
            x, y = x.cpu(), y.cpu()
            if kind == "up" and k.upconv_fold_supported(tuple(x.shape), 64):
                want, tol = _folded_fp64(x, plan[name][3].cpu())
            else:
                conv = ref.get_submodule(name)
                w16 = conv.weight.detach().half()
                if x.shape[-1] > w16.shape[1]:                                  # the entry convolutions: zero-padded input channels
                    w16 = torch.nn.functional.pad(w16, (0, 0, 0, 0, 0, x.shape[-1] - w16.shape[1]))
                bias = None if conv.bias is None else conv.bias.detach().half()
                kw = {}
                if kind == "block":
                    kw = dict(relu_mid=not name.endswith("conv.4"), relu_out=name.endswith("conv.4"), residual=None if res is None else res.cpu())
                    assert (res is not None) == name.endswith("conv.4")
                elif kind == "c64":
                    kw = dict(relu_mid=which == "decode")
                elif kind == "down":
                    kw = dict(stride=2)
                elif kind == "up":
                    kw = dict(upsample=True)
                elif kind == "exit":
                    bias, kw = plan[name][3].cpu(), dict(out_scale=plan[name][4])
                want, tol = R.layer_fp64(x, w16, bias, **kw)
            assert tuple(y.shape) == tuple(want.shape), name
            ex = B.excess(y, want, tol)
            assert bool(torch.isfinite(y.float()).all()) and not bool((ex > 0).any()), \
                f"{name} ({kind}) at {tuple(x.shape)}: {int((ex > 0).sum())}/{ex.numel()} elements miss the bound, largest excess {float(ex.max()):.3e}"


@pytest.mark.parametrize("which", ("encode", "decode"))
def test_end_to_end_within_twice_the_fp16_storage_error(dev, pair, which):
    ref, hv = pair
    for t in _inputs()[which]:
        with torch.no_grad():
            exact = getattr(ref, which)(t)
            yard = float((R.run_fp16_storage(ref, t, which) - exact).abs().max())
        out = getattr(hv, which)(t.to(dev))
        got = (out.latents if which == "encode" else out.sample).cpu()
        assert got.dtype == torch.float32 and got.shape == exact.shape
        err = float((got - exact).abs().max())
        print(f"{which} {tuple(t.shape)}: HIP vs fp32 restatement {err:.3e}, fp16-storage variant vs fp32 restatement {yard:.3e}, "
              f"max |ref| {float(exact.abs().max()):.3e}")
        assert bool(torch.isfinite(got).all()) and err <= 2 * yard, (which, tuple(t.shape), err, yard)


def test_decode_of_a_batch_is_its_frames_decodes(dev, pair):
    _, hv = pair
    g = torch.Generator().manual_seed(5)
    for z in (torch.randn((3, 4, 5, 3), generator=g), torch.randn((4, 4, 4, 4), generator=g)):
        z = z.to(dev)
        whole = hv.decode(z).sample
        for i in range(z.shape[0]):
            assert torch.equal(whole[i: i + 1], hv.decode(z[i: i + 1]).sample), i
    x = (torch.rand((3, 3, 40, 24), generator=g) * 2 - 1).to(dev)
    lat = hv.encode(x).latents
    assert all(torch.equal(lat[i: i + 1], hv.encode(x[i: i + 1]).latents) for i in range(3))


def _small_pipe(vae, dev):
    from tests.parity import hip_unet_from_oracle, oracle_small_unet
    return pkg().I2VAdapterPipeline(vae=vae, unet=hip_unet_from_oracle(oracle_small_unet(), dev))


def _call_args():
    g = torch.Generator().manual_seed(3)
    image = PIL.Image.fromarray((torch.rand(80, 72, 3, generator=g) * 255).to(torch.uint8).numpy())
    h = lambda t: t.half().float()
    kw = dict(prompt_embeds=h(torch.randn(1, 7, 64, generator=g)), negative_prompt_embeds=h(torch.randn(1, 7, 64, generator=g)),
              condition_image=image, height=64, width=48, num_frames=4, num_inference_steps=4, guidance_scale=7.5,
              frame_similarity_sample_ratio=0.3)
    gens = lambda: dict(generator=torch.Generator().manual_seed(5), prior_mask_generator=torch.Generator().manual_seed(6),
                        prior_noise_generator=torch.Generator().manual_seed(7))
    return image, kw, gens


def test_pipeline_with_autoencoder_tiny(dev, pair):
    from tests.parity import host_threads
    host_threads()
    _, hv = pair
    pipe = _small_pipe(hv, dev)
    assert pipe.vae_scale_factor == 8
    image, kw, gens = _call_args()
    lat = pipe(output_type="latent", **kw, **gens()).frames
    vid = pipe(output_type="pt", **kw, **gens()).frames
    assert lat.shape == (1, 4, 4, 8, 6) and vid.shape == (1, 4, 3, 64, 48) and bool(torch.isfinite(vid).all())
    assert torch.equal(vid[0], hv.decode(lat[0] / hv.config["scaling_factor"]).sample)
    pipe.enable_vae_slicing()
    assert torch.equal(pipe(output_type="pt", **kw, **gens()).frames, vid)
    pre = pipe.image_processor.preprocess(image, height=64, width=48)
    got = pipe.encode_condition_image(image, 64, 48, generator=torch.Generator().manual_seed(5))
    assert got.shape == (1, 4, 8, 6) and torch.equal(got, hv.encode(pre.to(dev)).latents)
    with pytest.raises(NotImplementedError, match="tiled"):
        pipe.enable_vae_tiling()


def test_pipeline_with_autoencoder_kl_is_unchanged(dev):
    """the pipeline's two VAE steps with an AutoencoderKL are the VAE's own calls, as before: frames = vae.decode(latents / sf).sample
    and the condition latents = vae.encode(image).latent_dist.sample(generator) * sf, bit for bit"""
    from tests.parity import hip_model_random
    hv = hip_model_random(dict(block_out_channels=(32, 64, 64, 64), norm_num_groups=8, sample_size=32), dev, seed=31, cls=pkg().AutoencoderKL)
    pipe = _small_pipe(hv, dev)
    image, kw, gens = _call_args()
    sf = hv.config["scaling_factor"]
    lat = pipe(output_type="latent", **kw, **gens()).frames
    vid = pipe(output_type="pt", **kw, **gens()).frames
    assert torch.equal(vid[0], hv.decode((1 / sf * lat)[0]).sample)
    pre = pipe.image_processor.preprocess(image, height=64, width=48)
    got = pipe.encode_condition_image(image, 64, 48, generator=torch.Generator().manual_seed(5))
    assert torch.equal(got, hv.encode(pre.to(dev)).latent_dist.sample(torch.Generator().manual_seed(5)) * sf)
