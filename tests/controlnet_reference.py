"""fp32 CPU reference of diffusers 0.24 `ControlNetModel` (SD-1.5 layout) for the ControlNet tests: composed from `oracle.blocks`
(ResnetBlock2D, BasicTransformerBlock, Downsample2D, Timesteps, TimestepEmbedding) plus its own conditioning embedding, spatial
transformer wrapper and zero convolutions, with the state-dict keys of the product model, so that one state dict loads into both.
Weights are RANDOM everywhere, the "zero" convolutions included: a zero-initialised zero convolution tests nothing.

Also the small problem the GPU tests share (`small_*`), and the plain evaluations of `i2v_add_residuals_f16` in fp64.
"""
import torch
import torch.nn.functional as F
from torch import nn

from oracle.blocks import BasicTransformerBlock, Downsample2D, ResnetBlock2D, TimestepEmbedding, Timesteps

from tests.parity import SMALL_UNET, round_fp16_

SMALL_COND_CHANNELS = (8, 16, 16, 32)
SMALL_FRAMES, SMALL_LATENT, SMALL_TOKENS = 2, 16, 7


class RefTransformer2D(nn.Module):
    """diffusers Transformer2DModel, continuous input, one block: GroupNorm(eps 1e-6) -> 1x1 proj_in -> block -> 1x1 proj_out, + input."""

    def __init__(self, heads, channels, cross_attention_dim, groups):
        super().__init__()
        self.norm = nn.GroupNorm(groups, channels, eps=1e-6, affine=True)
        self.proj_in = nn.Conv2d(channels, channels, 1)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(channels, heads, channels // heads,
                                                                       cross_attention_dim=cross_attention_dim)])
        self.proj_out = nn.Conv2d(channels, channels, 1)

    def forward(self, x, ctx):
        n, c, h, w = x.shape
        t = self.proj_in(self.norm(x)).permute(0, 2, 3, 1).reshape(n, h * w, c)
        for blk in self.transformer_blocks:
            t = blk(t, encoder_hidden_states=ctx)
        return self.proj_out(t.reshape(n, h, w, c).permute(0, 3, 1, 2)) + x


class RefConditioningEmbedding(nn.Module):
    def __init__(self, out_channels, cond_channels, block_out_channels):
        super().__init__()
        self.conv_in = nn.Conv2d(cond_channels, block_out_channels[0], 3, padding=1)
        blocks = []
        for a, b in zip(block_out_channels[:-1], block_out_channels[1:]):
            blocks += [nn.Conv2d(a, a, 3, padding=1), nn.Conv2d(a, b, 3, padding=1, stride=2)]
        self.blocks = nn.ModuleList(blocks)
        self.conv_out = nn.Conv2d(block_out_channels[-1], out_channels, 3, padding=1)

    def forward(self, cond):
        x = F.silu(self.conv_in(cond))
        for b in self.blocks:
            x = F.silu(b(x))
        return self.conv_out(x)


class RefControlNet(nn.Module):
    def __init__(self, in_channels=4, conditioning_channels=3, block_out_channels=(320, 640, 1280, 1280), layers_per_block=2,
                 cross_attention_dim=768, attention_head_dim=8, norm_num_groups=32, norm_eps=1e-5,
                 conditioning_embedding_out_channels=(16, 32, 96, 256),
                 down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D")):
        super().__init__()
        c0, temb = block_out_channels[0], 4 * block_out_channels[0]
        heads = attention_head_dim
        self.conv_in = nn.Conv2d(in_channels, c0, 3, padding=1)
        self.time_proj = Timesteps(c0, True, 0)
        self.time_embedding = TimestepEmbedding(c0, temb)
        self.controlnet_cond_embedding = RefConditioningEmbedding(c0, conditioning_channels, conditioning_embedding_out_channels)
        self.down_blocks = nn.ModuleList()
        zero = [nn.Conv2d(c0, c0, 1)]
        oc = c0
        for i, t in enumerate(down_block_types):
            ic, oc = oc, block_out_channels[i]
            final = i == len(block_out_channels) - 1
            blk = nn.Module()
            blk.resnets = nn.ModuleList([ResnetBlock2D(ic if j == 0 else oc, oc, temb_channels=temb, eps=norm_eps, groups=norm_num_groups)
                                         for j in range(layers_per_block)])
            if "CrossAttn" in t:
                blk.attentions = nn.ModuleList([RefTransformer2D(heads, oc, cross_attention_dim, norm_num_groups)
                                                for _ in range(layers_per_block)])
            blk.downsamplers = None if final else nn.ModuleList([Downsample2D(oc, padding=1)])
            self.down_blocks.append(blk)
            zero += [nn.Conv2d(oc, oc, 1) for _ in range(layers_per_block + (0 if final else 1))]
        self.controlnet_down_blocks = nn.ModuleList(zero)
        c = block_out_channels[-1]
        self.controlnet_mid_block = nn.Conv2d(c, c, 1)
        self.mid_block = nn.Module()
        self.mid_block.attentions = nn.ModuleList([RefTransformer2D(heads, c, cross_attention_dim, norm_num_groups)])
        self.mid_block.resnets = nn.ModuleList([ResnetBlock2D(c, c, temb_channels=temb, eps=norm_eps, groups=norm_num_groups)
                                                for _ in range(2)])

    def forward(self, sample, timestep, ctx, cond, conditioning_scale=1.0):
        """sample (N, C, H, W) with N = B * F; timestep [B]; ctx [B, L, D]; cond (N, 3, 8 H, 8 W).  The frames of a clip share the
        clip's timestep and prompt (repeat_interleave, as the UNet does at unet:1344, 1355)."""
        n, b = sample.shape[0], ctx.shape[0]
        temb = self.time_embedding(self.time_proj(timestep.float().expand(b))).repeat_interleave(n // b, dim=0)
        ctx = ctx.repeat_interleave(n // b, dim=0)
        x = self.conv_in(sample) + self.controlnet_cond_embedding(cond)
        res = [x]
        for blk in self.down_blocks:
            for j, r in enumerate(blk.resnets):
                x = r(x, temb)
                if hasattr(blk, "attentions"):
                    x = blk.attentions[j](x, ctx)
                res.append(x)
            if blk.downsamplers is not None:
                x = blk.downsamplers[0](x)
                res.append(x)
        x = self.mid_block.resnets[0](x, temb)
        x = self.mid_block.attentions[0](x, ctx)
        x = self.mid_block.resnets[1](x, temb)
        down = tuple(z(r) * conditioning_scale for z, r in zip(self.controlnet_down_blocks, res))
        return down, self.controlnet_mid_block(x) * conditioning_scale


def small_config():
    """the product model's constructor arguments for the small problem (tests.parity.SMALL_UNET's encoder)"""
    return dict(block_out_channels=SMALL_UNET["block_out_channels"], attention_head_dim=SMALL_UNET["num_attention_heads"],
                norm_num_groups=SMALL_UNET["norm_num_groups"], cross_attention_dim=SMALL_UNET["cross_attention_dim"],
                conditioning_embedding_out_channels=SMALL_COND_CHANNELS)


def small_reference(seed=4321):
    """random weights everywhere (torch's default initialisers: the zero convolutions are ordinary convolutions here), norm affines
    jittered, every value representable in fp16"""
    torch.manual_seed(seed)
    m = RefControlNet(**small_config())
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (nn.GroupNorm, nn.LayerNorm)):
                mod.weight.add_(torch.randn(mod.weight.shape, generator=g) * 0.1)
                mod.bias.add_(torch.randn(mod.bias.shape, generator=g) * 0.1)
    return round_fp16_(m).eval()


def small_inputs(batch=1, seed=17):
    g = torch.Generator().manual_seed(seed)
    h = lambda t: t.half().float()
    n = batch * SMALL_FRAMES
    return dict(sample=h(torch.randn(n, 4, SMALL_LATENT, SMALL_LATENT, generator=g)),
                timestep=torch.tensor([481.0, 37.0][:batch]),
                ctx=h(torch.randn(batch, SMALL_TOKENS, SMALL_UNET["cross_attention_dim"], generator=g)),
                cond=h(torch.rand(n, 3, 8 * SMALL_LATENT, 8 * SMALL_LATENT, generator=g)))


# ---------------------------------------------------------------------------------------------- i2v_add_residuals_f16 in fp64
def add_residuals_fp64(skip, res, s, lo=None):
    """skip (+ lo) + s * res in fp64; skip / lo / res are fp16 tensors, s a python float that is exact in fp32"""
    ref = skip.double() + float(s) * res.double()
    return ref if lo is None else ref + lo.double()


def add_residuals_bound(skip, res, s, lo=None):
    """the per-element bounds derived in tests/test_controlnet_gpu.py's header (the issue's, with the terms the derivation gives tighter
    taken in the tighter form)"""
    sr = (float(s) * res.double()).abs()
    ref = add_residuals_fp64(skip, res, s, lo).abs()
    if lo is None:
        return 2.0 ** -11 * ref + 2.0 ** -24 * (skip.double().abs() + 2.0 * sr) + 2.0 ** -24
    return 2.0 ** -22 * ref + 2.0 ** -23 * (skip.double().abs() + lo.double().abs() + sr) + 2.0 ** -24


# the kernel test's problem: 13 tensors in one launch (8 values = one 16-byte chunk; 8 * 37 = a part of one tile; 8 * (256 * 4 + 3) = one
# 1024-chunk tile and three chunks of the next; exact tiles; several tiles = more than one workgroup), a 3-row table read at row 2
KERNEL_SIZES = (8, 8 * 37, 8 * (256 * 4 + 3), 8 * 1024, 8 * 2048, 8 * 1023, 8 * 1025, 16, 8 * 5000, 8 * 255, 8 * 257, 8 * 64, 8 * 3 * 1024 + 8)
KERNEL_SCALES = (0.0, 1.0, -0.75)
KERNEL_ROW = 2


def kernel_table(s):
    """3 rows, row 2 = s; its neighbour (row 1) differs from s by at least 0.5"""
    return torch.tensor([s + 2.0, s + 0.5, s], dtype=torch.float32)


def kernel_case(seed=3, sizes=KERNEL_SIZES):
    """(skips, lows, residuals): fp16 CPU tensors; skip + low is a proper pair (low = the fp16 rounding's remainder of an fp32 value)"""
    g = torch.Generator().manual_seed(seed)
    skips, lows, ress = [], [], []
    for n in sizes:
        x = torch.randn(n, generator=g) * 2.0
        hi = x.half()
        skips.append(hi)
        lows.append((x - hi.float()).half())
        ress.append((torch.randn(n, generator=g) * 0.7).half())
    return skips, lows, ress


def neighbour_residual(ress, i):
    """the residual of the neighbouring tensor, cut or tiled to tensor i's size (what a wrong prefix-sum walk would read)"""
    r = ress[(i + 1) % len(ress)]
    n = ress[i].numel()
    return r.repeat((n + r.numel() - 1) // r.numel())[:n]
