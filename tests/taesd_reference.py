"""AutoencoderTiny (TAESD) in plain torch: the specification of i2v_adapter_unofficial_amd.autoencoder_tiny.

diffusers is not installed where this was written, so the layout is restated from diffusers 0.24's `AutoencoderTiny` / `EncoderTiny` /
`DecoderTiny` / `AutoencoderTinyBlock` source; `tests/golden/taesd_keys.txt` is the resulting state-dict key list.  Three evaluations:

* `TaesdReference`: the fp32 restatement, built in the same `nn.Sequential` order (so the state-dict keys are diffusers').
* `run_fp16_storage`: the same layers with every STORED activation rounded to fp16 -- the entry map's output, every convolution's
  output after its ReLU (a block's closing convolution after the residual and the ReLU: one rounding), the fp32 exit not at all --
  and accumulation in fp32 (or fp64: `accumulate=`).  That is what any fp16-activation implementation computes, up to summation order.
* `layer_fp64`: one layer -- convolution + bias + residual + ReLUs (+ out_scale) -- in fp64 from fp16 operands, with the per-element
  accumulation bound of tests/gemm_bounds.py beside it, and five deliberately WRONG evaluations (`MUTANTS`) the bound must reject.
"""
import torch
import torch.nn.functional as F
from torch import nn

U23 = 2.0 ** -23
MUTANTS = ("tap_shift", "neighbour_halo", "no_bias", "relu_before_residual", "swap_halves")


# ------------------------------------------------------------------------------------------------------- the fp32 restatement
class TinyBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(c, c, 3, padding=1), nn.ReLU(), nn.Conv2d(c, c, 3, padding=1), nn.ReLU(),
                                  nn.Conv2d(c, c, 3, padding=1))
        self.skip = nn.Identity()
        self.fuse = nn.ReLU()

    def forward(self, x):
        return self.fuse(self.conv(x) + self.skip(x))


class _Layers(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layers = nn.Sequential(*layers)


def encoder_layers(in_channels=3, out_channels=4, num_blocks=(1, 3, 3, 3), widths=(64, 64, 64, 64)):
    layers = []
    for i, nb in enumerate(num_blocks):
        c = widths[i]
        layers.append(nn.Conv2d(in_channels, c, 3, padding=1) if i == 0 else nn.Conv2d(c, c, 3, padding=1, stride=2, bias=False))
        layers += [TinyBlock(c) for _ in range(nb)]
    layers.append(nn.Conv2d(widths[-1], out_channels, 3, padding=1))
    return layers


def decoder_layers(in_channels=4, out_channels=3, num_blocks=(3, 3, 3, 1), widths=(64, 64, 64, 64)):
    layers = [nn.Conv2d(in_channels, widths[0], 3, padding=1), nn.ReLU()]
    for i, nb in enumerate(num_blocks):
        final, c = i == len(num_blocks) - 1, widths[i]
        layers += [TinyBlock(c) for _ in range(nb)]
        if not final:
            layers.append(nn.Upsample(scale_factor=2))
        layers.append(nn.Conv2d(c, out_channels if final else c, 3, padding=1, bias=final))
    return layers


class TaesdReference(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = _Layers(encoder_layers())
        self.decoder = _Layers(decoder_layers())

    def encode(self, x):
        return self.encoder.layers((x + 1) / 2)

    def decode(self, z):
        return self.decoder.layers(3 * torch.tanh(z / 3)) * 2 - 1


def seeded_reference(seed=0, gain=1.0):
    """a TaesdReference with seeded weights that are fp16 values (every evaluation then reads the same numbers): torch's default
    Conv2d law U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) times sqrt(3) `gain` -- unit-variance-preserving at gain 1, so that 40 layers
    neither die out nor blow up -- and biases U(-0.1, 0.1)"""
    g = torch.Generator().manual_seed(seed)
    m = TaesdReference().float().eval()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.Conv2d):
                bound = gain * (3.0 / mod.weight[0].numel()) ** 0.5
                mod.weight.copy_(((torch.rand(mod.weight.shape, generator=g) * 2 - 1) * bound).half().float())
                if mod.bias is not None:
                    mod.bias.copy_(((torch.rand(mod.bias.shape, generator=g) * 2 - 1) * 0.1).half().float())
    return m


# ------------------------------------------------------------------------------------------------------- fp16 storage
def _r16(t):
    return t.half().to(t.dtype)


def _conv(x, conv, dt):
    return F.conv2d(x.to(dt), conv.weight.to(dt), None if conv.bias is None else conv.bias.to(dt), stride=conv.stride, padding=1)


@torch.no_grad()
def run_fp16_storage(model, t, which, accumulate=torch.float32):
    """`encode` / `decode` of a TaesdReference with every stored activation rounded to fp16; returns fp32"""
    dt = accumulate
    t = t.to(dt)
    if which == "encode":
        x, mods = _r16((t + 1) / 2), list(model.encoder.layers)
    else:
        x, mods = _r16(3 * torch.tanh(t / 3)), list(model.decoder.layers)
    i = 0
    while i < len(mods):
        m = mods[i]
        last = i == len(mods) - 1
        if isinstance(m, TinyBlock):
            h = _r16(F.relu(_conv(x, m.conv[0], dt)))
            h = _r16(F.relu(_conv(h, m.conv[2], dt)))
            x = _r16(F.relu(_conv(h, m.conv[4], dt) + x))
        elif isinstance(m, nn.Upsample):
            x = _r16(_conv(F.interpolate(x, scale_factor=2, mode="nearest"), mods[i + 1], dt))
            i += 1
        elif isinstance(m, nn.Conv2d):
            y = _conv(x, m, dt)
            if not last and isinstance(mods[i + 1], nn.ReLU):
                y = F.relu(y)
                i += 1
            x = y if last else _r16(y)
        else:
            raise NotImplementedError(type(m).__name__)
        i += 1
    if which == "decode":
        x = x * 2 - 1
    return x.float()


# ------------------------------------------------------------------------------------------------------- one layer in fp64
def layer_fp64(x, w, bias=None, residual=None, relu_mid=False, relu_out=False, stride=1, upsample=False, out_scale=1.0, mutant=None):
    """out_scale * act_out(act_mid(conv3x3(x) + bias) + residual) in fp64 from fp16 operands.

    x [N, H, W, Cin] (token-major), w [Cout, Cin, 3, 3], bias [Cout], residual [N, H', W', Cout]; pad 1; `upsample`: nearest-2x first.
    Returns (ref [N, H', W', Cout], tol): tol = K 2^-23 S |out_scale| with K = 9 Cin and S = |x| * |w| + |bias| + |residual| -- the
    accumulation term of tests/gemm_bounds.py for an fp32 accumulation of exact fp16 products in any order.  ReLU is 1-Lipschitz, so
    an error bound of its argument is one of its value: the term passes through both activations unchanged.
    mutant: one of MUTANTS -- the same layer evaluated WRONGLY (the returned tol is then meaningless)."""
    xd = x.double().permute(0, 3, 1, 2)
    wd = w.double()
    if upsample:
        xd = F.interpolate(xd, scale_factor=2, mode="nearest")
    n, cin, h, wdt = xd.shape
    if mutant == "swap_halves":            # the two 32-channel halves of the contraction against each other
        wd = torch.cat([wd[:, cin // 2:], wd[:, : cin // 2]], dim=1)
    xp = F.pad(xd, (1, 1, 1, 1))
    if mutant == "neighbour_halo":         # the rows above / below an image are its neighbours' in memory, not zeros
        xp[:, :, 0, 1:-1] = xd.roll(1, 0)[:, :, -1]
        xp[:, :, -1, 1:-1] = xd.roll(-1, 0)[:, :, 0]
    oh, ow = (h - 1) // stride + 1, (wdt - 1) // stride + 1
    acc = torch.zeros((n, w.shape[0], oh, ow), dtype=torch.float64)
    S = torch.zeros_like(acc)
    xq = F.pad(xp, (0, 1, 0, 0))            # (room for the shifted tap)
    for ky in range(3):
        for kx in range(3):
            sx = kx + 1 if (mutant == "tap_shift" and ky == 1 and kx == 1) else kx      # the centre tap reads one pixel to the right
            win = xq[:, :, ky: ky + stride * (oh - 1) + 1: stride, sx: sx + stride * (ow - 1) + 1: stride]
            acc += torch.einsum("nchw,oc->nohw", win, wd[:, :, ky, kx])
            S += torch.einsum("nchw,oc->nohw", win.abs(), wd[:, :, ky, kx].abs())
    if bias is not None and mutant != "no_bias":
        acc = acc + bias.double()[None, :, None, None]
        S = S + bias.double().abs()[None, :, None, None]
    if mutant == "relu_before_residual":
        acc = F.relu(acc)
        if residual is not None:
            acc = acc + residual.double().permute(0, 3, 1, 2)
    else:
        if relu_mid:
            acc = F.relu(acc)
        if residual is not None:
            acc = acc + residual.double().permute(0, 3, 1, 2)
            S = S + residual.double().abs().permute(0, 3, 1, 2)
        if relu_out:
            acc = F.relu(acc)
    K = 9 * cin
    return (acc * out_scale).permute(0, 2, 3, 1).contiguous(), (K * U23 * abs(out_scale) * S).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------------- the kernel's test cases
SIZES = ((1, 1, 1), (2, 8, 16), (3, 9, 17), (2, 5, 40))       # (N, H, W): one pixel; exactly one 8 x 16 tile; one past in both; ragged
# (name, bias, relu_mid, relu_out, residual: None / "own" / "out", input pixel stride, output pixel stride)
CONFIGS = (("bias-mid", True, True, False, None, 64, 72),
           ("plain", False, False, False, None, 72, 64),
           ("bias-out-res", True, False, True, "own", 72, 72),
           ("bias-both-inplace", True, True, True, "out", 64, 64),
           ("out-res", False, False, True, "own", 72, 72))
CASES = tuple((s, c) for s in SIZES for c in CONFIGS)


def case_id(case):
    (n, h, w), cfg = case
    return f"{n}x{h}x{w}-{cfg[0]}"


def mutants_of(cfg):
    """the wrong evaluations that CAN differ for a configuration: a missing bias needs a bias, the misplaced ReLU a residual behind a
    closing ReLU"""
    out = ["tap_shift", "neighbour_halo", "swap_halves"]
    if cfg[1]:
        out.append("no_bias")
    if cfg[3] and cfg[4]:
        out.append("relu_before_residual")
    return out


def case_inputs(case):
    """fp16 CPU operands of a case, seeded by its name: x, w, bias, residual (None where the configuration has none)"""
    import zlib
    (n, h, w), cfg = case
    g = torch.Generator().manual_seed(zlib.crc32(case_id(case).encode()))
    x = torch.randn((n, h, w, 64), generator=g).half()
    wt = ((torch.rand((64, 64, 3, 3), generator=g) * 2 - 1) * (3.0 / 576) ** 0.5).half()
    bias = ((torch.rand(64, generator=g) * 2 - 1) * 0.5).half() if cfg[1] else None
    res = torch.randn((n, h, w, 64), generator=g).half() if cfg[4] else None
    return x, wt, bias, res
