"""Real-ESRGAN's compact upscaler (SRVGGNetCompact) in plain torch: the specification of i2v_adapter_unofficial_amd.upscaler.

Real-ESRGAN is not installed where this was written and no released checkpoint is at hand, so the layout is restated from its
`realesrgan/archs/srvgg_arch.py`; `tests/golden/srvgg_keys.txt` is the resulting state-dict key list for num_conv 16 and 32.

* `SRVGGReference`: the fp32 restatement, `body` built in upstream's order (so the state-dict keys are upstream's).
* `seeded_reference`: seeded weights that are fp16 values, slopes that are arbitrary fp32.
* `run_fp16_storage`: the same layers with every STORED activation rounded to fp16 -- the entry map's output, every convolution's
  output after its activation, the exit convolution's output -- and accumulation in fp32 (or fp64: `accumulate=`); the base of the
  exit is the unrounded source.  That is what any fp16-activation implementation computes, up to summation order.
* `layer_fp64`: one layer -- convolution + bias + PReLU + residual + closing ReLU -- in fp64 from fp16 operands with its bound, and
  four deliberately WRONG evaluations (`LAYER_MUTANTS`) the bound must reject.
* `exit_fp64`: the exit kernel -- pixel shuffle + nearest base + clamp + range map -- in fp64 with its bound, and five wrong ones
  (`EXIT_MUTANTS`).
"""
import zlib

import torch
import torch.nn.functional as F
from torch import nn

from tests import taesd_reference as T

U22 = 2.0 ** -22
LAYER_MUTANTS = ("slope_rot8", "slope_swap_halves", "slope_after_residual", "relu_for_prelu")
EXIT_MUTANTS = ("dy_dx_transposed", "colour_minor", "no_base", "bilinear_base", "clamp_after_range")


# ------------------------------------------------------------------------------------------------------- the fp32 restatement
class SRVGGReference(nn.Module):
    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=64, num_conv=16, upscale=4, act_type="prelu"):
        super().__init__()
        self.num_in_ch, self.num_out_ch, self.num_feat, self.num_conv, self.upscale, self.act_type = \
            num_in_ch, num_out_ch, num_feat, num_conv, upscale, act_type

        def act():
            if act_type == "relu":
                return nn.ReLU(inplace=True)
            if act_type == "prelu":
                return nn.PReLU(num_parameters=num_feat)
            return nn.LeakyReLU(negative_slope=0.1, inplace=True)

        self.body = nn.ModuleList()
        self.body.append(nn.Conv2d(num_in_ch, num_feat, 3, 1, 1))
        self.body.append(act())
        for _ in range(num_conv):
            self.body.append(nn.Conv2d(num_feat, num_feat, 3, 1, 1))
            self.body.append(act())
        self.body.append(nn.Conv2d(num_feat, num_out_ch * upscale * upscale, 3, 1, 1))
        self.upsampler = nn.PixelShuffle(upscale)

    def forward(self, x):
        out = x
        for m in self.body:
            out = m(out)
        out = self.upsampler(out)
        return out + F.interpolate(x, scale_factor=self.upscale, mode="nearest")


def entry_map(frames):
    """[-1, 1] frames -> the network's RGB in [0, 1]"""
    return ((frames + 1) / 2).clamp(0, 1)


def leave_map(v, signed):
    """the caller's clamp, and the way back to [-1, 1]"""
    v = v.clamp(0, 1)
    return 2 * v - 1 if signed else v


# second moment of PReLU(v) per unit of v's, v symmetric, slope a ~ U(-0.3, 1.3):  (1 + E a^2) / 2 = (1 + 0.25 + 1.6^2 / 12) / 2
_ACT_MOMENT = (1 + 0.25 + 1.6 ** 2 / 12) / 2


def seeded_reference(num_conv=16, upscale=4, seed=0, exit_gain=0.05):
    """a SRVGGReference with seeded weights that are fp16 values (every evaluation then reads the same numbers) and slopes that are
    arbitrary fp32 in (-0.3, 1.3) with an exact 0 at channel 5 and an exact 1 at channel 37 of every PReLU.  Weights U(-b, b): a
    layer's output second moment is fan_in b^2 / 3 times its input's, and a PReLU with such slopes keeps 0.73 of it, so b =
    sqrt(3 / (0.73 fan_in)) for the 64 -> 64 layers holds the activations at order 1 over 34 layers -- neither dying nor blowing up;
    the entry layer reads U(0, 1) pixels (second moment 1 / 3): b = sqrt(9 / fan_in).  The exit layer's b is `exit_gain` times the
    preserving one and its bias U(-0.02, 0.02), so that the body adds a few percent of the range to the base and few outputs
    saturate (`saturated_fraction`); the other biases are U(-0.1, 0.1)."""
    g = torch.Generator().manual_seed(seed)
    m = SRVGGReference(num_conv=num_conv, upscale=upscale).float().eval()
    last = len(m.body) - 1
    with torch.no_grad():
        for i, mod in enumerate(m.body):
            if isinstance(mod, nn.Conv2d):
                fan_in = mod.weight[0].numel()
                bound = (9.0 / fan_in) ** 0.5 if i == 0 else (3.0 / (_ACT_MOMENT * fan_in)) ** 0.5 * (exit_gain if i == last else 1.0)
                mod.weight.copy_(((torch.rand(mod.weight.shape, generator=g) * 2 - 1) * bound).half().float())
                mod.bias.copy_(((torch.rand(mod.bias.shape, generator=g) * 2 - 1) * (0.02 if i == last else 0.1)).half().float())
            elif isinstance(mod, nn.PReLU):
                a = torch.rand(mod.weight.shape, generator=g) * 1.6 - 0.3
                a[5], a[37] = 0.0, 1.0
                mod.weight.copy_(a)
    return m


@torch.no_grad()
def saturated_fraction(model, x):
    """the fraction of the fp32 reference's outputs that the caller's clamp to [0, 1] changes or pins (x in [0, 1])"""
    v = model(x)
    return float(((v <= 0) | (v >= 1)).float().mean())


# ------------------------------------------------------------------------------------------------------- fp16 storage
def _r16(t):
    return t.half().to(t.dtype)


@torch.no_grad()
def run_fp16_storage(model, x, accumulate=torch.float32):
    """`model(x)` (x in [0, 1], before the caller's clamp) with every stored activation rounded to fp16; returns fp32"""
    dt = accumulate
    x = x.to(dt)
    h = _r16(x)
    mods = list(model.body)
    for i in range(0, len(mods) - 1, 2):
        conv, act = mods[i], mods[i + 1]
        v = F.conv2d(h, conv.weight.to(dt), conv.bias.to(dt), padding=1)
        if isinstance(act, nn.PReLU):
            v = torch.where(v >= 0, v, act.weight.to(dt)[None, :, None, None] * v)
        elif isinstance(act, nn.LeakyReLU):
            v = torch.where(v >= 0, v, act.negative_slope * v)
        else:
            v = F.relu(v)
        h = _r16(v)
    y = _r16(F.conv2d(h, mods[-1].weight.to(dt), mods[-1].bias.to(dt), padding=1))
    return (F.pixel_shuffle(y, model.upscale) + F.interpolate(x, scale_factor=model.upscale, mode="nearest")).float()


# ------------------------------------------------------------------------------------------------------- one layer in fp64
def layer_fp64(x, w, bias=None, slope=None, residual=None, relu_out=False, mutant=None):
    """relu_out( prelu(conv3x3(x) + bias; slope) + residual ) in fp64 from fp16 operands and an fp32 slope.

    x [N, H, W, 64] token-major, w [64, 64, 3, 3], bias [64], slope fp32 [64] (None: no activation), residual [N, H, W, 64].
    Returns (ref, tol).  tol: the accumulation term K 2^-23 S of tests/taesd_reference.layer_fp64 (K = 576, S = |x| * |w| + |bias|)
    bounds the error of the PReLU's argument; PReLU with slope a is max(1, |a|)-Lipschitz, so max(1, |slope[c]|) times it bounds the
    error of its value (the product's own rounding, 2^-24 relative, is far inside the factor K); the residual adds K 2^-23 |residual|
    as it does there, and the closing ReLU is 1-Lipschitz.  The caller adds tests/gemm_bounds.py's 2^-10 |ref| + 2^-24 (`excess`).
    mutant: one of LAYER_MUTANTS -- the same layer evaluated WRONGLY (the returned tol is then meaningless)."""
    pre, tol = T.layer_fp64(x, w, bias)                       # conv + bias, [N, H, W, 64], and K 2^-23 (S_conv + |bias|)
    a = None if slope is None else slope.double()
    if a is not None:
        if mutant == "slope_rot8":
            a = a.roll(8)
        elif mutant == "slope_swap_halves":
            a = torch.cat([a[32:], a[:32]])
        elif mutant == "relu_for_prelu":
            a = torch.zeros_like(a)
    res = None if residual is None else residual.double()
    if mutant == "slope_after_residual" and a is not None:
        v = pre if res is None else pre + res
        v = torch.where(v >= 0, v, a * v)
    else:
        v = pre if a is None else torch.where(pre >= 0, pre, a * pre)
        if res is not None:
            v = v + res
    if a is not None:
        tol = tol * slope.double().abs().clamp(min=1.0)
    if res is not None:
        tol = tol + 576 * T.U23 * res.abs()
    if relu_out:
        v = F.relu(v)
    return v.contiguous(), tol.contiguous()


# the PReLU launch's test cases: tests/taesd_reference.SIZES x {bias, none} x {no residual, own residual + relu_out} x strides
# (name, bias, residual + relu_out, input pixel stride, output pixel stride)
LAYER_CONFIGS = tuple((f"{'bias' if b else 'nobias'}-{'res-out' if r else 'plain'}-{ldx}-{ldo}", b, r, ldx, ldo)
                      for b in (True, False) for r in (False, True) for ldx, ldo in ((64, 72), (72, 64)))
LAYER_CASES = tuple((s, c) for s in T.SIZES for c in LAYER_CONFIGS)


def layer_case_id(case):
    (n, h, w), cfg = case
    return f"{n}x{h}x{w}-{cfg[0]}"


def layer_mutants_of(cfg):
    """the wrong evaluations that CAN differ for a configuration: the misplaced slope needs a residual"""
    return [m for m in LAYER_MUTANTS if m != "slope_after_residual" or cfg[2]]


def layer_case_inputs(case):
    """CPU operands of a case, seeded by its name: x, w, bias (fp16), slope (fp32, with an exact 0 and 1), residual"""
    (n, h, w), cfg = case
    g = torch.Generator().manual_seed(zlib.crc32(("srvgg-" + layer_case_id(case)).encode()))
    x = torch.randn((n, h, w, 64), generator=g).half()
    wt = ((torch.rand((64, 64, 3, 3), generator=g) * 2 - 1) * (3.0 / 576) ** 0.5).half()
    bias = ((torch.rand(64, generator=g) * 2 - 1) * 0.5).half() if cfg[1] else None
    slope = torch.rand(64, generator=g) * 1.6 - 0.3
    slope[5], slope[37] = 0.0, 1.0
    res = torch.randn((n, h, w, 64), generator=g).half() if cfg[2] else None
    return x, wt, bias, slope, res


# ------------------------------------------------------------------------------------------------------- the exit in fp64
def exit_fp64(y, src, s, unit_in=False, clamp=True, signed_out=False, mutant=None):
    """out[n, col, s i + dy, s j + dx] = range( clamp( y[n, i, j, (col s + dy) s + dx] + entry(src[n, col, i, j]) ) ) in fp64.

    y [N, H, W, >= 3 s^2] token-major fp16, src [N, 3, H, W] fp32 / fp16 before the entry map (unit_in: clamp((v + 1) / 2, 0, 1)).
    Returns (ref [N, 3, s H, s W], tol) with tol = 2^-22 (|y| + |base| + 1): the kernel rounds three times in fp32 -- the entry
    map's add, the sum, 2 v - 1 (the halving and the clamps are exact) -- values of magnitude at most |y| + |base| + 1, each by at
    most 2^-24 of that; 2^-22 leaves a factor 4/3.      mutant: one of EXIT_MUTANTS (the tol is then meaningless)."""
    n, h, w, _ = y.shape
    yd = y.double()[..., : 3 * s * s]
    base = src.double()
    if unit_in:
        base = ((base + 1) / 2).clamp(0, 1)
    if mutant == "dy_dx_transposed":             # k = (col s + dx) s + dy
        t = yd.view(n, h, w, 3, s, s).permute(0, 3, 1, 5, 2, 4)            # [n, col, i, (axis 5 of the view) , j, (axis 4)]
    elif mutant == "colour_minor":               # k = (dy s + dx) 3 + col
        t = yd.view(n, h, w, s, s, 3).permute(0, 5, 1, 3, 2, 4)
    else:
        t = yd.view(n, h, w, 3, s, s).permute(0, 3, 1, 4, 2, 5)            # [n, col, i, dy, j, dx]
    shuffled = t.reshape(n, 3, s * h, s * w)
    if mutant == "bilinear_base":                # the bilinear resize's value at (s i, s j), for all of the pixel's outputs
        bl = F.interpolate(base, scale_factor=s, mode="bilinear", align_corners=False)[:, :, ::s, ::s]
        up = F.interpolate(bl, scale_factor=s, mode="nearest")
    else:
        up = F.interpolate(base, scale_factor=s, mode="nearest")
    v = shuffled if mutant == "no_base" else shuffled + up
    tol = U22 * (shuffled.abs() + up.abs() + 1)
    if mutant == "clamp_after_range":
        if signed_out:
            v = 2 * v - 1
        if clamp:
            v = v.clamp(0, 1)
    else:
        if clamp:
            v = v.clamp(0, 1)
        if signed_out:
            v = 2 * v - 1
    return v.contiguous(), tol.contiguous()


EXIT_SIZES = ((1, 1, 1), (2, 5, 7), (1, 9, 17))
# (size, s, source is fp32, signed in + out, pixel stride)
EXIT_CASES = tuple((size, s, f32, signed, ld) for size in EXIT_SIZES for s in (1, 2, 3, 4) for f32 in (True, False)
                   for signed in (True, False) for ld in (64, 72))


def exit_case_id(case):
    (n, h, w), s, f32, signed, ld = case
    return f"{n}x{h}x{w}-s{s}-{'f32' if f32 else 'f16'}-{'signed' if signed else 'unit'}-ld{ld}"


def exit_mutants_of(case):
    """the wrong evaluations that CAN differ for a case: the channel orders coincide at s = 1, a bilinear resize is the identity at
    s = 1 and constant on one pixel, the misplaced clamp needs the range map"""
    (n, h, w), s, f32, signed, ld = case
    out = ["no_base"]
    if s > 1:
        out += ["dy_dx_transposed", "colour_minor"]
        if h * w > 1:
            out.append("bilinear_base")
    if signed:
        out.append("clamp_after_range")
    return out


def exit_case_inputs(case):
    """CPU operands of a case, seeded by its name: y fp16 [N, H, W, 64] (all 64 channels filled: the kernel reads 3 s^2) and src.
    The first pixel's first two channels are +1.5 and -1.5: values on both sides of [0, 1] before the clamp, at every size; its
    third is 0.25 over a base of 0.5 (a source of 0 before the signed entry map): one value the clamp leaves alone, at every size"""
    (n, h, w), s, f32, signed, ld = case
    g = torch.Generator().manual_seed(zlib.crc32(("exit-" + exit_case_id(case)).encode()))
    y = (torch.randn((n, h, w, 64), generator=g) * 0.5).half()
    y[0, 0, 0, 0], y[0, 0, 0, 1], y[0, 0, 0, 2] = 1.5, -1.5, 0.25
    src = torch.rand((n, 3, h, w), generator=g)
    if signed:
        src = src * 2.4 - 1.2                     # past [-1, 1] on both sides: the entry map's clamp works
    src[0, 2 if s == 1 else 0, 0, 0] = 0.0 if signed else 0.5        # (channel 2 is colour 2 at s = 1, colour 0 otherwise)
    return y, src.to(torch.float32 if f32 else torch.float16)
