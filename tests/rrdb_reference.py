"""Real-ESRGAN's RRDBNet (`RealESRGAN_x4plus`, `RealESRGAN_x4plus_anime_6B`) in plain torch: the specification of
i2v_adapter_unofficial_amd.upscaler.RRDBNet.

BasicSR / Real-ESRGAN are not installed where this was written and no released checkpoint is at hand, so the layout is restated from
`basicsr/archs/rrdbnet_arch.py`; `tests/golden/rrdb_keys.txt` is the resulting state-dict key list for num_block 6 and 23.  This
restatement IS the specification: no released file has been loaded.

* `RRDBReference`: the fp32 restatement, built with upstream's module names (so the state-dict keys are upstream's).
* `seeded_reference`: seeded weights that are fp16 values.
* `run_fp16_storage`: the same layers with every STORED activation rounded to fp16 -- the entry map's output, conv_first's output, each
  x1..x4, each dense block's output, each RRDB's output, the sum feat + conv_body(.), every tail convolution's output after its
  activation -- and accumulation in fp32 (or fp64: `accumulate=`).  What any fp16-activation implementation computes, up to summation order.
* `dense_layer_fp64`: ONE launch of the dense kernel in fp64 from fp16 operands with its bound, and nine deliberately WRONG evaluations
  (`DENSE_MUTANTS`) the bound must reject.
* `up2_layer_fp64` / `exit_fp64`: the folded-upsample launch and the exit launch, with their bounds and wrong evaluations.
"""
import zlib

import torch
import torch.nn.functional as F
from torch import nn

from tests import taesd_reference as T

U22 = 2.0 ** -22
LRELU = 0.2
CINS = (64, 96, 128, 160, 192)
TILE = (16, 16)                                   # the dense kernel's output tile (rows, columns)
DENSE_MUTANTS = ("slope_0.1", "window_shift32", "swap_x2_x3", "no_s1", "stages_swapped", "no_r2", "swap_cout_halves", "tap_shift",
                 "neighbour_halo")
UP2_MUTANTS = ("round_up_shift", "bilinear")
EXIT_MUTANTS = ("clamp_after_range",)


# ------------------------------------------------------------------------------------------------------- the fp32 restatement
class ResidualDenseBlock(nn.Module):
    def __init__(self, num_feat=64, num_grow_ch=32):
        super().__init__()
        self.conv1 = nn.Conv2d(num_feat, num_grow_ch, 3, 1, 1)
        self.conv2 = nn.Conv2d(num_feat + num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv3 = nn.Conv2d(num_feat + 2 * num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv4 = nn.Conv2d(num_feat + 3 * num_grow_ch, num_grow_ch, 3, 1, 1)
        self.conv5 = nn.Conv2d(num_feat + 4 * num_grow_ch, num_feat, 3, 1, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=LRELU, inplace=True)

    def forward(self, x):
        x1 = self.lrelu(self.conv1(x))
        x2 = self.lrelu(self.conv2(torch.cat((x, x1), 1)))
        x3 = self.lrelu(self.conv3(torch.cat((x, x1, x2), 1)))
        x4 = self.lrelu(self.conv4(torch.cat((x, x1, x2, x3), 1)))
        x5 = self.conv5(torch.cat((x, x1, x2, x3, x4), 1))
        return x5 * 0.2 + x


class RRDB(nn.Module):
    def __init__(self, num_feat, num_grow_ch=32):
        super().__init__()
        self.rdb1 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb2 = ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb3 = ResidualDenseBlock(num_feat, num_grow_ch)

    def forward(self, x):
        out = self.rdb3(self.rdb2(self.rdb1(x)))
        return out * 0.2 + x


class RRDBReference(nn.Module):
    """scale 4 only: scale 2 / 1 pixel-unshuffle the input upstream (12 / 48 input channels) and are out of scope"""

    def __init__(self, num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block=23, num_grow_ch=32):
        super().__init__()
        assert scale == 4
        self.scale, self.num_block = scale, num_block
        self.conv_first = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[RRDB(num_feat, num_grow_ch) for _ in range(num_block)])
        self.conv_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=LRELU, inplace=True)

    def forward(self, x):
        feat = self.conv_first(x)
        feat = feat + self.conv_body(self.body(feat))
        feat = self.lrelu(self.conv_up1(F.interpolate(feat, scale_factor=2, mode="nearest")))
        feat = self.lrelu(self.conv_up2(F.interpolate(feat, scale_factor=2, mode="nearest")))
        return self.conv_last(self.lrelu(self.conv_hr(feat)))


def entry_map(frames):
    """[-1, 1] frames -> the network's RGB in [0, 1]"""
    return ((frames + 1) / 2).clamp(0, 1)


def leave_map(v, signed):
    """the caller's clamp, and the way back to [-1, 1]"""
    v = v.clamp(0, 1)
    return 2 * v - 1 if signed else v


_ACT_MOMENT = 0.52          # second moment LeakyReLU(0.2) keeps of a symmetric argument: (1 + 0.04) / 2


def seeded_reference(num_block=1, seed=0):
    """an RRDBReference with seeded weights that are fp16 values, U(-b, b) per layer (fan_in = 9 Cin):
        conv_first: b = sqrt(9 / fan_in) (U(0, 1) pixels);   each rdb*.conv1 and conv_body (their input is no activation's output):
        b = sqrt(3 / fan_in);   every other convolution: b = sqrt(3 / (0.52 fan_in));   conv_last: 0.15 times that.
    conv_last.bias = 0.5 + U(-0.02, 0.02), every other bias U(-0.1, 0.1).  The activations' rms then grows about 1.2 x per RRDB, and
    few outputs of a 1- or 2-block network leave (0, 1) (`saturated_fraction`)."""
    g = torch.Generator().manual_seed(seed)
    m = RRDBReference(num_block=num_block).float().eval()
    with torch.no_grad():
        for name, mod in m.named_modules():
            if not isinstance(mod, nn.Conv2d):
                continue
            fan_in = mod.weight[0].numel()
            if name == "conv_first":
                b = (9.0 / fan_in) ** 0.5
            elif name.endswith(".conv1") or name == "conv_body":
                b = (3.0 / fan_in) ** 0.5
            else:
                b = (3.0 / (_ACT_MOMENT * fan_in)) ** 0.5 * (0.15 if name == "conv_last" else 1.0)
            mod.weight.copy_(((torch.rand(mod.weight.shape, generator=g) * 2 - 1) * b).half().float())
            if name == "conv_last":
                mod.bias.copy_((0.5 + (torch.rand(mod.bias.shape, generator=g) * 2 - 1) * 0.02).half().float())
            else:
                mod.bias.copy_(((torch.rand(mod.bias.shape, generator=g) * 2 - 1) * 0.1).half().float())
    return m


@torch.no_grad()
def saturated_fraction(model, x):
    """the fraction of the fp32 reference's outputs that the caller's clamp to [0, 1] changes or pins (x in [0, 1])"""
    v = model(x)
    return float(((v <= 0) | (v >= 1)).float().mean())


# the end-to-end cases: (num_block, (N, H, W)) -- 6 and 23 blocks are tested for keys, loading and the launch plan, and teacher-forced
E2E_CASES = ((1, (2, 9, 17)), (2, (2, 9, 17)), (2, (1, 16, 32)))
TEACHER_CASES = ((1, (2, 9, 17)), (2, (1, 16, 32)), (6, (2, 9, 17)))


def e2e_frames(case):
    """seeded frames in [-1.2, 1.2] (past the VAE's range on both sides: the entry map's clamp works), fp32 [N, 3, H, W]"""
    nb, (n, h, w) = case
    g = torch.Generator().manual_seed(zlib.crc32(f"rrdb-e2e-{nb}-{n}x{h}x{w}".encode()))
    return torch.rand((n, 3, h, w), generator=g) * 2.4 - 1.2


# ------------------------------------------------------------------------------------------------------- fp16 storage
def _r16(t):
    return t.half().to(t.dtype)


def _lrelu(v):
    return torch.where(v >= 0, v, LRELU * v)


@torch.no_grad()
def run_fp16_storage(model, x, accumulate=torch.float32):
    """`model(x)` (x in [0, 1], before the caller's clamp) with every stored activation rounded to fp16; returns fp32"""
    dt = accumulate

    def conv(t, c):
        return F.conv2d(t, c.weight.to(dt), c.bias.to(dt), padding=1)

    def block(b, t):
        x1 = _r16(_lrelu(conv(t, b.conv1)))
        x2 = _r16(_lrelu(conv(torch.cat((t, x1), 1), b.conv2)))
        x3 = _r16(_lrelu(conv(torch.cat((t, x1, x2), 1), b.conv3)))
        x4 = _r16(_lrelu(conv(torch.cat((t, x1, x2, x3), 1), b.conv4)))
        return conv(torch.cat((t, x1, x2, x3, x4), 1), b.conv5) * 0.2 + t          # (rounded by the caller: an RRDB's last is one rounding)

    feat = _r16(conv(_r16(x.to(dt)), model.conv_first))
    h = feat
    for rrdb in model.body:
        x0 = h
        h = _r16(block(rrdb.rdb1, h))
        h = _r16(block(rrdb.rdb2, h))
        h = _r16(block(rrdb.rdb3, h) * 0.2 + x0)
    h = _r16(feat + conv(h, model.conv_body))
    h = _r16(_lrelu(conv(F.interpolate(h, scale_factor=2, mode="nearest"), model.conv_up1)))
    h = _r16(_lrelu(conv(F.interpolate(h, scale_factor=2, mode="nearest"), model.conv_up2)))
    h = _r16(_lrelu(conv(h, model.conv_hr)))
    return _r16(conv(h, model.conv_last)).float()


# ------------------------------------------------------------------------------------------------------- one dense launch in fp64
def _f32(s):
    """the scalar as the kernel holds it: rounded to fp32"""
    return float(torch.tensor(float(s), dtype=torch.float32))


def dense_layer_fp64(buffer, cin, w, bias=None, slope=LRELU, s1=1.0, r1=None, s2=1.0, r2=None, mutant=None):
    """s2 (s1 lrelu(conv3x3(buffer[..., :cin]) + bias; slope) + r1) + r2 in fp64 from fp16 operands and fp32 scalars.

    buffer [N, H, W, C >= cin] token-major (finite in every channel here: the GPU test poisons channels >= cin itself), w [cout, cin,
    3, 3], bias [cout], r1 / r2 [N, H, W, cout].  Returns (ref [N, H, W, cout], tol).  tol: the accumulation term K 2^-23 S of
    tests/taesd_reference.layer_fp64 (K = 9 cin, S = |x| * |w| + |bias|) bounds the error of the leaky ReLU's argument; the leaky ReLU
    is 1-Lipschitz for |slope| <= 1; the two stages scale that by |s1 s2| and each rounds once, by at most 2^-24 of |s1 v| + |r1| and
    of |s2 (.)| + |r2| -- far inside K 2^-23 (|s2| |r1| + |r2|), the term a residual adds there:
        tol = K 2^-23 (|s1 s2| S + |s2| |r1| + |r2|).        The caller adds tests/gemm_bounds.py's 2^-10 |ref| + 2^-24 (`excess`).
    mutant: one of DENSE_MUTANTS -- the same launch evaluated WRONGLY (the returned tol is then meaningless)."""
    assert abs(slope) <= 1.0
    x = buffer[..., :cin]
    if mutant == "window_shift32":               # the input window starts 32 channels late (and wraps at the buffer's end)
        x = buffer.roll(-32, dims=-1)[..., :cin]
    elif mutant == "swap_x2_x3":                 # x2's slot (96..127) read where x3's (128..159) belongs, and back
        x = torch.cat([buffer[..., :96], buffer[..., 128:160], buffer[..., 96:128], buffer[..., 160:]], dim=-1)[..., :cin]
    pre, tol = T.layer_fp64(x.contiguous(), w, bias, mutant=mutant if mutant in ("tap_shift", "neighbour_halo") else None)
    a = 0.1 if mutant == "slope_0.1" else _f32(slope)
    v = torch.where(pre >= 0, pre, a * pre)
    if mutant == "swap_cout_halves":
        hc = v.shape[-1] // 2
        v = torch.cat([v[..., hc:], v[..., :hc]], dim=-1)
    a1, a2 = _f32(s1), _f32(s2)
    z1 = torch.zeros_like(v) if r1 is None else r1.double()
    z2 = torch.zeros_like(v) if r2 is None else r2.double()
    if mutant == "stages_swapped":
        out = a2 * a1 * v + z1 + z2
    else:
        out = a2 * ((v if mutant == "no_s1" else a1 * v) + z1) + (0 if mutant == "no_r2" else z2)
    tol = abs(a1 * a2) * tol + 9 * cin * T.U23 * (abs(a2) * z1.abs() + z2.abs())
    return out.contiguous(), tol.contiguous()


# the dense launch's cases: sizes x cin x configuration x buffer pixel stride
#   sizes: one pixel; exactly one tile; one pixel past a tile in both directions; ragged; three images of four tiles (the multi-tile walk)
DENSE_SIZES = ((1, 1, 1), (2, TILE[0], TILE[1]), (1, TILE[0] + 1, TILE[1] + 1), (2, 5, 40), (3, TILE[0] + 1, TILE[1] + 1))
# (name, cout, slope, s1, r1: the buffer's own channels 0..63, s2, r2: None / "own" / "out")
DENSE_CONFIGS = (("grow", 32, LRELU, 1.0, False, 1.0, None),                 # a block's convolutions 1..4: in place at channel offset cin
                 ("close", 64, 1.0, 0.2, True, 1.0, None),                   # conv5 of rdb1 / rdb2
                 ("close-rrdb", 64, 1.0, 0.2, True, 0.2, "own"),             # conv5 of rdb3, out and r2 apart
                 ("close-rrdb-inplace", 64, 1.0, 0.2, True, 0.2, "out"))     # ... out IS r2
DENSE_STRIDES = (192, 200)
DENSE_CASES = tuple((s, cin, cfg, ld) for s in DENSE_SIZES for cin in CINS for cfg in DENSE_CONFIGS for ld in DENSE_STRIDES)


def dense_case_id(case):
    (n, h, w), cin, cfg, ld = case
    return f"{n}x{h}x{w}-cin{cin}-{cfg[0]}-ld{ld}"


def dense_mutants_of(case):
    """the wrong evaluations that CAN differ for a case"""
    (n, h, w), cin, cfg, ld = case
    _, cout, slope, s1, r1, s2, r2 = cfg
    out = ["window_shift32", "swap_cout_halves", "tap_shift"]
    if n > 1:
        out.append("neighbour_halo")
    if slope != 1.0:
        out.append("slope_0.1")
    if cin >= 160:
        out.append("swap_x2_x3")
    if s1 != 1.0:
        out.append("no_s1")
    if r1 and s2 != 1.0:
        out.append("stages_swapped")
    if r2:
        out.append("no_r2")
    return out


def dense_case_inputs(case):
    """fp16 CPU operands of a case, seeded by its size, cin and configuration (not its stride): the block's buffer [N, H, W, 192] with
    every channel finite, w [cout, cin, 3, 3], bias [cout], r2 [N, H, W, cout] or None.  r1, where the configuration has one, is the
    buffer's channels 0..63."""
    (n, h, w), cin, cfg, _ = case
    _, cout, slope, s1, r1, s2, r2 = cfg
    g = torch.Generator().manual_seed(zlib.crc32(f"rrdb-dense-{n}x{h}x{w}-{cin}-{cfg[0]}".encode()))
    buf = torch.randn((n, h, w, 192), generator=g).half()
    wt = ((torch.rand((cout, cin, 3, 3), generator=g) * 2 - 1) * (3.0 / (9 * cin)) ** 0.5).half()
    bias = ((torch.rand(cout, generator=g) * 2 - 1) * 0.5).half()
    res2 = torch.randn((n, h, w, cout), generator=g).half() if r2 else None
    return buf, wt, bias, res2


def dense_case_reference(case, mutant=None):
    buf, wt, bias, res2 = dense_case_inputs(case)
    _, cin, cfg, _ = case
    _, cout, slope, s1, r1, s2, r2 = cfg
    return dense_layer_fp64(buf, cin, wt, bias, slope, s1, buf[..., :64] if r1 else None, s2, res2, mutant=mutant)


# ------------------------------------------------------------------------------------------------------- the tail's launches in fp64
def up2_layer_fp64(x, w, bias=None, slope=LRELU, mutant=None):
    """lrelu(conv3x3(nearest_2x(x)) + bias; slope) in fp64: x [N, H, W, 64] -> (ref [N, 2 H, 2 W, 64], tol), the bound of
    tests/taesd_reference.layer_fp64 (the leaky ReLU is 1-Lipschitz).  Output pixel (y, x) of the upsampled image is source pixel
    (y >> 1, x >> 1).  mutant: "round_up_shift" -- (y + 1) >> 1 (clamped to the image) --, "bilinear"."""
    n, h, wd, c = x.shape
    if mutant == "bilinear":
        xu = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    else:
        iy, ix = torch.arange(2 * h), torch.arange(2 * wd)
        if mutant == "round_up_shift":
            iy, ix = ((iy + 1) >> 1).clamp(max=h - 1), ((ix + 1) >> 1).clamp(max=wd - 1)
        else:
            iy, ix = iy >> 1, ix >> 1
        xu = x[:, iy][:, :, ix]
    pre, tol = T.layer_fp64(xu.contiguous(), w, bias)
    return torch.where(pre >= 0, pre, _f32(slope) * pre).contiguous(), tol


UP2_SIZES = T.SIZES                     # the SOURCE's (N, H, W): the 64-channel kernel's cases
UP2_CASES = tuple((s, ldx, ldo) for s in UP2_SIZES for ldx, ldo in ((64, 72), (72, 64)))


def up2_case_id(case):
    (n, h, w), ldx, ldo = case
    return f"{n}x{h}x{w}-{ldx}-{ldo}"


def up2_case_inputs(case):
    (n, h, w), _, _ = case
    g = torch.Generator().manual_seed(zlib.crc32(f"rrdb-up2-{n}x{h}x{w}".encode()))
    x = torch.randn((n, h, w, 64), generator=g).half()
    wt = ((torch.rand((64, 64, 3, 3), generator=g) * 2 - 1) * (3.0 / 576) ** 0.5).half()
    bias = ((torch.rand(64, generator=g) * 2 - 1) * 0.5).half()
    return x, wt, bias


def up2_mutants_of(case):
    """a one-pixel source has one upsampling, whatever the rule"""
    (n, h, w), _, _ = case
    return list(UP2_MUTANTS) if h * w > 1 else []


def exit_fp64(y, clamp=True, signed_out=False, mutant=None):
    """out[n, col, y, x] = range(clamp(y[n, y, x, col])) in fp64: y [N, H, W, >= 3] token-major fp16 -> (ref [N, 3, H, W], tol) with
    tol = 2^-22 (|v| + 1): the clamp is exact and 2 v - 1 rounds once, by at most 2^-24.  mutant: "clamp_after_range"."""
    v = y.double()[..., :3].permute(0, 3, 1, 2)
    tol = U22 * (v.abs().clamp(max=1.0) + 1)
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


EXIT_CASES = tuple((size, signed, ld) for size in ((1, 1, 1), (2, 5, 7), (1, 9, 65)) for signed in (True, False) for ld in (3, 8))


def exit_case_id(case):
    (n, h, w), signed, ld = case
    return f"{n}x{h}x{w}-{'signed' if signed else 'unit'}-ld{ld}"


def exit_case_inputs(case):
    """y fp16 [N, H, W, 3]; the first pixel holds +1.5, -1.5 and 0.25: values on both sides of [0, 1] and one inside, at every size"""
    (n, h, w), signed, ld = case
    g = torch.Generator().manual_seed(zlib.crc32(("rrdb-exit-" + exit_case_id(case)).encode()))
    y = (torch.randn((n, h, w, 3), generator=g) * 0.5 + 0.5).half()
    y[0, 0, 0, 0], y[0, 0, 0, 1], y[0, 0, 0, 2] = 1.5, -1.5, 0.25
    return y


def exit_mutants_of(case):
    """the misplaced clamp needs the range map"""
    return ["clamp_after_range"] if case[1] else []
