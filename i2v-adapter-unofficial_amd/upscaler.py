"""Real-ESRGAN's compact video upscalers (`realesr-animevideov3`, `realesr-general-x4v3`) on the HIP kernels: the pixel-space step the
AnimateDiff front ends run after sampling.

Mirror of Real-ESRGAN's `SRVGGNetCompact(num_in_ch=3, num_out_ch=3, num_feat=64, num_conv, upscale, act_type)`: a chain of stride-1
3x3 convolutions at 64 channels with a per-channel PReLU between them, no norm, no attention, a pixel shuffle at the end.  The module
tree is upstream's `body` ModuleList, so that a released state dict loads by key:

    body:  0 Conv(3 -> 64)  1 act    then num_conv x [Conv(64 -> 64), act]    last Conv(64 -> 3 s^2)
    act:   PReLU(64) (the released files), ReLU or LeakyReLU(0.1) -- each a module of its own; only PReLU has a weight
    forward(x) = PixelShuffle(s)(body(x)) + nearest_upsample(x, s)          x RGB in [0, 1]; the caller clamps the result to [0, 1]

Real-ESRGAN is not installed where this was written and no released `.pth` is at hand: the layout is restated from its source,
`tests/srvgg_reference.py` is the specification, and no released file has been loaded.

Launches: `i2v_taesd_prep_f16` moves the NCHW frames to token-major fp16 with 64 channels (the padding ones zero; frames
in [-1, 1] through its "unit_clamp" map); the entry convolution (weights zero-padded to 64 input channels) and the num_conv body
convolutions are one `i2v_conv3x3_c64_prelu_f16` launch each -- ReLU and leaky ReLU are that epilogue with slope 0 and 0.1 --; the
exit convolution is one `i2v_conv3x3_c64_f16` launch with its 3 s^2 output channels zero-padded to 64; `i2v_pixel_shuffle_add_f32`
shuffles, adds the nearest-upsampled source, clamps and maps the range.  Two activation buffers are reused in turn.

The second half of the file is `RRDBNet` (RealESRGAN_x4plus, RealESRGAN_x4plus_anime_6B) on the dense-block kernel, and
`load_upscaler`, which picks the class by a file's keys.
"""
import math
import os
import re

import torch
from torch import nn

from . import kernels as K
from ._lib import HipLibraryError
from .blocks import HipModule, w16

f16 = torch.float16
WIDTH = 64
ACT_TYPES = ("prelu", "relu", "leakyrelu")
LEAKY_SLOPE = 0.1
_KEY = re.compile(r"^body\.(\d+)\.(weight|bias)$")


def _check_config(num_in_ch, num_out_ch, num_feat, num_conv, upscale, act_type):
    if num_feat != WIDTH:
        raise NotImplementedError(f"SRVGGNetCompact: num_feat={num_feat}: the HIP path is the 64-channel convolution kernel")
    if num_in_ch != 3:
        raise NotImplementedError(f"SRVGGNetCompact: num_in_ch={num_in_ch}: RGB frames only (3)")
    if num_out_ch != 3:
        raise NotImplementedError(f"SRVGGNetCompact: num_out_ch={num_out_ch}: RGB frames only (3)")
    if upscale not in (1, 2, 3, 4):
        raise NotImplementedError(f"SRVGGNetCompact: upscale={upscale}: the exit kernel takes 1..4 (3 s^2 <= 64 channels)")
    if act_type not in ACT_TYPES:
        raise NotImplementedError(f"SRVGGNetCompact: act_type={act_type!r}: one of {', '.join(ACT_TYPES)}")
    if not isinstance(num_conv, int) or num_conv < 0:
        raise ValueError(f"SRVGGNetCompact: num_conv={num_conv!r} must be a non-negative integer")


def unwrap_state_dict(state):
    """a released file's dict -> the state dict: `params_ema` first, then `params`, else the dict itself"""
    for k in ("params_ema", "params"):
        if isinstance(state, dict) and k in state and isinstance(state[k], dict):
            return state[k]
    return state


def infer_config(state, act_type=None):
    """constructor arguments from a state dict's keys and shapes.  Every key must be `body.{i}.weight|bias`; convolutions sit at the
    even indices 0 .. 2 (num_conv + 1) and the PReLU weights ([64]) at the odd ones between them.  A dict without PReLU weights says
    nothing about its activation: `act_type` "relu" or "leakyrelu" is then required."""
    if not isinstance(state, dict) or not state:
        raise ValueError("SRVGGNetCompact: an empty state dict")
    convs, prelus = {}, {}
    for k, v in state.items():
        m = _KEY.match(k)
        if m is None or not isinstance(v, torch.Tensor):
            raise NotImplementedError(f"SRVGGNetCompact: unknown key `{k}` (the keys of SRVGGNetCompact are body.<i>.weight / body.<i>.bias)")
        i, what = int(m.group(1)), m.group(2)
        weight = state.get(f"body.{i}.weight")
        if what == "weight" and v.dim() == 4:
            convs[i] = v
        elif what == "weight" and v.dim() == 1:
            prelus[i] = v
        elif not (what == "bias" and v.dim() == 1 and isinstance(weight, torch.Tensor) and weight.dim() == 4):      # a convolution's
            raise NotImplementedError(f"SRVGGNetCompact: unknown key `{k}` of shape {tuple(v.shape)}")
    last = max(convs) if convs else -1
    if last < 2 or last % 2 or sorted(convs) != list(range(0, last + 1, 2)):
        raise NotImplementedError(f"SRVGGNetCompact: convolutions at body indices {sorted(convs)}: expected 0, 2, .., 2 (num_conv + 1)")
    first, exit_w = convs[0], convs[last]
    num_feat, num_in_ch = int(first.shape[0]), int(first.shape[1])
    for i, w in convs.items():
        if tuple(w.shape[2:]) != (3, 3) or (i < last and w.shape[0] != num_feat) or (i > 0 and w.shape[1] != num_feat):
            raise NotImplementedError(f"SRVGGNetCompact: unknown key `body.{i}.weight` of shape {tuple(w.shape)} in a {num_feat}-channel body")
    out_ch = int(exit_w.shape[0])
    s = math.isqrt(out_ch // 3) if out_ch % 3 == 0 else 0
    if s >= 1 and 3 * s * s == out_ch:
        num_out_ch, upscale = 3, s
    else:
        # not 3 s^2: read as upscale 4 / 2 / 1 of another channel count, the largest that divides
        upscale = next(u for u in (4, 2, 1) if out_ch % (u * u) == 0)
        num_out_ch = out_ch // (upscale * upscale)
    if prelus:
        if sorted(prelus) != list(range(1, last, 2)):
            raise NotImplementedError(f"SRVGGNetCompact: PReLU weights at body indices {sorted(prelus)}: expected 1, 3, .., {last - 1}")
        if act_type not in (None, "prelu"):
            raise ValueError(f"SRVGGNetCompact: act_type={act_type!r}, but the state dict holds PReLU weights")
        act_type = "prelu"
    elif act_type is None or act_type == "prelu":
        raise ValueError("SRVGGNetCompact: the state dict holds no PReLU weights: pass act_type='relu' or 'leakyrelu'")
    return dict(num_in_ch=num_in_ch, num_out_ch=num_out_ch, num_feat=num_feat, num_conv=last // 2 - 1, upscale=upscale, act_type=act_type)


def load_state_file(path):
    """`.pth` / `.pt` (torch.load, weights only) or `.safetensors` -> the unwrapped state dict"""
    if not os.path.isfile(path):
        raise EnvironmentError(f"SRVGGNetCompact: no file at {path}")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    if path.endswith((".pth", ".pt")):
        return unwrap_state_dict(torch.load(path, map_location="cpu", weights_only=True))
    raise ValueError(f"SRVGGNetCompact: {path}: a .pth, .pt or .safetensors file")


class SRVGGNetCompact(HipModule):
    def __init__(self, num_in_ch=3, num_out_ch=3, num_feat=WIDTH, num_conv=16, upscale=4, act_type="prelu"):
        _check_config(num_in_ch, num_out_ch, num_feat, num_conv, upscale, act_type)
        super().__init__()
        self.num_in_ch, self.num_out_ch, self.num_feat, self.num_conv = num_in_ch, num_out_ch, num_feat, num_conv
        self.upscale, self.act_type = upscale, act_type
        self.config = dict(num_in_ch=num_in_ch, num_out_ch=num_out_ch, num_feat=num_feat, num_conv=num_conv, upscale=upscale,
                           act_type=act_type)
        act = {"prelu": lambda: nn.PReLU(num_parameters=num_feat), "relu": lambda: nn.ReLU(inplace=True),
               "leakyrelu": lambda: nn.LeakyReLU(negative_slope=LEAKY_SLOPE, inplace=True)}[act_type]
        body = [nn.Conv2d(num_in_ch, num_feat, 3, 1, 1), act()]
        for _ in range(num_conv):
            body += [nn.Conv2d(num_feat, num_feat, 3, 1, 1), act()]
        body.append(nn.Conv2d(num_feat, num_out_ch * upscale * upscale, 3, 1, 1))
        self.body = nn.ModuleList(body)
        self.upsampler = nn.PixelShuffle(upscale)
        self._trace = None          # a list: every launch appends (name, kind, input, output, extra) -- the tests' teacher-forced gate

    # ------------------------------------------------------------------------------------------------ files
    @classmethod
    def from_pretrained(cls, path_or_dict, act_type=None):
        """a released `.pth` / `.pt` (`{"params_ema": ...}` or `{"params": ...}` around the state dict, or the dict bare), a
        `.safetensors` file written by `save_pretrained`, or a state dict.  num_conv, upscale and the activation come from the keys and
        shapes (`infer_config`); what the HIP path does not implement is a NotImplementedError naming the value."""
        state = unwrap_state_dict(path_or_dict) if isinstance(path_or_dict, dict) else load_state_file(str(path_or_dict))
        model = cls(**infer_config(state, act_type))
        model.load_state_dict(state, strict=True)
        return model.eval()

    def save_pretrained(self, path):
        """the state dict as one `.safetensors` file (`from_pretrained` reads it back)"""
        if not str(path).endswith(".safetensors"):
            raise ValueError(f"SRVGGNetCompact.save_pretrained: {path}: a .safetensors file name")
        from safetensors.torch import save_file
        os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
        save_file({k: v.detach().to("cpu").contiguous() for k, v in self.state_dict().items()}, str(path), metadata={"format": "pt"})

    @property
    def device(self):
        return self.body[0].weight.device

    @property
    def dtype(self):
        return self.body[0].weight.dtype

    # ------------------------------------------------------------------------------------------------ the launch plan
    def _pack(self):
        """[(name, packed weight, bias fp16 [64], slope fp32 [64] or None)]: the 1 + num_conv PReLU launches, then the exit convolution
        with its 3 s^2 output channels (weight rows and bias) zero-padded to 64 -- here, not in `pack_conv_c64`, which refuses them"""
        dev, ops, mods = self.device, [], list(self.body)
        for i in range(0, len(mods) - 1, 2):
            conv, act = mods[i], mods[i + 1]
            if isinstance(act, nn.PReLU):
                slope = act.weight.detach().float().contiguous()
            else:
                slope = torch.full((WIDTH,), 0.0 if isinstance(act, nn.ReLU) else LEAKY_SLOPE, dtype=torch.float32, device=dev)
            ops.append((f"body.{i}", K.pack_conv_c64(conv.weight), w16(conv.bias), slope))
        last = mods[-1]
        pad = WIDTH - last.out_channels
        w = torch.nn.functional.pad(last.weight.detach(), (0, 0, 0, 0, 0, 0, 0, pad))
        b = torch.nn.functional.pad(last.bias.detach(), (0, pad))
        ops.append((f"body.{len(mods) - 1}", K.pack_conv_c64(w), w16(b), None))
        return dict(ops=ops)

    def _note(self, name, kind, x, y, extra=None):
        if self._trace is not None:
            self._trace.append((name, kind, x, y, extra))
        return y

    @torch.no_grad()
    def forward(self, frames: torch.Tensor, signed: bool = True) -> torch.Tensor:
        """frames [N, 3, H, W] fp32 / fp16 on the GPU -> fp32 [N, 3, s H, s W], clamped.  signed: frames in [-1, 1] in and out (the
        VAE's range: mapped to [0, 1] and clamped on the way in, back on the way out); otherwise [0, 1] in and out.  Every frame is
        upscaled on its own: a batch equals its frames' results."""
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f"frames must be [N, 3, H, W], got {tuple(getattr(frames, 'shape', ()))}")
        if not frames.is_cuda:
            raise HipLibraryError(f"frames are on {frames.device}: the HIP path has no CPU fallback")
        src = (frames if frames.dtype in (torch.float32, f16) else frames.float()).contiguous()
        ops = self.packed()["ops"]
        n, _, h, w = src.shape
        tracing = self._trace is not None
        # two activation buffers in turn: a launch's `out` may never be its `x` (a traced run keeps every tensor instead)
        bufs = [torch.empty((n, h, w, WIDTH), dtype=f16, device=src.device) for _ in range(2)]
        x = self._note("prep", "prep", src, K.taesd_prep(src, "unit_clamp" if signed else "identity", out=bufs[0]))
        for i, (name, wp, b, slope) in enumerate(ops):
            out = None if tracing else bufs[(i + 1) & 1]
            if slope is not None:
                x = self._note(name, "prelu", x, K.conv3x3_c64(x, wp, b, slope=slope, out=out), slope)
            else:
                x = self._note(name, "exit_conv", x, K.conv3x3_c64(x, wp, b, out=out))
        y = K.pixel_shuffle_add(x, src, self.upscale, unit_in=signed, clamp=True, signed_out=signed)
        return self._note("exit", "exit", x, y, src)


# ====================================================================================================== RRDBNet (Real-ESRGAN x4plus)
# Mirror of BasicSR's `RRDBNet(num_in_ch=3, num_out_ch=3, scale=4, num_feat=64, num_block, num_grow_ch=32)` (RealESRGAN_x4plus: 23
# blocks, RealESRGAN_x4plus_anime_6B: 6), with upstream's module tree so that a released state dict loads by key:
#
#     ResidualDenseBlock: conv1 64 -> 32, conv2 96 -> 32, conv3 128 -> 32, conv4 160 -> 32, conv5 192 -> 64; each reads the concatenation
#         of x and the x_i before it; LeakyReLU(0.2) after conv1..4;  returns 0.2 x5 + x
#     RRDB: rdb1, rdb2, rdb3;  returns 0.2 rdb3(rdb2(rdb1(x))) + x
#     forward(x) = conv_last(lrelu(conv_hr(lrelu(conv_up2(up2(lrelu(conv_up1(up2(feat + conv_body(body(conv_first(x)))))))))))
#
# tests/rrdb_reference.py is the specification; no released file has been loaded.
#
# Launches: a dense block lives in ONE token-major buffer [N, H, W, 192] -- channels 0..63 its input, 64..191 x1..x4 -- and
# each of its five convolutions is one `i2v_conv3x3_dense_f16` launch: conv1..4 write 32 channels of the buffer they read, conv5 writes
# channels 0..63 of the next block's buffer with `0.2 x5 + x` in its epilogue, and rdb3's conv5 also applies `0.2 (.) + x0` and writes
# over x0.  An RRDB is 15 launches on three buffers in rotation; torch.cat and the adds never run.  conv_first and conv_body
# (`residual=feat`) are `i2v_conv3x3_c64_f16` launches, conv_up1 / conv_up2 `i2v_conv3x3_c64_up2_prelu_f16` launches (the upsampled
# tensor is never written), conv_hr an `i2v_conv3x3_c64_prelu_f16` launch, conv_last goes through `K.conv3x3` (the narrow-output
# kernel) and `i2v_rgb_exit_f32` moves, clamps and maps the range.
RRDB_GROW = 32
RRDB_SLOPE = 0.2
RRDB_TAIL = ("conv_first", "conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last")
RRDB_TAIL_LAUNCHES = 8          # prep, conv_first, conv_body, conv_up1, conv_up2, conv_hr, conv_last, exit
_RRDB_KEY = re.compile(r"^body\.(\d+)\.rdb([123])\.conv([1-5])\.(weight|bias)$")
_RRDB_TAIL_KEY = re.compile(r"^(" + "|".join(RRDB_TAIL) + r")\.(weight|bias)$")
_OLD_ESRGAN_KEY = re.compile(r"^model\.\d+\.|RDB[123]\.conv[1-5]\.0\.")


def is_rrdb_state_dict(state):
    """whether every key of the dict is one of RRDBNet's (and there is at least one)"""
    return (isinstance(state, dict) and len(state) > 0
            and all(isinstance(k, str) and (_RRDB_KEY.match(k) or _RRDB_TAIL_KEY.match(k)) for k in state))


def _check_rrdb_config(num_in_ch, num_out_ch, scale, num_feat, num_block, num_grow_ch):
    if num_feat != WIDTH:
        raise NotImplementedError(f"RRDBNet: num_feat={num_feat}: the HIP path is the 64-channel trunk (64)")
    if num_grow_ch != RRDB_GROW:
        raise NotImplementedError(f"RRDBNet: num_grow_ch={num_grow_ch}: the dense-block kernel grows by 32 channels (32)")
    if scale != 4:
        raise NotImplementedError(f"RRDBNet: scale={scale}: only scale 4 (scale 2 and 1 pixel-unshuffle the input: RealESRGAN_x2plus)")
    if num_in_ch != 3:
        raise NotImplementedError(f"RRDBNet: num_in_ch={num_in_ch}: RGB frames only (3)")
    if num_out_ch != 3:
        raise NotImplementedError(f"RRDBNet: num_out_ch={num_out_ch}: RGB frames only (3)")
    if isinstance(num_block, bool) or not isinstance(num_block, int) or num_block < 1:
        raise ValueError(f"RRDBNet: num_block={num_block!r} must be a positive integer")


def infer_rrdb_config(state):
    """RRDBNet's constructor arguments from a state dict's keys and shapes: num_block from the `body.{i}` indices, num_feat and
    num_grow_ch from conv_first / rdb1.conv1, the scale from conv_first's input channels (3 -> 4; 12 and 48 are the pixel-unshuffled
    inputs of scale 2 and 1).  Unknown and missing keys are errors naming the key."""
    if not isinstance(state, dict) or not state:
        raise ValueError("RRDBNet: an empty state dict")
    blocks = set()
    for k, v in state.items():
        m = _RRDB_KEY.match(k) if isinstance(k, str) else None
        if isinstance(k, str) and _OLD_ESRGAN_KEY.search(k):
            raise NotImplementedError(f"RRDBNet: key `{k}` is the old ESRGAN architecture's naming (model.N / RDB1.conv1.0): "
                                      "convert the file to BasicSR's RRDBNet keys first")
        if not isinstance(v, torch.Tensor) or (m is None and not _RRDB_TAIL_KEY.match(k)):
            raise NotImplementedError(f"RRDBNet: unknown key `{k}` (the keys of RRDBNet are conv_first, body.<i>.rdb<1-3>.conv<1-5>, "
                                      "conv_body, conv_up1, conv_up2, conv_hr, conv_last)")
        if m is not None:
            blocks.add(int(m.group(1)))
    for name in RRDB_TAIL:
        for what in ("weight", "bias"):
            if f"{name}.{what}" not in state:
                raise NotImplementedError(f"RRDBNet: missing key `{name}.{what}`")
    if not blocks or sorted(blocks) != list(range(max(blocks) + 1)):
        raise NotImplementedError(f"RRDBNet: RRDBs at body indices {sorted(blocks)}: expected 0 .. num_block - 1")
    first = state["conv_first.weight"]
    if first.dim() != 4 or tuple(first.shape[2:]) != (3, 3):
        raise NotImplementedError(f"RRDBNet: unknown key `conv_first.weight` of shape {tuple(first.shape)}")
    num_feat, cin0 = int(first.shape[0]), int(first.shape[1])
    w1 = state.get("body.0.rdb1.conv1.weight")
    if w1 is None:
        raise NotImplementedError("RRDBNet: missing key `body.0.rdb1.conv1.weight`")
    num_grow_ch = int(w1.shape[0])
    num_out_ch = int(state["conv_last.weight"].shape[0])
    if cin0 in (12, 48):
        scale = 2 if cin0 == 12 else 1
        raise NotImplementedError(f"RRDBNet: conv_first reads {cin0} channels: a scale-{scale} network (a pixel-unshuffled RGB input, "
                                  "RealESRGAN_x2plus); only scale 4 is implemented")
    return dict(num_in_ch=cin0, num_out_ch=num_out_ch, scale=4, num_feat=num_feat, num_block=max(blocks) + 1, num_grow_ch=num_grow_ch)


class _ResidualDenseBlock(nn.Module):
    def __init__(self, num_feat, num_grow_ch):
        super().__init__()
        for i in range(1, 6):
            setattr(self, f"conv{i}", nn.Conv2d(num_feat + (i - 1) * num_grow_ch, num_grow_ch if i < 5 else num_feat, 3, 1, 1))


class _RRDB(nn.Module):
    def __init__(self, num_feat, num_grow_ch):
        super().__init__()
        self.rdb1 = _ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb2 = _ResidualDenseBlock(num_feat, num_grow_ch)
        self.rdb3 = _ResidualDenseBlock(num_feat, num_grow_ch)


class RRDBNet(HipModule):
    def __init__(self, num_in_ch=3, num_out_ch=3, scale=4, num_feat=WIDTH, num_block=23, num_grow_ch=RRDB_GROW):
        _check_rrdb_config(num_in_ch, num_out_ch, scale, num_feat, num_block, num_grow_ch)
        super().__init__()
        self.num_in_ch, self.num_out_ch, self.scale, self.num_feat = num_in_ch, num_out_ch, scale, num_feat
        self.num_block, self.num_grow_ch = num_block, num_grow_ch
        self.upscale = scale
        self.config = dict(num_in_ch=num_in_ch, num_out_ch=num_out_ch, scale=scale, num_feat=num_feat, num_block=num_block,
                           num_grow_ch=num_grow_ch)
        self.conv_first = nn.Conv2d(num_in_ch, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[_RRDB(num_feat, num_grow_ch) for _ in range(num_block)])
        self.conv_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_last = nn.Conv2d(num_feat, num_out_ch, 3, 1, 1)
        self._trace = None          # a list: every launch appends (name, kind, input, output, extra) -- the tests' teacher-forced gate

    # ------------------------------------------------------------------------------------------------ files
    @classmethod
    def from_pretrained(cls, path_or_dict):
        """a released `.pth` / `.pt` (`{"params_ema": ...}` or `{"params": ...}` around the state dict, or the dict bare), a
        `.safetensors` file written by `save_pretrained`, or a state dict.  num_block comes from the keys (`infer_rrdb_config`);
        what the HIP path does not implement is a NotImplementedError naming the value, raised before anything is built."""
        state = unwrap_state_dict(path_or_dict) if isinstance(path_or_dict, dict) else load_state_file(str(path_or_dict))
        model = cls(**infer_rrdb_config(state))
        model.load_state_dict(state, strict=True)
        return model.eval()

    def save_pretrained(self, path):
        """the state dict as one `.safetensors` file (`from_pretrained` reads it back)"""
        if not str(path).endswith(".safetensors"):
            raise ValueError(f"RRDBNet.save_pretrained: {path}: a .safetensors file name")
        from safetensors.torch import save_file
        os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
        save_file({k: v.detach().to("cpu").contiguous() for k, v in self.state_dict().items()}, str(path), metadata={"format": "pt"})

    @property
    def device(self):
        return self.conv_first.weight.device

    @property
    def dtype(self):
        return self.conv_first.weight.dtype

    # ------------------------------------------------------------------------------------------------ the launch plan
    def _pack(self):
        """first / body_conv / up1 / up2 / hr: (packed weight, bias fp16); last: (`pack_conv3x3` weight, bias); dense: per RRDB, per
        block, the five (packed weight, bias) of `conv3x3_dense`; slope: the leaky ReLU as the PReLU launches' fp32 [64]"""
        from .blocks import pack_conv3x3
        c64 = lambda conv: (K.pack_conv_c64(conv.weight), w16(conv.bias))
        dense = [[[(K.pack_conv_dense(getattr(rdb, f"conv{i}").weight), w16(getattr(rdb, f"conv{i}").bias)) for i in range(1, 6)]
                  for rdb in (rrdb.rdb1, rrdb.rdb2, rrdb.rdb3)] for rrdb in self.body]
        return dict(first=c64(self.conv_first), body_conv=c64(self.conv_body), up1=c64(self.conv_up1), up2=c64(self.conv_up2),
                    hr=c64(self.conv_hr), last=(pack_conv3x3(self.conv_last.weight), w16(self.conv_last.bias)), dense=dense,
                    slope=torch.full((WIDTH,), RRDB_SLOPE, dtype=torch.float32, device=self.device))

    def _note(self, name, kind, x, y, extra=None):
        if self._trace is not None:
            self._trace.append((name, kind, x, y.clone() if kind == "dense" else y, extra))
        return y

    def _dense(self, name, buf, cin, wb, out, **kw):
        """one dense launch; a traced run keeps copies of what it read (the buffers are rewritten in place later)"""
        tracing = self._trace is not None
        snap = buf.clone() if tracing else None
        extra = dict(cin=cin, **{k: (v.clone() if tracing and isinstance(v, torch.Tensor) else v) for k, v in kw.items()}) if tracing else None
        K.conv3x3_dense(buf, cin, wb[0], wb[1], out=out, **kw)
        return self._note(name, "dense", snap, out, extra)

    @torch.no_grad()
    def forward(self, frames: torch.Tensor, signed: bool = True) -> torch.Tensor:
        """frames [N, 3, H, W] fp32 / fp16 on the GPU -> fp32 [N, 3, 4 H, 4 W], clamped.  signed: frames in [-1, 1] in and out (the
        VAE's range: mapped to [0, 1] and clamped on the way in, back on the way out); otherwise [0, 1] in and out.  Every frame is
        upscaled on its own: a batch equals its frames' results."""
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f"frames must be [N, 3, H, W], got {tuple(getattr(frames, 'shape', ()))}")
        if not frames.is_cuda:
            raise HipLibraryError(f"frames are on {frames.device}: the HIP path has no CPU fallback")
        src = (frames if frames.dtype in (torch.float32, f16) else frames.float()).contiguous()
        pk = self.packed()
        n, _, h, w = src.shape
        dev = src.device
        x = self._note("prep", "prep", src, K.taesd_prep(src, "unit_clamp" if signed else "identity"))
        feat = self._note("conv_first", "c64", x, K.conv3x3_c64(x, pk["first"][0], pk["first"][1]))
        del x
        # three dense-block buffers in rotation; the trunk is channels 0..63 of the one a block reads
        bufs = [torch.empty((n, h, w, WIDTH + 4 * RRDB_GROW), dtype=f16, device=dev) for _ in range(3)]
        bufs[0][..., :WIDTH].copy_(feat)
        for i, rrdb in enumerate(pk["dense"]):
            x0 = bufs[0][..., :WIDTH]                                   # the RRDB's input, and (written by rdb3's conv5) its output
            for j, convs in enumerate(rrdb):
                buf, name = bufs[j], f"body.{i}.rdb{j + 1}"
                for k in range(4):
                    cin = WIDTH + RRDB_GROW * k
                    self._dense(f"{name}.conv{k + 1}", buf, cin, convs[k], buf[..., cin: cin + RRDB_GROW], slope=RRDB_SLOPE)
                cin, own = WIDTH + 4 * RRDB_GROW, buf[..., :WIDTH]
                if j < 2:
                    self._dense(f"{name}.conv5", buf, cin, convs[4], bufs[j + 1][..., :WIDTH], slope=1.0, s1=0.2, r1=own)
                else:
                    self._dense(f"{name}.conv5", buf, cin, convs[4], x0, slope=1.0, s1=0.2, r1=own, s2=0.2, r2=x0)
        trunk = bufs[0][..., :WIDTH]
        t = self._note("conv_body", "c64_res", trunk, K.conv3x3_c64(trunk, pk["body_conv"][0], pk["body_conv"][1], residual=feat), feat)
        del bufs, trunk, feat
        u1 = self._note("conv_up1", "up2", t, K.conv3x3_c64_up2(t, pk["up1"][0], pk["up1"][1], pk["slope"]))
        del t
        u2 = self._note("conv_up2", "up2", u1, K.conv3x3_c64_up2(u1, pk["up2"][0], pk["up2"][1], pk["slope"]))
        del u1
        hr = self._note("conv_hr", "prelu", u2, K.conv3x3_c64(u2, pk["hr"][0], pk["hr"][1], slope=pk["slope"]))
        del u2
        last = self._note("conv_last", "last", hr, K.conv3x3(hr, pk["last"][0], pk["last"][1]))
        del hr
        return self._note("exit", "exit", last, K.rgb_exit(last, clamp=True, signed_out=signed))


def load_upscaler(path_or_dict, act_type=None):
    """the upscaler of a file or state dict, by its keys: a dict whose keys are all RRDBNet's (conv_first, body.<i>.rdb<j>.conv<k>, ...)
    is an `RRDBNet` (`act_type` must then be None: the architecture fixes LeakyReLU(0.2)); anything else goes to
    `SRVGGNetCompact.from_pretrained`, which names what it does not know."""
    state = unwrap_state_dict(path_or_dict) if isinstance(path_or_dict, dict) else load_state_file(str(path_or_dict))
    if isinstance(state, dict) and any(isinstance(k, str) and _OLD_ESRGAN_KEY.search(k) for k in state):
        infer_rrdb_config(state)          # (raises, naming the key)
    if is_rrdb_state_dict(state):
        if act_type is not None:
            raise ValueError(f"act_type={act_type!r} with an RRDBNet state dict: the architecture's activation is LeakyReLU(0.2)")
        return RRDBNet.from_pretrained(state)
    return SRVGGNetCompact.from_pretrained(state, act_type=act_type)
