"""T2IAdapter on the HIP kernels: diffusers 0.24 `T2IAdapter` with `adapter_type="full_adapter"` (the SD-1.5 layout of the
TencentARC `t2iadapter_*_sd15v2` folders: same module tree, state-dict keys and config keys, so `config.json` +
`diffusion_pytorch_model.safetensors` load by key through PretrainedMixin).

    adapter = FullAdapter: PixelUnshuffle(8) -> conv_in (3x3) -> body[0..3]
    body[i] = AdapterBlock: AvgPool2d(2, ceil_mode=True) for i > 0, a 1x1 in_conv where the width changes, num_res_blocks x
              AdapterResnetBlock (x + block2(relu(block1(x))), block1 3x3, block2 1x1)

The adapter reads the control frames only -- never the latents or the timestep.  Its four feature maps (one per down level of the
UNet, at H/8 and the ceil halves of it) are therefore computed ONCE per sample (`embed`), and a denoising step only adds them to the
UNet's down path (`down_intrablock_additional_residuals`, K.add_broadcast_residual): no network runs per step.

Activations are token-major fp16 ([N, H, W, C]); every launch is a library launch -- the movers of csrc/t2i_adapter.hip and the
existing conv3x3 / gemm entry points -- nothing here computes with torch ops and nothing falls back to the CPU.
"""
from typing import List, Tuple

import torch
from torch import nn

from . import kernels as K
from ._lib import HipLibraryError
from .blocks import HipModule, pack_conv3x3, w16
from .checkpoint import PretrainedMixin
from .unet_motion_cross_frame_attn import _Config

f16 = torch.float16


def _packed_from(module, leaves):
    """`HipModule.packed` keyed on the module's OWN leaf parameters (its children pack themselves)"""
    key = tuple((q.data_ptr(), q._version, q.dtype) for q in leaves)
    if module._packed is None or key != module._packed_key:
        for q in leaves:
            if not q.is_cuda:
                raise HipLibraryError(f"{type(module).__name__} has parameters on {q.device}: the HIP path has no CPU fallback")
        with torch.no_grad():
            module._packed = module._pack()
        module._packed_key = key
    return module._packed


class AdapterResnetBlock(HipModule):
    """diffusers' AdapterResnetBlock: block2(relu(block1(x))) + x, block1 3x3 / pad 1, block2 1x1."""

    def __init__(self, channels: int):
        super().__init__()
        self.block1 = nn.Conv2d(channels, channels, kernel_size=3, padding=1)
        self.act = nn.ReLU()
        self.block2 = nn.Conv2d(channels, channels, kernel_size=1)

    def _pack(self):
        c = self.block2.out_channels
        return dict(w1=pack_conv3x3(self.block1.weight), b1=w16(self.block1.bias), w2=w16(self.block2.weight.reshape(c, c)),
                    b2=w16(self.block2.bias))

    def _fwd(self, x):
        p = self.packed()
        h = K.conv3x3(x, p["w1"], p["b1"])
        K.relu(h, out=h)
        n, hh, ww, c = x.shape
        return K.gemm(h.view(-1, c), p["w2"], p["b2"], residual=x.view(-1, c)).view(n, hh, ww, c)


class AdapterBlock(HipModule):
    """diffusers' AdapterBlock: downsample (AvgPool2d(2, stride 2, ceil_mode=True)) -> in_conv (1x1, only where the width changes) ->
    resnets."""

    def __init__(self, in_channels: int, out_channels: int, num_res_blocks: int, down: bool = False):
        super().__init__()
        self.downsample = nn.AvgPool2d(kernel_size=2, stride=2, ceil_mode=True) if down else None
        self.in_conv = nn.Conv2d(in_channels, out_channels, kernel_size=1) if in_channels != out_channels else None
        self.resnets = nn.Sequential(*[AdapterResnetBlock(out_channels) for _ in range(num_res_blocks)])

    def _pack(self):
        if self.in_conv is None:
            return {}
        c = self.in_conv
        return dict(w_in=w16(c.weight.reshape(c.out_channels, c.in_channels)), b_in=w16(c.bias))

    def packed(self):
        # only the block's own in_conv feeds this pack (the resnets pack themselves)
        return _packed_from(self, [] if self.in_conv is None else [self.in_conv.weight, self.in_conv.bias])

    def _fwd(self, x):
        p = self.packed()
        if self.downsample is not None:
            x = K.avgpool2x(x)
        if self.in_conv is not None:
            n, hh, ww, c = x.shape
            x = K.gemm(x.view(-1, c), p["w_in"], p["b_in"]).view(n, hh, ww, -1)
        for r in self.resnets:
            x = r._fwd(x)
        return x


class FullAdapter(HipModule):
    """diffusers' FullAdapter: unshuffle, conv_in, body."""

    def __init__(self, in_channels: int, channels: Tuple[int, ...], num_res_blocks: int, downscale_factor: int):
        super().__init__()
        self.in_channels = in_channels
        self.unshuffle = nn.PixelUnshuffle(downscale_factor)
        self.conv_in = nn.Conv2d(in_channels * downscale_factor ** 2, channels[0], kernel_size=3, padding=1)
        self.body = nn.ModuleList([AdapterBlock(channels[0], channels[0], num_res_blocks)] +
                                  [AdapterBlock(channels[i - 1], channels[i], num_res_blocks, down=True) for i in range(1, len(channels))])
        self.total_downscale_factor = downscale_factor * 2 ** (len(channels) - 1)

    def _pack(self):
        return dict(w_in=pack_conv3x3(self.conv_in.weight), b_in=w16(self.conv_in.bias))

    def packed(self):
        return _packed_from(self, [self.conv_in.weight, self.conv_in.bias])

    def _fwd(self, frames):
        p = self.packed()
        x = K.conv3x3(K.pixel_unshuffle8(frames), p["w_in"], p["b_in"])
        features = []
        for block in self.body:
            x = block._fwd(x)
            features.append(x)
        return features


class T2IAdapter(PretrainedMixin, HipModule):
    """diffusers 0.24 T2IAdapter, adapter_type "full_adapter" (SD-1.5)."""

    def __init__(self, in_channels: int = 3, channels: Tuple[int, ...] = (320, 640, 1280, 1280), num_res_blocks: int = 2,
                 downscale_factor: int = 8, adapter_type: str = "full_adapter"):
        super().__init__()
        channels = tuple(int(c) for c in channels)
        self.config = _Config(in_channels=in_channels, channels=channels, num_res_blocks=num_res_blocks,
                              downscale_factor=downscale_factor, adapter_type=adapter_type)
        if adapter_type in ("light_adapter", "full_adapter_xl"):
            raise NotImplementedError(f"adapter_type={adapter_type!r} is not implemented: only 'full_adapter' (the SD-1.5 T2I-Adapters) is")
        if adapter_type != "full_adapter":
            raise ValueError(f"Unsupported adapter_type: '{adapter_type}'. Choose either 'full_adapter' or 'full_adapter_xl' or "
                             "'light_adapter'.")
        if downscale_factor != 8:
            raise NotImplementedError(f"downscale_factor={downscale_factor!r}: only 8 (the factor of the SD-1.5 VAE, so that the features "
                                      "meet the UNet's down levels) is implemented")
        if in_channels not in (1, 3):
            raise NotImplementedError(f"in_channels={in_channels!r}: the control frames have 1 (canny, sketch) or 3 channels")
        if len(channels) != 4 or any(c < 8 or c % 8 for c in channels):
            raise NotImplementedError(f"channels={channels!r}: four positive multiples of 8, one per down level of the UNet")
        if num_res_blocks < 1:
            raise ValueError(f"num_res_blocks={num_res_blocks!r} must be positive")
        self.adapter = FullAdapter(in_channels, channels, num_res_blocks, downscale_factor)

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def total_downscale_factor(self):
        return self.adapter.total_downscale_factor

    @property
    def downscale_factor(self):
        """the factor of the first feature map (diffusers' property of the same name)"""
        return self.config.downscale_factor

    def weight_signature(self):
        """identity and versions of every parameter"""
        return tuple((q.data_ptr(), q._version) for q in self.parameters())

    def _check_frames(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.config.in_channels:
            raise ValueError(f"the adapter's input must be (N, {self.config.in_channels}, height, width), got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        if x.shape[2] % 8 or x.shape[3] % 8 or x.shape[2] < 8 or x.shape[3] < 8:
            raise ValueError(f"the adapter's input height and width must be positive multiples of 8 (PixelUnshuffle(8)), got "
                             f"{tuple(x.shape[2:])}")
        if not x.is_cuda:
            raise HipLibraryError(f"the adapter's input is on {x.device}: the HIP path has no CPU fallback")
        if x.dtype not in (torch.float32, f16):
            raise TypeError(f"the adapter's input must be fp32 or fp16, got {x.dtype}")

    def embed(self, frames) -> List[torch.Tensor]:
        """frames (N, in_channels, 8 H, 8 W) in [0, 1] -> the four feature maps as tokens fp16 [N, h_i, w_i, C_i], h_0 = H and each
        further level the ceil half of the one before: the sizes of the UNet's four down levels.  Depends on the control frames only:
        once per sample, not per step."""
        self._check_frames(frames)
        return self.adapter._fwd(frames)

    def forward(self, x) -> List[torch.Tensor]:
        """diffusers' T2IAdapter.forward: (N, in_channels, 8 H, 8 W) -> a list of four NCHW tensors (N, C_i, h_i, w_i) in x's dtype"""
        self._check_frames(x)
        return [K.tokens_to_nchw(t, dtype=x.dtype) for t in self.adapter._fwd(x)]


def adapter_scale_table(num_steps: int, conditioning_scale: float = 1.0, conditioning_factor: float = 1.0):
    """diffusers' StableDiffusionAdapterPipeline rule, one value per executed step: the features are added at
    `adapter_conditioning_scale` on the steps i < int(num_steps * adapter_conditioning_factor) and not at all afterwards."""
    if not (0.0 <= conditioning_factor <= 1.0):
        raise ValueError(f"adapter_conditioning_factor must lie in [0, 1], got {conditioning_factor}")
    if num_steps < 1:
        raise ValueError(f"num_steps must be positive, got {num_steps}")
    on = int(num_steps * conditioning_factor)
    return [float(conditioning_scale) if i < on else 0.0 for i in range(num_steps)]
