"""AutoencoderTiny (TAESD) on the HIP kernels: the cheap VAE that goes with few-step sampling (LCMScheduler + LCM-LoRA).

Mirror of diffusers 0.24's `AutoencoderTiny`: a 64-channel, ReLU-only autoencoder without GroupNorm or attention, whose module tree
is two `nn.Sequential`s, so that a `taesd/` folder (config.json + diffusion_pytorch_model.safetensors) loads by key:

    encoder.layers:  0 Conv(3 -> 64)  1 Block  2 Conv(s2, no bias)  3-5 Block  6 Conv(s2)  7-9 Block  10 Conv(s2)  11-13 Block  14 Conv(64 -> 4)
    decoder.layers:  0 Conv(4 -> 64)  1 ReLU  2-4 Block  5 Upsample  6 Conv(no bias)  7-9 Block  10 Upsample  11 Conv  12-14 Block
                     15 Upsample  16 Conv  17 Block  18 Conv(64 -> 3)
    Block(x) = relu(conv.4(relu(conv.2(relu(conv.0(x))))) + x)
    encode(x).latents = encoder.layers((x + 1) / 2)            decode(z).sample = decoder.layers(3 tanh(z / 3)) * 2 - 1

diffusers is not installed where this was written: the layout is restated from its 0.24 source, `tests/taesd_reference.py` is the
specification, and no real TAESD checkpoint has been loaded.

Launches: `i2v_taesd_prep_f16` moves the NCHW input to token-major fp16 with 64 channels (the padding ones zero) through
the model's entry map; every stride-1 64 -> 64 convolution -- the blocks' with their ReLUs and the residual, and the two entry
convolutions with weights zero-padded to 64 input channels -- is one `i2v_conv3x3_c64_f16` launch; the stride-2 convolutions, the
up-sampling convolutions (nearest-2x folded into the weights) and the two narrow exits run on `kernels.conv3x3`, the decoder's
`* 2 - 1` folded into its `out_scale` and bias.
"""
from typing import Tuple

import torch
from torch import nn

from . import kernels as K
from ._lib import HipLibraryError
from .blocks import HipModule, pack_conv3x3, pack_upconv_fold, w16
from .checkpoint import PretrainedMixin
from .vae import _Config, _Out

f16 = torch.float16
WIDTH = 64


class AutoencoderTinyBlock(nn.Module):
    """diffusers `AutoencoderTinyBlock(64, 64, "relu")`: conv = Sequential(Conv, ReLU, Conv, ReLU, Conv), an identity skip, ReLU"""

    def __init__(self, channels: int = WIDTH):
        super().__init__()
        conv = lambda: nn.Conv2d(channels, channels, 3, padding=1)
        self.conv = nn.Sequential(conv(), nn.ReLU(), conv(), nn.ReLU(), conv())
        self.skip = nn.Identity()
        self.fuse = nn.ReLU()


class EncoderTiny(nn.Module):
    def __init__(self, in_channels, out_channels, num_blocks, block_out_channels):
        super().__init__()
        layers = []
        for i, nb in enumerate(num_blocks):
            c = block_out_channels[i]
            layers.append(nn.Conv2d(in_channels, c, 3, padding=1) if i == 0 else nn.Conv2d(c, c, 3, padding=1, stride=2, bias=False))
            layers += [AutoencoderTinyBlock(c) for _ in range(nb)]
        layers.append(nn.Conv2d(block_out_channels[-1], out_channels, 3, padding=1))
        self.layers = nn.Sequential(*layers)


class DecoderTiny(nn.Module):
    def __init__(self, in_channels, out_channels, num_blocks, block_out_channels, upsampling_scaling_factor):
        super().__init__()
        layers = [nn.Conv2d(in_channels, block_out_channels[0], 3, padding=1), nn.ReLU()]
        for i, nb in enumerate(num_blocks):
            final, c = i == len(num_blocks) - 1, block_out_channels[i]
            layers += [AutoencoderTinyBlock(c) for _ in range(nb)]
            if not final:
                layers.append(nn.Upsample(scale_factor=upsampling_scaling_factor))
            layers.append(nn.Conv2d(c, out_channels if final else c, 3, padding=1, bias=final))
        self.layers = nn.Sequential(*layers)


class AutoencoderTiny(PretrainedMixin, HipModule):
    def __init__(self, in_channels=3, out_channels=3, encoder_block_out_channels: Tuple[int, ...] = (64, 64, 64, 64),
                 decoder_block_out_channels: Tuple[int, ...] = (64, 64, 64, 64), act_fn="relu", latent_channels=4,
                 upsampling_scaling_factor=2, num_encoder_blocks: Tuple[int, ...] = (1, 3, 3, 3),
                 num_decoder_blocks: Tuple[int, ...] = (3, 3, 3, 1), latent_magnitude=3, latent_shift=0.5, force_upcast=False,
                 scaling_factor=1.0, **unknown):
        super().__init__()
        for k in unknown:
            if not k.startswith("_"):
                raise NotImplementedError(f"AutoencoderTiny: config key `{k}` is not implemented")
        enc_w, dec_w = tuple(encoder_block_out_channels), tuple(decoder_block_out_channels)
        nenc, ndec = tuple(int(v) for v in num_encoder_blocks), tuple(int(v) for v in num_decoder_blocks)
        if any(c != WIDTH for c in enc_w) or len(enc_w) != len(nenc) or len(enc_w) < 1:
            raise NotImplementedError(f"AutoencoderTiny: encoder_block_out_channels={enc_w}: the HIP path is the 64-channel model, one "
                                      "width per entry of num_encoder_blocks")
        if any(c != WIDTH for c in dec_w) or len(dec_w) != len(ndec) or len(dec_w) < 1:
            raise NotImplementedError(f"AutoencoderTiny: decoder_block_out_channels={dec_w}: the HIP path is the 64-channel model, one "
                                      "width per entry of num_decoder_blocks")
        if act_fn != "relu":
            raise NotImplementedError(f"AutoencoderTiny: act_fn={act_fn!r}: the convolution kernel's epilogue is ReLU")
        if upsampling_scaling_factor != 2:
            raise NotImplementedError(f"AutoencoderTiny: upsampling_scaling_factor={upsampling_scaling_factor}: nearest-2x only")
        if len(enc_w) != len(dec_w):
            raise NotImplementedError(f"AutoencoderTiny: num_encoder_blocks={nenc} and num_decoder_blocks={ndec} scale differently")
        if not (1 <= in_channels <= WIDTH and 1 <= latent_channels <= WIDTH):
            raise NotImplementedError(f"AutoencoderTiny: in_channels={in_channels} / latent_channels={latent_channels} must be 1..64")
        if any(v < 0 for v in nenc + ndec):
            raise ValueError("AutoencoderTiny: block counts must be non-negative")
        self.config = _Config(in_channels=in_channels, out_channels=out_channels, encoder_block_out_channels=enc_w,
                              decoder_block_out_channels=dec_w, act_fn=act_fn, latent_channels=latent_channels,
                              upsampling_scaling_factor=upsampling_scaling_factor, num_encoder_blocks=nenc, num_decoder_blocks=ndec,
                              latent_magnitude=latent_magnitude, latent_shift=latent_shift, force_upcast=force_upcast,
                              scaling_factor=scaling_factor, block_out_channels=dec_w)      # (registered by diffusers: vae_scale_factor)
        self.encoder = EncoderTiny(in_channels, latent_channels, nenc, enc_w)
        self.decoder = DecoderTiny(latent_channels, out_channels, ndec, dec_w, upsampling_scaling_factor)
        self.latent_magnitude, self.latent_shift = latent_magnitude, latent_shift
        self.spatial_scale_factor = 2 ** (len(enc_w) - 1)
        self.use_tiling = False
        self._trace = None          # a list: every launch appends (name, kind, input, output, residual) -- the tests' teacher-forced gate

    @classmethod
    def from_config(cls, config):
        # (block_out_channels is derived, not a constructor argument; everything else goes to __init__, which names what it refuses)
        return cls(**{k: v for k, v in dict(config).items() if k != "block_out_channels"})

    @property
    def device(self):
        return self.decoder.layers[0].weight.device

    @property
    def dtype(self):
        return self.decoder.layers[0].weight.dtype

    def enable_tiling(self, use_tiling: bool = True):
        raise NotImplementedError("AutoencoderTiny: tiled encode / decode is not implemented (enable_vae_slicing bounds the memory: "
                                  "one frame at a time)")

    def disable_tiling(self):
        self.use_tiling = False

    def scale_latents(self, x: torch.Tensor) -> torch.Tensor:
        """raw latents -> [0, 1] (diffusers: for storing them as an 8-bit image)"""
        return x.div(2 * self.latent_magnitude).add(self.latent_shift).clamp(0, 1)

    def unscale_latents(self, x: torch.Tensor) -> torch.Tensor:
        """[0, 1] -> raw latents"""
        return x.sub(self.latent_shift).mul(2 * self.latent_magnitude)

    # ------------------------------------------------------------------------------------------------ the launch plan
    def _plan(self, seq: nn.Sequential, prefix: str, exit_affine: bool):
        """the Sequential as a list of launches: ("c64", name, w, b, relu) / ("block", name, [(w, b)] * 3) / ("down", name, w) /
        ("up", name, w, w_folded) / ("exit", name, w, b, out_scale)"""
        ops, mods, i = [], list(seq), 0
        while i < len(mods):
            m, name = mods[i], f"{prefix}.layers.{i}"
            if isinstance(m, AutoencoderTinyBlock):
                ops.append(("block", name, [(K.pack_conv_c64(c.weight), w16(c.bias)) for c in (m.conv[0], m.conv[2], m.conv[4])]))
            elif isinstance(m, nn.Upsample):
                conv = mods[i + 1]
                ops.append(("up", f"{prefix}.layers.{i + 1}", pack_conv3x3(conv.weight), pack_upconv_fold(conv.weight)))
                i += 1
            elif isinstance(m, nn.Conv2d) and m.stride == (2, 2):
                ops.append(("down", name, pack_conv3x3(m.weight)))
            elif isinstance(m, nn.Conv2d) and m.out_channels == WIDTH:
                relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                ops.append(("c64", name, K.pack_conv_c64(m.weight), w16(m.bias), relu))
                i += int(relu)
            elif isinstance(m, nn.Conv2d):
                # the decoder's `* 2 - 1`:  ((acc + b) * 2 - 1) = (acc + (b - 1/2)) * 2
                b = m.bias.detach().float()
                ops.append(("exit", name, pack_conv3x3(m.weight), w16(b - 0.5 if exit_affine else b), 2.0 if exit_affine else 1.0))
            else:
                raise NotImplementedError(f"{name}: {type(m).__name__}")
            i += 1
        return ops

    def _pack(self):
        return dict(encoder=self._plan(self.encoder.layers, "encoder", False), decoder=self._plan(self.decoder.layers, "decoder", True))

    def _note(self, name, kind, x, y, residual=None):
        if self._trace is not None:
            self._trace.append((name, kind, x, y, residual))
        return y

    def _run(self, ops, x):
        """x token-major fp16 [N, H, W, 64] -> the exit convolution's fp32 [N, h, w, C]"""
        for op in ops:
            kind, name = op[0], op[1]
            if kind == "c64":
                x = self._note(name, kind, x, K.conv3x3_c64(x, op[2], op[3], relu_mid=op[4]))
            elif kind == "block":
                (w0, b0), (w1, b1), (w2, b2) = op[2]
                h0 = self._note(f"{name}.conv.0", kind, x, K.conv3x3_c64(x, w0, b0, relu_mid=True))
                h1 = self._note(f"{name}.conv.2", kind, h0, K.conv3x3_c64(h0, w1, b1, relu_mid=True))
                # (the first buffer is free again: neither the input nor the residual of the closing convolution)
                x = self._note(f"{name}.conv.4", kind, h1, K.conv3x3_c64(h1, w2, b2, residual=x, relu_out=True,
                                                                         out=h0 if self._trace is None else None), x)
            elif kind == "down":
                x = self._note(name, kind, x, K.conv3x3(x, op[2], None, stride=2))
            elif kind == "up":
                if K.upconv_fold_supported(x.shape, WIDTH):
                    y = K.conv3x3(x, op[2], None, upsample=True, w_folded=op[3])
                else:
                    y = K.conv3x3(x, op[2], None, upsample=True)
                x = self._note(name, kind, x, y)
            else:
                x = self._note(name, kind, x, K.conv3x3(x, op[2], op[3], out_scale=op[4], out_f32=True))
        return x

    def _input(self, t, what, channels):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != channels:
            raise ValueError(f"{what} must be [N, {channels}, H, W], got {tuple(getattr(t, 'shape', ()))}")
        if not t.is_cuda:
            raise HipLibraryError(f"{what} is on {t.device}: the HIP path has no CPU fallback")
        return t if t.dtype in (torch.float32, f16) else t.float()

    @torch.no_grad()
    def encode(self, x: torch.Tensor):
        """x (N, 3, H, W) in [-1, 1], H and W multiples of 8 -> `.latents` (N, 4, H / 8, W / 8) fp32.  Deterministic: there is no
        `latent_dist`."""
        x = self._input(x, "x", self.config.in_channels)
        s = self.spatial_scale_factor
        if x.shape[2] % s or x.shape[3] % s:
            raise ValueError(f"AutoencoderTiny.encode: {x.shape[2]} x {x.shape[3]} pixels are not multiples of {s}")
        t = self._note("encoder.prep", "prep", x, K.taesd_prep(x, "unit"))
        y = self._run(self.packed()["encoder"], t)
        return _Out(latents=K.tokens_to_nchw(y, dtype=torch.float32))

    @torch.no_grad()
    def decode(self, z: torch.Tensor):
        """z (N, 4, h, w) -> `.sample` (N, 3, 8h, 8w) fp32.  Every frame is decoded on its own: a batch equals its frames' decodes."""
        z = self._input(z, "z", self.config.latent_channels)
        t = self._note("decoder.prep", "prep", z, K.taesd_prep(z, "clamp"))
        y = self._run(self.packed()["decoder"], t)
        return _Out(sample=K.tokens_to_nchw(y, dtype=torch.float32))
