"""UNetMotionCrossFrameAttnModel on the HIP kernels: drop-in for
/root/reference/src/models/unet_motion_cross_frame_attn.py (block factories unet:29-162, block classes
unet:164-694, model unet:696-1451).  Same class names, ctor kwargs, attribute names, state-dict keys,
tensor layouts ((B, F, C, H, W) sample) and error behaviour; the arithmetic runs in libi2v_hip.so.

Inside the model activations stay token-major fp16 ([N, H, W, C]) from conv_in to conv_out: NCHW exists only at
the API edge.  Text / image context K,V are projected once per clip (not once per frame): the reference's
`repeat_interleave(num_frames)` of the context (unet:1355) and of the time embedding (unet:1344) become
index arithmetic (kv_group / rows_per_vec) inside the kernels.
"""
import inspect
from typing import Any, Dict, Optional, Tuple, Union

import torch
from torch import nn

from . import kernels as K
from ._lib import HipLibraryError
from .blocks import (Attention, DownBlockMotion, Downsample2D, HipModule, ImageProjection, MotionAdapter, Resampler,
                     ProjectedContext, ProjectedTemb, ResnetBlock2D, SampleProjectionMixin, TimestepEmbedding, Timesteps,
                     UpBlockMotion, freeu_scales, Upsample2D, _as_f16_matrix, _motion, from_tokens, pack_conv3x3, precise_stream, to_tokens, w16)
from .checkpoint import PretrainedMixin
from .i2v_adapter import I2VAdapterModule, I2VAdapterTransformer2DModel
from .lora import UNetLoraMixin

f16 = torch.float16


def _split_ctx(block, encoder_hidden_states):
    """(text tokens, IP tokens) of a reference-style concatenated context (unet:1353)."""
    t2d = block.attentions[0]
    return t2d.transformer_blocks[0]._split_ctx(encoder_hidden_states)


class CrossFrameAttnDownBlockMotion(nn.Module):
    """unet:164-340."""

    def __init__(self, in_channels: int, out_channels: int, temb_channels: int, dropout: float = 0.0,
                 num_layers: int = 1, transformer_layers_per_block: int = 1, resnet_eps: float = 1e-6,
                 resnet_time_scale_shift: str = "default", resnet_act_fn: str = "swish", resnet_groups: int = 32,
                 resnet_pre_norm: bool = True, num_attention_heads: int = 1, cross_attention_dim: int = 1280,
                 output_scale_factor: float = 1.0, downsample_padding: int = 1, add_downsample: bool = True,
                 dual_cross_attention: bool = False, use_linear_projection: bool = False,
                 only_cross_attention: bool = False, upcast_attention: bool = False,
                 attention_type: str = "default", temporal_cross_attention_dim: Optional[int] = None,
                 temporal_num_attention_heads: int = 8, temporal_max_seq_length: int = 32):
        super().__init__()
        self.has_cross_attention = True
        self.num_attention_heads = num_attention_heads
        resnets, attentions, motion_modules = [], [], []
        for i in range(num_layers):
            cin = in_channels if i == 0 else out_channels
            resnets.append(ResnetBlock2D(cin, out_channels, temb_channels=temb_channels, eps=resnet_eps,
                                         groups=resnet_groups, output_scale_factor=output_scale_factor))
            attentions.append(I2VAdapterTransformer2DModel(
                num_attention_heads, out_channels // num_attention_heads, in_channels=out_channels,
                num_layers=transformer_layers_per_block, cross_attention_dim=cross_attention_dim,
                norm_num_groups=resnet_groups, use_linear_projection=use_linear_projection,
                only_cross_attention=only_cross_attention))
            motion_modules.append(_motion(out_channels, temporal_num_attention_heads, resnet_groups,
                                          temporal_cross_attention_dim, temporal_max_seq_length))
        self.attentions = nn.ModuleList(attentions)
        self.resnets = nn.ModuleList(resnets)
        self.motion_modules = nn.ModuleList(motion_modules)
        self.downsamplers = (nn.ModuleList([Downsample2D(out_channels, use_conv=True, out_channels=out_channels,
                                                         padding=downsample_padding, name="op")])
                             if add_downsample else None)

    def _fwd(self, x, temb_act, enable, ctx_text, ctx_ip, num_frames, additional_residuals=None, cfg_shared=False,
             residual_scale=None):
        """cfg_shared (first down block only, unet._fwd_tokens): x is ONE of the two identical CFG halves; the first resnet
        and the prompt-independent stage of the first transformer run on it, the outputs carry both halves.
        additional_residuals (unet:329-330; a T2I-Adapter's feature map): tokens shaped like the last layer's output, or with a
        batch that divides it (one copy serves every repetition, K.add_broadcast_residual); residual_scale = (fp32 table, int32 step
        counter) on the device, or None for scale 1."""
        states = ()
        n_layers = len(self.resnets)
        for i, (resnet, attn, motion) in enumerate(zip(self.resnets, self.attentions, self.motion_modules)):
            shared = cfg_shared and i == 0
            x = resnet._fwd(x, temb_act.first_half() if shared else temb_act)         # unet:312
            x = attn._fwd(x, enable, num_frames, ctx_text, ctx_ip, cfg_expand=shared)   # unet:313-322
            x = motion._fwd(x, num_frames)                                            # unet:323-326
            if i == n_layers - 1 and additional_residuals is not None:                # unet:329-330
                x = K.add_broadcast_residual(x, additional_residuals, scale=residual_scale)
            states += (x,)
        if self.downsamplers is not None:                                             # unet:334-338
            for d in self.downsamplers:
                x = d._fwd(x)
            states += (x,)
        return x, states

    def forward(self, hidden_states, temb=None, enable_cross_frame_attn: bool = False,
                encoder_hidden_states=None, attention_mask=None, num_frames: int = 1,
                encoder_attention_mask=None, cross_attention_kwargs=None, additional_residuals=None):
        if attention_mask is not None or encoder_attention_mask is not None:
            raise NotImplementedError("attention masks are never passed on the hot path (SURVEY 8b)")
        ta = K.silu(_as_f16_matrix(temb)) if temb is not None else None
        ct, ci = _split_ctx(self, encoder_hidden_states)
        x, states = self._fwd(to_tokens(hidden_states), ta, enable_cross_frame_attn, ct, ci, num_frames,
                              None if additional_residuals is None else to_tokens(additional_residuals))
        dt = hidden_states.dtype
        return from_tokens(x, dt), tuple(from_tokens(s, dt) for s in states)


class CrossFrameAttnUpBlockMotion(nn.Module):
    """unet:342-529."""

    def __init__(self, in_channels: int, out_channels: int, prev_output_channel: int, temb_channels: int,
                 resolution_idx: Optional[int] = None, dropout: float = 0.0, num_layers: int = 1,
                 transformer_layers_per_block: int = 1, resnet_eps: float = 1e-6,
                 resnet_time_scale_shift: str = "default", resnet_act_fn: str = "swish", resnet_groups: int = 32,
                 resnet_pre_norm: bool = True, num_attention_heads: int = 1, cross_attention_dim: int = 1280,
                 output_scale_factor: float = 1.0, add_upsample: bool = True, dual_cross_attention: bool = False,
                 use_linear_projection: bool = False, only_cross_attention: bool = False,
                 upcast_attention: bool = False, attention_type: str = "default",
                 temporal_cross_attention_dim: Optional[int] = None, temporal_num_attention_heads: int = 8,
                 temporal_max_seq_length: int = 32):
        super().__init__()
        self.has_cross_attention = True
        self.num_attention_heads = num_attention_heads
        resnets, attentions, motion_modules = [], [], []
        for i in range(num_layers):
            res_skip_channels = in_channels if (i == num_layers - 1) else out_channels
            resnet_in_channels = prev_output_channel if i == 0 else out_channels
            resnets.append(ResnetBlock2D(resnet_in_channels + res_skip_channels, out_channels,
                                         temb_channels=temb_channels, eps=resnet_eps, groups=resnet_groups,
                                         output_scale_factor=output_scale_factor))
            attentions.append(I2VAdapterTransformer2DModel(
                num_attention_heads, out_channels // num_attention_heads, in_channels=out_channels,
                num_layers=transformer_layers_per_block, cross_attention_dim=cross_attention_dim,
                norm_num_groups=resnet_groups, use_linear_projection=use_linear_projection,
                only_cross_attention=only_cross_attention))
            motion_modules.append(_motion(out_channels, temporal_num_attention_heads, resnet_groups,
                                          temporal_cross_attention_dim, temporal_max_seq_length))
        self.attentions = nn.ModuleList(attentions)
        self.resnets = nn.ModuleList(resnets)
        self.motion_modules = nn.ModuleList(motion_modules)
        self.upsamplers = (nn.ModuleList([Upsample2D(out_channels, use_conv=True, out_channels=out_channels)])
                           if add_upsample else None)
        self.resolution_idx = resolution_idx

    def _fwd(self, x, res_tuple, temb_act, enable, ctx_text, ctx_ip, num_frames, upsample_size=None):
        fu = freeu_scales(self)
        for resnet, attn, motion in zip(self.resnets, self.attentions, self.motion_modules):
            skip = res_tuple[-1]
            res_tuple = res_tuple[:-1]
            if fu is not None:                                    # apply_freeu (unet:453-478): one launch, new tensors
                x, skip = K.freeu(x, skip, *fu)
            x = resnet._fwd(x, temb_act, x2=skip)                 # cat([x, skip], 1) (unet:478) never materialised
            x = attn._fwd(x, enable, num_frames, ctx_text, ctx_ip)
            x = motion._fwd(x, num_frames)
        if self.upsamplers is not None:
            for u in self.upsamplers:
                x = u._fwd(x, upsample_size)
        return x

    def forward(self, hidden_states, res_hidden_states_tuple, temb=None, enable_cross_frame_attn: bool = False,
                encoder_hidden_states=None, cross_attention_kwargs=None, upsample_size=None,
                attention_mask=None, encoder_attention_mask=None, num_frames: int = 1):
        if attention_mask is not None or encoder_attention_mask is not None:
            raise NotImplementedError("attention masks are never passed on the hot path (SURVEY 8b)")
        ta = K.silu(_as_f16_matrix(temb)) if temb is not None else None
        ct, ci = _split_ctx(self, encoder_hidden_states)
        res = tuple(to_tokens(r) for r in res_hidden_states_tuple)
        x = self._fwd(to_tokens(hidden_states), res, ta, enable_cross_frame_attn, ct, ci, num_frames, upsample_size)
        return from_tokens(x, hidden_states.dtype)


class UNetMidBlockCrossFrameAttnMotion(nn.Module):
    """unet:531-694."""

    def __init__(self, in_channels: int, temb_channels: int, dropout: float = 0.0, num_layers: int = 1,
                 transformer_layers_per_block: int = 1, resnet_eps: float = 1e-6,
                 resnet_time_scale_shift: str = "default", resnet_act_fn: str = "swish", resnet_groups: int = 32,
                 resnet_pre_norm: bool = True, num_attention_heads: int = 1, output_scale_factor: float = 1.0,
                 cross_attention_dim: int = 1280, dual_cross_attention=False, use_linear_projection=False,
                 upcast_attention=False, attention_type: str = "default", temporal_num_attention_heads: int = 1,
                 temporal_cross_attention_dim: Optional[int] = None, temporal_max_seq_length: int = 32):
        super().__init__()
        self.has_cross_attention = True
        self.num_attention_heads = num_attention_heads
        resnet_groups = resnet_groups if resnet_groups is not None else min(in_channels // 4, 32)

        def res():
            return ResnetBlock2D(in_channels, in_channels, temb_channels=temb_channels, eps=resnet_eps,
                                 groups=resnet_groups, output_scale_factor=output_scale_factor)

        resnets, attentions, motion_modules = [res()], [], []
        for _ in range(num_layers):
            attentions.append(I2VAdapterTransformer2DModel(
                num_attention_heads, in_channels // num_attention_heads, in_channels=in_channels,
                num_layers=transformer_layers_per_block, cross_attention_dim=cross_attention_dim,
                norm_num_groups=resnet_groups, use_linear_projection=use_linear_projection))
            resnets.append(res())
            motion_modules.append(_motion(in_channels, temporal_num_attention_heads, resnet_groups,
                                          temporal_cross_attention_dim, temporal_max_seq_length))
        self.attentions = nn.ModuleList(attentions)
        self.resnets = nn.ModuleList(resnets)
        self.motion_modules = nn.ModuleList(motion_modules)

    def _fwd(self, x, temb_act, enable, ctx_text, ctx_ip, num_frames):
        x = self.resnets[0]._fwd(x, temb_act)                                         # unet:639
        for attn, resnet, motion in zip(self.attentions, self.resnets[1:], self.motion_modules):
            x = attn._fwd(x, enable, num_frames, ctx_text, ctx_ip)                    # unet:678-692
            x = motion._fwd(x, num_frames)
            x = resnet._fwd(x, temb_act)
        return x

    def forward(self, hidden_states, temb=None, enable_cross_frame_attn: bool = False,
                encoder_hidden_states=None, attention_mask=None, cross_attention_kwargs=None,
                encoder_attention_mask=None, num_frames: int = 1):
        if attention_mask is not None or encoder_attention_mask is not None:
            raise NotImplementedError("attention masks are never passed on the hot path (SURVEY 8b)")
        ta = K.silu(_as_f16_matrix(temb)) if temb is not None else None
        ct, ci = _split_ctx(self, encoder_hidden_states)
        return from_tokens(self._fwd(to_tokens(hidden_states), ta, enable_cross_frame_attn, ct, ci, num_frames),
                           hidden_states.dtype)


def get_down_block(down_block_type, num_layers, in_channels, out_channels, temb_channels, add_downsample,
                   resnet_eps, resnet_act_fn, num_attention_heads, resnet_groups=None, cross_attention_dim=None,
                   downsample_padding=None, dual_cross_attention=False, use_linear_projection=True,
                   only_cross_attention=False, upcast_attention=False, resnet_time_scale_shift="default",
                   temporal_num_attention_heads=8, temporal_max_seq_length=32, transformer_layers_per_block=1):
    """unet:29-92."""
    if down_block_type == "DownBlockMotion":
        return DownBlockMotion(num_layers=num_layers, in_channels=in_channels, out_channels=out_channels,
                               temb_channels=temb_channels, add_downsample=add_downsample, resnet_eps=resnet_eps,
                               resnet_groups=resnet_groups, downsample_padding=downsample_padding,
                               temporal_num_attention_heads=temporal_num_attention_heads,
                               temporal_max_seq_length=temporal_max_seq_length)
    if down_block_type == "CrossFrameAttnDownBlockMotion":
        if cross_attention_dim is None:
            raise ValueError("cross_attention_dim must be specified for CrossFrameAttnDownBlockMotion")
        return CrossFrameAttnDownBlockMotion(
            num_layers=num_layers, in_channels=in_channels, out_channels=out_channels,
            temb_channels=temb_channels, add_downsample=add_downsample, resnet_eps=resnet_eps,
            resnet_groups=resnet_groups, downsample_padding=downsample_padding,
            cross_attention_dim=cross_attention_dim, num_attention_heads=num_attention_heads,
            use_linear_projection=use_linear_projection, only_cross_attention=only_cross_attention,
            temporal_num_attention_heads=temporal_num_attention_heads,
            temporal_max_seq_length=temporal_max_seq_length)
    raise ValueError(f"{down_block_type} does not exist.")


def get_up_block(up_block_type, num_layers, in_channels, out_channels, prev_output_channel, temb_channels,
                 add_upsample, resnet_eps, resnet_act_fn, num_attention_heads, resolution_idx=None,
                 resnet_groups=None, cross_attention_dim=None, dual_cross_attention=False,
                 use_linear_projection=True, only_cross_attention=False, upcast_attention=False,
                 resnet_time_scale_shift="default", temporal_num_attention_heads=8,
                 temporal_cross_attention_dim=None, temporal_max_seq_length=32, transformer_layers_per_block=1,
                 dropout=0.0):
    """unet:94-162."""
    if up_block_type == "UpBlockMotion":
        return UpBlockMotion(num_layers=num_layers, in_channels=in_channels, out_channels=out_channels,
                             prev_output_channel=prev_output_channel, temb_channels=temb_channels,
                             add_upsample=add_upsample, resnet_eps=resnet_eps, resnet_groups=resnet_groups,
                             resolution_idx=resolution_idx,
                             temporal_num_attention_heads=temporal_num_attention_heads,
                             temporal_max_seq_length=temporal_max_seq_length)
    if up_block_type == "CrossFrameAttnUpBlockMotion":
        if cross_attention_dim is None:
            raise ValueError("cross_attention_dim must be specified for CrossFrameAttnUpBlockMotion")
        return CrossFrameAttnUpBlockMotion(
            num_layers=num_layers, in_channels=in_channels, out_channels=out_channels,
            prev_output_channel=prev_output_channel, temb_channels=temb_channels, add_upsample=add_upsample,
            resnet_eps=resnet_eps, resnet_groups=resnet_groups, cross_attention_dim=cross_attention_dim,
            num_attention_heads=num_attention_heads, use_linear_projection=use_linear_projection,
            only_cross_attention=only_cross_attention, resolution_idx=resolution_idx,
            temporal_num_attention_heads=temporal_num_attention_heads,
            temporal_max_seq_length=temporal_max_seq_length)
    raise ValueError(f"{up_block_type} does not exist.")


class _Config(dict):
    __getattr__ = dict.get

    def __setattr__(self, k, v):
        self[k] = v


class UNet3DConditionOutput:
    def __init__(self, sample):
        self.sample = sample


class AttnProcessorHIP:
    """What `attn_processors` reports for an Attention module: the reference holds diffusers processor objects
    (`AttnProcessor2_0`, `IPAdapterAttnProcessor2_0(hidden_size, cross_attention_dim, num_tokens, scale)`,
    unet:1258-1279); here the attention arithmetic is the HIP kernel and the processor is a descriptor of the
    branch configuration (`num_tokens` = 0: plain attention; > 0: + decoupled image cross-attention)."""

    def __init__(self, num_tokens: int = 0, scale: float = 1.0):
        self.num_tokens, self.scale = num_tokens, scale

    def __repr__(self):
        if self.num_tokens:
            return f"IPAdapterAttnProcessorHIP(num_tokens={self.num_tokens}, scale={self.scale})"
        return "AttnProcessorHIP()"

    def __eq__(self, other):
        return isinstance(other, AttnProcessorHIP) and (self.num_tokens, self.scale) == (other.num_tokens, other.scale)


def convert_ip_adapter_plus_image_proj(image_proj):
    """the `image_proj` part of an IP-Adapter Plus file (the original repository's Resampler: `to_kv` fused, `norm1` / `norm2`) ->
    (constructor arguments of `blocks.Resampler`, its state dict).  The geometry is read off the file's shapes; every key the Resampler
    has must be there with its shape and no other may be: ValueError names the first that is not.  Nothing is built or modified."""
    sd = dict(image_proj)

    def need(key, dims):
        if key not in sd:
            raise ValueError(f"image_proj: missing key {key}")
        if sd[key].dim() != dims:
            raise ValueError(f"image_proj: {key} has shape {tuple(sd[key].shape)}, expected {dims} dimensions")
        return sd[key]

    latents = need("latents", 3)
    w_in, w_out = need("proj_in.weight", 2), need("proj_out.weight", 2)
    depth = 1 + max((int(k.split(".")[1]) for k in sd if k.startswith("layers.") and k.split(".")[1].isdigit()), default=-1)
    if depth < 1:
        raise ValueError("image_proj: missing key layers.0.0.to_q.weight")
    wq, w1 = need("layers.0.0.to_q.weight", 2), need("layers.0.1.1.weight", 2)
    hidden = latents.shape[2]
    if wq.shape[0] % 64 != 0 or wq.shape[0] == 0:
        raise ValueError(f"image_proj: layers.0.0.to_q.weight has {wq.shape[0]} rows, not a multiple of the head dimension 64")
    if w1.shape[0] % hidden != 0:
        raise ValueError(f"image_proj: layers.0.1.1.weight has {w1.shape[0]} rows, not a multiple of the latents' width {hidden}")
    kwargs = dict(embed_dims=w_in.shape[1], output_dims=w_out.shape[0], hidden_dims=hidden, depth=depth, dim_head=64,
                  heads=wq.shape[0] // 64, num_queries=latents.shape[1], ffn_ratio=w1.shape[0] // hidden)
    inner, ff = wq.shape[0], w1.shape[0]
    out, used = {}, set()

    def take(src, dst, shape):
        if src not in sd:
            raise ValueError(f"image_proj: missing key {src}")
        if tuple(sd[src].shape) != tuple(shape):
            raise ValueError(f"image_proj: {src} has shape {tuple(sd[src].shape)}, expected {tuple(shape)}")
        used.add(src)
        if dst is not None:
            out[dst] = sd[src]
        return sd[src]

    take("latents", "latents", (1, kwargs["num_queries"], hidden))
    for name, shape in (("proj_in", (hidden, kwargs["embed_dims"])), ("proj_out", (kwargs["output_dims"], hidden))):
        take(f"{name}.weight", f"{name}.weight", shape)
        take(f"{name}.bias", f"{name}.bias", shape[:1])
    for sfx in ("weight", "bias"):
        take(f"norm_out.{sfx}", f"norm_out.{sfx}", (kwargs["output_dims"],))
    for i in range(depth):
        for sfx in ("weight", "bias"):
            take(f"layers.{i}.0.norm1.{sfx}", f"layers.{i}.0.{sfx}", (hidden,))
            take(f"layers.{i}.0.norm2.{sfx}", f"layers.{i}.1.{sfx}", (hidden,))
            take(f"layers.{i}.1.0.{sfx}", f"layers.{i}.3.0.{sfx}", (hidden,))
        take(f"layers.{i}.0.to_q.weight", f"layers.{i}.2.to_q.weight", (inner, hidden))
        kv = take(f"layers.{i}.0.to_kv.weight", None, (2 * inner, hidden))
        out[f"layers.{i}.2.to_k.weight"], out[f"layers.{i}.2.to_v.weight"] = kv.chunk(2, dim=0)
        take(f"layers.{i}.0.to_out.weight", f"layers.{i}.2.to_out.0.weight", (hidden, inner))
        take(f"layers.{i}.1.1.weight", f"layers.{i}.3.1.net.0.proj.weight", (ff, hidden))
        take(f"layers.{i}.1.3.weight", f"layers.{i}.3.1.net.2.weight", (hidden, ff))
    for k in sd:
        if k not in used:
            raise ValueError(f"image_proj: unexpected key {k}")
    return kwargs, out


class UNetMotionCrossFrameAttnModel(UNetLoraMixin, SampleProjectionMixin, PretrainedMixin, HipModule):
    """unet:696-1451."""

    def __init__(self, sample_size: Optional[int] = None, in_channels: int = 4, out_channels: int = 4,
                 down_block_types: Tuple[str, ...] = ("CrossFrameAttnDownBlockMotion",
                                                      "CrossFrameAttnDownBlockMotion",
                                                      "CrossFrameAttnDownBlockMotion", "DownBlockMotion"),
                 up_block_types: Tuple[str, ...] = ("UpBlockMotion", "CrossFrameAttnUpBlockMotion",
                                                    "CrossFrameAttnUpBlockMotion", "CrossFrameAttnUpBlockMotion"),
                 block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280), layers_per_block: int = 2,
                 downsample_padding: int = 1, mid_block_scale_factor: float = 1, act_fn: str = "silu",
                 norm_num_groups: int = 32, norm_eps: float = 1e-5, cross_attention_dim: int = 1280,
                 use_linear_projection: bool = False, num_attention_heads: Union[int, Tuple[int, ...]] = 8,
                 motion_max_seq_length: int = 32, motion_num_attention_heads: int = 8,
                 use_motion_mid_block: int = True, encoder_hid_dim: Optional[int] = None,
                 encoder_hid_dim_type: Optional[str] = None):
        super().__init__()
        self.config = _Config(
            sample_size=sample_size, in_channels=in_channels, out_channels=out_channels,
            down_block_types=tuple(down_block_types), up_block_types=tuple(up_block_types),
            block_out_channels=tuple(block_out_channels), layers_per_block=layers_per_block,
            downsample_padding=downsample_padding, mid_block_scale_factor=mid_block_scale_factor, act_fn=act_fn,
            norm_num_groups=norm_num_groups, norm_eps=norm_eps, cross_attention_dim=cross_attention_dim,
            use_linear_projection=use_linear_projection, num_attention_heads=num_attention_heads,
            motion_max_seq_length=motion_max_seq_length, motion_num_attention_heads=motion_num_attention_heads,
            use_motion_mid_block=use_motion_mid_block, encoder_hid_dim=encoder_hid_dim,
            encoder_hid_dim_type=encoder_hid_dim_type)
        self.sample_size = sample_size
        self.layers_per_block = layers_per_block
        self.num_attention_heads = num_attention_heads
        if act_fn not in ("silu", "swish"):
            raise NotImplementedError("hot path uses act_fn='silu'")
        if len(down_block_types) != len(up_block_types):
            raise ValueError(
                f"Must provide the same number of `down_block_types` as `up_block_types`. `down_block_types`: "
                f"{down_block_types}. `up_block_types`: {up_block_types}.")
        if len(block_out_channels) != len(down_block_types):
            raise ValueError(
                f"Must provide the same number of `block_out_channels` as `down_block_types`. "
                f"`block_out_channels`: {block_out_channels}. `down_block_types`: {down_block_types}.")
        if not isinstance(num_attention_heads, int) and len(num_attention_heads) != len(down_block_types):
            raise ValueError(
                f"Must provide the same number of `num_attention_heads` as `down_block_types`. "
                f"`num_attention_heads`: {num_attention_heads}. `down_block_types`: {down_block_types}.")

        self.conv_in = nn.Conv2d(in_channels, block_out_channels[0], kernel_size=3, padding=1)   # unet:757
        time_embed_dim = block_out_channels[0] * 4
        self.time_proj = Timesteps(block_out_channels[0], True, 0)                               # unet:763
        self.time_embedding = TimestepEmbedding(block_out_channels[0], time_embed_dim, act_fn=act_fn)
        self.encoder_hid_proj = None
        self.down_blocks = nn.ModuleList([])
        self.up_blocks = nn.ModuleList([])
        if isinstance(num_attention_heads, int):
            num_attention_heads = (num_attention_heads,) * len(down_block_types)

        output_channel = block_out_channels[0]
        for i, t in enumerate(down_block_types):                                                 # unet:783-807
            input_channel = output_channel
            output_channel = block_out_channels[i]
            is_final = i == len(block_out_channels) - 1
            self.down_blocks.append(get_down_block(
                t, num_layers=layers_per_block, in_channels=input_channel, out_channels=output_channel,
                temb_channels=time_embed_dim, add_downsample=not is_final, resnet_eps=norm_eps,
                resnet_act_fn=act_fn, resnet_groups=norm_num_groups, cross_attention_dim=cross_attention_dim,
                num_attention_heads=num_attention_heads[i], downsample_padding=downsample_padding,
                use_linear_projection=use_linear_projection,
                temporal_num_attention_heads=motion_num_attention_heads,
                temporal_max_seq_length=motion_max_seq_length))

        self.mid_block = UNetMidBlockCrossFrameAttnMotion(                                       # unet:810-822
            in_channels=block_out_channels[-1], temb_channels=time_embed_dim, resnet_eps=norm_eps,
            output_scale_factor=mid_block_scale_factor, cross_attention_dim=cross_attention_dim,
            num_attention_heads=num_attention_heads[-1], resnet_groups=norm_num_groups,
            temporal_num_attention_heads=motion_num_attention_heads,
            temporal_max_seq_length=motion_max_seq_length)

        self.num_upsamplers = 0
        rev_ch = list(reversed(block_out_channels))
        rev_heads = list(reversed(num_attention_heads))
        output_channel = rev_ch[0]
        for i, t in enumerate(up_block_types):                                                   # unet:831-866
            is_final = i == len(block_out_channels) - 1
            prev_output_channel = output_channel
            output_channel = rev_ch[i]
            input_channel = rev_ch[min(i + 1, len(block_out_channels) - 1)]
            add_upsample = not is_final
            if add_upsample:
                self.num_upsamplers += 1
            self.up_blocks.append(get_up_block(
                t, num_layers=layers_per_block + 1, in_channels=input_channel, out_channels=output_channel,
                prev_output_channel=prev_output_channel, temb_channels=time_embed_dim,
                add_upsample=add_upsample, resnet_eps=norm_eps, resnet_act_fn=act_fn,
                resnet_groups=norm_num_groups, cross_attention_dim=cross_attention_dim,
                num_attention_heads=rev_heads[i], resolution_idx=i, use_linear_projection=use_linear_projection,
                temporal_num_attention_heads=motion_num_attention_heads,
                temporal_max_seq_length=motion_max_seq_length))

        if norm_num_groups is not None:                                                          # unet:869-876
            self.conv_norm_out = nn.GroupNorm(num_channels=block_out_channels[0], num_groups=norm_num_groups,
                                              eps=norm_eps)
            self.conv_act = nn.SiLU()
        else:
            raise NotImplementedError("norm_num_groups=None is not on the hot path")
        self.conv_out = nn.Conv2d(block_out_channels[0], out_channels, kernel_size=3, padding=1)

    # ------------------------------------------------------------------ weight assembly
    @property
    def dtype(self):
        return next(self.parameters()).dtype

    @property
    def device(self):
        return next(self.parameters()).device

    @classmethod
    def from_unet2d(cls, unet, motion_adapter, i2v_adapter: Optional[I2VAdapterModule] = None,
                    load_weights: bool = True):
        """unet:883-977."""
        config = dict(unet.config)
        config["_class_name"] = cls.__name__
        config["down_block_types"] = ["CrossFrameAttnDownBlockMotion" if "CrossAttn" in t else "DownBlockMotion"
                                      for t in config["down_block_types"]]
        config["up_block_types"] = ["CrossFrameAttnUpBlockMotion" if "CrossAttn" in t else "UpBlockMotion"
                                    for t in config["up_block_types"]]
        config["motion_num_attention_heads"] = motion_adapter.config["motion_num_attention_heads"]
        config["motion_max_seq_length"] = motion_adapter.config["motion_max_seq_length"]
        config["use_motion_mid_block"] = motion_adapter.config["use_motion_mid_block"]
        if not config.get("num_attention_heads"):
            config["num_attention_heads"] = config["attention_head_dim"]                 # unet:918-919
        model = cls.from_config(config)
        if not load_weights:
            return model
        model.conv_in.load_state_dict(unet.conv_in.state_dict())
        model.time_embedding.load_state_dict(unet.time_embedding.state_dict())
        for i, down_block in enumerate(unet.down_blocks):
            model.down_blocks[i].resnets.load_state_dict(down_block.resnets.state_dict())
            if hasattr(model.down_blocks[i], "attentions"):
                for mine, theirs in zip(model.down_blocks[i].attentions, down_block.attentions):
                    mine.from_transformer2d_model(theirs)
            if model.down_blocks[i].downsamplers:
                model.down_blocks[i].downsamplers.load_state_dict(down_block.downsamplers.state_dict())
        for i, up_block in enumerate(unet.up_blocks):
            model.up_blocks[i].resnets.load_state_dict(up_block.resnets.state_dict())
            if hasattr(model.up_blocks[i], "attentions"):
                for mine, theirs in zip(model.up_blocks[i].attentions, up_block.attentions):
                    mine.from_transformer2d_model(theirs)
            if model.up_blocks[i].upsamplers:
                model.up_blocks[i].upsamplers.load_state_dict(up_block.upsamplers.state_dict())
        model.mid_block.resnets.load_state_dict(unet.mid_block.resnets.state_dict())
        if hasattr(model.mid_block, "attentions"):
            for mine, theirs in zip(model.mid_block.attentions, unet.mid_block.attentions):
                mine.from_transformer2d_model(theirs)
        if unet.conv_norm_out is not None:
            model.conv_norm_out.load_state_dict(unet.conv_norm_out.state_dict())
        model.conv_out.load_state_dict(unet.conv_out.state_dict())
        model.load_motion_modules(motion_adapter)
        if i2v_adapter is not None:
            model.load_i2v_adapter(i2v_adapter)
        p = next(unet.parameters())
        model.to(device=p.device, dtype=p.dtype)                                         # unet:975
        return model

    def freeze_unet_params(self, freeze_animatediff=True) -> None:
        """unet:979-1026: the adapter's to_q / to_out train; with freeze_animatediff=False (`--update_motion_modules`) every
        motion-module parameter too.  (training.UNetAdapterTrainer / AdapterOptimizer take the same switch.)"""
        for p in self.parameters():
            p.requires_grad = False
        for name, p in self.named_parameters():
            if ".i2v_adapter.to_q." in name or ".i2v_adapter.to_out." in name:
                p.requires_grad = True
            if not freeze_animatediff and ".motion_modules." in name:
                p.requires_grad = True

    def load_motion_modules(self, motion_adapter) -> None:
        """unet:1028-1036."""
        for i, down_block in enumerate(motion_adapter.down_blocks):
            self.down_blocks[i].motion_modules.load_state_dict(down_block.motion_modules.state_dict())
        for i, up_block in enumerate(motion_adapter.up_blocks):
            self.up_blocks[i].motion_modules.load_state_dict(up_block.motion_modules.state_dict())
        if hasattr(self.mid_block, "motion_modules"):
            self.mid_block.motion_modules.load_state_dict(motion_adapter.mid_block.motion_modules.state_dict())

    def load_i2v_adapter(self, i2v_adapter: I2VAdapterModule):
        """unet:1038-1041."""
        self.down_blocks.load_state_dict(i2v_adapter.down_blocks.state_dict(), strict=False)
        self.up_blocks.load_state_dict(i2v_adapter.up_blocks.state_dict(), strict=False)
        self.mid_block.load_state_dict(i2v_adapter.mid_block.state_dict(), strict=False)

    def obtain_i2v_adapter_modules(self):
        """unet:1043-1058."""
        sd = {k: v for k, v in self.state_dict().items() if "i2v_adapter" in k}
        m = I2VAdapterModule(self.layers_per_block, self.config.block_out_channels, self.num_attention_heads)
        m.load_state_dict(sd)
        return m

    def obtain_motion_modules(self):
        """unet:1060-1078."""
        sd = {k: v for k, v in self.state_dict().items() if "motion_modules" in k}
        ma = MotionAdapter(block_out_channels=self.config["block_out_channels"],
                           motion_layers_per_block=self.config["layers_per_block"],
                           motion_norm_num_groups=self.config["norm_num_groups"],
                           motion_num_attention_heads=self.config["motion_num_attention_heads"],
                           motion_max_seq_length=self.config["motion_max_seq_length"],
                           use_motion_mid_block=self.config["use_motion_mid_block"])
        ma.load_state_dict(sd)
        return ma

    def save_i2v_adapter_modules(self, save_directory: str, is_main_process: bool = True,
                                 safe_serialization: bool = True, variant: Optional[str] = None,
                                 push_to_hub: bool = False, **kwargs):
        """unet:1080-1097."""
        self.obtain_i2v_adapter_modules().save_pretrained(
            save_directory=save_directory, is_main_process=is_main_process, safe_serialization=safe_serialization,
            variant=variant, push_to_hub=push_to_hub, **kwargs)

    def save_motion_modules(self, save_directory: str, is_main_process: bool = True,
                            safe_serialization: bool = True, variant: Optional[str] = None,
                            push_to_hub: bool = False, **kwargs) -> None:
        """unet:1099-1116."""
        self.obtain_motion_modules().save_pretrained(
            save_directory=save_directory, is_main_process=is_main_process, safe_serialization=safe_serialization,
            variant=variant, push_to_hub=push_to_hub, **kwargs)

    @property
    def attn_processors(self) -> Dict[str, AttnProcessorHIP]:
        """unet:1118-1136: {"<module path>.processor": processor} for every Attention, in registration order."""
        modules = dict(self.named_modules())
        out = {}
        for name in self.attn_processor_names():
            a = modules[name[: -len(".processor")]]
            out[name] = AttnProcessorHIP(a.ip_num_tokens, a.ip_scale)
        return out

    def set_attn_processor(self, processor, _remove_lora=False):
        """unet:1138-1161.  Accepts one descriptor for all layers or a dict keyed like `attn_processors`.  A
        descriptor can change the IP branch's scale or switch the branch off (num_tokens = 0); switching it ON
        needs weights and goes through `_load_ip_adapter_weights`."""
        names = self.attn_processor_names()
        if isinstance(processor, dict) and len(processor) != len(names):
            raise ValueError(
                f"A dict of processors was passed, but the number of processors {len(processor)} does not match the"
                f" number of attention layers: {len(names)}. Please make sure to pass {len(names)} processor classes.")
        modules = dict(self.named_modules())
        for name in names:
            proc = processor[name] if isinstance(processor, dict) else processor
            if not isinstance(proc, AttnProcessorHIP):
                raise TypeError(f"{name}: expected an AttnProcessorHIP descriptor, got {type(proc).__name__}")
            a = modules[name[: -len(".processor")]]
            if proc.num_tokens and a.to_k_ip is None:
                raise ValueError(f"{name}: the IP-Adapter branch has no weights; load them with "
                                 "`_load_ip_adapter_weights` first")
            a.ip_num_tokens, a.ip_scale = proc.num_tokens, proc.scale

    def attn_processor_names(self):
        """Enumeration order of the reference's `attn_processors` (unet:1118-1136): one entry per Attention,
        walking named_children() => down_blocks, up_blocks, mid_block (registration order unet:776-777,810)."""
        names = []

        def rec(name, module):
            if isinstance(module, Attention):
                names.append(f"{name}.processor")
            for sub, child in module.named_children():
                rec(f"{name}.{sub}", child)

        for name, module in self.named_children():
            rec(name, module)
        return names

    def _load_ip_adapter_weights(self, state_dict, num_image_tokens: Optional[int] = None):
        """unet:1230-1287, branching on the file as the reference does: `proj.weight` is the plain IP-Adapter (4 image tokens through
        ImageProjection); `proj.3.weight` is Full Face, which raises NotImplementedError; anything else is IP-Adapter Plus
        (`latents.shape[1]` image tokens through the Resampler).  A Plus file is converted and validated, and the
        Resampler built, before any module is touched: a missing or unexpected key, or a `to_q` whose rows are no multiple of 64, raises
        ValueError naming the key; a geometry outside i2v_perceiver_attention_f16's envelope (more than 64 queries; with
        `num_image_tokens` = the image encoder's token count given, more than 288 tokens + queries) raises NotImplementedError with the
        limit.  More than 16 image tokens do load: i2v_cross_attn_fused_f16 takes at most 16, and the transformer blocks then run the
        text and image attention through the un-fused kernels (BasicTransformerBlock's fall-back), slower per step."""
        ip = state_dict["image_proj"]
        if "proj.weight" in ip:
            num_tokens = 4
            clip_dim = ip["proj.weight"].shape[-1]
            cross_dim = ip["proj.weight"].shape[0] // 4
            proj = ImageProjection(image_embed_dim=clip_dim, cross_attention_dim=cross_dim, num_image_text_embeds=num_tokens)
            proj.load_state_dict({"image_embeds.weight": ip["proj.weight"], "image_embeds.bias": ip["proj.bias"],
                                  "norm.weight": ip["norm.weight"], "norm.bias": ip["norm.bias"]})
        elif "proj.3.weight" in ip:
            raise NotImplementedError("IP-Adapter Full Face (257 image tokens through MLPProjection) is not implemented: the plain "
                                      "IP-Adapter and IP-Adapter Plus are")
        else:
            kwargs, converted = convert_ip_adapter_plus_image_proj(ip)
            num_tokens = kwargs["num_queries"]
            proj = Resampler(**kwargs)
            if num_image_tokens is not None:
                proj.check_tokens(num_image_tokens)
            proj.load_state_dict(converted)
        modules = dict(self.named_modules())
        targets = [modules[name[: -len(".processor")]] for name in self.attn_processor_names()
                   if name.endswith("attn2.processor") and "motion_modules" not in name]      # unet:1258-1262
        if isinstance(proj, Resampler) and proj.output_dims != self.config.cross_attention_dim:
            raise ValueError(f"proj_out.weight: {proj.output_dims} output channels, the UNet's cross_attention_dim is "
                             f"{self.config.cross_attention_dim}")
        for i in range(len(targets)):
            for k in (f"{2 * i + 1}.to_k_ip.weight", f"{2 * i + 1}.to_v_ip.weight"):        # key_id 1, 3, 5, ... (unet:1279)
                if k not in state_dict["ip_adapter"]:
                    raise ValueError(f"ip_adapter: missing key {k}")
        self.encoder_hid_proj = None
        for i, attn in enumerate(targets):
            attn.install_ip_adapter(state_dict["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"],
                                    state_dict["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"], num_tokens=num_tokens, scale=1.0)
        self.encoder_hid_proj = proj.to(device=self.device, dtype=self.dtype)
        self.config.encoder_hid_dim_type = "ip_image_proj"

    # ------------------------------------------------------------------ forward
    def _pack(self):
        cin_pad = K.pad8(self.config.in_channels)
        return dict(w_in=pack_conv3x3(self.conv_in.weight, cin_pad=cin_pad), b_in=w16(self.conv_in.bias),
                    g_out=w16(self.conv_norm_out.weight), be_out=w16(self.conv_norm_out.bias),
                    w_out=pack_conv3x3(self.conv_out.weight), b_out=w16(self.conv_out.bias), cin_pad=cin_pad)

    def packed(self):
        self._sync_lora()
        # only the UNet's own leaf parameters feed this pack (children pack themselves)
        leaves = [self.conv_in.weight, self.conv_in.bias, self.conv_norm_out.weight, self.conv_norm_out.bias,
                  self.conv_out.weight, self.conv_out.bias]
        key = tuple((p.data_ptr(), p._version, p.dtype) for p in leaves)
        if self._packed is None or key != self._packed_key:
            with torch.no_grad():
                self._packed = self._pack()
            self._packed_key = key
        return self._packed

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float) -> None:
        """unet:1213-1219 (https://arxiv.org/abs/2309.11497): the four scales as attributes of every up block.  The blocks with
        resolution_idx 0 (b1, s1) and 1 (b2, s2) then scale the first half of the backbone channels by b and the four lowest
        spatial frequencies of each skip tensor by s ahead of every skip concatenation (i2v_freeu_f16); a zero or None among the
        four leaves FreeU off, as in the reference.  The values are launch arguments: a captured step is re-captured."""
        for blk in self.up_blocks:
            blk.s1, blk.s2, blk.b1, blk.b2 = s1, s2, b1, b2

    def disable_freeu(self) -> None:
        """unet:1221-1228."""
        for blk in self.up_blocks:
            for k in ("s1", "s2", "b1", "b2"):
                if getattr(blk, k, None) is not None:
                    setattr(blk, k, None)

    def freeu_signature(self):
        """what FreeU bakes into the launches of a forward: (b, s) of every up block that applies it (None where it does not)"""
        return tuple(freeu_scales(blk) for blk in self.up_blocks)

    def _motion_modules(self):
        from .blocks import TransformerTemporalModel
        return [m for m in self.modules() if isinstance(m, TransformerTemporalModel)]

    def enable_free_noise(self, context_length: int = 16, context_stride: int = 4, weighting_scheme: str = "pyramid",
                          noise_type: str = "shuffle_context") -> None:
        """diffusers AnimateDiffFreeNoiseMixin.enable_free_noise (FreeNoise, https://arxiv.org/abs/2310.15169): clips longer than
        `context_length` frames.  Every motion module then runs its temporal attention on sliding windows of `context_length` frames,
        `context_stride` apart (positions restart in each), and takes per frame the mean of the windows that cover it, weighted over
        the position in the window by `weighting_scheme` ("flat", "pyramid", "delayed_reverse_sawtooth"); everything else -- entry
        GroupNorm, projections, feed-forward, the spatial path -- runs on all frames as before.  `noise_type` ("shuffle_context",
        "repeat_context", "random") is the pipeline's rescheduling of the initial noise.  A forward of at most `context_length`
        frames is unchanged; the settings are checked here and against num_frames in the forward."""
        from . import free_noise
        settings = free_noise.check_free_noise_args(context_length, context_stride, weighting_scheme, noise_type,
                                                    self.config["motion_max_seq_length"])
        for m in self._motion_modules():
            m.set_free_noise(settings)
        self._free_noise = settings

    def disable_free_noise(self) -> None:
        """diffusers disable_free_noise: the motion modules attend over the whole clip again (at most motion_max_seq_length frames)"""
        for m in self._motion_modules():
            m.set_free_noise(None)
        self._free_noise = None

    _free_noise = None      # FreeNoiseSettings while enabled (class default: modules built before the switch existed read None)

    def free_noise_signature(self):
        """the FreeNoise settings: None when disabled, else (context_length, context_stride, weighting_scheme, noise_type).  The
        first three decide the launches of a forward (`free_noise_launch_signature`); noise_type only the pipeline's initial noise."""
        fn = self._free_noise
        return None if fn is None else tuple(fn)

    def free_noise_launch_signature(self):
        """what FreeNoise bakes into the launches of a forward (the captured step's key): None, or (context_length, context_stride,
        weighting_scheme)"""
        sig = self.free_noise_signature()
        return None if sig is None else sig[:3]

    def _cross_attention_layers(self):
        """the spatial blocks' attn2 modules, in attn_processors order."""
        modules = dict(self.named_modules())
        return [modules[n[: -len(".processor")]] for n in self.attn_processor_names()
                if n.endswith("attn2.processor") and "motion_modules" not in n]

    def _fwd_tokens(self, x, temb, enable_cross_frame_attn, ctx_text, ctx_ip, num_frames, cfg_shared=False, temb_proj=None,
                    forward_upsample_size=False, down_residuals=None, mid_residual=None, residual_scale=None,
                    intrablock_residuals=None, intrablock_scale=None, residual_sets=None):
        """x: model-input tokens [B*F, H, W, cin_pad] fp16; temb [B, 4*C0] fp16 (pre-SiLU) -- or temb_proj [B or 1, sum Cout]:
        the resnets' time-embedding projections already computed (project_time_table); ctx_text [B, Lt, D]
        (+ ctx_ip [B, 4, D]) or a ProjectedContext; returns noise-prediction tokens [B*F, H, W, out_channels].
        down_residuals / mid_residual (a ControlNet's outputs, unet:1299-1300): token tensors shaped like the skip tensors (full
        batch, also under cfg_shared) and like the mid block's output; residual_scale = (fp32 table, int32 step counter) on the
        device, or None for scale 1 (K.add_residuals).
        residual_sets (several ControlNets' outputs, instead of down_residuals / mid_residual): a list of N (down tensors, mid
        tensor) pairs, each as above; residual_scale then carries an fp32 [N, rows] table, one row per set.  All sets are added in
        one launch for the skip tensors and one for the mid tensor (K.add_multi_residuals): summed in fp32, rounded once.
        intrablock_residuals (a T2I-Adapter's features, diffusers' down_intrablock_additional_residuals): one token tensor per down
        block, [n, h, w, C] of that block's level with n dividing the full batch (also under cfg_shared); intrablock_scale as
        residual_scale.  A block with cross-attention adds its tensor to the output of its last layer, before that is recorded as a
        skip tensor and before the down-sampler (unet:329-330); a block without adds it to the hidden state it returns, in place --
        which is also its last skip tensor and, for the last block, the mid block's input."""
        if self._free_noise is not None:
            from .free_noise import check_num_frames
            check_num_frames(num_frames, self._free_noise)
        if intrablock_residuals is not None:
            intrablock_residuals = list(intrablock_residuals)
            self._check_intrablock_residuals(intrablock_residuals, tuple(x.shape))
        if residual_sets is not None and (down_residuals is not None or mid_residual is not None):
            raise ValueError("residual_sets comes instead of down_residuals / mid_residual, not beside them")
        p = self.packed()
        wt, bt, slices = self._temb_pack()
        # ResnetBlock2D: time_emb_proj(nonlinearity(temb)) of all 22 resnets in one GEMM
        temb_act = ProjectedTemb(temb_proj if temb_proj is not None else K.gemm(K.silu(temb), wt, bt), slices)
        temb_rows = temb_proj.shape[0] if temb_proj is not None else temb.shape[0]
        # cfg_shared: the caller's batch is [unconditional half ; conditional half] of the SAME latents at the SAME timestep
        # (pipe:672-673 `torch.cat([latents] * 2)`).  Until the first text cross-attention the two halves are the same
        # numbers -- conv_in, the first resnet, GroupNorm / proj_in and the whole self- + cross-frame attention stage of the
        # first transformer (two 4096 x 4096 attentions per frame at 512 x 512) -- so they are computed once and duplicated
        # where the prompt enters.  Same arithmetic per element; the bits are identical whenever the dispatcher picks the same
        # kernel forms for the half and the full batch (it does at 16 f x 512 x 512), else equal to reduction-order rounding
        # (tests/test_full_width_gpu.py).
        cfg_shared = (cfg_shared and x.shape[0] % (2 * num_frames) == 0 and (temb_rows == 1 or temb_rows % 2 == 0) and
                      isinstance(self.down_blocks[0], CrossFrameAttnDownBlockMotion))
        if cfg_shared:
            x = x[: x.shape[0] // 2]
        x = K.conv3x3(x, p["w_in"], p["b_in"], precise=precise_stream())                # unet:1359
        res = (K.duplicate_batch(x) if cfg_shared else x,)
        for bi, blk in enumerate(self.down_blocks):                                     # unet:1362-1377
            feat = None if intrablock_residuals is None else intrablock_residuals[bi]
            if getattr(blk, "has_cross_attention", False):
                x, r = blk._fwd(x, temb_act, enable_cross_frame_attn, ctx_text, ctx_ip, num_frames, additional_residuals=feat,
                                cfg_shared=cfg_shared and bi == 0, residual_scale=intrablock_scale)
            else:
                x, r = blk._fwd(x, temb_act, num_frames, additional_residuals=feat, residual_scale=intrablock_scale)
            res += r
        if down_residuals is not None:                                                  # unet:1379-1389
            if len(down_residuals) != len(res):
                raise ValueError(f"down_block_additional_residuals: {len(down_residuals)} tensors for {len(res)} skip tensors")
            # new tensors: the last skip tensor IS the mid block's input, which takes no residual (no down-sampler after the last
            # block); an in-place add would change what the mid block reads
            res = tuple(K.add_residuals(res, down_residuals, scale=residual_scale))
        elif residual_sets is not None:
            for k, (down, _) in enumerate(residual_sets):
                if len(down) != len(res):
                    raise ValueError(f"residual set {k}: {len(down)} tensors for {len(res)} skip tensors")
            res = tuple(K.add_multi_residuals(res, [down for down, _ in residual_sets], scale=residual_scale))
        x = self.mid_block._fwd(x, temb_act, enable_cross_frame_attn, ctx_text, ctx_ip, num_frames)
        if mid_residual is not None:                                                    # unet:1402-1403
            x, = K.add_residuals([x], [mid_residual], scale=residual_scale, out=[x])
        elif residual_sets is not None:
            x, = K.add_multi_residuals([x], [[mid] for _, mid in residual_sets], scale=residual_scale, out=[x])
        upsample_size = None
        for bi, blk in enumerate(self.up_blocks):                                       # unet:1406-1436
            r = res[-len(blk.resnets):]
            res = res[: -len(blk.resnets)]
            if bi + 1 < len(self.up_blocks) and forward_upsample_size:                  # unet:1414-1415
                upsample_size = tuple(res[-1].shape[1:3])
            if getattr(blk, "has_cross_attention", False):
                x = blk._fwd(x, r, temb_act, enable_cross_frame_attn, ctx_text, ctx_ip, num_frames, upsample_size)
            else:
                x = blk._fwd(x, r, temb_act, num_frames, upsample_size)
        x = K.groupnorm(x, p["g_out"], p["be_out"], self.config.norm_num_groups, self.config.norm_eps, silu=True)
        # the 4-channel noise prediction stays fp32: the CFG combine (pipe:686-688) would amplify an fp16 rounding here
        # by up to 2 * guidance - 1, and the reference returns `sample`'s dtype (fp32 latents in its driver)
        return K.conv3x3(x, p["w_out"], p["b_out"], out_f32=True)                       # unet:1439-1443

    def _check_intrablock_residuals(self, feats, x_shape):
        """one tensor per down block, each [n, h, w, C] of the level where its block adds it, n dividing the batch; `x_shape`: the
        model-input tokens [batch, H, W, cin_pad].  ValueError naming the level otherwise (before anything is launched)."""
        if len(feats) != len(self.down_blocks):
            raise ValueError(f"down_intrablock_additional_residuals: {len(feats)} tensors for {len(self.down_blocks)} down blocks "
                             "(one per block)")
        batch, hh, ww = x_shape[0], x_shape[1], x_shape[2]
        for i, (blk, t) in enumerate(zip(self.down_blocks, feats)):
            if not getattr(blk, "has_cross_attention", False) and blk.downsamplers is not None:
                hh, ww = (hh + 1) // 2, (ww + 1) // 2          # (a block without cross-attention adds behind its down-sampler)
            want = (hh, ww, self.config.block_out_channels[i])
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or tuple(t.shape[1:]) != want or t.shape[0] < 1 or batch % t.shape[0]:
                got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"down_intrablock_additional_residuals: level {i} takes (n, height {want[0]}, width {want[1]}, "
                                 f"channels {want[2]}) with n dividing the batch {batch}, got tokens {got}")
            if getattr(blk, "has_cross_attention", False) and blk.downsamplers is not None:
                hh, ww = (hh + 1) // 2, (ww + 1) // 2

    def _embed_time(self, timesteps_f32, t_index=None):
        """Timesteps -> TimestepEmbedding (unet:1336-1343); one row per sample (the per-frame repeat of unet:1344
        is index arithmetic in the conv epilogue)."""
        self._sync_lora()
        t_emb = K.timestep_embedding(timesteps_f32, self.config.block_out_channels[0], t_index=t_index)
        return self.time_embedding(t_emb)

    def _project_image_embeds(self, added_cond_kwargs):
        self._sync_lora()
        if self.encoder_hid_proj is not None and self.config.encoder_hid_dim_type == "ip_image_proj":
            if added_cond_kwargs is None or "image_embeds" not in added_cond_kwargs:
                raise ValueError(
                    f"{self.__class__} has the config param `encoder_hid_dim_type` set to 'ip_image_proj' which "
                    "requires the keyword argument `image_embeds` to be passed in  `added_conditions`")
            return self.encoder_hid_proj(added_cond_kwargs.get("image_embeds"))          # unet:1351-1352
        return None

    def _expand_image_tokens(self, ctx_ip, rows):
        """the IP-Adapter's projected image tokens [n, Li, D], one set per sample, as one set per context row [rows, Li, D] with
        rows = n * F: row r reads sample r // F (the w = 0 gather of K.interp_rows).  Per-frame text contexts need it: the fused
        cross-attention indexes the image fragments with the text's context index and `_cross` uses one kv_group for both.
        None, or tokens that already have `rows` rows, pass through."""
        if ctx_ip is None or ctx_ip.shape[0] == rows:
            return ctx_ip
        if rows % ctx_ip.shape[0] != 0:
            raise ValueError(f"{ctx_ip.shape[0]} sets of image tokens do not divide {rows} text contexts")
        idx = torch.arange(ctx_ip.shape[0]).repeat_interleave(rows // ctx_ip.shape[0])
        return K.interp_rows(ctx_ip.contiguous(), idx, idx, torch.zeros(rows))

    def forward(self, sample, timestep, enable_cross_frame_attn: bool, encoder_hidden_states,
                timestep_cond=None, attention_mask=None, cross_attention_kwargs: Optional[Dict[str, Any]] = None,
                added_cond_kwargs: Optional[Dict[str, torch.Tensor]] = None,
                down_block_additional_residuals=None, mid_block_additional_residual=None,
                return_dict: bool = True, down_intrablock_additional_residuals=None):
        """unet:1289-1451.  sample (B, F, C, H, W) -> noise prediction (B, F, C, H, W) in sample's dtype.
        `encoder_hidden_states`: [B, L, D], one context per sample (the reference's `repeat_interleave(num_frames)`, unet:1355, is index
        arithmetic in the kernels) -- or [B * F, L, D], one context per frame in the order of the frames of `sample` (prompt travel:
        every cross-attention then runs with kv_group = 1); with an IP-Adapter its image tokens, one set per sample, are repeated per
        frame here.  A `ProjectedContext` made from either form is taken as it is.
        `down_intrablock_additional_residuals` (diffusers' UNet2DConditionModel argument, a T2I-Adapter's output): one NCHW tensor per
        down block, (n, C_i, h_i, w_i) with n = B * F or a divisor of it (see _fwd_tokens).
        `cross_attention_kwargs={"scale": s}`: the global LoRA scale of this call (lora.py).
        `cross_attention_kwargs={"cfg_shared_prefix": True}` (an addition; the reference ignores the dict on this path): the
        caller asserts that sample[B/2:] == sample[:B/2] and that all timesteps are equal -- the classifier-free-guidance
        batch of pipe:672-673 -- and the prompt-independent prefix of the network is computed once (see _fwd_tokens)."""
        if cross_attention_kwargs and cross_attention_kwargs.get("scale") is not None:
            # the LoRA scale of THIS call (diffusers' cross_attention_kwargs={"scale": s}): merged at s, the previous scale restored
            rest = {k: v for k, v in cross_attention_kwargs.items() if k != "scale"}
            prev = self.set_lora_scale(cross_attention_kwargs["scale"])
            try:
                return self.forward(sample, timestep, enable_cross_frame_attn, encoder_hidden_states, timestep_cond=timestep_cond,
                                    attention_mask=attention_mask, cross_attention_kwargs=rest, added_cond_kwargs=added_cond_kwargs,
                                    down_block_additional_residuals=down_block_additional_residuals,
                                    mid_block_additional_residual=mid_block_additional_residual, return_dict=return_dict,
                                    down_intrablock_additional_residuals=down_intrablock_additional_residuals)
            finally:
                self.set_lora_scale(prev)
        self._sync_lora()      # (a LoRA change since the last call: merge before any weight or pack is read)
        if attention_mask is not None:
            raise NotImplementedError("attention masks are never passed on the hot path (SURVEY 8b)")
        intra = down_intrablock_additional_residuals
        if intra is not None and sample.dim() == 5:      # the adapter's features: checked on the host, before anything is launched
            intra = list(intra)
            for i, t in enumerate(intra):
                if not isinstance(t, torch.Tensor) or t.dim() != 4:
                    raise ValueError(f"down_intrablock_additional_residuals: level {i} must be a (n, channels, height, width) tensor, got "
                                     f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            self._check_intrablock_residuals([t.permute(0, 2, 3, 1) for t in intra],
                                             (sample.shape[0] * sample.shape[1],) + tuple(sample.shape[3:]))
        if not sample.is_cuda:
            raise HipLibraryError(f"sample is on {sample.device}: the HIP path has no CPU fallback")
        if sample.dim() != 5:
            raise ValueError(f"sample must be (batch, frames, channels, height, width), got {tuple(sample.shape)}")
        b, num_frames, c, hh, ww = sample.shape
        # unet:1304-1311: sizes that do not halve exactly at every level forward the skip tensors' sizes to the up-samplers
        forward_upsample_size = any(s % (2 ** self.num_upsamplers) != 0 for s in (hh, ww))
        timesteps = timestep                                                              # unet:1319-1334
        if not torch.is_tensor(timesteps):
            timesteps = torch.tensor([timesteps], dtype=torch.float32, device=sample.device)
        elif timesteps.dim() == 0:
            timesteps = timesteps[None]
        timesteps = timesteps.to(device=sample.device, dtype=torch.float32).expand(b).contiguous()
        temb = self._embed_time(timesteps)
        if isinstance(encoder_hidden_states, ProjectedContext):     # K / V^T already projected (project_context)
            ctx_text, ctx_ip = encoder_hidden_states, encoder_hidden_states.ip
            if self.encoder_hid_proj is not None and ctx_ip is None:
                self._project_image_embeds(None)                                          # raises like unet:1347-1350
        else:
            ctx_text = _as_f16_matrix(encoder_hidden_states)
            ctx_ip = self._project_image_embeds(added_cond_kwargs)
            if ctx_text.dim() != 3 or ctx_text.shape[0] not in (b, b * num_frames):
                raise ValueError(f"encoder_hidden_states must be [B, L, D] or [B * F, L, D] with B = {b}, F = {num_frames}, got "
                                 f"{tuple(ctx_text.shape)}")
            if ctx_text.shape[0] == b * num_frames:      # one context per frame
                ctx_ip = self._expand_image_tokens(ctx_ip, ctx_text.shape[0])
        p = self.packed()
        x = K.nchw_to_tokens(sample.reshape(b * num_frames, c, hh, ww), p["cin_pad"])     # unet:1358
        cfg_shared = bool(cross_attention_kwargs and cross_attention_kwargs.get("cfg_shared_prefix", False))
        # ControlNet residuals (unet:1299-1300): NCHW (B * F, C, h, w) like the skip tensors -> tokens
        down_res = mid_res = None
        if down_block_additional_residuals is not None:
            down_res = [K.nchw_to_tokens(r) for r in down_block_additional_residuals]
        if mid_block_additional_residual is not None:
            mid_res = K.nchw_to_tokens(mid_block_additional_residual)
        if intra is not None:
            intra = [K.nchw_to_tokens(t) for t in intra]
        y = self._fwd_tokens(x, temb, enable_cross_frame_attn, ctx_text, ctx_ip, num_frames, cfg_shared=cfg_shared,
                             forward_upsample_size=forward_upsample_size, down_residuals=down_res, mid_residual=mid_res,
                             intrablock_residuals=intra)
        out_dt = sample.dtype if sample.dtype in (torch.float32, f16) else f16
        out = K.tokens_to_nchw(y, dtype=out_dt).reshape(b, num_frames, -1, hh, ww)        # unet:1446
        if not return_dict:
            return (out,)
        return UNet3DConditionOutput(sample=out)



# ---------------------------------------------------------------------------------------------------------
# Weight container standing in for diffusers `UNet2DConditionModel` (SD-1.5 layout), the *source* argument of
# `from_unet2d` (unet:883): same module tree / state-dict keys, no forward.
class _Transformer2DSource(I2VAdapterTransformer2DModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        for blk in self.transformer_blocks:
            del blk.i2v_adapter


class UNet2DConditionModel(PretrainedMixin, nn.Module):
    def __init__(self, sample_size=None, in_channels=4, out_channels=4,
                 down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D",
                                   "DownBlock2D"),
                 up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
                 block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, downsample_padding=1,
                 mid_block_scale_factor=1, act_fn="silu", norm_num_groups=32, norm_eps=1e-5,
                 cross_attention_dim=768, attention_head_dim=8, use_linear_projection=False):
        super().__init__()
        self.config = _Config(sample_size=sample_size, in_channels=in_channels, out_channels=out_channels,
                              down_block_types=tuple(down_block_types), up_block_types=tuple(up_block_types),
                              block_out_channels=tuple(block_out_channels), layers_per_block=layers_per_block,
                              downsample_padding=downsample_padding,
                              mid_block_scale_factor=mid_block_scale_factor, act_fn=act_fn,
                              norm_num_groups=norm_num_groups, norm_eps=norm_eps,
                              cross_attention_dim=cross_attention_dim, attention_head_dim=attention_head_dim,
                              use_linear_projection=use_linear_projection)
        heads = attention_head_dim
        temb = block_out_channels[0] * 4
        self.conv_in = nn.Conv2d(in_channels, block_out_channels[0], 3, padding=1)
        self.time_proj = Timesteps(block_out_channels[0], True, 0)
        self.time_embedding = TimestepEmbedding(block_out_channels[0], temb)

        def t2d(c):
            return _Transformer2DSource(heads, c // heads, in_channels=c, cross_attention_dim=cross_attention_dim,
                                        norm_num_groups=norm_num_groups,
                                        use_linear_projection=use_linear_projection)

        def res(cin, cout):
            return ResnetBlock2D(cin, cout, temb_channels=temb, eps=norm_eps, groups=norm_num_groups)

        self.down_blocks = nn.ModuleList()
        oc = block_out_channels[0]
        for i, t in enumerate(down_block_types):
            ic, oc = oc, block_out_channels[i]
            blk = nn.Module()
            blk.resnets = nn.ModuleList([res(ic if j == 0 else oc, oc) for j in range(layers_per_block)])
            if "CrossAttn" in t:
                blk.attentions = nn.ModuleList([t2d(oc) for _ in range(layers_per_block)])
            blk.downsamplers = (nn.ModuleList([Downsample2D(oc, padding=downsample_padding)])
                                if i != len(block_out_channels) - 1 else None)
            self.down_blocks.append(blk)
        c = block_out_channels[-1]
        self.mid_block = nn.Module()
        self.mid_block.resnets = nn.ModuleList([res(c, c), res(c, c)])
        self.mid_block.attentions = nn.ModuleList([t2d(c)])
        self.up_blocks = nn.ModuleList()
        rev = list(reversed(block_out_channels))
        oc = rev[0]
        for i, t in enumerate(up_block_types):
            prev, oc = oc, rev[i]
            ic = rev[min(i + 1, len(rev) - 1)]
            blk = nn.Module()
            n = layers_per_block + 1
            blk.resnets = nn.ModuleList([
                res((prev if j == 0 else oc) + (ic if j == n - 1 else oc), oc) for j in range(n)])
            if "CrossAttn" in t:
                blk.attentions = nn.ModuleList([t2d(oc) for _ in range(n)])
            blk.upsamplers = nn.ModuleList([Upsample2D(oc)]) if i != len(rev) - 1 else None
            self.up_blocks.append(blk)
        self.conv_norm_out = nn.GroupNorm(norm_num_groups, block_out_channels[0], eps=norm_eps)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(block_out_channels[0], out_channels, 3, padding=1)
