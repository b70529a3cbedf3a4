"""ControlNetModel on the HIP kernels: diffusers 0.24 `ControlNetModel` in the SD-1.5 layout (same module tree, state-dict keys
and config keys: `control_v11*_sd15_*/diffusion_pytorch_model.safetensors` + `config.json` load by key through PretrainedMixin).

A ControlNet is the UNet's encoder half without motion modules and without the adapter: ResnetBlock2D, the spatial transformer in
its adapter-less form (`I2VAdapterTransformer2DModel(with_adapter=False)`) and Downsample2D, plus an eight-convolution embedding of
the control image and thirteen 1x1 "zero" convolutions.  It is a 2-D model: it runs per frame, the frames of a clip are a batch.
Its 12 + 1 outputs are the `down_block_additional_residuals` / `mid_block_additional_residual` of the UNet (unet:1299-1300).

Activations are token-major fp16 ([N, H, W, C]) from the edge to the edge; every launch is a library launch, nothing here computes
with torch ops and nothing falls back to the CPU.  The ControlNet always runs the default residual stream.
"""
from typing import Optional, Tuple, Union

import torch
from torch import nn

from . import kernels as K
from ._lib import HipLibraryError
from .blocks import (Attention, Downsample2D, HipModule, ProjectedTemb, ResnetBlock2D, SampleProjectionMixin, TimestepEmbedding,
                     Timesteps, _as_f16_matrix, pack_conv3x3, set_precise_stream, w16)
from .checkpoint import PretrainedMixin
from .i2v_adapter import I2VAdapterTransformer2DModel
from .unet_motion_cross_frame_attn import _Config

f16 = torch.float16


class ControlNetOutput:
    """diffusers' ControlNetOutput: `down_block_res_samples` (a tuple, one per skip tensor of the UNet) and `mid_block_res_sample`."""

    def __init__(self, down_block_res_samples, mid_block_res_sample):
        self.down_block_res_samples, self.mid_block_res_sample = down_block_res_samples, mid_block_res_sample

    def __iter__(self):
        return iter((self.down_block_res_samples, self.mid_block_res_sample))


class ControlNetConditioningEmbedding(HipModule):
    """diffusers' ControlNetConditioningEmbedding: conv_in, blocks.0 .. 2 n - 3 (alternating 3x3 / 3x3 stride 2), conv_out, SiLU after
    every convolution but the last.  (N, 3, 8 H, 8 W) -> tokens [N, H, W, C0]."""

    def __init__(self, conditioning_embedding_channels: int, conditioning_channels: int = 3,
                 block_out_channels: Tuple[int, ...] = (16, 32, 96, 256)):
        super().__init__()
        self.conditioning_channels = conditioning_channels
        self.conv_in = nn.Conv2d(conditioning_channels, block_out_channels[0], kernel_size=3, padding=1)
        blocks = []
        for i in range(len(block_out_channels) - 1):
            cin, cout = block_out_channels[i], block_out_channels[i + 1]
            blocks.append(nn.Conv2d(cin, cin, kernel_size=3, padding=1))
            blocks.append(nn.Conv2d(cin, cout, kernel_size=3, padding=1, stride=2))
        self.blocks = nn.ModuleList(blocks)
        self.conv_out = nn.Conv2d(block_out_channels[-1], conditioning_embedding_channels, kernel_size=3, padding=1)
        nn.init.zeros_(self.conv_out.weight)
        nn.init.zeros_(self.conv_out.bias)

    def _pack(self):
        cin_pad = K.pad8(self.conditioning_channels)
        convs = [(pack_conv3x3(self.conv_in.weight, cin_pad=cin_pad), w16(self.conv_in.bias), 1)]
        for b in self.blocks:
            convs.append((pack_conv3x3(b.weight), w16(b.bias), b.stride[0]))
        convs.append((pack_conv3x3(self.conv_out.weight), w16(self.conv_out.bias), 1))
        return dict(convs=convs, cin_pad=cin_pad)

    def _fwd(self, cond_nchw):
        p = self.packed()
        if cond_nchw.dim() != 4 or cond_nchw.shape[1] != self.conditioning_channels:
            raise ValueError(f"controlnet_cond must be (N, {self.conditioning_channels}, height, width), got {tuple(cond_nchw.shape)}")
        x = K.nchw_to_tokens(cond_nchw, p["cin_pad"])
        last = len(p["convs"]) - 1
        for i, (w, b, stride) in enumerate(p["convs"]):
            x = K.conv3x3(x, w, b, stride=stride)
            if i != last:
                x = K.silu(x)
        return x

    def forward(self, conditioning):
        return K.tokens_to_nchw(self._fwd(conditioning), dtype=conditioning.dtype if conditioning.dtype in (torch.float32, f16) else f16)


def _t2d(channels, heads, cross_attention_dim, groups, use_linear_projection):
    return I2VAdapterTransformer2DModel(heads, channels // heads, in_channels=channels, cross_attention_dim=cross_attention_dim,
                                        norm_num_groups=groups, use_linear_projection=use_linear_projection, with_adapter=False)


class CrossAttnDownBlock2D(nn.Module):
    """diffusers' CrossAttnDownBlock2D: [resnet -> spatial transformer] x layers, down-sampler: the UNet's
    CrossFrameAttnDownBlockMotion minus the motion modules and the adapter."""

    def __init__(self, in_channels, out_channels, temb_channels, num_layers, resnet_eps, resnet_groups, num_attention_heads,
                 cross_attention_dim, downsample_padding, add_downsample, use_linear_projection):
        super().__init__()
        self.has_cross_attention = True
        self.resnets = nn.ModuleList([ResnetBlock2D(in_channels if i == 0 else out_channels, out_channels, temb_channels=temb_channels,
                                                    eps=resnet_eps, groups=resnet_groups) for i in range(num_layers)])
        self.attentions = nn.ModuleList([_t2d(out_channels, num_attention_heads, cross_attention_dim, resnet_groups, use_linear_projection)
                                         for _ in range(num_layers)])
        self.downsamplers = (nn.ModuleList([Downsample2D(out_channels, use_conv=True, out_channels=out_channels,
                                                         padding=downsample_padding, name="op")]) if add_downsample else None)

    def _fwd(self, x, temb_act, ctx):
        states = ()
        for resnet, attn in zip(self.resnets, self.attentions):
            x = resnet._fwd(x, temb_act)
            x = attn._fwd(x, False, None, ctx, None)
            states += (x,)
        if self.downsamplers is not None:
            for d in self.downsamplers:
                x = d._fwd(x)
            states += (x,)
        return x, states


class DownBlock2D(nn.Module):
    """diffusers' DownBlock2D: resnets, down-sampler."""

    def __init__(self, in_channels, out_channels, temb_channels, num_layers, resnet_eps, resnet_groups, downsample_padding,
                 add_downsample):
        super().__init__()
        self.has_cross_attention = False
        self.resnets = nn.ModuleList([ResnetBlock2D(in_channels if i == 0 else out_channels, out_channels, temb_channels=temb_channels,
                                                    eps=resnet_eps, groups=resnet_groups) for i in range(num_layers)])
        self.downsamplers = (nn.ModuleList([Downsample2D(out_channels, use_conv=True, out_channels=out_channels,
                                                         padding=downsample_padding, name="op")]) if add_downsample else None)

    def _fwd(self, x, temb_act, ctx):
        states = ()
        for resnet in self.resnets:
            x = resnet._fwd(x, temb_act)
            states += (x,)
        if self.downsamplers is not None:
            for d in self.downsamplers:
                x = d._fwd(x)
            states += (x,)
        return x, states


class UNetMidBlock2DCrossAttn(nn.Module):
    """diffusers' UNetMidBlock2DCrossAttn: resnet, [spatial transformer, resnet]."""

    def __init__(self, in_channels, temb_channels, resnet_eps, resnet_groups, num_attention_heads, cross_attention_dim,
                 output_scale_factor, use_linear_projection):
        super().__init__()
        self.has_cross_attention = True

        def res():
            return ResnetBlock2D(in_channels, in_channels, temb_channels=temb_channels, eps=resnet_eps, groups=resnet_groups,
                                 output_scale_factor=output_scale_factor)

        self.attentions = nn.ModuleList([_t2d(in_channels, num_attention_heads, cross_attention_dim, resnet_groups, use_linear_projection)])
        self.resnets = nn.ModuleList([res(), res()])

    def _fwd(self, x, temb_act, ctx):
        x = self.resnets[0]._fwd(x, temb_act)
        for attn, resnet in zip(self.attentions, self.resnets[1:]):
            x = attn._fwd(x, False, None, ctx, None)
            x = resnet._fwd(x, temb_act)
        return x


def _zero_conv(channels):
    conv = nn.Conv2d(channels, channels, kernel_size=1)
    nn.init.zeros_(conv.weight)
    nn.init.zeros_(conv.bias)
    return conv


class ControlNetModel(SampleProjectionMixin, PretrainedMixin, HipModule):
    """diffusers 0.24 ControlNetModel (SD-1.5 layout)."""

    def __init__(self, in_channels: int = 4, conditioning_channels: int = 3, flip_sin_to_cos: bool = True, freq_shift: int = 0,
                 down_block_types: Tuple[str, ...] = ("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D",
                                                      "DownBlock2D"),
                 only_cross_attention: Union[bool, Tuple[bool, ...]] = False,
                 block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280), layers_per_block: int = 2,
                 downsample_padding: int = 1, mid_block_scale_factor: float = 1, act_fn: str = "silu",
                 norm_num_groups: Optional[int] = 32, norm_eps: float = 1e-5, cross_attention_dim: int = 768,
                 transformer_layers_per_block: Union[int, Tuple[int, ...]] = 1, encoder_hid_dim: Optional[int] = None,
                 encoder_hid_dim_type: Optional[str] = None, attention_head_dim: Union[int, Tuple[int, ...]] = 8,
                 num_attention_heads: Optional[Union[int, Tuple[int, ...]]] = None, use_linear_projection: bool = False,
                 class_embed_type: Optional[str] = None, addition_embed_type: Optional[str] = None,
                 addition_time_embed_dim: Optional[int] = None, num_class_embeds: Optional[int] = None,
                 upcast_attention: bool = False, resnet_time_scale_shift: str = "default",
                 projection_class_embeddings_input_dim: Optional[int] = None, controlnet_conditioning_channel_order: str = "rgb",
                 conditioning_embedding_out_channels: Optional[Tuple[int, ...]] = (16, 32, 96, 256),
                 global_pool_conditions: bool = False, addition_embed_type_num_heads: int = 64):
        super().__init__()
        self.config = _Config(
            in_channels=in_channels, conditioning_channels=conditioning_channels, flip_sin_to_cos=flip_sin_to_cos, freq_shift=freq_shift,
            down_block_types=tuple(down_block_types),
            only_cross_attention=only_cross_attention if isinstance(only_cross_attention, bool) else tuple(only_cross_attention),
            block_out_channels=tuple(block_out_channels), layers_per_block=layers_per_block, downsample_padding=downsample_padding,
            mid_block_scale_factor=mid_block_scale_factor, act_fn=act_fn, norm_num_groups=norm_num_groups, norm_eps=norm_eps,
            cross_attention_dim=cross_attention_dim, transformer_layers_per_block=transformer_layers_per_block,
            encoder_hid_dim=encoder_hid_dim, encoder_hid_dim_type=encoder_hid_dim_type,
            attention_head_dim=attention_head_dim if isinstance(attention_head_dim, int) else tuple(attention_head_dim),
            num_attention_heads=num_attention_heads if num_attention_heads is None or isinstance(num_attention_heads, int)
            else tuple(num_attention_heads),
            use_linear_projection=use_linear_projection, class_embed_type=class_embed_type, addition_embed_type=addition_embed_type,
            addition_time_embed_dim=addition_time_embed_dim, num_class_embeds=num_class_embeds, upcast_attention=upcast_attention,
            resnet_time_scale_shift=resnet_time_scale_shift, projection_class_embeddings_input_dim=projection_class_embeddings_input_dim,
            controlnet_conditioning_channel_order=controlnet_conditioning_channel_order,
            conditioning_embedding_out_channels=tuple(conditioning_embedding_out_channels), global_pool_conditions=global_pool_conditions,
            addition_embed_type_num_heads=addition_embed_type_num_heads)
        for key, val in (("class_embed_type", class_embed_type), ("num_class_embeds", num_class_embeds),
                         ("addition_embed_type", addition_embed_type), ("encoder_hid_dim_type", encoder_hid_dim_type),
                         ("encoder_hid_dim", encoder_hid_dim)):
            if val is not None:
                raise NotImplementedError(f"{key}={val!r}: class / addition / encoder-hidden embeddings are not implemented "
                                          "(SD-1.5 ControlNets have none)")
        if global_pool_conditions:
            raise NotImplementedError("global_pool_conditions=True is not implemented")
        if controlnet_conditioning_channel_order != "rgb":
            raise NotImplementedError(f"controlnet_conditioning_channel_order={controlnet_conditioning_channel_order!r}: only 'rgb' is "
                                      "implemented")
        if (only_cross_attention if isinstance(only_cross_attention, bool) else any(only_cross_attention)):
            raise NotImplementedError("only_cross_attention=True is not implemented")
        if act_fn not in ("silu", "swish"):
            raise NotImplementedError(f"act_fn={act_fn!r}: only 'silu' is implemented")
        if resnet_time_scale_shift != "default":
            raise NotImplementedError(f"resnet_time_scale_shift={resnet_time_scale_shift!r}: only 'default' is implemented")
        tl = transformer_layers_per_block
        if (tl if isinstance(tl, int) else max(tl)) != 1 or (not isinstance(tl, int) and min(tl) != 1):
            raise NotImplementedError(f"transformer_layers_per_block={tl!r}: only 1 is implemented")
        if norm_num_groups is None:
            raise NotImplementedError("norm_num_groups=None is not implemented")
        if len(block_out_channels) != len(down_block_types):
            raise ValueError(f"Must provide the same number of `block_out_channels` as `down_block_types`. `block_out_channels`: "
                             f"{block_out_channels}. `down_block_types`: {down_block_types}.")
        # as in SD-1.5's UNet config, `attention_head_dim` is the NUMBER of heads (diffusers: num_attention_heads or attention_head_dim)
        heads = num_attention_heads if num_attention_heads is not None else attention_head_dim
        if isinstance(heads, int):
            heads = (heads,) * len(down_block_types)
        if len(heads) != len(down_block_types):
            raise ValueError(f"Must provide the same number of `num_attention_heads` as `down_block_types`. `num_attention_heads`: "
                             f"{heads}. `down_block_types`: {down_block_types}.")

        c0 = block_out_channels[0]
        self.conv_in = nn.Conv2d(in_channels, c0, kernel_size=3, padding=1)
        time_embed_dim = c0 * 4
        self.time_proj = Timesteps(c0, flip_sin_to_cos, freq_shift)
        self.time_embedding = TimestepEmbedding(c0, time_embed_dim, act_fn=act_fn)
        self.controlnet_cond_embedding = ControlNetConditioningEmbedding(c0, conditioning_channels, tuple(conditioning_embedding_out_channels))
        self.down_blocks = nn.ModuleList([])
        self.controlnet_down_blocks = nn.ModuleList([_zero_conv(c0)])
        out_ch = c0
        for i, t in enumerate(down_block_types):
            in_ch, out_ch = out_ch, block_out_channels[i]
            is_final = i == len(block_out_channels) - 1
            if t == "CrossAttnDownBlock2D":
                blk = CrossAttnDownBlock2D(in_ch, out_ch, time_embed_dim, layers_per_block, norm_eps, norm_num_groups, heads[i],
                                           cross_attention_dim, downsample_padding, not is_final, use_linear_projection)
            elif t == "DownBlock2D":
                blk = DownBlock2D(in_ch, out_ch, time_embed_dim, layers_per_block, norm_eps, norm_num_groups, downsample_padding,
                                  not is_final)
            else:
                raise ValueError(f"{t} does not exist.")
            self.down_blocks.append(blk)
            for _ in range(layers_per_block + (0 if is_final else 1)):
                self.controlnet_down_blocks.append(_zero_conv(out_ch))
        self.controlnet_mid_block = _zero_conv(block_out_channels[-1])
        self.mid_block = UNetMidBlock2DCrossAttn(block_out_channels[-1], time_embed_dim, norm_eps, norm_num_groups, heads[-1],
                                                 cross_attention_dim, mid_block_scale_factor, use_linear_projection)

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    @property
    def device(self):
        return next(self.parameters()).device

    # ------------------------------------------------------------------ weight assembly
    @classmethod
    def from_unet(cls, unet, controlnet_conditioning_channel_order: str = "rgb",
                  conditioning_embedding_out_channels: Optional[Tuple[int, ...]] = (16, 32, 96, 256), load_weights_from_unet: bool = True,
                  conditioning_channels: int = 3):
        """diffusers' ControlNetModel.from_unet for a `UNetMotionCrossFrameAttnModel` or the `UNet2DConditionModel` container: the
        encoder's geometry from the UNet's config; conv_in, time_embedding and the down / mid blocks' resnets, attentions and
        down-samplers copied (the UNet's motion modules and adapter have no counterpart here).  The zero convolutions and the
        embedding's conv_out stay zero: the new ControlNet contributes nothing until it is trained."""
        cfg = unet.config
        heads = cfg.get("num_attention_heads") or cfg.get("attention_head_dim")
        model = cls(in_channels=cfg["in_channels"],
                    down_block_types=tuple("CrossAttnDownBlock2D" if "Attn" in t else "DownBlock2D" for t in cfg["down_block_types"]),
                    block_out_channels=tuple(cfg["block_out_channels"]), layers_per_block=cfg["layers_per_block"],
                    downsample_padding=cfg.get("downsample_padding", 1), mid_block_scale_factor=cfg.get("mid_block_scale_factor", 1),
                    act_fn=cfg.get("act_fn", "silu"), norm_num_groups=cfg["norm_num_groups"], norm_eps=cfg.get("norm_eps", 1e-5),
                    cross_attention_dim=cfg["cross_attention_dim"], attention_head_dim=heads,
                    use_linear_projection=cfg.get("use_linear_projection", False),
                    controlnet_conditioning_channel_order=controlnet_conditioning_channel_order,
                    conditioning_embedding_out_channels=conditioning_embedding_out_channels, conditioning_channels=conditioning_channels)
        if load_weights_from_unet:
            def plain(sd):                      # (the UNet's transformer blocks carry the adapter's Attention beside attn1 / attn2)
                return {k: v for k, v in sd.items() if ".i2v_adapter." not in k}

            model.conv_in.load_state_dict(unet.conv_in.state_dict())
            model.time_embedding.load_state_dict(unet.time_embedding.state_dict())
            for mine, theirs in zip(model.down_blocks, unet.down_blocks):
                mine.resnets.load_state_dict(theirs.resnets.state_dict())
                if mine.has_cross_attention:
                    mine.attentions.load_state_dict(plain(theirs.attentions.state_dict()))
                if mine.downsamplers is not None:
                    mine.downsamplers.load_state_dict(theirs.downsamplers.state_dict())
            model.mid_block.resnets.load_state_dict(unet.mid_block.resnets.state_dict())
            model.mid_block.attentions.load_state_dict(plain(unet.mid_block.attentions.state_dict()))
        p = next(unet.parameters())
        return model.to(device=p.device, dtype=p.dtype)

    # ------------------------------------------------------------------ packs
    def _zero_convs(self):
        return list(self.controlnet_down_blocks) + [self.controlnet_mid_block]

    def _pack(self):
        cin_pad = K.pad8(self.config.in_channels)
        return dict(w_in=pack_conv3x3(self.conv_in.weight, cin_pad=cin_pad), b_in=w16(self.conv_in.bias), cin_pad=cin_pad,
                    zero=[(w16(c.weight.reshape(c.out_channels, c.in_channels)), w16(c.bias)) for c in self._zero_convs()])

    def packed(self):
        # only the model's own leaf parameters feed this pack (children pack themselves)
        leaves = [self.conv_in.weight, self.conv_in.bias] + [q for c in self._zero_convs() for q in (c.weight, c.bias)]
        key = tuple((q.data_ptr(), q._version, q.dtype) for q in leaves)
        if self._packed is None or key != self._packed_key:
            for q in leaves:
                if not q.is_cuda:
                    raise HipLibraryError(f"{type(self).__name__} has parameters on {q.device}: the HIP path has no CPU fallback")
            with torch.no_grad():
                self._packed = self._pack()
            self._packed_key = key
        return self._packed

    def weight_signature(self):
        """identity and versions of every parameter: what a captured step that launches this model was captured against"""
        return tuple((q.data_ptr(), q._version) for q in self.parameters())

    # ------------------------------------------------------------------ once per sample
    def embed_condition(self, controlnet_cond):
        """controlnet_cond (N, 3, 8 H, 8 W) in [0, 1] -> tokens [N, H, W, C0]: the eight-convolution embedding.  It depends on the control
        images only: once per sample, not per step."""
        if not controlnet_cond.is_cuda:
            raise HipLibraryError(f"controlnet_cond is on {controlnet_cond.device}: the HIP path has no CPU fallback")
        return self.controlnet_cond_embedding._fwd(controlnet_cond)

    def _cross_attention_layers(self):
        return [m for name, m in self.named_modules() if isinstance(m, Attention) and name.endswith("attn2")]

    def _embed_time(self, timesteps_f32):
        return self.time_embedding(K.timestep_embedding(timesteps_f32, self.config.block_out_channels[0]))

    # ------------------------------------------------------------------ forward
    def _fwd_tokens(self, x, temb_proj, ctx, cond_tokens, out_scale: float = 1.0):
        """x: model-input tokens [N, H, W, cin_pad] fp16; temb_proj [B or 1, sum Cout] (project_time_table rows); ctx [B, Lt, D] or a
        ProjectedContext of THIS model (N % B == 0: the frames of a clip share a prompt; B = N with prompt travel, one context per frame
        in the order of the token rows); cond_tokens [N, H, W, C0]
        (embed_condition).  Returns (12 down tensors, mid tensor), token-major fp16, each times out_scale."""
        p = self.packed()
        _, _, slices = self._temb_pack()
        temb_act = ProjectedTemb(temb_proj, slices)
        prev = set_precise_stream(False)            # a ControlNet's outputs are residuals, not the stream: one fp16 tensor each
        try:
            x = K.conv3x3(x, p["w_in"], p["b_in"], residual=cond_tokens)            # conv_in(sample) + controlnet_cond_embedding(cond)
            res = (x,)
            for blk in self.down_blocks:
                x, r = blk._fwd(x, temb_act, ctx)
                res += r
            x = self.mid_block._fwd(x, temb_act, ctx)
        finally:
            set_precise_stream(prev)
        outs = []
        for t, (w, b) in zip(res + (x,), p["zero"]):                                 # the 13 1x1 convolutions as GEMMs
            n, hh, ww, c = t.shape
            outs.append(K.gemm(t.view(-1, c), w, b, out_scale=float(out_scale)).view(n, hh, ww, -1))
        return tuple(outs[:-1]), outs[-1]

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale: float = 1.0,
                class_labels=None, timestep_cond=None, attention_mask=None, added_cond_kwargs=None, cross_attention_kwargs=None,
                guess_mode: bool = False, return_dict: bool = True):
        """sample (B, F, C, H, W) or (N, C, H, W); timestep a number, a scalar or [B]; encoder_hidden_states [B, L, D] with N % B == 0;
        controlnet_cond (N, 3, 8 H, 8 W) in [0, 1].  Returns NCHW tensors (N, C_i, h_i, w_i) in sample's dtype."""
        down, mid, dt = self._forward_checked(sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale, class_labels,
                                              timestep_cond, attention_mask, added_cond_kwargs, guess_mode)
        down = tuple(K.tokens_to_nchw(t, dtype=dt) for t in down)
        mid = K.tokens_to_nchw(mid, dtype=dt)
        if not return_dict:
            return down, mid
        return ControlNetOutput(down_block_res_samples=down, mid_block_res_sample=mid)

    def _forward_checked(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale, class_labels, timestep_cond,
                         attention_mask, added_cond_kwargs, guess_mode):
        """`forward`'s argument checks and its launches up to the token-major outputs: (12 down tensors, mid tensor, the dtype `forward`
        returns).  MultiControlNetModel runs every net through here."""
        if guess_mode:
            raise NotImplementedError("guess_mode=True is not implemented")
        if attention_mask is not None:
            raise NotImplementedError("attention masks are never passed on the hot path (SURVEY 8b)")
        if class_labels is not None or timestep_cond is not None or added_cond_kwargs is not None:
            raise NotImplementedError("class_labels / timestep_cond / added_cond_kwargs: SD-1.5 ControlNets take none")
        if not sample.is_cuda:
            raise HipLibraryError(f"sample is on {sample.device}: the HIP path has no CPU fallback")
        if sample.dim() == 5:
            sample = sample.reshape((-1,) + tuple(sample.shape[2:]))
        if sample.dim() != 4:
            raise ValueError(f"sample must be (batch, frames, channels, height, width) or (images, channels, height, width), got "
                             f"{tuple(sample.shape)}")
        n, c, hh, ww = sample.shape
        ctx = _as_f16_matrix(encoder_hidden_states)
        b = ctx.shape[0]
        if n % b != 0:
            raise ValueError(f"context batch {b} does not divide the {n} images")
        if tuple(controlnet_cond.shape) != (n, self.config.conditioning_channels, 8 * hh, 8 * ww):
            raise ValueError(f"controlnet_cond must be {(n, self.config.conditioning_channels, 8 * hh, 8 * ww)}, got "
                             f"{tuple(controlnet_cond.shape)}")
        timesteps = timestep
        if not torch.is_tensor(timesteps):
            timesteps = torch.tensor([timesteps], dtype=torch.float32, device=sample.device)
        elif timesteps.dim() == 0:
            timesteps = timesteps[None]
        timesteps = timesteps.to(device=sample.device, dtype=torch.float32).expand(b).contiguous()
        p = self.packed()
        x = K.nchw_to_tokens(sample, p["cin_pad"])
        down, mid = self._fwd_tokens(x, self.project_time_table(timesteps), ctx, self.embed_condition(controlnet_cond),
                                     out_scale=conditioning_scale)
        return down, mid, sample.dtype if sample.dtype in (torch.float32, f16) else f16


class MultiControlNetModel(nn.Module):
    """diffusers' MultiControlNetModel: 1 .. I2V_ADD_RES_NETS_MAX ControlNetModels in `.nets` whose outputs are summed.  The nets may
    differ in their conditioning channels (a 1-channel edge net beside a 3-channel pose net); they serve one UNet, so their outputs
    have one geometry.  The pipeline takes it as `controlnet=` and then takes one list entry per net for `control_image` (and a float
    or a list for the scale and the window); its captured step runs the nets one after the other and adds all their residuals in one
    launch (K.add_multi_residuals)."""

    def __init__(self, controlnets):
        super().__init__()
        if not isinstance(controlnets, (list, tuple, nn.ModuleList)):
            raise TypeError(f"MultiControlNetModel takes a list of ControlNetModels, got {type(controlnets)}")
        nets = list(controlnets)
        if not 1 <= len(nets) <= K._lib.I2V_ADD_RES_NETS_MAX:
            raise ValueError(f"MultiControlNetModel holds 1 .. {K._lib.I2V_ADD_RES_NETS_MAX} ControlNets (the residuals of all of them are "
                             f"added in one launch), got {len(nets)}")
        for i, net in enumerate(nets):
            if not isinstance(net, ControlNetModel):
                raise TypeError(f"MultiControlNetModel: entry {i} is a {type(net).__name__}, not a ControlNetModel")
        self.nets = nn.ModuleList(nets)

    def __len__(self):
        return len(self.nets)

    @property
    def dtype(self):
        return self.nets[0].dtype

    @property
    def device(self):
        return self.nets[0].device

    def weight_signature(self):
        """the nets' signatures, concatenated: what a captured step that launches all of them was captured against"""
        return tuple(e for net in self.nets for e in net.weight_signature())

    # ------------------------------------------------------------------ diffusers' folder names: dir, dir_1, dir_2, ...
    def save_pretrained(self, save_directory: str, **kwargs):
        for i, net in enumerate(self.nets):
            net.save_pretrained(save_directory if i == 0 else f"{save_directory}_{i}", **kwargs)

    @classmethod
    def from_pretrained(cls, pretrained_model_path: str, **kwargs):
        import os
        nets, path = [], pretrained_model_path
        while os.path.isdir(path):
            nets.append(ControlNetModel.from_pretrained(path, **kwargs))
            path = f"{pretrained_model_path}_{len(nets)}"
        if not nets:
            raise ValueError(f"No ControlNets found under {os.path.dirname(pretrained_model_path)}. Expected at least "
                             f"{pretrained_model_path}.")
        return cls(nets)

    def _per_net(self, value, name):
        if isinstance(value, (list, tuple)):
            if len(value) != len(self.nets):
                raise ValueError(f"`{name}` holds {len(value)} entries for {len(self.nets)} ControlNets")
            return list(value)
        return [value] * len(self.nets)

    def forward(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale, class_labels=None,
                timestep_cond=None, attention_mask=None, added_cond_kwargs=None, cross_attention_kwargs=None,
                guess_mode: bool = False, return_dict: bool = True):
        """diffusers' MultiControlNetModel.forward: `controlnet_cond` and `conditioning_scale` are lists with one entry per net (a
        float is taken for all nets); the other arguments are ControlNetModel.forward's and are checked by every net.  Each net runs
        unscaled; the scaled outputs are summed in fp32 in net order and rounded once (K.add_multi_residuals onto zeros).  Returns the
        summed (down_block_res_samples, mid_block_res_sample), NCHW in sample's dtype."""
        if not isinstance(controlnet_cond, (list, tuple)):
            raise ValueError(f"`controlnet_cond` is a list with one entry per ControlNet, got {type(controlnet_cond)}")
        conds = self._per_net(controlnet_cond, "controlnet_cond")
        scales = [float(s) for s in self._per_net(conditioning_scale, "conditioning_scale")]
        sets, dt = [], None
        for net, cond in zip(self.nets, conds):
            down, mid, dt = net._forward_checked(sample, timestep, encoder_hidden_states, cond, 1.0, class_labels, timestep_cond,
                                                 attention_mask, added_cond_kwargs, guess_mode)
            sets.append(list(down) + [mid])
        table = torch.tensor(scales, dtype=torch.float32, device=sets[0][0].device).view(len(scales), 1)
        summed = K.add_multi_residuals([torch.zeros_like(t) for t in sets[0]], sets, scale=(table, None))
        outs = [K.tokens_to_nchw(t, dtype=dt) for t in summed]
        down, mid = tuple(outs[:-1]), outs[-1]
        if not return_dict:
            return down, mid
        return ControlNetOutput(down_block_res_samples=down, mid_block_res_sample=mid)


def controlnet_keep_table(num_steps: int, conditioning_scale: float = 1.0, control_guidance_start: float = 0.0,
                          control_guidance_end: float = 1.0):
    """diffusers' `controlnet_keep` times the conditioning scale, one value per executed step:
    scale[i] = conditioning_scale * (0 if i / n < start or (i + 1) / n > end else 1)."""
    if not (0.0 <= control_guidance_start < control_guidance_end <= 1.0):
        raise ValueError(f"control guidance needs 0 <= start < end <= 1, got start {control_guidance_start}, end {control_guidance_end}")
    if num_steps < 1:
        raise ValueError(f"num_steps must be positive, got {num_steps}")
    n = num_steps
    return [float(conditioning_scale) * (0.0 if (i / n < control_guidance_start or (i + 1) / n > control_guidance_end) else 1.0)
            for i in range(n)]
