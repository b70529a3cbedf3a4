"""CLIP image encoder on the HIP kernels: what `encode_image` (pipe:323-345) calls to turn the IP-Adapter's image prompt into the
`[B, 1024]` `image_embeds` of the UNet's decoupled cross-attention.

Host mirror of transformers' `CLIPVisionModelWithProjection` with the checkpoint's state-dict keys (IP-Adapter `models/image_encoder`,
OpenCLIP ViT-H/14: `vision_model.embeddings.{class_embedding, patch_embedding.weight, position_embedding.weight}`,
`vision_model.pre_layrnorm.*` -- the upstream spelling --, `vision_model.encoder.layers.{i}.{layer_norm1,layer_norm2,self_attn.{q,k,v,out}_proj,
mlp.{fc1,fc2}}.*`, `vision_model.post_layernorm.*`, `visual_projection.weight`), so an `image_encoder/` folder loads by key.  The forward is
library launches only, no torch ops on the data:

    patchify (i2v_clip_patchify_f16: the im2col of the stride-14 convolution, K padded 588 -> 592) -> patch GEMM without bias
    -> class token + positions (i2v_clip_vision_embed_f16) -> pre_layrnorm
    -> per layer, on the modules and helpers of clip_text.py: LN1 folded into ONE q|k|v GEMM -> bidirectional attention
       (i2v_clip_vision_attention_f16: 257 tokens, head_dim 80, q / k / v read in place) -> out_proj + residual -> LN2 folded into fc1
       with the erf-GELU epilogue ("quick_gelu": i2v_quick_gelu_f16) -> fc2 + residual
    -> post_layernorm on the class rows, read in place -> visual_projection GEMM

Not per-step work: an image is encoded once per sample.  Resize, crop and normalisation stay in transformers'
`CLIPImageProcessor` on the host, as tokenisation does.  IP-Adapter Plus reads `hidden_states[-2]` of this tower (blocks.Resampler, DESIGN
4.13).  Out of scope: `CLIPVisionModel` without projection, 336-px towers (577 tokens), training through the tower.
"""
from typing import Optional

import torch
from torch import nn

from . import kernels as K
from ._lib import HipLibraryError
from .blocks import HipModule, w16
from .checkpoint import PretrainedMixin
from .clip_text import CLIPEncoder, _Config, encoder_layer, pack_layers

f16 = torch.float16
HEAD_DIMS, MAX_TOKENS = (64, 80), 288          # the envelope of i2v_clip_vision_attention_f16
PREFIX = "vision_model."


class CLIPVisionModelOutput:
    """transformers' `CLIPVisionModelOutput` as far as the pipeline reads it: attribute access, and integer indexing over the fields
    that are not None (`out[0]` the image embeds, `out[1]` the last hidden state, `out[-1]` the hidden-states tuple when requested)."""

    def __init__(self, image_embeds, last_hidden_state, hidden_states=None):
        self.image_embeds, self.last_hidden_state, self.hidden_states = image_embeds, last_hidden_state, hidden_states

    def to_tuple(self):
        return tuple(v for v in (self.image_embeds, self.last_hidden_state, self.hidden_states) if v is not None)

    def __getitem__(self, i):
        return self.to_tuple()[i]

    def __len__(self):
        return len(self.to_tuple())


class CLIPVisionEmbeddings(nn.Module):
    def __init__(self, hidden, channels, image_size, patch_size):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.zeros(hidden))
        self.patch_embedding = nn.Conv2d(channels, hidden, kernel_size=patch_size, stride=patch_size, bias=False)
        self.position_embedding = nn.Embedding((image_size // patch_size) ** 2 + 1, hidden)


class CLIPVisionTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = CLIPVisionEmbeddings(cfg.hidden_size, cfg.num_channels, cfg.image_size, cfg.patch_size)
        self.pre_layrnorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.encoder = CLIPEncoder(cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size, cfg.layer_norm_eps)
        self.post_layernorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class CLIPVisionModelWithProjection(PretrainedMixin, HipModule):
    """transformers `CLIPVisionModelWithProjection` (config defaults: IP-Adapter's `models/image_encoder`, OpenCLIP ViT-H/14)."""

    weights_name = "pytorch_model.bin"
    safetensors_weights_name = "model.safetensors"

    def __init__(self, hidden_size=1280, intermediate_size=5120, projection_dim=1024, num_hidden_layers=32, num_attention_heads=16,
                 num_channels=3, image_size=224, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5, **_unused):
        super().__init__()
        if hidden_size % num_attention_heads != 0 or hidden_size // num_attention_heads not in HEAD_DIMS:
            raise NotImplementedError(f"hidden_size {hidden_size} with {num_attention_heads} heads: the attention kernel "
                                      f"(i2v_clip_vision_attention_f16) implements head_dim {' and '.join(map(str, HEAD_DIMS))} only")
        if patch_size <= 0 or image_size <= 0 or image_size % patch_size != 0:
            raise NotImplementedError(f"image_size {image_size} is not a multiple of patch_size {patch_size}: the patch kernel "
                                      "(i2v_clip_patchify_f16) takes whole patches only")
        tokens = (image_size // patch_size) ** 2 + 1
        if tokens > MAX_TOKENS:
            raise NotImplementedError(f"image_size {image_size} / patch_size {patch_size}: {tokens} tokens, the attention kernel "
                                      f"(i2v_clip_vision_attention_f16) takes at most {MAX_TOKENS}")
        if hidden_act not in ("quick_gelu", "gelu"):
            raise NotImplementedError(f"hidden_act {hidden_act!r}: one of 'quick_gelu', 'gelu'")
        if intermediate_size % 8 != 0 or projection_dim % 8 != 0:
            raise NotImplementedError(f"intermediate_size {intermediate_size} and projection_dim {projection_dim} must be multiples of 8 "
                                      "(i2v_gemm_f16)")
        self.config = _Config(hidden_size=hidden_size, intermediate_size=intermediate_size, projection_dim=projection_dim,
                              num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads, num_channels=num_channels,
                              image_size=image_size, patch_size=patch_size, hidden_act=hidden_act, layer_norm_eps=layer_norm_eps)
        self.vision_model = CLIPVisionTransformer(self.config)
        self.visual_projection = nn.Linear(hidden_size, projection_dim, bias=False)

    @property
    def device(self):
        return self.visual_projection.weight.device

    @property
    def dtype(self):
        return self.visual_projection.weight.dtype

    @classmethod
    def _convert_state_dict(cls, state, target):
        """the `position_ids` buffer of older files is not a weight"""
        return {k: v for k, v in state.items() if not k.endswith("embeddings.position_ids")}

    # ------------------------------------------------------------------------------------------ kernel-layout weights
    def _pack(self):
        vm, cfg = self.vision_model, self.config
        wp = vm.embeddings.patch_embedding.weight.detach().flatten(1)                   # [hidden, C p p], columns (c, dy, dx)
        wpad = torch.zeros((wp.shape[0], K.pad8(wp.shape[1])), dtype=f16, device=wp.device)
        wpad[:, : wp.shape[1]] = wp.to(f16)
        ln = lambda m: (w16(m.weight), w16(m.bias))
        return dict(patch=wpad, cls=w16(vm.embeddings.class_embedding), pos=w16(vm.embeddings.position_embedding.weight),
                    pre=ln(vm.pre_layrnorm), post=ln(vm.post_layernorm), proj=w16(self.visual_projection.weight),
                    layers=pack_layers(vm.encoder.layers), eps=cfg.layer_norm_eps, fold={})

    @torch.no_grad()
    def forward(self, pixel_values, output_hidden_states: Optional[bool] = False, **_unused):
        cfg = self.config
        if not isinstance(pixel_values, torch.Tensor) or pixel_values.dim() != 4:
            raise ValueError("pixel_values must be a [batch, channels, height, width] tensor")
        if tuple(pixel_values.shape[1:]) != (cfg.num_channels, cfg.image_size, cfg.image_size):
            raise ValueError(f"pixel_values {tuple(pixel_values.shape)}: expected [batch, {cfg.num_channels}, {cfg.image_size}, "
                             f"{cfg.image_size}] (the position table has one row per patch of that size)")
        if not pixel_values.is_cuda:
            raise HipLibraryError(f"pixel_values is on {pixel_values.device}: the HIP path has no CPU fallback")
        p = self.packed()
        b, heads, hid = pixel_values.shape[0], cfg.num_attention_heads, cfg.hidden_size
        l = p["pos"].shape[0]
        cols = K.clip_patchify(pixel_values.to(f16).contiguous(), cfg.patch_size, ld=p["patch"].shape[1])
        x = K.clip_vision_embed(p["cls"], K.gemm(cols, p["patch"], None), p["pos"], batch=b)
        x = K.layernorm(x, p["pre"][0], p["pre"][1], p["eps"])
        hidden = [x]
        attention = lambda qkv: K.clip_vision_attention(qkv, batch=b, length=l, heads=heads, head_dim=hid // heads)
        for lp in p["layers"]:
            x = encoder_layer(p, lp, x, attention, cfg.hidden_act == "quick_gelu")
            hidden.append(x)
        last = x.view(b, l, hid)
        pooled = K.layernorm(last[:, :1], p["post"][0], p["post"][1], p["eps"])           # the class rows, read in place
        return CLIPVisionModelOutput(image_embeds=K.gemm(pooled, p["proj"], None), last_hidden_state=last,
                                     hidden_states=tuple(t.view(b, l, hid) for t in hidden) if output_hidden_states else None)


@torch.no_grad()
def init_clip_vision_weights_(model: CLIPVisionModelWithProjection, seed: int = 0, qk_gain: float = 1.0) -> CLIPVisionModelWithProjection:
    """Synthetic weights for tests and probes (there are no pretrained files offline), drawn on the model's own device by transformers'
    CLIP initialisation law; q_proj / k_proj weights times `qk_gain` (the law's logits have std 0.25: attention is nearly uniform)."""
    cfg = model.config
    g = torch.Generator(device=model.device).manual_seed(seed)
    h, n = cfg.hidden_size, cfg.num_hidden_layers
    in_std, out_std, fc_std = h ** -0.5 * (2 * n) ** -0.5, h ** -0.5, (2 * h) ** -0.5
    for name, prm in model.named_parameters():
        if "norm" in name:
            prm.copy_((torch.randn(prm.shape, generator=g, device=prm.device) * 0.1 + (1.0 if name.endswith("weight") else 0.0)).to(prm.dtype))
            continue
        std = 0.02
        if name.endswith("class_embedding") or name.endswith("visual_projection.weight"):
            std = out_std
        elif name.endswith("proj.weight") or name.endswith("fc2.weight"):
            std = out_std if "out_proj" in name else in_std * (qk_gain if ("q_proj" in name or "k_proj" in name) else 1.0)
        elif name.endswith("fc1.weight"):
            std = fc_std
        prm.copy_((torch.randn(prm.shape, generator=g, device=prm.device) * std).to(prm.dtype))
    return model
