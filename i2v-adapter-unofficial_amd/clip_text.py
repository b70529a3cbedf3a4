"""CLIP text encoder on the HIP kernels: what `encode_prompt` (pipe:348-527) calls to turn token ids into the `[B, 77, 768]` context of
the UNet's text cross-attention.

Host mirror of transformers' `CLIPTextModel` with the checkpoint's state-dict keys (SD-1.5 `text_encoder/model.safetensors`:
`text_model.embeddings.{token,position}_embedding.weight`, `text_model.encoder.layers.{i}.{layer_norm1,layer_norm2,self_attn.{q,k,v,out}_proj,
mlp.{fc1,fc2}}.{weight,bias}`, `text_model.final_layer_norm.{weight,bias}`), so a `text_encoder/` folder loads by key.  The tower is 12 pre-LN
layers of width 768, 12 heads of 64, 77 tokens; per layer the forward is

    LN1 folded into ONE q|k|v GEMM -> causal attention (i2v_clip_attention_f16, q / k / v read in place from the packed GEMM result)
    -> out_proj GEMM + residual -> LN2 folded into fc1 -> quick-GELU (i2v_quick_gelu_f16; "gelu": the GEMM's erf-GELU epilogue)
    -> fc2 GEMM + residual

after the embedding lookup (i2v_clip_embed_f16) and before the final LayerNorm: library launches only, no torch ops, like the UNet.  A
LayerNorm is folded where the library says it folds this problem (`gemm(..., query_ln_support=True)`) and materialised otherwise.  The
1 / sqrt(d) of the attention is applied to the logits in fp32 inside the kernel.  Not per-step work: a prompt is encoded once per sample
(DESIGN 4.11).  Out of scope: padding attention masks (`use_attention_mask`; SD-1.5 does not use them, pipe:433-436), `pooler_output`, text
projection (the CLIP vision tower is clip_vision.py, on the same layer modules and helpers).
"""
from typing import Optional

import torch
from torch import nn

from . import kernels as K
from ._lib import I2V_EPI_GELU, I2V_EPI_NONE, HipLibraryError
from .blocks import HipModule, fold_layernorm, w16
from .checkpoint import PretrainedMixin

f16 = torch.float16
HEAD_DIM, MAX_POSITIONS = 64, 128          # the envelope of i2v_clip_attention_f16
PREFIX = "text_model."


class _Config(dict):
    __getattr__ = dict.get


class CLIPTextModelOutput:
    """transformers' `BaseModelOutputWithPooling` as far as the pipeline reads it: attribute access, and integer indexing over the fields
    that are not None (`out[0]` the last hidden state, `out[-1]` the hidden-states tuple when it was requested)."""

    def __init__(self, last_hidden_state, pooler_output=None, hidden_states=None):
        self.last_hidden_state, self.pooler_output, self.hidden_states = last_hidden_state, pooler_output, hidden_states

    def to_tuple(self):
        return tuple(v for v in (self.last_hidden_state, self.pooler_output, self.hidden_states) if v is not None)

    def __getitem__(self, i):
        return self.to_tuple()[i]

    def __len__(self):
        return len(self.to_tuple())


class FinalLayerNorm(nn.LayerNorm):
    """`text_model.final_layer_norm`, callable on its own (`clip_skip`, pipe:453): [..., H] fp16 on the device -> the same shape"""

    def forward(self, x):
        if not x.is_cuda:
            raise HipLibraryError(f"final_layer_norm input is on {x.device}: the HIP path has no CPU fallback")
        y = K.layernorm(x.to(f16).reshape(-1, x.shape[-1]), w16(self.weight), w16(self.bias), self.eps)
        return y.view(x.shape)


class CLIPAttention(nn.Module):
    def __init__(self, hidden):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(hidden, hidden) for _ in range(4))


class CLIPMLP(nn.Module):
    def __init__(self, hidden, inter):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(hidden, inter), nn.Linear(inter, hidden)


class CLIPEncoderLayer(nn.Module):
    def __init__(self, hidden, inter, eps):
        super().__init__()
        self.layer_norm1 = nn.LayerNorm(hidden, eps=eps)
        self.self_attn = CLIPAttention(hidden)
        self.layer_norm2 = nn.LayerNorm(hidden, eps=eps)
        self.mlp = CLIPMLP(hidden, inter)


class CLIPEncoder(nn.Module):
    def __init__(self, n, hidden, inter, eps):
        super().__init__()
        self.layers = nn.ModuleList([CLIPEncoderLayer(hidden, inter, eps) for _ in range(n)])


def pack_layers(layers):
    """kernel-layout operands of CLIPEncoderLayers (shared by the text and the vision tower): q | k | v as one GEMM, both LayerNorms in
    their plain and their folded form"""
    out = []
    for lyr in layers:
        a, m = lyr.self_attn, lyr.mlp
        wqkv = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], dim=0)
        bqkv = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], dim=0)
        out.append(dict(
            ln1=(w16(lyr.layer_norm1.weight), w16(lyr.layer_norm1.bias)), qkv=(w16(wqkv), w16(bqkv)),
            qkv_fold=fold_layernorm(wqkv, bqkv, lyr.layer_norm1.weight, lyr.layer_norm1.bias),
            out=(w16(a.out_proj.weight), w16(a.out_proj.bias)),
            ln2=(w16(lyr.layer_norm2.weight), w16(lyr.layer_norm2.bias)), fc1=(w16(m.fc1.weight), w16(m.fc1.bias)),
            fc1_fold=fold_layernorm(m.fc1.weight, m.fc1.bias, lyr.layer_norm2.weight, lyr.layer_norm2.bias),
            fc2=(w16(m.fc2.weight), w16(m.fc2.bias))))
    return out


def ln_gemm(p, x, plain, folded, ln, epilogue):
    """LayerNorm + Linear: folded into the GEMM where the library folds this problem, LayerNorm kernel + GEMM otherwise.  p: the pack
    (`eps`, and `fold`, the cache of the library's answers)"""
    wf, wsum, bf = folded
    key = (x.shape[0], wf.shape, epilogue)
    if key not in p["fold"]:
        p["fold"][key] = K.gemm(x, wf, bf, ln=(wsum, p["eps"]), epilogue=epilogue, query_ln_support=True)
    if p["fold"][key]:
        return K.gemm(x, wf, bf, ln=(wsum, p["eps"]), epilogue=epilogue)
    return K.gemm(K.layernorm(x, ln[0], ln[1], p["eps"]), plain[0], plain[1], epilogue=epilogue)


def encoder_layer(p, lp, x, attention, quick_gelu):
    """one pre-LN CLIP layer on the [B * L, hidden] stream: LN1 | q|k|v GEMM -> `attention(qkv)` -> out_proj + residual -> LN2 | fc1
    (erf-GELU epilogue, or quick-GELU after it) -> fc2 + residual"""
    qkv = ln_gemm(p, x, lp["qkv"], lp["qkv_fold"], lp["ln1"], I2V_EPI_NONE)
    x = K.gemm(attention(qkv), lp["out"][0], lp["out"][1], residual=x)
    h = ln_gemm(p, x, lp["fc1"], lp["fc1_fold"], lp["ln2"], I2V_EPI_NONE if quick_gelu else I2V_EPI_GELU)
    if quick_gelu:
        K.quick_gelu(h, out=h)
    return K.gemm(h, lp["fc2"][0], lp["fc2"][1], residual=x)


class CLIPTextEmbeddings(nn.Module):
    def __init__(self, vocab, positions, hidden):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, hidden)
        self.position_embedding = nn.Embedding(positions, hidden)


class CLIPTextTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = CLIPTextEmbeddings(cfg.vocab_size, cfg.max_position_embeddings, cfg.hidden_size)
        self.encoder = CLIPEncoder(cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size, cfg.layer_norm_eps)
        self.final_layer_norm = FinalLayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class CLIPTextModel(PretrainedMixin, HipModule):
    """transformers `CLIPTextModel` (config defaults: SD-1.5's text encoder, openai/clip-vit-large-patch14's text tower)."""

    weights_name = "pytorch_model.bin"
    safetensors_weights_name = "model.safetensors"

    def __init__(self, vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                 max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2, use_attention_mask=False,
                 **_unused):
        super().__init__()
        if hidden_size % num_attention_heads != 0 or hidden_size // num_attention_heads != HEAD_DIM:
            raise NotImplementedError(f"hidden_size {hidden_size} with {num_attention_heads} heads: the causal attention kernel "
                                      f"(i2v_clip_attention_f16) implements head_dim {HEAD_DIM} only")
        if not 1 <= max_position_embeddings <= MAX_POSITIONS:
            raise NotImplementedError(f"max_position_embeddings {max_position_embeddings}: the causal attention kernel "
                                      f"(i2v_clip_attention_f16) takes at most {MAX_POSITIONS} positions")
        if use_attention_mask:
            raise NotImplementedError("use_attention_mask: padding attention masks are not implemented (SD-1.5's text encoder "
                                      "does not use one, pipe:433-436)")
        if hidden_act not in ("quick_gelu", "gelu"):
            raise NotImplementedError(f"hidden_act {hidden_act!r}: one of 'quick_gelu', 'gelu'")
        if intermediate_size % 8 != 0:
            raise NotImplementedError(f"intermediate_size {intermediate_size} must be a multiple of 8")
        self.config = _Config(vocab_size=vocab_size, hidden_size=hidden_size, intermediate_size=intermediate_size,
                              num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
                              max_position_embeddings=max_position_embeddings, hidden_act=hidden_act, layer_norm_eps=layer_norm_eps,
                              eos_token_id=eos_token_id)
        self.text_model = CLIPTextTransformer(self.config)

    @property
    def device(self):
        return self.text_model.final_layer_norm.weight.device

    @property
    def dtype(self):
        return self.text_model.final_layer_norm.weight.dtype

    @classmethod
    def _convert_state_dict(cls, state, target):
        """keys with or without `text_model.` (every published SD checkpoint has the prefix, transformers 5.x saves without it); the
        `position_ids` buffer of older files is not a weight"""
        out = {}
        for k, v in state.items():
            if k.endswith("embeddings.position_ids"):
                continue
            out[PREFIX + k if k not in target and PREFIX + k in target else k] = v
        return out

    @torch.no_grad()
    def resize_token_embeddings(self, new_num_tokens: int):
        """transformers' `resize_token_embeddings` for the token table (textual inversion, textual_inversion.py): the table and
        `config.vocab_size` grow (or shrink) to `new_num_tokens` rows.  The rows both tables have keep their bits; new rows are zero
        until the loader writes them.  The kernel-layout pack is dropped (`i2v_clip_embed_f16` takes the row count as an argument
        and the wrapper bounds-checks the ids against it on the host).  Returns the table."""
        if isinstance(new_num_tokens, bool) or not isinstance(new_num_tokens, int) or new_num_tokens < 1:
            raise ValueError(f"new_num_tokens must be an int >= 1, got {new_num_tokens!r}")
        emb = self.text_model.embeddings
        old = emb.token_embedding.weight
        if new_num_tokens != old.shape[0]:
            new = nn.Embedding(new_num_tokens, old.shape[1], device=old.device, dtype=old.dtype)
            new.weight.zero_()
            keep = min(new_num_tokens, old.shape[0])
            new.weight[:keep] = old[:keep]
            new.weight.requires_grad_(old.requires_grad)
            emb.token_embedding = new
            self.config["vocab_size"] = new_num_tokens
        self._packed, self._packed_key = None, None
        return emb.token_embedding

    # ------------------------------------------------------------------------------------------ kernel-layout weights
    def _pack(self):
        tm = self.text_model
        return dict(tok=w16(tm.embeddings.token_embedding.weight), pos=w16(tm.embeddings.position_embedding.weight),
                    layers=pack_layers(tm.encoder.layers), eps=self.config.layer_norm_eps, fold={})

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, output_hidden_states: Optional[bool] = False, **_unused):
        if attention_mask is not None:
            raise NotImplementedError("attention_mask: padding attention masks are not implemented (SD-1.5's text encoder does not "
                                      "use one, pipe:433-436)")
        cfg = self.config
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2:
            raise ValueError("input_ids must be a [batch, length] tensor of token ids")
        b, l = input_ids.shape
        if l > cfg.max_position_embeddings:
            raise ValueError(f"{l} tokens for a position table of {cfg.max_position_embeddings} rows")
        p = self.packed()
        heads, hid = cfg.num_attention_heads, cfg.hidden_size
        x = K.clip_embed(p["tok"], p["pos"], input_ids)
        hidden = [x]
        attention = lambda qkv: K.clip_attention(qkv, batch=b, length=l, heads=heads, head_dim=HEAD_DIM)
        for lp in p["layers"]:
            x = encoder_layer(p, lp, x, attention, cfg.hidden_act == "quick_gelu")
            hidden.append(x)
        last = self.text_model.final_layer_norm(x).view(b, l, hid)
        return CLIPTextModelOutput(last_hidden_state=last, pooler_output=None,
                                   hidden_states=tuple(t.view(b, l, hid) for t in hidden) if output_hidden_states else None)


@torch.no_grad()
def init_clip_weights_(model: CLIPTextModel, seed: int = 0, qk_gain: float = 1.0) -> CLIPTextModel:
    """Synthetic weights for tests and probes (there are no pretrained files offline), drawn on the model's own device by transformers'
    CLIP initialisation law; q_proj / k_proj weights times `qk_gain` (the law's logits have std 0.25: attention is nearly uniform)."""
    cfg = model.config
    g = torch.Generator(device=model.device).manual_seed(seed)
    h, n = cfg.hidden_size, cfg.num_hidden_layers
    in_std, out_std, fc_std = h ** -0.5 * (2 * n) ** -0.5, h ** -0.5, (2 * h) ** -0.5
    for name, prm in model.named_parameters():
        if "layer_norm" in name:
            prm.copy_((torch.randn(prm.shape, generator=g, device=prm.device) * 0.1 + (1.0 if name.endswith("weight") else 0.0)).to(prm.dtype))
            continue
        std = 0.02
        if name.endswith("proj.weight") or name.endswith("fc2.weight"):
            std = out_std if "out_proj" in name else in_std * (qk_gain if ("q_proj" in name or "k_proj" in name) else 1.0)
        elif name.endswith("fc1.weight"):
            std = fc_std
        prm.copy_((torch.randn(prm.shape, generator=g, device=prm.device) * std).to(prm.dtype))
    return model
