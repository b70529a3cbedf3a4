"""Plain-torch restatement of the CLIP vision tower (transformers `CLIPVisionModelWithProjection` as the pipeline's `encode_image` uses
it): the bias-free patch convolution, class token + position embeddings, `pre_layrnorm`, bidirectional pre-LN transformer layers with
erf GELU (or quick-GELU), `post_layernorm` on the class token, the visual projection, and the hidden-states list (whose entry 0 is
AFTER `pre_layrnorm`, as transformers has it).  It is the yardstick of tests/test_clip_vision*.py, pinned there against transformers
itself and against a committed fixture; it runs in the dtype of its weights -- fp32 / fp64, or fp16 after `.half()` (CPU or device).
No product code imports it."""
import math
import os

import torch
import torch.nn.functional as F

PREFIX = "vision_model."

VIT_H = dict(hidden_size=1280, intermediate_size=5120, projection_dim=1024, num_hidden_layers=32, num_attention_heads=16,
             num_channels=3, image_size=224, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5)
SMALL = dict(hidden_size=160, intermediate_size=160, projection_dim=64, num_hidden_layers=2, num_attention_heads=2,
             num_channels=3, image_size=224, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POS = PREFIX + "embeddings.position_embedding.weight"


def load_fixture():
    """(everything in tests/golden/clip_vision_small{,_224}.safetensors, the fp16 state dict among it)"""
    from safetensors.torch import load_file
    blob = load_file(os.path.join(GOLDEN, "clip_vision_small.safetensors"))
    blob.update(load_file(os.path.join(GOLDEN, "clip_vision_small_224.safetensors")))
    return blob, {k: v for k, v in blob.items() if k.startswith(PREFIX) or k.startswith("visual_projection")}


def fixture_state(size):
    """fp32 state of the fixture's model for a 224-px (the model's position table) or a 56-px input (the second, 17-row table)"""
    blob, state = load_fixture()
    st = {k: v.float() for k, v in state.items()}
    if size == 56:
        st[POS] = blob["position_embedding_56.weight"].float()
    return blob, st


def drop_buffers(state):
    """the `position_ids` buffer of older files is not a weight"""
    return {k: v for k, v in state.items() if not k.endswith("embeddings.position_ids")}


def state_dict_keys(num_layers):
    """the sorted key names of IP-Adapter's image_encoder state dict for `num_layers` layers (without the `position_ids` buffer)"""
    keys = ["vision_model.embeddings.class_embedding", "vision_model.embeddings.patch_embedding.weight",
            "vision_model.embeddings.position_embedding.weight", "visual_projection.weight"]
    for i in range(num_layers):
        for m in ("layer_norm1", "layer_norm2", "mlp.fc1", "mlp.fc2", "self_attn.k_proj", "self_attn.out_proj", "self_attn.q_proj",
                  "self_attn.v_proj"):
            keys += [f"vision_model.encoder.layers.{i}.{m}.bias", f"vision_model.encoder.layers.{i}.{m}.weight"]
    for ln in ("pre_layrnorm", "post_layernorm"):
        keys += [f"vision_model.{ln}.bias", f"vision_model.{ln}.weight"]
    return sorted(keys)


def seeded_state(config, seed=0, qk_gain=1.0, dtype=torch.float32):
    """transformers' CLIP initialisation law (factor 1) drawn from one seeded generator, values fp16-representable; q_proj / k_proj
    weights times `qk_gain` (3: logits of std ~2 instead of 0.25, so that masking and softmax errors show)"""
    g = torch.Generator().manual_seed(seed)
    h, inter, n = config["hidden_size"], config["intermediate_size"], config["num_hidden_layers"]
    c, p = config["num_channels"], config["patch_size"]
    tokens = (config["image_size"] // p) ** 2 + 1
    rn = lambda shape, std: (torch.randn(shape, generator=g) * std).half().to(dtype)
    st = {"vision_model.embeddings.class_embedding": rn((h,), h ** -0.5),
          "vision_model.embeddings.patch_embedding.weight": rn((h, c, p, p), 0.02),
          "vision_model.embeddings.position_embedding.weight": rn((tokens, h), 0.02)}
    in_std, out_std, fc_std = h ** -0.5 * (2 * n) ** -0.5, h ** -0.5, (2 * h) ** -0.5
    for i in range(n):
        pre = f"vision_model.encoder.layers.{i}."
        for name, shape, std in (("self_attn.q_proj", (h, h), in_std * qk_gain), ("self_attn.k_proj", (h, h), in_std * qk_gain),
                                 ("self_attn.v_proj", (h, h), in_std), ("self_attn.out_proj", (h, h), out_std),
                                 ("mlp.fc1", (inter, h), fc_std), ("mlp.fc2", (h, inter), in_std)):
            st[pre + name + ".weight"] = rn(shape, std)
            st[pre + name + ".bias"] = rn((shape[0],), 0.02)
        for ln in ("layer_norm1", "layer_norm2"):
            st[pre + ln + ".weight"] = (1 + rn((h,), 0.1)).half().to(dtype)
            st[pre + ln + ".bias"] = rn((h,), 0.05)
    for ln in ("pre_layrnorm", "post_layernorm"):
        st[f"vision_model.{ln}.weight"] = (1 + rn((h,), 0.1)).half().to(dtype)
        st[f"vision_model.{ln}.bias"] = rn((h,), 0.05)
    st["visual_projection.weight"] = rn((config["projection_dim"], h), out_std)
    return st


def pixel_like(batch, size, seed=0, channels=3):
    """fp16-representable pixel values with the statistics of a normalised image (|v| up to ~2.5, smooth + noise)"""
    g = torch.Generator().manual_seed(seed)
    low = F.interpolate(torch.randn(batch, channels, 4, 4, generator=g), size=(size, size), mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(batch, channels, size, size, generator=g)).clamp(-2.5, 2.5).half().float()


def pattern_pixels(batch, size, channels=3):
    """pixel values from integer arithmetic alone (multiples of 1/16 in [-2, 2): exact in fp16, the same on every machine), what the
    committed fixture's outputs were computed from; no two rows, columns, channels or images alike"""
    b, c, y, x = torch.meshgrid(torch.arange(batch), torch.arange(channels), torch.arange(size), torch.arange(size), indexing="ij")
    return (((y * 31 + x * 17 + c * 7 + b * 5 + (y * x) % 11 + (y * y) % 7) % 64 - 32).float() / 16.0)


def attention(q, k, v, scale):
    """softmax(q k^T scale) v over [..., L, d] in the operands' dtype: every key visible"""
    return torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale, dim=-1), v)


class ClipVisionReference:
    def __init__(self, state, config):
        self.w = drop_buffers(state)
        self.config = dict(config)

    def _like(self, fn):
        return ClipVisionReference({k: fn(v) for k, v in self.w.items()}, self.config)

    def half(self):
        return self._like(lambda t: t.half())

    def float(self):
        return self._like(lambda t: t.float())

    def double(self):
        return self._like(lambda t: t.double())

    def to(self, device):
        return self._like(lambda t: t.to(device))

    def _linear(self, x, name):
        return F.linear(x, self.w[name + ".weight"], self.w.get(name + ".bias"))

    def _ln(self, x, name):
        return F.layer_norm(x, (x.shape[-1],), self.w[name + ".weight"], self.w[name + ".bias"], self.config["layer_norm_eps"])

    def _act(self, x):
        act = self.config.get("hidden_act", "gelu")
        if act == "quick_gelu":
            return x * torch.sigmoid(1.702 * x)
        if act == "gelu":
            return F.gelu(x)
        raise ValueError(act)

    def __call__(self, pixel_values, output_hidden_states=False):
        """-> (image_embeds [B, projection_dim], last_hidden_state [B, L, H], hidden_states: tuple of num_layers + 1 tensors, the first
        after pre_layrnorm, or None)"""
        cfg = self.config
        heads, p = cfg["num_attention_heads"], cfg["patch_size"]
        wpatch = self.w[PREFIX + "embeddings.patch_embedding.weight"]
        px = pixel_values.to(device=wpatch.device, dtype=wpatch.dtype)
        B = px.shape[0]
        n = px.shape[-1] // p                     # the bias-free stride-p convolution as the matrix product it is: [B, P, C p p] x W^T
        cols = px.view(B, px.shape[1], n, p, n, p).permute(0, 2, 4, 1, 3, 5).reshape(B, n * n, -1)
        patches = torch.matmul(cols, wpatch.flatten(1).t())                                      # [B, P, H]
        cls = self.w[PREFIX + "embeddings.class_embedding"].expand(B, 1, -1)
        x = torch.cat([cls, patches], dim=1)
        L = x.shape[1]
        x = x + self.w[PREFIX + "embeddings.position_embedding.weight"][:L][None]
        x = self._ln(x, PREFIX + "pre_layrnorm")
        d = x.shape[-1] // heads
        hidden = [x]
        for i in range(cfg["num_hidden_layers"]):
            pre = f"{PREFIX}encoder.layers.{i}."
            h = self._ln(x, pre + "layer_norm1")
            split = lambda t: t.view(B, L, heads, d).transpose(1, 2)
            q, k, v = (split(self._linear(h, pre + "self_attn." + n)) for n in ("q_proj", "k_proj", "v_proj"))
            a = attention(q, k, v, 1.0 / math.sqrt(d)).transpose(1, 2).reshape(B, L, heads * d)
            x = x + self._linear(a, pre + "self_attn.out_proj")
            h = self._ln(x, pre + "layer_norm2")
            x = x + self._linear(self._act(self._linear(h, pre + "mlp.fc1")), pre + "mlp.fc2")
            hidden.append(x)
        pooled = self._ln(x[:, 0], PREFIX + "post_layernorm")
        return self._linear(pooled, "visual_projection"), x, (tuple(hidden) if output_hidden_states else None)


class StubFeatureExtractor:
    """CLIPImageProcessor's call interface: PIL images / arrays / CHW tensors in [0, 255] or [0, 1] -> `.pixel_values` [B, 3, S, S] fp32,
    nearest-neighbour resize to S and CLIP's mean / std normalisation"""
    mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)

    def __init__(self, size=224):
        self.size, self.calls = size, 0

    def _one(self, im):
        import numpy as np
        t = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.asarray(im).copy())
        if t.dim() == 3 and t.shape[-1] in (1, 3):
            t = t.permute(2, 0, 1)
        t = t.float()
        if t.max() > 1.5:
            t = t / 255.0
        t = F.interpolate(t[None], size=(self.size, self.size), mode="nearest")[0]
        return (t - torch.tensor(self.mean)[:, None, None]) / torch.tensor(self.std)[:, None, None]

    def __call__(self, images, return_tensors="pt"):
        self.calls += 1
        ims = images if isinstance(images, (list, tuple)) else [images]
        pv = torch.stack([self._one(im) for im in ims])

        class _Enc:
            pixel_values = pv
        return _Enc()
