"""Plain-torch restatement of the CLIP text tower (transformers `CLIPTextModel` as the pipeline's `encode_prompt` uses it): token +
position embeddings, causal pre-LN transformer layers with quick-GELU (or erf GELU), the final LayerNorm, the hidden-states list and
the `clip_skip` selection.  It is the yardstick of tests/test_clip_text*.py, pinned there against transformers itself and against a
committed fixture; it runs in the dtype of its weights -- fp32 / fp64, or fp16 after `.half()` (CPU or device).  No product code
imports it."""
import math

import torch
import torch.nn.functional as F

PREFIX = "text_model."


def strip_prefix(state):
    """the checkpoint's keys without `text_model.` (published SD checkpoints carry it, transformers 5.x saves without it); the
    `position_ids` buffer of older files is dropped"""
    out = {}
    for k, v in state.items():
        k = k[len(PREFIX):] if k.startswith(PREFIX) else k
        if not k.endswith("embeddings.position_ids"):
            out[k] = v
    return out


def state_dict_keys(num_layers):
    """the key names of SD-1.5's text_encoder/model.safetensors for `num_layers` layers, in file order"""
    keys = ["text_model.embeddings.position_embedding.weight", "text_model.embeddings.token_embedding.weight"]
    for i in range(num_layers):
        for m in ("layer_norm1", "layer_norm2", "mlp.fc1", "mlp.fc2", "self_attn.k_proj", "self_attn.out_proj", "self_attn.q_proj",
                  "self_attn.v_proj"):
            keys += [f"text_model.encoder.layers.{i}.{m}.bias", f"text_model.encoder.layers.{i}.{m}.weight"]
    return keys + ["text_model.final_layer_norm.bias", "text_model.final_layer_norm.weight"]


def seeded_state(config, seed=0, qk_gain=1.0, dtype=torch.float32):
    """transformers' CLIP initialisation law (factor 1) drawn from one seeded generator, values fp16-representable; q_proj / k_proj
    weights times `qk_gain` (3: logits of std ~2 instead of 0.25, so that masking and softmax errors show)"""
    g = torch.Generator().manual_seed(seed)
    h, inter, n = config["hidden_size"], config["intermediate_size"], config["num_hidden_layers"]
    rn = lambda shape, std: (torch.randn(shape, generator=g) * std).half().to(dtype)
    st = {"embeddings.token_embedding.weight": rn((config["vocab_size"], h), 0.02),
          "embeddings.position_embedding.weight": rn((config["max_position_embeddings"], h), 0.02)}
    in_std, out_std, fc_std = h ** -0.5 * (2 * n) ** -0.5, h ** -0.5, (2 * h) ** -0.5
    for i in range(n):
        p = f"encoder.layers.{i}."
        for name, shape, std in (("self_attn.q_proj", (h, h), in_std * qk_gain), ("self_attn.k_proj", (h, h), in_std * qk_gain),
                                 ("self_attn.v_proj", (h, h), in_std), ("self_attn.out_proj", (h, h), out_std),
                                 ("mlp.fc1", (inter, h), fc_std), ("mlp.fc2", (h, inter), in_std)):
            st[p + name + ".weight"] = rn(shape, std)
            st[p + name + ".bias"] = rn((shape[0],), 0.02)
        for ln in ("layer_norm1", "layer_norm2"):
            st[p + ln + ".weight"] = (1 + rn((h,), 0.1)).half().to(dtype)
            st[p + ln + ".bias"] = rn((h,), 0.05)
    st["final_layer_norm.weight"] = (1 + rn((h,), 0.1)).half().to(dtype)
    st["final_layer_norm.bias"] = rn((h,), 0.05)
    return {PREFIX + k: v for k, v in st.items()}


def prompt_like_ids(batch, length, vocab, seed=0, full_row=True):
    """ids shaped like tokenised prompts: BOS (vocab - 2), a few tokens, EOS (vocab - 1) padding to `length`; the last row is full
    length when `full_row` (and there is more than one row)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((batch, length), vocab - 1, dtype=torch.int64)
    ids[:, 0] = vocab - 2
    for b in range(batch):
        n = length - 2 if (full_row and b == batch - 1 and batch > 1) else min(length - 2, 3 + 4 * b)
        if n > 0:
            ids[b, 1:1 + n] = torch.randint(0, vocab - 2, (n,), generator=g)
    return ids


def causal_attention(q, k, v, scale):
    """softmax(q k^T scale + mask) v over [..., L, d] in the operands' dtype: mask -inf above the diagonal"""
    L = q.shape[-2]
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    mask = torch.full((L, L), float("-inf"), dtype=s.dtype, device=s.device).triu(1)
    return torch.matmul(torch.softmax(s + mask, dim=-1), v)


class ClipTextReference:
    def __init__(self, state, config):
        self.w = strip_prefix(state)
        self.config = dict(config)

    def _like(self, fn):
        return ClipTextReference({k: fn(v) for k, v in self.w.items()}, self.config)

    def half(self):
        return self._like(lambda t: t.half())

    def float(self):
        return self._like(lambda t: t.float())

    def double(self):
        return self._like(lambda t: t.double())

    def to(self, device):
        return self._like(lambda t: t.to(device))

    def _linear(self, x, name):
        return F.linear(x, self.w[name + ".weight"], self.w[name + ".bias"])

    def _ln(self, x, name):
        return F.layer_norm(x, (x.shape[-1],), self.w[name + ".weight"], self.w[name + ".bias"], self.config["layer_norm_eps"])

    def final_layer_norm(self, x):
        return self._ln(x, "final_layer_norm")

    def _act(self, x):
        act = self.config.get("hidden_act", "quick_gelu")
        if act == "quick_gelu":
            return x * torch.sigmoid(1.702 * x)
        if act == "gelu":
            return F.gelu(x)
        raise ValueError(act)

    def __call__(self, input_ids, output_hidden_states=False):
        """-> (last_hidden_state [B, L, H], hidden_states: tuple of num_layers + 1 tensors, all before the final LayerNorm, or None)"""
        cfg = self.config
        heads = cfg["num_attention_heads"]
        B, L = input_ids.shape
        dev = self.w["embeddings.token_embedding.weight"].device
        ids = input_ids.to(dev).long()
        x = self.w["embeddings.token_embedding.weight"][ids] + self.w["embeddings.position_embedding.weight"][:L][None]
        d = x.shape[-1] // heads
        hidden = [x]
        for i in range(cfg["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            h = self._ln(x, p + "layer_norm1")
            split = lambda t: t.view(B, L, heads, d).transpose(1, 2)
            q, k, v = (split(self._linear(h, p + "self_attn." + n)) for n in ("q_proj", "k_proj", "v_proj"))
            a = causal_attention(q, k, v, 1.0 / math.sqrt(d)).transpose(1, 2).reshape(B, L, heads * d)
            x = x + self._linear(a, p + "self_attn.out_proj")
            h = self._ln(x, p + "layer_norm2")
            x = x + self._linear(self._act(self._linear(h, p + "mlp.fc1")), p + "mlp.fc2")
            hidden.append(x)
        return self.final_layer_norm(x), (tuple(hidden) if output_hidden_states else None)

    def encode(self, input_ids, clip_skip=None):
        """what `encode_prompt` takes from the tower (pipe:438-453)"""
        if clip_skip is None:
            return self(input_ids)[0]
        return self.final_layer_norm(self(input_ids, output_hidden_states=True)[1][-(clip_skip + 1)])


class StubTokenizer:
    """CLIPTokenizer's call interface over characters: BOS (vocab - 2), one id per character, EOS (vocab - 1), EOS padding"""

    def __init__(self, model_max_length=77, vocab_size=256):
        self.model_max_length, self.vocab_size = model_max_length, vocab_size
        self.calls = []

    def _encode(self, text):
        return [self.vocab_size - 2] + [ord(c) % (self.vocab_size - 2) for c in text] + [self.vocab_size - 1]

    def __call__(self, text, padding="longest", max_length=None, truncation=False, return_tensors="pt"):
        texts = [text] if isinstance(text, str) else list(text)
        self.calls.append((tuple(texts), padding, max_length))
        rows = [self._encode(t) for t in texts]
        if truncation and max_length is not None:
            rows = [r if len(r) <= max_length else r[:max_length - 1] + [self.vocab_size - 1] for r in rows]
        width = max_length if padding == "max_length" else max(len(r) for r in rows)
        ids = torch.tensor([r + [self.vocab_size - 1] * (width - len(r)) for r in rows], dtype=torch.int64)

        class _Enc:
            input_ids = ids
            attention_mask = torch.ones_like(ids)
        return _Enc()

    def batch_decode(self, ids):
        return ["".join(chr(int(i)) for i in row) for row in ids]
