"""IP-Adapter Plus for the tests: the Resampler in plain torch (the yardstick of blocks.Resampler), a seeded Plus file in the ORIGINAL
checkpoint layout (`to_kv` fused, `norm1` / `norm2`), and a helper that puts the same adapter on the oracle's UNet.

    latents = self.latents repeated over B;  x = proj_in(x)
    per layer:  kv_in   = cat([ln0(x), ln1(latents)], dim=-2)
                latents = to_out(softmax(to_q(ln1(latents)) to_k(kv_in)^T / sqrt(dim_head)) to_v(kv_in)) + latents
                latents = ff(latents) + latents                        ff = LayerNorm -> Linear -> erf-GELU -> Linear, no Linear biases
    return norm_out(proj_out(latents))

`ResamplerReference(state, dtype)` takes the CONVERTED (diffusers-named) state dict.  dtype float32 / float64 is the yardstick; float16
is torch's own fp16 evaluation of the same operands (every op in half on the CPU), the base line of `tests.parity.fp16_gate`."""
import torch
import torch.nn.functional as F

DIM_HEAD = 64


class ResamplerReference(torch.nn.Module):
    def __init__(self, state, dtype=torch.float32):
        super().__init__()
        self.state = {k: v.detach().to("cpu", dtype) for k, v in state.items()}
        self.dtype_ = dtype
        self.depth = 1 + max(int(k.split(".")[1]) for k in self.state if k.startswith("layers."))
        self.heads = self.state["layers.0.2.to_q.weight"].shape[0] // DIM_HEAD
        self.num_queries = self.state["latents"].shape[1]

    def half(self):
        return ResamplerReference(self.state, torch.float16)

    def _ln(self, x, name):
        w = self.state[name + ".weight"]
        return F.layer_norm(x, w.shape, w, self.state[name + ".bias"], 1e-5)

    def _split(self, t):
        b, l, _ = t.shape
        return t.view(b, l, self.heads, DIM_HEAD).transpose(1, 2)

    @torch.no_grad()
    def forward(self, x):
        s = self.state
        x = x.detach().to("cpu", self.dtype_)
        b = x.shape[0]
        latents = s["latents"].repeat(b, 1, 1)
        x = F.linear(x, s["proj_in.weight"], s["proj_in.bias"])
        for i in range(self.depth):
            p = f"layers.{i}."
            ln_lat = self._ln(latents, p + "1")
            kv_in = torch.cat([self._ln(x, p + "0"), ln_lat], dim=-2)
            q = self._split(F.linear(ln_lat, s[p + "2.to_q.weight"]))
            k = self._split(F.linear(kv_in, s[p + "2.to_k.weight"]))
            v = self._split(F.linear(kv_in, s[p + "2.to_v.weight"]))
            w = torch.softmax((q @ k.transpose(-1, -2)) * DIM_HEAD ** -0.5, dim=-1)
            o = (w @ v).transpose(1, 2).reshape(b, -1, self.heads * DIM_HEAD)
            latents = F.linear(o, s[p + "2.to_out.0.weight"]) + latents
            h = F.gelu(F.linear(self._ln(latents, p + "3.0"), s[p + "3.1.net.0.proj.weight"]))
            latents = F.linear(h, s[p + "3.1.net.2.weight"]) + latents
        return self._ln(F.linear(latents, s["proj_out.weight"], s["proj_out.bias"]), "norm_out")


def _attn2_names(unet):
    return [n for n in unet.attn_processor_names() if n.endswith("attn2.processor") and "motion_modules" not in n]


def plus_state_dict(unet, embed_dims=48, hidden=128, heads=2, depth=2, num_queries=8, seed=7, ffn_ratio=4, qk_gain=1.0):
    """{"image_proj", "ip_adapter"} of an IP-Adapter Plus file for `unet` (any UNet of this family, oracle or HIP) in the original
    layout; seeded, every value fp16-representable.  to_q / to_kv's K half times `qk_gain` (logits of std ~ qk_gain^2)."""
    g = torch.Generator().manual_seed(seed)
    cross = unet.config["cross_attention_dim"]
    inner, ff = heads * DIM_HEAD, hidden * ffn_ratio
    r = lambda *shape, s: (torch.randn(*shape, generator=g) * s).half().float()
    gamma = lambda n: (1 + 0.1 * torch.randn(n, generator=g)).half().float()
    ip = {"latents": r(1, num_queries, hidden, s=hidden ** -0.5 * 4),
          "proj_in.weight": r(hidden, embed_dims, s=embed_dims ** -0.5), "proj_in.bias": r(hidden, s=0.1),
          "proj_out.weight": r(cross, hidden, s=hidden ** -0.5), "proj_out.bias": r(cross, s=0.1),
          "norm_out.weight": gamma(cross), "norm_out.bias": r(cross, s=0.1)}
    for i in range(depth):
        p = f"layers.{i}."
        for n in ("0.norm1", "0.norm2", "1.0"):
            ip[p + n + ".weight"], ip[p + n + ".bias"] = gamma(hidden), r(hidden, s=0.1)
        ip[p + "0.to_q.weight"] = r(inner, hidden, s=hidden ** -0.5 * qk_gain)
        kv = r(2 * inner, hidden, s=hidden ** -0.5)
        kv[:inner] = (kv[:inner] * qk_gain).half().float()
        ip[p + "0.to_kv.weight"] = kv
        ip[p + "0.to_out.weight"] = r(hidden, inner, s=inner ** -0.5)
        ip[p + "1.1.weight"] = r(ff, hidden, s=hidden ** -0.5)
        ip[p + "1.3.weight"] = r(hidden, ff, s=ff ** -0.5)
    sd = {"image_proj": ip, "ip_adapter": {}}
    mods = dict(unet.named_modules())
    for i, n in enumerate(_attn2_names(unet)):
        a = mods[n[: -len(".processor")]]
        sd["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"] = r(a.inner_dim, cross, s=cross ** -0.5)
        sd["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"] = r(a.inner_dim, cross, s=cross ** -0.5)
    return sd


def converted_image_proj(state):
    """the diffusers-named Resampler state dict of a Plus file, by the project's converter"""
    from i2v_adapter_unofficial_amd.unet_motion_cross_frame_attn import convert_ip_adapter_plus_image_proj
    return convert_ip_adapter_plus_image_proj(state["image_proj"])[1]


def install_plus_on_oracle(oracle_unet, state):
    """the oracle's UNet with the Plus adapter `state`: to_k_ip / to_v_ip on every non-motion attn2 in attn_processors order (key ids
    1, 3, ...: what the oracle's own loader does for the plain adapter), `encoder_hid_proj` = the fp32 ResamplerReference."""
    ref = ResamplerReference(converted_image_proj(state), torch.float32)
    mods = dict(oracle_unet.named_modules())
    oracle_unet.encoder_hid_proj = None
    for i, n in enumerate(_attn2_names(oracle_unet)):
        mods[n[: -len(".processor")]].install_ip_adapter(state["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"],
                                                         state["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"],
                                                         num_tokens=ref.num_queries, scale=1.0)
    oracle_unet.encoder_hid_proj = ref
    oracle_unet.config.encoder_hid_dim_type = "ip_image_proj"
    return oracle_unet
