"""LoRA references for the tests: the merge in fp64, seeded random LoRAs for a model's Linear / conv weights in every key spelling
the loader accepts, and oracle models whose state dict was merged by `merge_reference` (the oracle itself has no LoRA code: a LoRA'd
oracle is an oracle with merged weights)."""
import contextlib

import torch

ATTN_PROJ = (".to_q", ".to_k", ".to_v", ".to_out.0")


def merge_reference(base, adapters):
    """base + sum_j scale_j * up_j @ down_j in fp64; base [out, in] or a conv weight (flattened to [out, in] and reshaped back),
    adapters = [(down [rank, in ...], up [out, rank ...], scale)]."""
    n_out = base.shape[0]
    acc = base.detach().double().cpu().reshape(n_out, -1).clone()
    for down, up, scale in adapters:
        rank = down.shape[0]
        acc += float(scale) * (up.detach().double().cpu().reshape(n_out, rank) @ down.detach().double().cpu().reshape(rank, -1))
    return acc.reshape(base.shape)


def target_shapes(model):
    """{module path: weight shape} of every Linear / conv of a model (oracle or product: the names are the same)"""
    return {n: tuple(m.weight.shape) for n, m in model.named_modules()
            if n and isinstance(m, (torch.nn.Linear, torch.nn.Conv2d))}


def random_lora(shapes, rank, seed, std=0.05, paths=None, alpha=None, dtype=torch.float16):
    """normalised LoRA {path: (down [rank, in], up [out, rank], alpha or None)} with N(0, std^2) factors, fp16-representable"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for path in (paths if paths is not None else sorted(shapes)):
        shape = shapes[path]
        n_in = 1
        for s in shape[1:]:
            n_in *= s
        down = (torch.randn(rank, n_in, generator=g) * std).to(dtype)
        up = (torch.randn(shape[0], rank, generator=g) * std).to(dtype)
        out[path] = (down, up, alpha)
    return out


def attention_paths(shapes):
    return [p for p in sorted(shapes) if p.endswith(ATTN_PROJ)]


def to_state_dict(lora, shapes, spelling, prefix=""):
    """the normalised LoRA as a file's state dict.  spelling: "diffusers" (<path>.lora.down.weight), "processor" (the old attention
    processors: <attn>.processor.to_q_lora.down.weight; attention projections only), "peft" (lora_A / lora_B), "kohya"
    (lora_unet_<flattened>.lora_down.weight, conv factors 4-D, alpha as a 0-d tensor).  Linear `to_out.0` is written `to_out` by the
    first two, as diffusers does."""
    sd = {}
    for path, (down, up, alpha) in lora.items():
        shape = shapes[path]
        if spelling == "kohya":
            stem = "lora_unet_" + path.replace(".", "_")
            d, u = down, up
            if len(shape) == 4:
                d, u = down.reshape(down.shape[0], *shape[1:]), up.reshape(shape[0], -1, 1, 1)
            sd[stem + ".lora_down.weight"], sd[stem + ".lora_up.weight"] = d, u
            if alpha is not None:
                sd[stem + ".alpha"] = torch.tensor(float(alpha))
            continue
        if spelling == "processor":
            assert path.endswith(ATTN_PROJ), path
            attn, proj = path[: -len(".0")].rsplit(".", 1) if path.endswith(".0") else path.rsplit(".", 1)
            dk, uk = f"{attn}.processor.{proj}_lora.down.weight", f"{attn}.processor.{proj}_lora.up.weight"
            ak = path + ".alpha"
        else:
            p = path[: -len(".0")] if path.endswith(".to_out.0") and spelling == "diffusers" else path
            names = ("lora.down", "lora.up") if spelling == "diffusers" else ("lora_A", "lora_B")
            dk, uk, ak = f"{p}.{names[0]}.weight", f"{p}.{names[1]}.weight", f"{p}.alpha"
        sd[prefix + dk], sd[prefix + uk] = down, up
        if alpha is not None:
            sd[prefix + ak] = torch.tensor(float(alpha))
    return sd


def merged_state_dict(model, loras):
    """the model's state dict with `loras` = [(normalised LoRA, weight)] merged by merge_reference and rounded to fp16 once
    (what the product's fp16 weights hold after `i2v_lora_merge`), as fp32 tensors"""
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    per_path = {}
    for lora, weight in loras:
        for path, (down, up, alpha) in lora.items():
            s = weight * (1.0 if alpha is None else alpha / down.shape[0])
            per_path.setdefault(path, []).append((down, up, s))
    for path, ads in per_path.items():
        key = path + ".weight"
        sd[key] = merge_reference(sd[key], ads).half().float()
    return sd


@contextlib.contextmanager
def merged_oracle(oracle, loras):
    """the oracle carrying the merged weights inside the `with` block; its own weights come back afterwards (bit for bit)"""
    own = {k: v.clone() for k, v in oracle.state_dict().items()}
    oracle.load_state_dict(merged_state_dict(oracle, loras))
    try:
        yield oracle
    finally:
        oracle.load_state_dict(own)
