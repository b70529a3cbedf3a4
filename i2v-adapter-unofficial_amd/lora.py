"""LoRA for the UNet (the reference pipeline's LoraLoaderMixin / its UNet's UNet2DConditionLoadersMixin, pipe:57, unet:108):
`load_lora_weights`, `set_adapters`, `fuse_lora` / `unfuse_lora` and the per-call `cross_attention_kwargs={"scale": s}`.

The adapters are MERGED into the weights (one `i2v_lora_merge` launch per targeted weight) instead of run beside every
GEMM: the fused kernels take packed weights, `HipModule.packed()` rebuilds a pack when its parameter's version changes and the
pipeline's graph key hashes the same versions, so a merged LoRA costs nothing per denoising step.

  * reading:  `read_lora_file` (a .safetensors / .bin file or a dict) -> `parse_lora_state_dict` (pure, no GPU): the diffusers, old
    attention-processor, PEFT and kohya key spellings -> {module path: (down, up, alpha or None)} + a report.  Text-encoder keys are
    skipped and counted (CLIP is out of scope).  Factors are kept on the device in fp16: a file in fp32 or bf16 is rounded
    ONCE when it is loaded.  The effective scale of a layer is alpha / rank where the file has an alpha, else 1.
  * state:    `UNetLoraMixin` on UNetMotionCrossFrameAttnModel: named adapters, the active names with their weights, one global scale
    and, for every targeted parameter, a STASH of its original values (a device clone in the parameter's dtype; a plain attribute, not
    a buffer: state-dict keys do not change).  Every change only marks the state dirty; `_sync_lora()` -- at the top of every entry
    point that reads weights -- re-merges each targeted parameter FROM ITS STASH with scale_j = adapter weight x global scale x
    alpha / rank, so the result never depends on what was merged before, and restores a parameter no active adapter touches any more
    with `copy_` from the stash: unloading is bit-exact.  (Weights loaded into a targeted parameter while a LoRA is loaded --
    `load_state_dict`, an optimiser step -- are overwritten by the next merge: unload first; training refuses, training.py.
    Reads see the merged values too: `state_dict()`, `save_pretrained`, `save_i2v_adapter_modules` / `save_motion_modules` and
    `sharding.broadcast_model_weights` with a LoRA merged write or send the MERGED weights, not the originals -- what `fuse_lora`
    is for when it is wanted, and a reason to `unload_lora()` first when it is not.)
"""
import os
import re
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from ._lib import I2V_LORA_MAX_ADAPTERS, I2V_LORA_MAX_RANK, HipLibraryError

f16 = torch.float16

_TE_PREFIXES = ("text_encoder.", "text_encoder_2.", "lora_te_", "lora_te1_", "lora_te2_")
# (suffix pattern, which factor): down = lora_A, up = lora_B
_SUFFIXES = (
    (re.compile(r"^(.*)\.lora\.(down|up)\.weight$"), None),
    (re.compile(r"^(.*)\.lora_(A|B)(?:\.[^.]+)?\.weight$"), None),
    (re.compile(r"^(.*)\.lora_(down|up)\.weight$"), None),
    (re.compile(r"^(.*)\.processor\.(to_q|to_k|to_v|to_out)_lora\.(down|up)\.weight$"), "processor"),
)
_WHICH = {"down": 0, "A": 0, "up": 1, "B": 1}


def lora_target_shapes(model: nn.Module) -> Dict[str, Tuple[int, ...]]:
    """{module path: weight shape} of everything a LoRA may target: every nn.Linear and nn.Conv2d of the model (attention projections
    of the spatial, cross-frame-adapter and motion-module blocks, feed-forwards, proj_in / proj_out, resnet convs, time_emb_proj,
    down- and up-samplers, ...)."""
    return {name: tuple(m.weight.shape) for name, m in model.named_modules()
            if name and isinstance(m, (nn.Linear, nn.Conv2d))}


def kohya_name_table(paths) -> Dict[str, str]:
    """kohya flattens a module path by writing `_` for `.`: {flattened: path} over the model's own module names.  Two paths that
    flatten to one name would make a kohya key ambiguous: asserted."""
    table = {}
    for p in paths:
        flat = p.replace(".", "_")
        assert flat not in table, f"kohya names are ambiguous for this model: {table[flat]!r} and {p!r} both flatten to {flat!r}"
        table[flat] = p
    return table


def read_lora_file(pretrained_model_name_or_path_or_dict, weight_name: Optional[str] = None, subfolder: Optional[str] = None) -> dict:
    """a LoRA state dict from a dict (returned as it is), a .safetensors file or a torch .bin / .pt file; `subfolder` and
    `weight_name` are joined to the path as `load_ip_adapter` does."""
    if isinstance(pretrained_model_name_or_path_or_dict, dict):
        return pretrained_model_name_or_path_or_dict
    path = pretrained_model_name_or_path_or_dict
    if subfolder:
        path = os.path.join(path, subfolder)
    if weight_name:
        path = os.path.join(path, weight_name)
    if not os.path.isfile(path):
        raise EnvironmentError(f"LoRA weights not found at {path}")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    return torch.load(path, map_location="cpu", weights_only=True)


def parse_lora_state_dict(state_dict: dict, target_shapes: Dict[str, Tuple[int, ...]]):
    """{key: tensor} in any accepted spelling -> ({module path: (down [rank, in] , up [out, rank], alpha or None)}, report).
    Pure: no GPU, tensors keep their device and dtype (2-D views of the file's tensors).  Accepted, each with an optional `unet.`:
      diffusers   <path>.lora.down.weight / .lora.up.weight            PEFT   <path>.lora_A[.<name>].weight / .lora_B[.<name>].weight
      old         <attention>.processor.to_q_lora.down.weight ...       kohya  lora_unet_<path with _ for .>.lora_down.weight /
      alpha       <path>.alpha beside any of them                              .lora_up.weight / .alpha
    `to_out` means `to_out.0`.  Text-encoder keys are skipped and counted in report["text_encoder_keys"].  A UNet key that names no
    nn.Linear / nn.Conv2d of the model, a factor without its partner, or factors that do not fit the weight raise ValueError naming
    the key."""
    table = None
    found: Dict[str, list] = {}
    report = {"text_encoder_keys": 0, "unet_keys": 0}

    def resolve(path, key):
        if path in target_shapes:
            return path
        if path.endswith(".to_out") and path + ".0" in target_shapes:
            return path + ".0"
        raise ValueError(f"LoRA key {key!r} matches no Linear / conv module of the UNet (looked for {path!r})")

    for key, t in state_dict.items():
        if key.startswith(_TE_PREFIXES):
            report["text_encoder_keys"] += 1
            continue
        k = key[len("unet."):] if key.startswith("unet.") else key
        kohya = k.startswith("lora_unet_")
        if kohya:
            k = k[len("lora_unet_"):]
        which = path = None
        if k.endswith(".alpha"):
            path, which = k[: -len(".alpha")], 2
        else:
            for rx, kind in _SUFFIXES:
                m = rx.match(k)
                if m:
                    if kind == "processor":
                        path, which = f"{m.group(1)}.{m.group(2)}", _WHICH[m.group(3)]
                    else:
                        path, which = m.group(1), _WHICH[m.group(2)]
                    break
        if path is None:
            raise ValueError(f"LoRA key {key!r} is in no known spelling (diffusers, attention-processor, PEFT, kohya)")
        if kohya:
            if table is None:
                table = kohya_name_table(target_shapes)
            if path in table:
                path = table[path]
            elif path.endswith("_to_out") and path + "_0" in table:
                path = table[path + "_0"]
            else:
                raise ValueError(f"LoRA key {key!r} matches no Linear / conv module of the UNet (kohya name {path!r})")
        else:
            path = resolve(path, key)
        slot = found.setdefault(path, [None, None, None, [None, None, None]])
        if slot[which] is not None:
            raise ValueError(f"LoRA key {key!r} repeats {slot[3][which]!r} in another spelling")
        slot[which], slot[3][which] = t, key
        report["unet_keys"] += 1

    out = {}
    for path, (down, up, alpha, keys) in found.items():
        if down is None or up is None:
            have = next(k for k in keys if k is not None)
            raise ValueError(f"LoRA key {have!r}: {path!r} has no {'down' if down is None else 'up'} factor")
        shape = target_shapes[path]
        n_out, n_in = shape[0], 1
        for s in shape[1:]:
            n_in *= s
        rank = down.shape[0] if down.dim() >= 2 else 0
        if rank < 1 or down.numel() != rank * n_in:
            raise ValueError(f"LoRA key {keys[0]!r}: down factor {tuple(down.shape)} does not fit the weight {shape} of {path!r}")
        if up.dim() < 2 or up.shape[0] != n_out or up.numel() != n_out * rank:
            raise ValueError(f"LoRA key {keys[1]!r}: up factor {tuple(up.shape)} does not fit the weight {shape} of {path!r} at rank {rank}")
        if alpha is not None:
            alpha = float(alpha.reshape(-1)[0]) if torch.is_tensor(alpha) else float(alpha)
        out[path] = (down.reshape(rank, n_in), up.reshape(n_out, rank), alpha)
    return out, report


class UNetLoraMixin:
    """LoRA state and its merge for a model whose Linear / conv weights feed version-keyed packs (module docstring)."""

    def _lora_state(self):
        st = self.__dict__.get("_lora")
        if st is None:
            st = dict(adapters={}, active={}, scale=1.0, stash={}, epoch=0, merged=None, fused=False)
            self.__dict__["_lora"] = st
        return st

    def _lora_wanted(self):
        st = self._lora_state()
        # (the active adapters IN ORDER: the merge sums them in this order in fp32, so the merged weights are a function of this key)
        return (st["epoch"], tuple(st["active"].items()), float(st["scale"]))

    def has_lora(self) -> bool:
        st = self.__dict__.get("_lora")
        return bool(st and (st["adapters"] or st["stash"]))

    def lora_parameter_names(self):
        """state-dict names of the parameters that carry LoRA state (a stash): what a trainer must not write in place"""
        st = self.__dict__.get("_lora")
        return [] if not st else [p + ".weight" for p in st["stash"]]

    # ------------------------------------------------------------------ the public surface
    def load_lora(self, pretrained_model_name_or_path_or_dict, adapter_name: Optional[str] = None, weight_name: Optional[str] = None,
                  subfolder: Optional[str] = None):
        """read a LoRA (file or dict, any accepted spelling), keep its factors on the device in fp16 under `adapter_name` (default
        `default_<n>`) and make it active with weight 1 beside the adapters already active.  Returns the parser's report plus the
        adapter's name and the number of targeted modules.  The merge happens at the next forward (`_sync_lora`)."""
        st = self._lora_state()
        if st["fused"]:
            raise ValueError("a fused LoRA is in the weights (fuse_lora): call unfuse_lora() before loading another")
        dev = self.device
        if dev.type != "cuda":
            raise HipLibraryError(f"the UNet is on {dev}: LoRA factors and stashes live on the device (there is no CPU path)")
        sd = read_lora_file(pretrained_model_name_or_path_or_dict, weight_name=weight_name, subfolder=subfolder)
        entries, report = parse_lora_state_dict(sd, lora_target_shapes(self))
        if not entries:
            raise ValueError("the LoRA holds no UNet keys" + (f" ({report['text_encoder_keys']} text-encoder keys were skipped)"
                                                              if report["text_encoder_keys"] else ""))
        if adapter_name is None:
            n = len(st["adapters"])
            while f"default_{n}" in st["adapters"]:
                n += 1
            adapter_name = f"default_{n}"
        if adapter_name in st["adapters"]:
            raise ValueError(f"adapter {adapter_name!r} is already loaded: delete_adapters({adapter_name!r}) first")
        modules = dict(self.named_modules())
        held = {}
        for path, (down, up, alpha) in entries.items():
            rank = down.shape[0]
            if rank > I2V_LORA_MAX_RANK:
                raise ValueError(f"LoRA for {path!r} has rank {rank}: at most {I2V_LORA_MAX_RANK}")
            held[path] = (down.to(dev, f16).contiguous(), up.to(dev, f16).contiguous(), 1.0 if alpha is None else alpha / rank)
        with torch.no_grad():
            for path in held:
                if path not in st["stash"]:
                    st["stash"][path] = modules[path].weight.detach().clone()
        st["adapters"][adapter_name] = held
        st["active"][adapter_name] = 1.0
        st["epoch"] += 1
        report = dict(report, adapter_name=adapter_name, modules=len(held))
        return report

    def set_adapters(self, adapter_names, adapter_weights=None):
        """the active adapters and their weights (one name or a list; weights default to 1)"""
        st = self._lora_state()
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        if adapter_weights is None:
            weights = [1.0] * len(names)
        elif isinstance(adapter_weights, (int, float)):
            weights = [float(adapter_weights)] * len(names)
        else:
            weights = [float(w) for w in adapter_weights]
        if len(weights) != len(names) or len(set(names)) != len(names):
            raise ValueError(f"{len(names)} adapter names (distinct) need {len(names)} weights, got {len(weights)}")
        for n in names:
            if n not in st["adapters"]:
                raise ValueError(f"adapter {n!r} is not loaded (loaded: {sorted(st['adapters'])})")
        st["active"] = dict(zip(names, weights))

    def get_active_adapters(self):
        return list(self._lora_state()["active"])

    def delete_adapters(self, adapter_names):
        st = self._lora_state()
        for n in ([adapter_names] if isinstance(adapter_names, str) else list(adapter_names)):
            if n not in st["adapters"]:
                raise ValueError(f"adapter {n!r} is not loaded (loaded: {sorted(st['adapters'])})")
            del st["adapters"][n]
            st["active"].pop(n, None)
        st["epoch"] += 1

    def unload_lora(self):
        """drop every adapter (and a fused one): the parameters get their original values back bit for bit and the stashes are freed"""
        st = self._lora_state()
        st["adapters"], st["active"], st["fused"] = {}, {}, False
        st["epoch"] += 1
        self._sync_lora()

    def set_lora_scale(self, scale: float) -> float:
        """the global scale (`cross_attention_kwargs={"scale": s}`); returns the previous one"""
        st = self._lora_state()
        prev, st["scale"] = st["scale"], float(scale)
        return prev

    def fuse_lora(self, lora_scale: float = 1.0):
        """merge the active adapters now at `lora_scale` and drop the factors; the stashes stay, so `unfuse_lora` restores the
        original weights exactly"""
        st = self._lora_state()
        if not st["adapters"]:
            raise ValueError("fuse_lora: no LoRA is loaded")
        prev = self.set_lora_scale(lora_scale)
        try:
            self._sync_lora()
        finally:
            st["scale"] = prev
        fused = {p for n in st["active"] for p in st["adapters"][n]}
        with torch.no_grad():
            modules = dict(self.named_modules())
            for path in [p for p in st["stash"] if p not in fused]:      # (targeted only by adapters that were not active)
                modules[path].weight.copy_(st["stash"].pop(path))
        st["adapters"], st["active"], st["fused"] = {}, {}, True
        st["epoch"] += 1
        st["merged"] = self._lora_wanted()

    def unfuse_lora(self):
        st = self._lora_state()
        if not st["fused"]:
            raise ValueError("unfuse_lora: no fused LoRA")
        st["fused"] = False
        st["epoch"] += 1
        self._sync_lora()

    # ------------------------------------------------------------------ the merge
    @torch.no_grad()
    def _sync_lora(self):
        """bring the weights to the wanted state (module docstring); a no-op when they are there already"""
        st = self.__dict__.get("_lora")
        if st is None or not st["stash"]:
            return
        wanted = self._lora_wanted()
        if st["merged"] == wanted or st["fused"]:
            return
        from . import kernels as K
        touched = {}
        for name, w in st["active"].items():
            for path, (down, up, layer_scale) in st["adapters"][name].items():
                touched.setdefault(path, []).append((down, up, w * st["scale"] * layer_scale))
        for path, ads in touched.items():
            if len(ads) > I2V_LORA_MAX_ADAPTERS:
                raise ValueError(f"{len(ads)} active adapters target {path!r}: at most {I2V_LORA_MAX_ADAPTERS} in one merge")
        loaded = {p for held in st["adapters"].values() for p in held}
        modules = dict(self.named_modules())
        for path in list(st["stash"]):
            w, stash = modules[path].weight, st["stash"][path]
            if stash.device != w.device or stash.dtype != w.dtype or stash.shape != w.shape:
                raise RuntimeError(f"the LoRA stash of {path!r} no longer matches its parameter ({stash.dtype} {stash.device} vs "
                                   f"{w.dtype} {w.device})")
            if path in touched:
                if not w.is_contiguous():
                    raise RuntimeError(f"{path}.weight is not contiguous")
                K.lora_merge(w, stash, touched[path])
            else:
                w.copy_(stash)
            if path not in loaded:
                del st["stash"][path]
        st["merged"] = wanted

    def _apply(self, fn, *args, **kwargs):
        """`.to(device / dtype)`, `.half()`, `.cuda()` with a LoRA loaded: the stashes go through the same function as the parameters
        (they keep the parameters' dtype), the factors move to the parameters' device and stay fp16; the next forward merges again."""
        out = super()._apply(fn, *args, **kwargs)
        st = self.__dict__.get("_lora")
        if st and st["stash"]:
            dev = next(self.parameters()).device
            st["stash"] = {p: fn(t) for p, t in st["stash"].items()}
            st["adapters"] = {n: {p: (d.to(dev), u.to(dev), s) for p, (d, u, s) in held.items()} for n, held in st["adapters"].items()}
            if st["fused"]:
                pass            # (the fused weights went through fn with the parameters)
            else:
                st["merged"] = None
        return out


def check_not_trained(unet, trained_names):
    """training.py: a trainer over parameters that carry LoRA state would have its in-place updates overwritten by the next merge
    (the stash holds the values from before the LoRA) -- refuse."""
    names = set(getattr(unet, "lora_parameter_names", lambda: [])())
    hit = sorted(n for n in trained_names if n in names)
    if hit:
        raise RuntimeError(f"{len(hit)} trained parameters carry LoRA state (first: {hit[0]!r}): the optimiser writes them in place and "
                           "the LoRA's stash of their original values would go stale -- call unet.unload_lora() (or fuse the LoRA into a "
                           "checkpoint) before training")
