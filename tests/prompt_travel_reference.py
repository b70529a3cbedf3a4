"""Prompt travel, restated: the specification the package's `prompt_travel.py`, `I2VAdapterPipeline.encode_prompt_travel` and
`i2v_interp_rows_f16` are tested against (tests/test_prompt_travel.py, tests/test_prompt_travel_gpu.py).

Semantics (diffusers 0.30 AnimateDiffFreeNoiseMixin `_encode_prompt_free_noise`, restated from memory; this file is the specification):
  * a prompt is a str or a dict {int frame: str}; sorted, the first key is 0 and the last is < num_frames; anything else is a ValueError
    that names the offending key;
  * if the last key is not num_frames - 1 the last prompt is held to the end of the clip;
  * between consecutive keyframes s < e, frame f gets (1 - w) E_s + w E_e with w = float32(linspace(0, 1, e - s + 1)[f - s]);
  * a keyframe's own frame gets its embedding exactly;
  * an interpolation callback (start_frame, end_frame, start_embeds, end_embeds) -> [e - s + 1, L, D] replaces the linear rule of that
    segment; segments are written in order, so a later segment's first row overwrites the shared keyframe's.

Written frame by frame, with no table arithmetic shared with the package.  The fp64 evaluation and the per-element error bound of the
kernel are here too, and the oracle UNet that takes one context per frame."""
import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------------- keyframes
def keyframes(prompt, num_frames):
    """sorted keys of a valid keyframe dict; ValueError whose text holds repr(key) of the offending key"""
    if not isinstance(prompt, dict) or len(prompt) == 0:
        raise ValueError("a keyframe dict with at least the key 0 is required")
    for k, v in prompt.items():
        if type(k) is not int:
            raise ValueError(f"key {k!r} is not an int")
        if type(v) is not str:
            raise ValueError(f"the value of key {k!r} is not a str")
    keys = sorted(prompt)
    if keys[0] != 0:
        raise ValueError(f"first key {keys[0]!r} is not 0")
    if keys[-1] >= num_frames:
        raise ValueError(f"last key {keys[-1]!r} is not below num_frames {num_frames}")
    return keys


def frame_sources(keys, num_frames):
    """per frame (index of the keyframe below, index of the keyframe above, float32 weight of the one above), by the rules above,
    one frame at a time.  Indices count the sorted keys."""
    out = []
    for f in range(num_frames):
        if f in keys:
            i = keys.index(f)
            out.append((i, i, np.float32(0.0)))
            continue
        below = max(i for i, k in enumerate(keys) if k < f)
        if below == len(keys) - 1:                               # behind the last keyframe: its prompt is held
            out.append((below, below, np.float32(0.0)))
            continue
        s, e = keys[below], keys[below + 1]
        out.append((below, below + 1, np.float32(np.linspace(0.0, 1.0, e - s + 1)[f - s])))
    return out


def batch_frame_sources(key_lists, num_frames, repeats=1):
    """(lo, hi, w) over a batch whose keyframe embeddings follow each other in one source matrix; every sample `repeats` times"""
    lo, hi, w, base = [], [], [], 0
    for keys in key_lists:
        rows = [(base + a, base + b, ww) for a, b, ww in frame_sources(keys, num_frames)]
        for _ in range(repeats):
            for a, b, ww in rows:
                lo.append(a), hi.append(b), w.append(ww)
        base += len(keys)
    return np.array(lo, dtype=np.int64), np.array(hi, dtype=np.int64), np.array(w, dtype=np.float32)


def interpolate(embeds, keys, num_frames, callback=None):
    """[num_frames, ...] float64: the per-frame embeddings of ONE sample from its keyframes' `embeds` [len(keys), ...] (any float
    dtype), evaluated in float64 with the float32 weights; `callback` as the module docstring says"""
    e64 = embeds.double()
    out = torch.empty((num_frames,) + tuple(embeds.shape[1:]), dtype=torch.float64)
    for f, (a, b, w) in enumerate(frame_sources(keys, num_frames)):
        out[f] = e64[a] if a == b else (1.0 - float(w)) * e64[a] + float(w) * e64[b]
    if callback is not None:
        for i, (s, e) in enumerate(zip(keys[:-1], keys[1:])):
            out[s:e + 1] = callback(s, e, embeds[i], embeds[i + 1]).double()
    return out


# ---------------------------------------------------------------------------------------------------------- the kernel's yardstick
def interp_rows_ref64(src, lo, hi, w):
    """float64 rows (1 - w) src[lo] + w src[hi]; a row with w == 0 (w == 1) is src[lo] (src[hi]) alone, so a NaN in the other does not
    count"""
    s = src.double()
    rows = []
    for a, b, ww in zip(lo, hi, w):
        ww = float(np.float32(ww))
        rows.append(s[int(a)] if ww == 0.0 else (s[int(b)] if ww == 1.0 else (1.0 - ww) * s[int(a)] + ww * s[int(b)]))
    return torch.stack(rows)


def interp_rows_bound(src, lo, hi, w):
    """per element: |out - ref64| <= 2^-11 |ref| + 2^-22 (|(1 - w) x| + |w y|) + 2^-25.
    One rounding of the fp32 result to fp16 costs half an ulp, 2^-11 relative for a normal result; a result below fp16's normal range
    is rounded to a multiple of the least subnormal 2^-24, at most half of it, 2^-25, away.  In fp32 the kernel rounds 1 - w, one
    product and the fused multiply-add: three roundings of 2^-24 relative on terms no larger than |(1 - w) x| + |w y|, and the fp16
    rounding then acts on a value that far from the exact one -- 2^-22 covers both with room (4 x 2^-24)."""
    s = src.double()
    w64 = torch.tensor([float(np.float32(v)) for v in w], dtype=torch.float64).view(-1, *([1] * (src.dim() - 1)))
    x, y = s[torch.as_tensor(lo, dtype=torch.long)], s[torch.as_tensor(hi, dtype=torch.long)]
    x = torch.where(w64 == 1.0, torch.zeros_like(x), x)           # the row that is not read
    y = torch.where(w64 == 0.0, torch.zeros_like(y), y)
    ref = (1.0 - w64) * x + w64 * y
    return 2.0 ** -11 * ref.abs() + 2.0 ** -22 * (((1.0 - w64) * x).abs() + (w64 * y).abs()) + 2.0 ** -25


def check_interp_rows(out, src, lo, hi, w):
    """(worst error / bound, passed) of an fp16 result against the fp64 reference"""
    ref = interp_rows_ref64(src, lo, hi, w)
    bound = interp_rows_bound(src, lo, hi, w)
    err = (out.double() - ref).abs()
    ok = torch.isfinite(out.double()).all().item() and bool((err <= bound).all())
    return float((err / bound).max()), ok


# ---------------------------------------------------------------------------------------------------------- the oracle, per frame
class _AlreadyPerFrame(torch.Tensor):
    """a context that holds one row per frame already: the oracle UNet's `repeat_interleave(num_frames)` leaves it as it is"""

    def repeat_interleave(self, *args, **kwargs):
        return self.as_subclass(torch.Tensor)


def per_frame_oracle_unet_class():
    """the oracle's UNet taking `encoder_hidden_states` [B * F, L, D], one context per frame in the order of the frames of `sample`:
    only the unconditional per-frame repeat of the context (unet:1355) is overridden -- the oracle's blocks take one context row per
    frame as they stand.  With an IP-Adapter the projected image tokens, one set per sample, are repeated per frame and appended, which
    is what the repeat did to them."""
    from oracle.unet_motion_cross_frame_attn import UNetMotionCrossFrameAttnModel as Base

    class PerFrameContextUNet(Base):
        def forward(self, sample, timestep, enable_cross_frame_attn, encoder_hidden_states, added_cond_kwargs=None, **kw):
            frames = sample.shape[1]
            ctx = encoder_hidden_states
            assert ctx.shape[0] == sample.shape[0] * frames, "one context per frame"
            proj, kind = self.encoder_hid_proj, self.config.encoder_hid_dim_type
            if proj is not None and kind == "ip_image_proj":
                image = proj(added_cond_kwargs["image_embeds"]).to(ctx.dtype)
                ctx = torch.cat([ctx, torch.repeat_interleave(image, frames, dim=0)], dim=1)
            self.encoder_hid_proj = None                        # (the context holds the image tokens already)
            try:
                return super().forward(sample, timestep, enable_cross_frame_attn, ctx.as_subclass(_AlreadyPerFrame), **kw)
            finally:
                self.encoder_hid_proj = proj

    return PerFrameContextUNet


def oracle_small_unet_per_frame(seed=1234, ip=False):
    """tests/parity.oracle_small_unet with the per-frame class: the same weights for the same seed"""
    from tests.parity import SMALL_UNET, randomize_adapter_out_, round_fp16_, small_ip_state_dict
    torch.manual_seed(seed)
    m = per_frame_oracle_unet_class()(**SMALL_UNET)
    randomize_adapter_out_(m)
    ipsd = None
    if ip:
        ipsd = small_ip_state_dict(m)
        ipsd = {k: {kk: vv.half().float() for kk, vv in v.items()} for k, v in ipsd.items()}
        m._load_ip_adapter_weights(ipsd)
    return round_fp16_(m).eval(), ipsd
