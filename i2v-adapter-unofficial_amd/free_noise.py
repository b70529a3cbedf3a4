"""FreeNoise (https://arxiv.org/abs/2310.15169; diffusers AnimateDiffFreeNoiseMixin.enable_free_noise, FreeNoiseTransformerBlock): the host
side -- settings, the sliding windows, their weights, the normalised blend coefficients as device tables, and the rescheduled
initial noise.  The device side is two row movers (csrc/freenoise.hip) around the unchanged attention kernels (blocks.py
`TemporalTransformerBlock._fwd_windows`).

With F = num_frames, L = context_length, S = context_stride:
  windows       starts range(0, F - L + 1, S); when the last of them ends before F, one trailing window [F - L, F) that contributes only
                to the frames no other window covers (it is still computed over all of its L frames)
  weights       over the position j in a window: "flat" 1; "pyramid" 1, 2, .., peak, .., 2, 1 (the peak twice for even L);
                "delayed_reverse_sawtooth" 0.01 up to the middle, then L/2 (twice for even L) down to 1
  coefficients  a[f][w] = weight[f - s_w] / (sum of the weights of the windows that contribute to f): fp64 on the host, rounded to
                fp32; a frame with one contributing window has exactly 1.0
"""
import collections
import math

import torch

WEIGHTING_SCHEMES = ("flat", "pyramid", "delayed_reverse_sawtooth")
NOISE_TYPES = ("shuffle_context", "repeat_context", "random")

FreeNoiseSettings = collections.namedtuple("FreeNoiseSettings", "context_length context_stride weighting_scheme noise_type")


def check_free_noise_args(context_length, context_stride, weighting_scheme, noise_type, max_length):
    """the checks of `enable_free_noise` (num_frames is checked in the call: `check_num_frames`); returns the settings"""
    for name, v in (("context_length", context_length), ("context_stride", context_stride)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"`{name}` must be an integer, got {v!r}")
    length, stride = int(context_length), int(context_stride)
    if length < 2:
        raise ValueError(f"`context_length` must be at least 2, got {length}")
    if length > max_length:
        raise ValueError(f"`context_length` {length} exceeds the motion modules' num_positional_embeddings ({max_length})")
    if stride < 1:
        raise ValueError(f"`context_stride` must be at least 1, got {stride}")
    if weighting_scheme not in WEIGHTING_SCHEMES:
        raise ValueError(f"`weighting_scheme` must be one of {WEIGHTING_SCHEMES}, got {weighting_scheme!r}")
    if noise_type not in NOISE_TYPES:
        raise ValueError(f"`noise_type` must be one of {NOISE_TYPES}, got {noise_type!r}")
    return FreeNoiseSettings(length, stride, weighting_scheme, noise_type)


def check_num_frames(num_frames, settings):
    if num_frames < settings.context_length:
        raise ValueError(f"FreeNoise: num_frames {num_frames} is below `context_length` {settings.context_length}")


def windows(num_frames, length, stride):
    """[(start, first contributing frame, end)]: window w covers [start, start + length) and contributes to [first, end)"""
    if length < 2 or stride < 1 or num_frames < length:
        raise ValueError(f"FreeNoise windows: num_frames {num_frames}, context_length {length}, context_stride {stride}")
    out = [(s, s, s + length) for s in range(0, num_frames - length + 1, stride)]
    last_end = out[-1][2]
    if last_end < num_frames:
        out.append((num_frames - length, last_end, num_frames))
    return out


def weights(length, scheme):
    if scheme == "flat":
        return [1.0] * length
    half, odd = length // 2, length % 2
    up = [float(v) for v in range(1, half + 1)]
    if scheme == "pyramid":
        return up + ([float(half + 1)] if odd else []) + up[::-1]
    if scheme == "delayed_reverse_sawtooth":
        if odd:
            m = half + 1
            return [0.01] * (m - 1) + [float(v) for v in range(m, 0, -1)]
        return [0.01] * (half - 1) + [float(half)] + [float(v) for v in range(half, 0, -1)]
    raise ValueError(f"`weighting_scheme` must be one of {WEIGHTING_SCHEMES}, got {scheme!r}")


def coefficients(num_frames, length, stride, scheme):
    """(starts, idx, coef): starts [windows]; per frame the padded lists idx[f] (row w * length + j of the window-major layout) and
    coef[f] (the fp64 quotients; `tables` rounds them to fp32; padding: index 0, coefficient 0)"""
    wins, wt = windows(num_frames, length, stride), weights(length, scheme)
    per_frame = [[] for _ in range(num_frames)]
    for w, (s, first, end) in enumerate(wins):
        for f in range(first, end):
            per_frame[f].append((w * length + f - s, wt[f - s]))
    pairs = max(len(p) for p in per_frame)
    idx, coef = [], []
    for p in per_frame:
        total = math.fsum(v for _, v in p)
        idx.append([i for i, _ in p] + [0] * (pairs - len(p)))
        coef.append([v / total for _, v in p] + [0.0] * (pairs - len(p)))
    return [s for s, _, _ in wins], idx, coef


_TABLES = {}


def tables(num_frames, settings, device):
    """(starts int32 [windows], idx int32 [F, pairs], coef fp32 [F, pairs]) on `device`, made once per (F, L, S, scheme) and kept:
    a captured step reads them on every replay.  The three are views of ONE 4-byte-per-element device block (`persistent_tables`)."""
    key = (str(device), num_frames, settings.context_length, settings.context_stride, settings.weighting_scheme)
    tab = _TABLES.get(key)
    if tab is None:
        starts, idx, coef = coefficients(num_frames, settings.context_length, settings.context_stride, settings.weighting_scheme)
        n_w, n_p = len(starts), num_frames * len(idx[0])
        host = torch.empty(n_w + 2 * n_p, dtype=torch.float32)
        host[:n_w].view(torch.int32).copy_(torch.tensor(starts, dtype=torch.int32))
        host[n_w: n_w + n_p].view(torch.int32).copy_(torch.tensor(idx, dtype=torch.int32).reshape(-1))
        host[n_w + n_p:].copy_(torch.tensor(coef, dtype=torch.float64).to(torch.float32).reshape(-1))    # fp64 -> fp32: one rounding
        block = host.to(device)
        tab = _TABLES[key] = (block[:n_w].view(torch.int32), block[n_w: n_w + n_p].view(torch.int32).view(num_frames, -1),
                              block[n_w + n_p:].view(num_frames, -1), block)
    return tab[:3]


def persistent_tables(device):
    """name -> the device block behind every table set cached for `device` (handle.persistent_tensors: a launch plan names the block
    it reads like a weight, as fp32 -- the registry knows fp16 and fp32 -- although its first two parts hold int32 bits: a host
    uploads it byte for byte)"""
    return {f"free_noise#{f}.{l}.{s}.{scheme}": tab[3] for (d, f, l, s, scheme), tab in _TABLES.items() if d == str(device)}


def _randperm(n, generator):
    gdev = generator.device if generator is not None else torch.device("cpu")
    return torch.randperm(n, generator=generator, device=gdev).tolist()


def _reschedule_one(draw, shape, settings, generator):
    b, num_frames = shape[0], shape[1]
    length, stride = settings.context_length, settings.context_stride
    first = draw((b, length) + tuple(shape[2:]), generator)
    if settings.noise_type == "repeat_context":
        return first.repeat((1, -(-num_frames // length)) + (1,) * (len(shape) - 2))[:, :num_frames].contiguous()
    noise = first.new_empty(tuple(shape))
    noise[:, :length] = first
    for i in range(length, num_frames, stride):              # permutations: on the host, after the L-frame draw
        lo, hi = i - length, min(num_frames, i - length + stride)
        order = [lo + k for k in _randperm(hi - lo, generator)]
        n = min(num_frames, i + len(order)) - i
        noise[:, i: i + n] = noise[:, order[:n]]
    return noise


def reschedule_noise(draw, shape, settings, generator):
    """the initial noise [B, F, ...] of a FreeNoise call.  draw(shape, generator) -> one seeded normal draw (a single generator or
    None).  "random": all F frames; "repeat_context": L frames tiled along the frame axis and cut to F; "shuffle_context": L frames,
    then for i in range(L, F, S) the frames [i - L, min(F, i - L + S)) in a random order written to [i, ...), cut to fit.  A list of
    generators draws (and shuffles) one sample per generator."""
    if isinstance(generator, (list, tuple)):
        if len(generator) != shape[0]:
            raise ValueError(f"{len(generator)} generators for a batch of {shape[0]}")
        return torch.cat([reschedule_noise(draw, (1,) + tuple(shape[1:]), settings, g) for g in generator], dim=0)
    check_num_frames(shape[1], settings)
    if settings.noise_type == "random" or shape[1] == settings.context_length:
        return draw(tuple(shape), generator)
    return _reschedule_one(draw, tuple(shape), settings, generator)
