"""FreeNoise written out literally (not a test): the windows, weights and coefficients in plain Python, the block loop over the
oracle's own BasicTransformerBlock sub-modules in the order of diffusers' FreeNoiseTransformerBlock (slice, per-window attention,
accumulate, divide by the total weight, feed-forward once), an oracle TransformerTemporalModel wrapper and UNet hook using it, and the
noise rescheduling with explicit generators.  Independent of i2v_adapter_unofficial_amd/free_noise.py on purpose."""
import contextlib
import types

import torch


# ------------------------------------------------------------------------------------------------ windows / weights / coefficients
def ref_windows(num_frames, length, stride):
    """[(start, end, first contributing frame)]"""
    if num_frames < length or length < 2 or stride < 1:
        raise ValueError("FreeNoise: bad (num_frames, context_length, context_stride)")
    wins = []
    for s in range(0, num_frames - length + 1, stride):
        wins.append((s, s + length, s))
    last_end = wins[-1][1]
    if last_end < num_frames:
        wins.append((num_frames - length, num_frames, last_end))
    return wins


def ref_weights(length, scheme):
    if scheme == "flat":
        return [1.0] * length
    if scheme == "pyramid":
        if length % 2 == 0:
            mid = length // 2
            return list(map(float, range(1, mid + 1))) + list(map(float, range(mid, 0, -1)))
        mid = (length + 1) // 2
        return list(map(float, range(1, mid))) + [float(mid)] + list(map(float, range(mid - 1, 0, -1)))
    if scheme == "delayed_reverse_sawtooth":
        if length % 2 == 0:
            mid = length // 2
            return [0.01] * (mid - 1) + [float(mid)] + list(map(float, range(mid, 0, -1)))
        mid = (length + 1) // 2
        return [0.01] * (mid - 1) + list(map(float, range(mid, 0, -1)))
    raise ValueError(f"unknown weighting scheme {scheme}")


def ref_coefficients(num_frames, length, stride, scheme):
    """{frame: [(window, position in the window, coefficient in fp64)]}"""
    wins, wt = ref_windows(num_frames, length, stride), ref_weights(length, scheme)
    out = {}
    for f in range(num_frames):
        terms = [(w, f - s, wt[f - s]) for w, (s, e, first) in enumerate(wins) if first <= f < e]
        total = sum(t[2] for t in terms)
        out[f] = [(w, j, v / total) for w, j, v in terms]
    return out


# ------------------------------------------------------------------------------------------------ the block loop
def ref_block_forward(block, hidden_states, length, stride, scheme):
    """oracle.blocks.BasicTransformerBlock (double self-attention, sinusoidal positions) with FreeNoise: hidden_states
    [pixels, F, C].  Every window is sliced out, runs the two attention sub-blocks with positions 0 .. L - 1, and is accumulated with
    its weights into the frames it contributes to; accumulated / total weight; then the feed-forward on all F frames."""
    num_frames = hidden_states.shape[1]
    wins = ref_windows(num_frames, length, stride)
    wt = torch.tensor(ref_weights(length, scheme), dtype=hidden_states.dtype)[None, :, None]
    accumulated = torch.zeros_like(hidden_states)
    total_weight = torch.zeros(1, num_frames, 1, dtype=hidden_states.dtype)
    for start, end, first in wins:
        c = hidden_states[:, start:end]
        n = block.pos_embed(block.norm1(c))
        c = block.attn1(n) + c
        n = block.pos_embed(block.norm2(c))
        c = block.attn2(n) + c
        keep = first - start                                      # the trailing window gives only its last frames
        accumulated[:, first:end] += (c * wt)[:, keep:]
        total_weight[:, first:end] += wt[:, keep:]
    out = accumulated / total_weight
    return block.ff(block.norm3(out)) + out


def ref_temporal_model(model, x, num_frames, length, stride, scheme):
    """oracle.blocks.TransformerTemporalModel.forward with its blocks run by `ref_block_forward`"""
    with hooked_blocks(model, length, stride, scheme):
        return model(x, num_frames=num_frames)[0]


@contextlib.contextmanager
def hooked_blocks(module, length, stride, scheme):
    """every BasicTransformerBlock inside a TransformerTemporalModel under `module` (a motion module, or a whole oracle UNet) runs the
    FreeNoise loop while the context is open (clips of more than `length` frames only, as FreeNoise is defined)"""
    from oracle.blocks import TransformerTemporalModel
    patched = []
    mods = [m for m in module.modules() if isinstance(m, TransformerTemporalModel)]
    for m in mods:
        for blk in m.transformer_blocks:
            def fwd(self, hidden_states, attention_mask=None, encoder_hidden_states=None, **_unused):
                if hidden_states.shape[1] <= length:
                    return type(self).forward(self, hidden_states)
                return ref_block_forward(self, hidden_states, length, stride, scheme)
            blk.forward = types.MethodType(fwd, blk)
            patched.append(blk)
    try:
        yield len(patched)
    finally:
        for blk in patched:
            del blk.forward


# ------------------------------------------------------------------------------------------------ noise
def ref_noise(shape, length, stride, noise_type, seed):
    """(noise [B, F, ...], sources): sources[f] = the frame < L that frame f's noise is a copy of"""
    g = torch.Generator().manual_seed(seed)
    b, num_frames = shape[0], shape[1]
    if noise_type == "random":
        return torch.randn(shape, generator=g, dtype=torch.float32), list(range(num_frames))
    first = torch.randn((b, length) + tuple(shape[2:]), generator=g, dtype=torch.float32)
    src = list(range(length))
    if noise_type == "repeat_context":
        src = [f % length for f in range(num_frames)]
    elif noise_type == "shuffle_context":
        src += [None] * (num_frames - length)
        for i in range(length, num_frames, stride):
            lo, hi = i - length, min(num_frames, i - length + stride)
            perm = torch.randperm(hi - lo, generator=g).tolist()
            for k, p in enumerate(perm):
                if i + k < num_frames:
                    src[i + k] = src[lo + p]
    else:
        raise ValueError(noise_type)
    return first[:, src].contiguous(), src
