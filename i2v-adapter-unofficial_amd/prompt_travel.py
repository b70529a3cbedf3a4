"""Prompt travel: keyframed prompts, one text context per frame (diffusers AnimateDiffFreeNoiseMixin, `prompt` as a dict
{frame_index: text}; `_encode_prompt_free_noise` of diffusers 0.30, restated in tests/prompt_travel_reference.py).

Host side only: the rules of a keyframe dict, the forms `prompt` / `negative_prompt` may take, and the (lo, hi, w) tables of the one
`i2v_interp_rows_f16` launch that makes every frame's embedding from the K encoded keyframe prompts:
    frame f between the keyframes s < e:   (1 - w) E_s + w E_e,   w = float32(linspace(0, 1, e - s + 1)[f - s])
a keyframe's own frame gets its embedding exactly (w = 0 on its own row), and the last prompt is held to the end of the clip."""
import numpy as np


def check_keyframes(prompt, num_frames, name="prompt"):
    """the sorted keys of a keyframe dict {int frame: str}: the first is 0, the last < num_frames.  ValueError naming the offending key
    otherwise."""
    if not isinstance(prompt, dict):
        raise ValueError(f"`{name}` must be a dict {{frame: text}}, got {type(prompt).__name__}")
    if len(prompt) == 0:
        raise ValueError(f"`{name}` is an empty dict: it needs at least the key 0")
    for k, v in prompt.items():
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"`{name}`: key {k!r} is not an int (the keys of a keyframe dict are frame indices)")
        if not isinstance(v, str):
            raise ValueError(f"`{name}`: the value of key {k!r} is {type(v).__name__}, not a str")
    keys = sorted(int(k) for k in prompt)
    if keys[0] != 0:
        raise ValueError(f"`{name}`: the first key is {keys[0]!r}, it must be 0 (the clip's first frame needs a prompt)")
    if keys[-1] >= num_frames:
        raise ValueError(f"`{name}`: key {keys[-1]!r} is not a frame of a clip of {num_frames} frames (the last key must be < num_frames)")
    return keys


def normalize_prompt(prompt, num_frames, name="prompt"):
    """(value, travels): `prompt` -- a str, a keyframe dict, or a list of either -- with every dict checked and every single-key dict
    replaced by its text (it takes the plain path: same launches, same bits); travels: a dict with two or more keys is left."""
    if prompt is None or isinstance(prompt, str):
        return prompt, False
    if isinstance(prompt, dict):
        check_keyframes(prompt, num_frames, name)
        if len(prompt) == 1:
            return next(iter(prompt.values())), False
        return prompt, True
    if isinstance(prompt, (list, tuple)):
        out, travels = [], False
        for i, p in enumerate(prompt):
            if not isinstance(p, (str, dict)):
                raise ValueError(f"`{name}[{i}]` has to be a `str` or a `dict` {{frame: text}} but is {type(p)}")
            v, t = normalize_prompt(p, num_frames, f"{name}[{i}]")
            out.append(v)
            travels = travels or t
        return out, travels
    raise ValueError(f"`{name}` has to be of type `str`, `dict` or `list` but is {type(prompt)}")


def per_sample_keyframes(prompt, batch_size, num_frames, name="prompt"):
    """`prompt` (a str, a dict or a list of either) as one checked keyframe dict per sample: a str is {0: str}; a single str / dict
    serves every sample of the batch"""
    if isinstance(prompt, (str, dict)):
        prompt = [prompt] * batch_size
    if len(prompt) != batch_size:
        raise ValueError(f"`{name}` holds {len(prompt)} entries for a batch of {batch_size}")
    out = []
    for i, p in enumerate(prompt):
        d = {0: p} if isinstance(p, str) else p
        check_keyframes(d, num_frames, f"{name}[{i}]" if batch_size > 1 else name)
        out.append({int(k): v for k, v in d.items()})
    return out


def segment_weights(start, end):
    """float32 weights of the frames start .. end of the segment between two keyframes"""
    return np.linspace(0.0, 1.0, end - start + 1).astype(np.float32)


def travel_tables(keys, num_frames, base=0):
    """(lo, hi, w) for one sample: `keys` sorted frame indices (keys[0] == 0, keys[-1] < num_frames) whose embeddings are the source
    rows base, base + 1, ...; frame f reads (1 - w[f]) src[lo[f]] + w[f] src[hi[f]].  A keyframe's own frame has lo = hi = its row and
    w = 0; the frames behind the last key repeat its row."""
    lo = np.zeros(num_frames, dtype=np.int32)
    hi = np.zeros(num_frames, dtype=np.int32)
    w = np.zeros(num_frames, dtype=np.float32)
    for i, (s, e) in enumerate(zip(keys[:-1], keys[1:])):
        ws = segment_weights(s, e)
        lo[s:e], hi[s:e], w[s:e] = base + i, base + i + 1, ws[:-1]
    last = len(keys) - 1
    lo[keys[-1]:], hi[keys[-1]:], w[keys[-1]:] = base + last, base + last, 0.0
    for i, k in enumerate(keys):                  # (w is already 0 there: a keyframe reads its own row alone)
        hi[k] = base + i
    return lo, hi, w


def batch_tables(keyframes, num_frames, repeats=1, base=0):
    """the tables of a batch: `keyframes` one sorted key list per sample, whose embeddings follow each other in the source from row
    `base`; every sample `repeats` times in a row (num_videos_per_prompt).  Returns (lo, hi, w) of len(keyframes) * repeats * num_frames
    rows and the row behind the last source row used."""
    los, his, ws = [], [], []
    for keys in keyframes:
        lo, hi, w = travel_tables(keys, num_frames, base)
        base += len(keys)
        for _ in range(repeats):
            los.append(lo), his.append(hi), ws.append(w)
    return np.concatenate(los), np.concatenate(his), np.concatenate(ws), base


def parse_travel_cell(cell):
    """a CSV cell of the driver's --prompt_travel_column: JSON {"0": "...", "32": "..."} -> {0: "...", 32: "..."}"""
    import json
    try:
        d = json.loads(cell)
    except (TypeError, ValueError) as e:
        raise ValueError(f"prompt travel: {cell!r} is not JSON") from e
    if not isinstance(d, dict):
        raise ValueError(f"prompt travel: {cell!r} is not a JSON object {{\"frame\": \"text\"}}")
    out = {}
    for k, v in d.items():
        try:
            out[int(k)] = v
        except ValueError as e:
            raise ValueError(f"prompt travel: key {k!r} is not a frame index") from e
    return out
