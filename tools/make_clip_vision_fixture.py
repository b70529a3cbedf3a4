"""Writes tests/golden/clip_vision_small.safetensors, tests/golden/clip_vision_small_224.safetensors and
tests/golden/clip_vision_keys.txt (run once, with transformers installed).

The fixture pins tests/clip_vision_reference.py to transformers' own `CLIPVisionModelWithProjection`: fp16-representable seeded weights
of a 2-layer model (hidden 160, 2 heads of 80, intermediate 160, projection 64, erf GELU, patch 14; q_proj / k_proj weights times 3)
and transformers' fp32 outputs -- the image embeds and all three hidden states -- for a 56-px input (17 tokens, with a second, 17-row
position table) and a 224-px input (257 tokens, the model's own table), batch 2.  The inputs are `pattern_pixels` (integer arithmetic,
nothing to store).  The 224-px outputs live in a file of their own: a committed file stays under 1 MiB.  The key list is what the
32-layer ViT-H `CLIPVisionModelWithProjection.state_dict()` holds, plus the `position_ids` buffer of older files.

    python tools/make_clip_vision_fixture.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.clip_vision_reference import PREFIX, SMALL, pattern_pixels, seeded_state, state_dict_keys  # noqa: E402

POS = PREFIX + "embeddings.position_embedding.weight"
POS_56 = "position_embedding_56.weight"


def transformers_model(config, state):
    """transformers' CLIPVisionModelWithProjection (eager attention) holding `state`"""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(**config, attn_implementation="eager")).eval()
    missing, unexpected = m.load_state_dict({k: v for k, v in state.items() if not k.endswith("position_ids")}, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return m


def small_states(seed=17):
    """(224-px state, 56-px state): the same weights, the second with its own 17-row position table"""
    state = seeded_state(SMALL, seed=seed, qk_gain=3.0)
    pos56 = (torch.randn(17, SMALL["hidden_size"], generator=torch.Generator().manual_seed(seed + 1)) * 0.02).half().float()
    return state, dict(state, **{POS: pos56})


def main():
    from safetensors.torch import save_file
    state, state56 = small_states()
    blob = {k: v.half() for k, v in state.items()}
    blob[POS_56] = state56[POS].half()
    big = {}
    for size, st, dst in ((56, state56, blob), (224, state, big)):
        with torch.no_grad():
            out = transformers_model(dict(SMALL, image_size=size), st)(pixel_values=pattern_pixels(2, size), output_hidden_states=True)
        dst[f"out{size}.image_embeds"] = out.image_embeds.float().contiguous()
        for i, t in enumerate(out.hidden_states):
            dst[f"out{size}.hidden_states.{i}"] = t.float().contiguous()
        assert torch.equal(out.last_hidden_state, out.hidden_states[-1])
    golden = os.path.join(ROOT, "tests", "golden")
    meta = {k: str(v) for k, v in SMALL.items()}
    save_file(blob, os.path.join(golden, "clip_vision_small.safetensors"), metadata=meta)
    save_file(big, os.path.join(golden, "clip_vision_small_224.safetensors"), metadata=meta)
    with open(os.path.join(golden, "clip_vision_keys.txt"), "w") as f:
        f.write("\n".join(sorted(state_dict_keys(32) + [PREFIX + "embeddings.position_ids"])) + "\n")
    for n in ("clip_vision_small.safetensors", "clip_vision_small_224.safetensors"):
        print("wrote", n, os.path.getsize(os.path.join(golden, n)), "bytes")


if __name__ == "__main__":
    main()
