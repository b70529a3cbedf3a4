"""Writes tests/golden/clip_text_small.safetensors and tests/golden/clip_text_keys.txt (run once, with transformers installed).

The fixture pins tests/clip_text_reference.py to transformers' own `CLIPTextModel`: fp16-representable seeded weights of a 2-layer
model (hidden 128, 2 heads, intermediate 256, vocab 256, 77 positions; q_proj / k_proj weights times 3), prompt-shaped ids, and
transformers' fp32 outputs -- the last hidden state and all three hidden states.  The key list is what a 12-layer
`CLIPTextModel.state_dict()` holds under the published `text_model.` prefix, plus the `position_ids` buffer of older files.

    python tools/make_clip_text_fixture.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.clip_text_reference import PREFIX, prompt_like_ids, seeded_state, state_dict_keys, strip_prefix  # noqa: E402

SMALL = dict(vocab_size=256, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
             max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=255)


def transformers_model(config, state):
    """transformers' CLIPTextModel holding `state` (keys with the prefix; mapped to whatever this transformers release calls them)"""
    from transformers import CLIPTextConfig, CLIPTextModel
    m = CLIPTextModel(CLIPTextConfig(**config, bos_token_id=config["vocab_size"] - 2, pad_token_id=config["eos_token_id"],
                                     attn_implementation="eager")).eval()
    own = m.state_dict()
    bare = strip_prefix(state)
    mapped = {}
    for k in own:
        if k.endswith("position_ids"):
            continue
        mapped[k] = bare[k[len(PREFIX):] if k.startswith(PREFIX) else k]
    missing, unexpected = m.load_state_dict(mapped, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    return m


def main():
    from safetensors.torch import save_file
    state = seeded_state(SMALL, seed=17, qk_gain=3.0)
    ids = prompt_like_ids(2, 77, SMALL["vocab_size"], seed=5)
    with torch.no_grad():
        out = transformers_model(SMALL, state)(input_ids=ids, output_hidden_states=True)
    blob = {k: v.half() for k, v in state.items()}
    blob["input_ids"] = ids.to(torch.int32)
    blob["last_hidden_state"] = out.last_hidden_state.float().contiguous()
    for i, t in enumerate(out.hidden_states):
        blob[f"hidden_states.{i}"] = t.float().contiguous()
    golden = os.path.join(ROOT, "tests", "golden")
    save_file(blob, os.path.join(golden, "clip_text_small.safetensors"), metadata={k: str(v) for k, v in SMALL.items()})
    with open(os.path.join(golden, "clip_text_keys.txt"), "w") as f:
        f.write("\n".join(sorted(state_dict_keys(12) + [PREFIX + "embeddings.position_ids"])) + "\n")
    print("wrote", os.path.getsize(os.path.join(golden, "clip_text_small.safetensors")), "bytes")


if __name__ == "__main__":
    main()
