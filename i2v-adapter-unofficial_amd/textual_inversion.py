"""Textual inversion (diffusers' `TextualInversionLoaderMixin`, which the reference's pipeline class inherits; the reference calls
`maybe_convert_prompt` on the prompt and on the negative prompt, pipe:409 / 491): learned token embeddings -- negative embeddings of the
`EasyNegative` kind, styles, subjects -- added to the tokenizer and to the text encoder's token table.

    load(pipe, source, token=None, weight_name=None, subfolder=None)     pipe.load_textual_inversion
    unload(pipe, tokens=None)                                            pipe.unload_textual_inversion
    convert_prompt(pipe, prompt, tokenizer)                              pipe.maybe_convert_prompt

Sources: a file (`.safetensors` through safetensors, anything else through `torch.load(..., weights_only=True)`), a directory plus
`weight_name`, a dict, or a list of these with a list of tokens.  Formats: diffusers' {token: tensor [D] or [n, D]} with exactly one key,
and A1111's {"string_to_param": {"*": tensor [n, D]}, "name": str}.  n vectors add the tokens tok, tok_1, ... tok_{n-1}, and
`maybe_convert_prompt` writes `tok` out as `tok tok_1 ... tok_{n-1}` wherever the tokenizer finds it in a prompt.

Of the tokenizer only `add_tokens(list) -> int`, `convert_tokens_to_ids`, `tokenize`, `len()` and the call interface are used -- and
`remove_tokens(list)` where it exists (transformers' CLIPTokenizer has none).  Host-only: the new rows are written into the text
encoder's own parameter, `CLIPTextModel.packed()` sees the change and `i2v_clip_embed_f16` reads the longer table.  No embedding file
of the wild has been loaded: the formats are restated in tests/textual_inversion_reference.py."""
import os
import re

import torch

_PROBE = "\x00i2v-no-such-token\x00"


def _read(source, weight_name, subfolder):
    if isinstance(source, dict):
        return source
    if not isinstance(source, (str, os.PathLike)):
        raise ValueError(f"a textual inversion is a path, a directory with `weight_name`, or a dict, got {type(source).__name__}")
    path = os.fspath(source)
    if os.path.isdir(path):
        if subfolder:
            path = os.path.join(path, subfolder)
        if not weight_name:
            raise ValueError(f"{path} is a directory: pass `weight_name`")
        path = os.path.join(path, weight_name)
    if not os.path.isfile(path):
        raise EnvironmentError(f"textual inversion weights not found at {path}")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


def parse_state(state, token=None):
    """(token, vectors [n, D]) of one state dict in either format; an explicit `token` overrides the file's"""
    if not isinstance(state, dict):
        raise ValueError(f"a textual inversion state is a dict, got {type(state).__name__}")
    if "string_to_param" in state:                                        # A1111
        params = state["string_to_param"]
        if not hasattr(params, "__getitem__") or "*" not in params:
            raise ValueError("an A1111 textual inversion holds its vectors at state['string_to_param']['*']")
        name, emb = state.get("name"), params["*"]
    else:
        if len(state) != 1:
            if token is None or len(state) == 0:
                raise ValueError(f"the state dict has {len(state)} keys ({sorted(map(str, state))[:4]} ...): a diffusers textual "
                                 "inversion holds exactly one {token: tensor}; pass `token=` to name one of several")
            if token not in state:
                raise ValueError(f"the state dict has {len(state)} keys and none of them is `token` {token!r}")
            name, emb = token, state[token]
        else:
            name, emb = next(iter(state.items()))
    name = token if token is not None else name
    if not isinstance(name, str) or not name:
        raise ValueError(f"a textual inversion needs a token (a non-empty str), got {name!r}")
    if not isinstance(emb, torch.Tensor) or emb.dim() not in (1, 2) or emb.numel() == 0:
        raise ValueError(f"the embedding of {name!r} must be a tensor [D] or [n, D], got "
                         f"{tuple(emb.shape) if isinstance(emb, torch.Tensor) else type(emb).__name__}")
    return name, emb.detach().reshape(-1, emb.shape[-1])


def token_names(token, n):
    return [token] + [f"{token}_{i}" for i in range(1, n)]


def _known(tokenizer, name):
    tid = tokenizer.convert_tokens_to_ids(name)
    return tid is not None and tid != tokenizer.convert_tokens_to_ids(_PROBE)


def _table(pipe):
    return pipe.text_encoder.text_model.embeddings.token_embedding


def load(pipe, source, token=None, weight_name=None, subfolder=None):
    if getattr(pipe, "text_encoder", None) is None or getattr(pipe, "tokenizer", None) is None:
        raise ValueError("load_textual_inversion needs a pipeline with both a `text_encoder` and a `tokenizer`")
    sources = list(source) if isinstance(source, (list, tuple)) else [source]
    if isinstance(token, (list, tuple)):
        tokens = list(token)
    else:
        tokens = [token] * len(sources)
        if token is not None and len(sources) > 1:
            raise ValueError(f"{len(sources)} textual inversions with one `token`: pass a list of {len(sources)} tokens")
    if len(tokens) != len(sources) or not sources:
        raise ValueError(f"{len(sources)} textual inversions with {len(tokens)} tokens: the lists must have one length >= 1")
    names_w = weight_name if isinstance(weight_name, (list, tuple)) else [weight_name] * len(sources)
    if len(names_w) != len(sources):
        raise ValueError(f"{len(sources)} textual inversions with {len(names_w)} weight names")
    tok, te = pipe.tokenizer, pipe.text_encoder
    hidden = te.config.hidden_size
    # everything is read and checked before anything is modified
    if len(tok) < _table(pipe).weight.shape[0]:
        raise ValueError(f"the tokenizer has {len(tok)} tokens and the text encoder's token table {_table(pipe).weight.shape[0]} rows: "
                         "a new token's id would fall on a row that is in use")
    items, seen = [], set()
    for src, t, wn in zip(sources, tokens, names_w):
        name, emb = parse_state(_read(src, wn, subfolder), t)
        if emb.shape[-1] != hidden:
            raise ValueError(f"the embedding of {name!r} has dimension {emb.shape[-1]}, the text encoder's hidden size is {hidden}")
        names = token_names(name, emb.shape[0])
        for n in names:
            if n in seen or _known(tok, n):
                hint = "" if n == name else f" (multi-vector name of {name!r}: {emb.shape[0]} vectors)"
                raise ValueError(f"token {n!r}{hint} is already in the tokenizer: pass another `token`, or unload it first")
            seen.add(n)
        items.append((name, names, emb))
    state = pipe.__dict__.setdefault("_textual_inversions", [])
    if not state:
        pipe._ti_base_vocab = _table(pipe).weight.shape[0]
    for name, names, emb in items:
        added = tok.add_tokens(names)
        ids = [tok.convert_tokens_to_ids(n) for n in names]
        if added != len(names) or any(i is None for i in ids):
            raise RuntimeError(f"the tokenizer added {added} of the {len(names)} tokens of {name!r}")
        te.resize_token_embeddings(max(len(tok), max(ids) + 1, _table(pipe).weight.shape[0]))
        w = _table(pipe).weight
        with torch.no_grad():
            w[torch.tensor(ids, device=w.device)] = emb.to(device=w.device, dtype=w.dtype)
        state.append(dict(token=name, names=names, ids=ids, vectors=emb.clone()))


def unload(pipe, tokens=None):
    state = getattr(pipe, "_textual_inversions", None)
    if not state:
        return
    if tokens is None:
        gone = list(state)
    else:
        tokens = [tokens] if isinstance(tokens, str) else list(tokens)
        unknown = [t for t in tokens if t not in [r["token"] for r in state]]
        if unknown:
            raise ValueError(f"no textual inversion with token {unknown[0]!r} is loaded (loaded: {[r['token'] for r in state]})")
        gone = [r for r in state if r["token"] in tokens]
    kept = [r for r in state if all(r is not g for g in gone)]
    tok, te, base = pipe.tokenizer, pipe.text_encoder, pipe._ti_base_vocab
    if hasattr(tok, "remove_tokens"):
        # the tokenizer gives ids back: all inversions out, the table back to its own rows, the kept ones in again at compact ids
        tok.remove_tokens([n for r in state for n in r["names"]])
        te.resize_token_embeddings(base)
        state.clear()
        for r in kept:
            load(pipe, {r["token"]: r["vectors"]})
    else:
        # the ids stay reserved in the tokenizer; the table keeps the rows up to the last id that is still loaded
        state[:] = kept
        te.resize_token_embeddings(max([base] + [i + 1 for r in kept for i in r["ids"]]))


def convert_prompt(pipe, prompt, tokenizer):
    state = getattr(pipe, "_textual_inversions", None)
    if not state:
        return prompt
    if isinstance(prompt, (list, tuple)):
        return [convert_prompt(pipe, p, tokenizer) for p in prompt]
    if not isinstance(prompt, str):
        return prompt
    found = set(tokenizer.tokenize(prompt))
    names = {r["token"]: r["names"] for r in state}
    if not any(len(n) > 1 and t in found for t, n in names.items()):
        return prompt
    # one pass over the text, longer names first: a token is not rewritten inside a longer loaded token, and the multi-vector names
    # tok_1, tok_2, ... (tokens of their own) stand for themselves
    every = sorted({n for ns in names.values() for n in ns}, key=len, reverse=True)
    return re.sub("|".join(re.escape(n) for n in every), lambda m: " ".join(names.get(m.group(0), [m.group(0)])), prompt)
