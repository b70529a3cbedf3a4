"""Textual inversion, restated: the rules `textual_inversion.py`, `I2VAdapterPipeline.load_textual_inversion` / `maybe_convert_prompt`
and `CLIPTextModel.resize_token_embeddings` are tested against (tests/test_textual_inversion.py, tests/test_textual_inversion_gpu.py),
after diffusers' `TextualInversionLoaderMixin` -- there is no diffusers here, so its rules are written out -- and a word-level stub
tokenizer with the members the loader may use.  No product code imports it.

    formats      diffusers {token: tensor [D] or [n, D]} (exactly one key), A1111 {"string_to_param": {"*": [n, D]}, "name": token}
    tokens       n vectors -> token, token_1, ... token_{n-1}, appended to the tokenizer; their ids index new rows of the token table
    conversion   every multi-vector token among tokenizer.tokenize(prompt) becomes "token token_1 ... token_{n-1}"
"""
import torch

WORDS = ("a red fox snow falls night blurry cute pig dog cat runs on the beach at sunset over hills masterpiece best quality low bad "
         "hands ugly photo of in forest with rain and wind sky blue green tall small").split()


class FixedWordTokenizer:
    """CLIPTokenizer's interface over whitespace-separated lower-case words.  ids: the words of WORDS, then w0, w1, ... up to
    vocab_size - 4; unk, bos, eos, pad are the last four ids -- pad is NOT eos, so a chunk layout that pads with eos shows.  Added
    tokens get the ids from `vocab_size` on.  Like transformers' tokenizer it cannot remove a token (WordTokenizer below can)."""

    def __init__(self, model_max_length=77, vocab_size=256):
        self.model_max_length, self.vocab_size = model_max_length, vocab_size
        n = vocab_size - 4
        words = list(WORDS)[:n]
        words += [f"w{i}" for i in range(n - len(words))]
        self.vocab = {w: i for i, w in enumerate(words)}
        self.words = words
        self.unk_id, self.bos_id, self.eos_id, self.pad_id = n, n + 1, n + 2, n + 3
        self.added = {}
        self._next = vocab_size
        self.calls = []

    def __len__(self):
        return self._next

    def add_tokens(self, tokens):
        count = 0
        for t in [tokens] if isinstance(tokens, str) else tokens:
            if t not in self.added and t not in self.vocab:
                self.added[t] = self._next
                self._next += 1
                count += 1
        return count

    def tokenize(self, text):
        return [w if w in self.added else w.lower() for w in text.split()]

    def convert_tokens_to_ids(self, tokens):
        one = lambda t: self.added.get(t, self.vocab.get(t, self.unk_id))
        return one(tokens) if isinstance(tokens, str) else [one(t) for t in tokens]

    def _encode(self, text):
        return [self.bos_id] + self.convert_tokens_to_ids(self.tokenize(text)) + [self.eos_id]

    def __call__(self, text, padding=False, max_length=None, truncation=False, return_tensors=None):
        single = isinstance(text, str)
        texts = [text] if single else list(text)
        self.calls.append((tuple(texts), padding, max_length))
        rows = [self._encode(t) for t in texts]
        if max_length is None:
            max_length = self.model_max_length
        if truncation:
            rows = [r if len(r) <= max_length else r[:max_length - 1] + [self.eos_id] for r in rows]
        if padding == "max_length":
            rows = [r + [self.pad_id] * (max_length - len(r)) for r in rows]
        elif padding in (True, "longest"):
            width = max(len(r) for r in rows)
            rows = [r + [self.pad_id] * (width - len(r)) for r in rows]
        if return_tensors == "pt":
            ids = torch.tensor(rows, dtype=torch.int64)
        else:
            ids = rows[0] if single else rows

        class _Enc:
            input_ids = ids
        return _Enc()

    def batch_decode(self, ids):
        names = {i: t for t, i in self.added.items()}
        special = {self.unk_id: "<unk>", self.bos_id: "<bos>", self.eos_id: "<eos>", self.pad_id: "<pad>"}
        word = lambda i: names.get(i) or special.get(i) or self.words[i]
        return [" ".join(word(int(i)) for i in row) for row in ids]


class WordTokenizer(FixedWordTokenizer):
    """the stub with `remove_tokens(list)`: removed ids are handed out again"""

    def remove_tokens(self, tokens):
        for t in tokens:
            self.added.pop(t, None)
        self._next = max([self.vocab_size] + [i + 1 for i in self.added.values()])


def parse_state(state, token=None):
    """(token, vectors [n, D]) by diffusers' rules; ValueError for several keys without a token"""
    if "string_to_param" in state:
        name, emb = state["name"], state["string_to_param"]["*"]
    elif len(state) == 1:
        (name, emb), = state.items()
    elif token is not None and token in state:
        name, emb = token, state[token]
    else:
        raise ValueError("several keys and no token")
    if token is not None:
        name = token
    return name, emb.reshape(-1, emb.shape[-1])


def names(token, n):
    return [token] + [f"{token}_{i}" for i in range(1, n)]


def convert(prompt, loaded, tokenizer):
    """`maybe_convert_prompt`: loaded = {token: n vectors}.  Word by word over the tokenizer's tokens of the prompt"""
    if isinstance(prompt, list):
        return [convert(p, loaded, tokenizer) for p in prompt]
    out = []
    for w in tokenizer.tokenize(prompt):
        out += names(w, loaded[w]) if loaded.get(w, 1) > 1 else [w]
    return " ".join(out)


def expected_table(base, loaded):
    """the token table after loading: base [V, D] with the vectors of `loaded` (a list of [n, D] tensors in load order) appended"""
    return torch.cat([base] + [v.to(base.dtype) for v in loaded])
