"""CLIP's byte-level BPE tokenizer in pure Python, for the text tower (engine.TextEngine).

[UPSTREAM-RECALL] what open-CLIP's ``SimpleTokenizer`` does, restated: the text is NFC-normalised, runs of whitespace become
one space, lower-cased; split by the CLIP pattern (contractions, letter runs, single digits, runs of anything else); every
piece is mapped byte by byte to printable code points, its last symbol gets ``</w>``, and the merges are applied lowest rank
first.  The vocabulary is the 256 byte symbols, the same 256 with ``</w>``, one entry per merge, then ``<|startoftext|>`` and
``<|endoftext|>``: start = vocab - 2, end = vocab - 1.  Pad id 0 ([UPSTREAM-RECALL]; whatever follows the end token cannot
change the result: attention is causal and the end token's row is the one pooled).

Upstream also runs ``ftfy.fix_text`` and ``html.unescape`` over the text first.  ``ftfy`` is not a dependency of this
package: mojibake is not repaired here.

The merges come from a file the user supplies -- upstream's ``bpe_simple_vocab_16e6.txt.gz`` (a header line, then one
``a b`` pair per line; plain text or gzip) named by an argument or by ``REVERSO_BPE_VOCAB`` -- or from a list of pairs.
"""
import gzip
import os
import unicodedata
from functools import lru_cache

VOCAB_ENV = "REVERSO_BPE_VOCAB"
_SPLIT = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"""


@lru_cache()
def _patterns():
    import regex        # \p{L} / \p{N}: the third-party `regex` module (needed only where strings are tokenized)
    return regex.compile(_SPLIT, regex.IGNORECASE), regex.compile(r"\s+")


@lru_cache()
def bytes_to_unicode():
    """byte -> a printable code point (the GPT-2 table): the printable Latin-1 bytes map to themselves, the others to
    256, 257, ... in byte order."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("\xa1"), ord("\xac") + 1)) + list(range(ord("\xae"), ord("\xff") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


def read_merges(path, vocab_size=49408):
    """The merges of a ``bpe_simple_vocab_16e6.txt.gz``-format file: the header line is skipped, and only as many lines
    are kept as a vocabulary of ``vocab_size`` has room for (upstream: 49152 - 256 - 2 of the file's 262 145)."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt", encoding="utf-8") as f:
        lines = f.read().split("\n")
    lines = lines[1:1 + max(0, vocab_size - 512 - 2)]
    return [tuple(ln.split()) for ln in lines if ln.strip()]


class ClipTokenizer:
    def __init__(self, merges=None, context_length=32, vocab_size=None):
        """merges: a list of ``(a, b)`` pairs or of ``"a b"`` strings, a path, or None (then ``REVERSO_BPE_VOCAB`` names
        the file).  vocab_size: when given, the vocabulary the model was trained with (a file's merges are cut to fit, and
        a mismatch is an error)."""
        if merges is None:
            merges = os.environ.get(VOCAB_ENV)
            if not merges:
                raise FileNotFoundError(
                    "no BPE merges: pass a merges file (the upstream bpe_simple_vocab_16e6.txt.gz format) or a list of pairs, "
                    f"or set {VOCAB_ENV}; token arrays can be embedded without one (TextEngine.embed_tokens)")
        if isinstance(merges, (str, os.PathLike)):
            merges = read_merges(merges, vocab_size if vocab_size else 49408)
        merges = [tuple(m.split()) if isinstance(m, str) else tuple(m) for m in merges]
        if any(len(m) != 2 for m in merges):
            raise ValueError("every merge must be a pair of symbols")
        b2u = bytes_to_unicode()
        vocab = list(b2u.values())
        vocab = vocab + [v + "</w>" for v in vocab]
        vocab += ["".join(m) for m in merges]
        vocab += ["<|startoftext|>", "<|endoftext|>"]
        if vocab_size is not None and len(vocab) != vocab_size:
            raise ValueError(f"{len(merges)} merges make a vocabulary of {len(vocab)}, the model has {vocab_size}")
        self.encoder = {v: i for i, v in enumerate(vocab)}
        self.ranks = {m: i for i, m in enumerate(merges)}
        self.byte_encoder = b2u
        self.vocab_size = len(vocab)
        self.sot, self.eot, self.pad = len(vocab) - 2, len(vocab) - 1, 0
        self.context_length = int(context_length)
        self._cache = {"<|startoftext|>": ("<|startoftext|>",), "<|endoftext|>": ("<|endoftext|>",)}

    @staticmethod
    def clean(text):
        return _patterns()[1].sub(" ", unicodedata.normalize("NFC", text)).lower().strip()

    def _bpe(self, token):
        if token in self._cache:
            return self._cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.ranks.get(p, float("inf")))
            if best not in self.ranks:
                break
            a, b = best
            out, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == a and word[i + 1] == b:
                    out.append(a + b)
                    i += 2
                else:
                    out.append(word[i])
                    i += 1
            word = tuple(out)
        self._cache[token] = word
        return word

    def encode(self, text):
        """The ids of ``text`` without the start and end tokens."""
        ids = []
        for piece in _patterns()[0].findall(self.clean(text)):
            piece = "".join(self.byte_encoder[b] for b in piece.encode("utf-8"))
            ids.extend(self.encoder[s] for s in self._bpe(piece))
        return ids

    def __call__(self, texts, context_length=None):
        """int32 numpy ``[n, context_length]``: start token, the ids, end token, padded with 0.  A prompt that does not
        fit is truncated and keeps the end token in the last slot."""
        import numpy as np
        if isinstance(texts, str):
            texts = [texts]
        L = int(context_length or self.context_length)
        out = np.full((len(texts), L), self.pad, dtype=np.int32)
        for i, t in enumerate(texts):
            ids = [self.sot] + self.encode(t) + [self.eot]
            if len(ids) > L:
                ids = ids[:L]
                ids[-1] = self.eot
            out[i, :len(ids)] = ids
        return out
