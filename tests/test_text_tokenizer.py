"""CPU: reverso_amd.tokenizer.ClipTokenizer against transformers.CLIPTokenizer on a synthetic CLIP-format vocabulary (the
256 byte symbols, the same with </w>, a handful of merges, the two specials: tests/_text_reference.synthetic_bpe), which
builds offline -- the real merges file is the user's to supply."""
import gzip
import os
import sys

import numpy as np
import pytest

from reverso_amd import _lib, tokenizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _text_reference as tr  # noqa: E402

TEXTS = [
    "the red car on the road",                 # plain words, merged and unmerged
    "A Red-Car, on  the road!",                # upper case, punctuation, a double space
    "it's 42 cars",                            # a contraction, digits (one piece per digit)
    "wait... what?!  (really)!!!",             # punctuation runs
    "café  ñandú",                             # non-ASCII, two bytes per letter
    "café",                              # NFC: e + combining acute = é
    "  tabs\tand\nnewlines  ",                 # whitespace of every kind, at the ends too
    "THE CARS' ROAD 2024",
    "",                                        # an empty string: start, end
    "日本語 text",
]


@pytest.fixture(scope="module")
def pair():
    from transformers import CLIPTokenizer
    vocab, merges = tr.synthetic_bpe()
    return tokenizer.ClipTokenizer(merges, context_length=16), CLIPTokenizer(vocab, merges), vocab


@pytest.mark.parametrize("text", TEXTS)
def test_ids_equal_the_independent_tokenizer(pair, text):
    ours, theirs, vocab = pair
    want = theirs(text)["input_ids"]
    got = [ours.sot] + ours.encode(text) + [ours.eot]
    assert got == want, (text, got, want)
    assert ours.sot == vocab["<|startoftext|>"] == len(vocab) - 2 and ours.eot == vocab["<|endoftext|>"] == len(vocab) - 1


def test_known_pieces(pair):
    ours, _, vocab = pair
    assert ours.encode("the red cars") == [vocab["the</w>"], vocab["red</w>"], vocab["cars</w>"]]
    assert ours.encode("it's 42") == [vocab["it</w>"], vocab["'s</w>"], vocab["4</w>"], vocab["2</w>"]]    # digits never merge across pieces
    assert ours.encode("!!!") == [vocab["!!!</w>"]]


def test_rows_padding_and_truncation(pair):
    ours, theirs, _ = pair
    rows = ours(["the road", "", "the " * 40])
    assert rows.dtype == np.int32 and rows.shape == (3, 16)
    assert rows[0].tolist()[:4] == [ours.sot] + ours.encode("the road") + [ours.eot] and not rows[0, 4:].any()
    assert rows[1].tolist()[:2] == [ours.sot, ours.eot] and not rows[1, 2:].any()
    # longer than the context: truncated, the end token in the last slot
    assert rows[2, 0] == ours.sot and rows[2, -1] == ours.eot and (rows[2, 1:-1] == ours.encode("the")[0]).all()
    want = theirs("the " * 40, truncation=True, max_length=16)["input_ids"]
    assert rows[2].tolist() == want
    # the end token is the row's largest id and comes first at its position: what the tower pools
    assert (rows.argmax(axis=1) == [3, 1, 15]).all()


def test_merges_from_a_file_in_the_upstream_format(tmp_path, monkeypatch):
    vocab, merges = tr.synthetic_bpe()
    body = '"bpe_simple_vocab_16e6.txt#version: 0.2\n' + "\n".join(" ".join(m) for m in merges) + "\nzz zz\nyy yy\n"
    path = tmp_path / "bpe.txt.gz"
    with gzip.open(path, "wt", encoding="utf-8") as f:
        f.write(body)
    # the vocabulary size of the model says how many of the file's lines are merges
    tok = tokenizer.ClipTokenizer(str(path), context_length=16, vocab_size=len(vocab))
    assert tok.encoder == vocab
    monkeypatch.setenv(tokenizer.VOCAB_ENV, str(path))
    assert tokenizer.ClipTokenizer(None, vocab_size=len(vocab)).encode("the cars") == tok.encode("the cars")
    with pytest.raises(ValueError, match="vocabulary"):
        tokenizer.ClipTokenizer(merges, vocab_size=49408)
    monkeypatch.delenv(tokenizer.VOCAB_ENV)
    with pytest.raises(FileNotFoundError, match=tokenizer.VOCAB_ENV):
        tokenizer.ClipTokenizer(None)
