"""GPU: text queries through the facade (SimpleReverso.load_text_model / embed_text / search_by_text / label_database)."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

import reverso_amd
from reverso_amd import engine, filters, store
from reverso_amd.core_system import SimpleReverso
from reverso_amd.tokenizer import ClipTokenizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _text_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reverso(tmp_path_factory):
    """The tiny image tower with a text tower of its width whose vocabulary is the synthetic BPE's, so strings work."""
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path_factory.mktemp("db")), max_batch=8)
    vocab, merges = tr.synthetic_bpe()
    cfg = dataclasses.replace(reverso_amd.get_text_config("PE-Tiny-Text-16"), vocab_size=len(vocab), out_dim=r.pe_model.cfg.out_dim)
    tok = ClipTokenizer(merges, context_length=cfg.context_length, vocab_size=cfg.vocab_size)
    r.text_model = engine.TextEngine.synthetic(cfg, seed=5, device=0, tokenizer=tok, randomize_affine=True)
    yield r
    r.text_model.close()


def _prompts(n):
    words = ["the", "red", "car", "road", "on", "and", "cars", "it's", "blue", "truck", "night", "dog"]
    return [f"{words[i % 12]} {words[(i // 12) % 12]} {words[(5 * i + 1) % 12]} {i}" for i in range(n)]


def test_search_by_text_finds_the_prompt_it_was_built_from(reverso):
    r = reverso
    text, items = r.search_by_text("the red car")
    assert text.startswith("❌ No database loaded") and items == []
    prompts = _prompts(200)
    emb = r.embed_text(prompts)
    assert emb.shape == (200, r.pe_model.cfg.out_dim) and float((emb.norm(dim=-1) - 1).abs().max()) <= 1e-5
    db = store.GalleryStore(emb.shape[1], device=0, capacity=256)
    db.upsert(emb.cpu(), [f"p{i}" for i in range(200)],
              [{"filename": f"f{i}.jpg", "image_source": f"/nowhere/f{i}.jpg", "bbox": [0, 0, i, i], "kind": i % 2} for i in range(200)])
    r.vector_db, r.current_database = db, "prompts"
    try:
        for i in (0, 1, 57, 123, 199):
            text, items = r.search_by_text(prompts[i], max_results=3)
            assert text.startswith("🎯 Found 3 similar regions:") and f"1. f{i}.jpg (Similarity: " in text
            assert items[0]["filename"] == f"f{i}.jpg" and items[0]["score"] >= 1 - 1e-5, (i, items[0])
            assert set(items[0]) == {"image", "score", "filename", "bbox"}
            assert items[0]["score"] >= items[1]["score"] >= items[2]["score"]
        # the same strings and result shape as search_similar; a threshold, a filter and a grouping are honoured
        text, items = r.search_by_text(prompts[57], similarity_threshold=1.5)
        assert items == [] and text == "❌ No similar regions found above threshold 1.5"
        flt = filters.Filter(must=[filters.FieldCondition("kind", match=filters.MatchValue(0))])
        text, items = r.search_by_text(prompts[57], max_results=4, query_filter=flt)
        assert len(items) == 4 and all(int(it["filename"][1:-4]) % 2 == 0 for it in items)
        text, items = r.search_by_text(prompts[57], max_results=2, group_by="kind")
        assert len(items) == 2 and items[0]["filename"] == "f57.jpg"
        # token arrays work without a tokenizer
        text, items = r.search_by_text(r.text_model.tokenizer([prompts[123]]), max_results=1)
        assert items[0]["filename"] == "f123.jpg"
    finally:
        r.vector_db, r.current_database = None, None
        db.close()


def test_label_database_is_the_exact_best_label_of_every_row(reverso):
    r = reverso
    N, D = 5000, r.pe_model.cfg.out_dim
    labels = ["a red car", "the road at night", "a dog", "it's a truck", "blue cars on the road", "42", "the"]
    text, out = r.label_database(labels)
    assert text.startswith("❌ No database loaded") and out == []
    g = torch.Generator().manual_seed(17)
    vec = torch.randn(N, D, generator=g)
    db = store.GalleryStore(D, device=0, capacity=N)
    db.upsert(vec, [f"p{i}" for i in range(N)],
              [{"filename": f"f{i}.jpg", "image_source": f"/nowhere/f{i}.jpg", "bbox": [0, 0, 1, 1], "kind": i % 3} for i in range(N)])
    r.vector_db, r.current_database = db, "random"
    try:
        # the oracle: a gallery of the label embeddings searched with every stored row, k = 1
        lab_emb = r.embed_text(labels)
        G = engine.Gallery(D, len(labels), device=0)
        G.add(lab_emb)
        s, i, _ = G.search(db.gallery.read(), k=1, score_threshold=None)
        want_lab, want_sc = i[:, 0].cpu().numpy(), s[:, 0].cpu().numpy()
        G.close()
        text, out = r.label_database(labels, members=4)
        assert text.startswith(f"🎯 {N} regions over {len(labels)} labels:")
        assert [o["label"] for o in out] == labels and sum(o["count"] for o in out) == N
        for j, o in enumerate(out):
            rows = np.nonzero(want_lab == j)[0]
            assert o["count"] == rows.size
            best = rows[np.lexsort((rows, -want_sc[rows]))][:4]
            assert [m["id"] for m in o["members"]] == [f"p{x}" for x in best]
            assert np.array_equal(np.array([m["score"] for m in o["members"]], dtype=np.float32), want_sc[best])      # score bits
        lab, sc = db.assign(lab_emb)
        assert np.array_equal(lab.cpu().numpy(), want_lab) and np.array_equal(sc.cpu().numpy().view(np.uint32), want_sc.view(np.uint32))
        # a filter: only the selected points are labelled
        flt = filters.Filter(must=[filters.FieldCondition("kind", match=filters.MatchValue(1))])
        text, some = r.label_database(labels, query_filter=flt, members=2)
        assert sum(o["count"] for o in some) == len(range(1, N, 3))
        for j, o in enumerate(some):
            assert o["count"] == int(((want_lab == j) & (np.arange(N) % 3 == 1)).sum())
            assert all(int(m["id"][1:]) % 3 == 1 for m in o["members"])
        assert r.label_database([])[1] == []
    finally:
        r.vector_db, r.current_database = None, None
        db.close()


def test_text_tower_loads_lazily_with_synthetic_weights(tmp_path, capsys):
    r = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
    assert r.text_model is None
    os.environ.pop("REVERSO_BPE_VOCAB", None)
    tokens = tr.prompts(reverso_amd.get_text_config("PE-Tiny-Text-16"), [3, 7], seed=1)
    e = r.embed_text(tokens)
    assert "text tower uses seeded random-init weights" in capsys.readouterr().out
    assert r.text_model is not None and e.shape == (2, r.pe_model.cfg.out_dim)
    assert torch.equal(r.embed_text(tokens), e) and r.load_text_model() is r.text_model
    text, items = r.search_by_text("a red pickup truck at night")          # strings need the user's merges file
    assert items == [] and text.startswith("❌")
    r.text_model.close()
