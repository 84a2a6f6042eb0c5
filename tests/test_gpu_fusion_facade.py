"""GPU: hybrid queries through the store and the facade (GalleryStore.query_fusion, SimpleReverso.search_by_text_and_image)
against Gallery.search_fusion, on the tiny towers of tests/test_gpu_text_facade.py."""
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
DEV = torch.device("cuda", 0)


def _store(N, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, D)).astype(np.float32)
    for r in range(0, N - 4, 50):                         # near-copies: lists that overlap
        x[r + 1:r + 4] = x[r] + 0.3 * rng.standard_normal((3, D)).astype(np.float32)
    payloads = [{"image_source": f"img{r}.jpg", "filename": f"img{r}.jpg", "detected_class": ["car", "person"][r % 2],
                 "bbox": [r, 0, r + 1, 1]} for r in range(N)]
    st = store.GalleryStore(D, device=0, capacity=N)
    st.upsert(torch.from_numpy(x), [f"p{r}" for r in range(N)], payloads)
    return st, x


def _as_points(st, out):
    s, i, c, r, ls = out
    n = int(c[0])
    return [(st.ids[j], sc, rk, lsc) for j, sc, rk, lsc in zip(i[0, :n].tolist(), s[0, :n].tolist(), r[0, :n].tolist(),
                                                                 ls[0, :n].tolist())]


def test_store_query_fusion():
    N, D = 5000, 256
    st, x = _store(N, D, seed=61)
    v = x[2001] + 0.2 * np.random.default_rng(1).standard_normal(D).astype(np.float32)
    # a point id and a vector; the point given by id is not part of the result
    hits = st.query_fusion(["p50", v], limit=8, prefetch_limit=40)
    q = torch.stack([st.gallery.read(50, 1)[0], torch.from_numpy(v).to(DEV)])[None]
    allow = torch.ones(N, dtype=torch.bool, device=DEV)
    allow[50] = False
    want = _as_points(st, st.gallery.search_fusion(q, k=8, limit=40, allow=allow, with_list_scores=True))
    assert len(hits) == 8 and [(h.id, h.score, h.ranks, h.scores) for h in hits] == want
    assert all(isinstance(h, store.FusedPoint) and h.payload is st.payloads[int(h.id[1:])] for h in hits)
    assert all(h.id != "p50" and len(h.ranks) == 2 and len(h.scores) == 2 and max(h.ranks) > 0 for h in hits)
    assert {"p51", "p52", "p53"} <= {h.id for h in st.query_fusion(["p50", v], limit=20, prefetch_limit=40)}
    # vectors only, DBSF, weights, a list threshold, a payload filter, a fused threshold
    flt = filters.Filter(must=[filters.FieldCondition("detected_class", match=filters.MatchValue("person"))])
    hits = st.query_fusion([x[100], v, x[2002]], limit=12, prefetch_limit=64, fusion="dbsf", weights=[1.0, 0.5, 2.0],
                           prefetch_thresholds=[None, 0.1, None], score_threshold=0.2, query_filter=flt)
    q = torch.from_numpy(np.stack([x[100], v, x[2002]]))[None].to(DEV)
    odd = torch.from_numpy(np.arange(N) % 2 == 1).to(DEV)
    want = _as_points(st, st.gallery.search_fusion(q, k=12, limit=64, method="dbsf", weights=[1.0, 0.5, 2.0],
                                                   list_thresholds=[None, 0.1, None], score_threshold=0.2, allow=odd,
                                                   with_list_scores=True))
    assert hits and [(h.id, h.score, h.ranks, h.scores) for h in hits] == want
    assert all(int(h.id[1:]) % 2 == 1 and h.score >= 0.2 for h in hits)
    # one prefetch is a plain search in RRF order; a single vector needs no list around it
    one = st.query_fusion(x[7], limit=5)
    assert [h.id for h in one] == [h.id for h in st.search(x[7], 5)] and [h.ranks for h in one] == [[1], [2], [3], [4], [5]]
    assert [h.scores[0] for h in one] == [h.score for h in st.search(x[7], 5)]
    assert st.query_fusion([x[7], v], limit=5, score_threshold=1.0) == []
    with pytest.raises(KeyError):
        st.query_fusion(["nobody", v])
    with pytest.raises(ValueError, match="at least one"):
        st.query_fusion([])
    with pytest.raises(ValueError, match="method"):
        st.query_fusion([v], fusion="max")
    st.close()


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


def test_search_by_text_and_image(reverso, tmp_path):
    r = reverso
    text, items = r.search_by_text_and_image("the red car")
    assert text == "❌ No query embeddings available. Please detect/process an image first." and items == []
    prompts = _prompts(200)
    emb = r.embed_text(prompts)
    D = emb.shape[1]
    g = torch.Generator().manual_seed(3)
    r.region_embeddings = [(emb[57].cpu() + 0.4 * torch.randn(D, generator=g) / D ** 0.5)]
    text, items = r.search_by_text_and_image("the red car")
    assert text == "❌ No database loaded. Please create or load a database first." and items == []
    db = store.GalleryStore(D, device=0, capacity=256)
    db.upsert(emb.cpu(), [f"p{i}" for i in range(200)],
              [{"filename": f"f{i}.jpg", "image_source": f"/nowhere/f{i}.jpg", "bbox": [0, 0, i, i], "kind": i % 2} for i in range(200)])
    r.vector_db, r.current_database = db, "prompts"
    try:
        text, items = r.search_by_text_and_image(prompts[123], max_results=6, candidates=50)
        assert text.startswith("🎯 Found 6 regions for the picture and the text (rrf):") and len(items) == 6
        assert all(set(it) == {"filename", "image_source", "bbox", "id", "score", "ranks", "scores"} for it in items)
        assert all(len(it["ranks"]) == 2 and len(it["scores"]) == 2 for it in items)
        assert [it["score"] for it in items] == sorted((it["score"] for it in items), reverse=True)
        want = db.query_fusion([r.region_embeddings[0], r.embed_text([prompts[123]])[0]], limit=6, prefetch_limit=50)
        assert [(it["id"], it["score"], it["ranks"], it["scores"]) for it in items] == [(h.id, h.score, h.ranks, h.scores) for h in want]
        assert f"1. {items[0]['filename']}  fused {items[0]['score']:.4f}" in text
        # several strings: one list each; the weights reach the kernel
        _, three = r.search_by_text_and_image([prompts[123], prompts[9]], max_results=4, candidates=50, fusion="dbsf",
                                              text_weight=0.5, image_weight=2.0)
        want = db.query_fusion([r.region_embeddings[0]] + list(r.embed_text([prompts[123], prompts[9]])), limit=4, prefetch_limit=50,
                               fusion="dbsf", weights=[2.0, 0.5, 0.5])
        assert [(it["id"], it["score"], it["ranks"]) for it in three] == [(h.id, h.score, h.ranks) for h in want]
        assert all(len(it["ranks"]) == 3 for it in three)
        # image_threshold removes image-list members; the text ranks, and the image ranks that remain, are not renumbered
        _, full = r.search_by_text_and_image(prompts[123], max_results=100, candidates=50)
        cut_at = sorted(it["scores"][0] for it in full if it["ranks"][0] > 0)[25]
        _, cut = r.search_by_text_and_image(prompts[123], max_results=100, candidates=50, image_threshold=cut_at)
        before = {it["id"]: it for it in full}
        # the region the picture came from leads the image list, the prompt's own region the text list
        assert before["p57"]["ranks"][0] == 1 and before["p123"]["ranks"][1] == 1 and before["p123"]["scores"][1] >= 1 - 1e-5
        assert 0 < len(cut) < len(full) and sum(it["ranks"][0] > 0 for it in cut) == 25
        for it in cut:
            was = before[it["id"]]
            assert it["ranks"][1] == was["ranks"][1] and it["scores"] == was["scores"]
            assert it["ranks"][0] == (was["ranks"][0] if it["scores"][0] >= cut_at else 0)
        assert max(it["ranks"][0] for it in cut) == 25 and all(it["ranks"][1] > 0 or it["ranks"][0] > 0 for it in cut)
        # a payload filter
        flt = {"must": [{"key": "kind", "match": {"value": 0}}]}
        _, even = r.search_by_text_and_image(prompts[123], max_results=5, query_filter=flt)
        assert len(even) == 5 and all(int(it["id"][1:]) % 2 == 0 for it in even)
        # a text model that cannot embed strings (no merges file): the siblings' string
        bare = SimpleReverso(model_name="PE-Tiny-T14-56", db_root=str(tmp_path / "db"), max_batch=8)
        os.environ.pop("REVERSO_BPE_VOCAB", None)
        bare.region_embeddings, bare.vector_db, bare.current_database = r.region_embeddings, db, "prompts"
        text, items = bare.search_by_text_and_image("a red pickup truck at night")
        assert items == [] and text.startswith("❌ Error embedding the text query:")
        bare.vector_db = None
        if bare.text_model is not None:
            bare.text_model.close()
    finally:
        r.vector_db, r.current_database, r.region_embeddings = None, None, None
        db.close()
