"""The case table of tests/test_facade_reports.py and scripts/facade_reports_record.py: every report the facade
(``SimpleReverso``, from ``search_similar`` to ``summarize_database``, and ``delete_images``) can return without a device or a
file, produced over a stub ``vector_db`` that answers with canned values and writes down what it was asked.

``RETURNS`` names, per method, every ``return`` of it; every case names the one it visits.  The one branch the table leaves
out lies inside the hits report of ``search_similar``: a thumbnail that actually decodes (font rendering is not portable).
The payloads' ``image_source`` paths do not exist, so every thumbnail is ``None`` and the items are JSON-clean."""
import dataclasses
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from reverso_amd import store as st
from reverso_amd.core_system import SimpleReverso

# what a stored point carries; some keys are missing on purpose (the reports' defaults: "Unknown", "", None)
PAYLOADS = [
    {"filename": "a.jpg", "image_source": "/nowhere/a.jpg", "bbox": [0, 0, 10, 10], "video": "v1"},
    {"filename": "b.jpg", "image_source": "/nowhere/b.jpg", "bbox": [1, 2, 3, 4], "video": "v1"},
    {"image_source": "/nowhere/c.jpg", "bbox": [5, 6, 7, 8], "video": "v2"},
    {"filename": "d.jpg", "bbox": [9, 9, 20, 20]},
    {"filename": "e.jpg", "image_source": "/nowhere/e.jpg"},
    {"filename": "f.jpg", "image_source": "/nowhere/f.jpg", "bbox": [2, 2, 4, 4], "video": "v2"},
]
IDS = [f"id-{r}" for r in range(len(PAYLOADS))]
SCORES = [0.98765, 0.9, 0.81234, 0.75, 0.70049, 0.5]


def _points(rows):
    return [st.ScoredPoint(IDS[r], SCORES[n], PAYLOADS[r]) for n, r in enumerate(rows)]


def _plain(x):
    """An argument as JSON holds it"""
    if torch.is_tensor(x):
        return {"tensor": x.tolist()}
    if isinstance(x, np.ndarray):
        return {"array": x.tolist()}
    if isinstance(x, Image.Image):
        return {"image": list(x.size)}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    return repr(x)


class StubStore:
    """``mode``: ``hits`` (the canned values), ``empty`` (nothing found), ``key_error`` / ``error`` (every question raises),
    ``no_points`` (a collection that holds nothing)."""

    def __init__(self, mode="hits"):
        self.mode = mode
        self.calls = []
        self.ids = [] if mode == "no_points" else list(IDS)
        self.payloads = [] if mode == "no_points" else list(PAYLOADS)
        self.path = "stub-path"
        self.collection = "stub"

    def __bool__(self):
        return True

    def __len__(self):
        return len(self.ids)

    def _answer(self, name, args, kwargs, value, nothing):
        self.calls.append([name, _plain(args), _plain(kwargs)])
        if self.mode == "key_error":
            raise KeyError("recommend: no point with id 'nope' in the store")
        if self.mode == "error":
            raise RuntimeError("stub store failure")
        return nothing if self.mode == "empty" else value

    def search(self, *a, **k):
        return self._answer("search", a, k, _points([2, 0, 5][: k.get("limit", 3)]), [])

    def search_groups(self, *a, **k):
        groups = [st.PointGroup("v1", _points([1])), st.PointGroup("v2", [st.ScoredPoint(IDS[2], 0.625, PAYLOADS[2])])]
        return self._answer("search_groups", a, k, st.GroupsResult(groups), st.GroupsResult([]))

    def query_fusion(self, *a, **k):
        hits = [st.FusedPoint(IDS[3], 0.03252, PAYLOADS[3], [1, 2], [0.9, 0.25]),
                st.FusedPoint(IDS[2], 0.01639, PAYLOADS[2], [0, 1], [0.5, 0.3125])]
        return self._answer("query_fusion", a, k, hits, [])

    def assign(self, *a, **k):
        labels = torch.tensor([0, 2, 0, -1, 2, 0], dtype=torch.int32)
        scores = torch.tensor([0.25, 0.5, 0.25, float("-inf"), 0.125, 0.375], dtype=torch.float32)
        return self._answer("assign", a, k, (labels, scores), (labels, scores))

    def search_multivector(self, *a, **k):
        res = [st.MultiVectorResult("/nowhere/a.jpg", 1.75, _points([0, 1])),
               st.MultiVectorResult("/nowhere/c.jpg", 1.5, _points([2, 2]))]
        return self._answer("search_multivector", a, k, res, [])

    def search_range(self, *a, **k):
        return self._answer("search_range", a, k, _points([4, 3, 2, 1]), [])

    def recommend(self, *a, **k):
        return self._answer("recommend", a, k, _points([5, 3]), [])

    def discover(self, *a, **k):
        return self._answer("discover", a, k, _points([0, 4, 2]), [])

    def search_mmr(self, *a, **k):
        return self._answer("search_mmr", a, k, _points([1, 5]), [])

    def duplicate_row_groups(self, *a, **k):
        return self._answer("duplicate_row_groups", a, k, [[0, 3], [1, 2, 4]], [])

    def duplicate_row_clusters(self, *a, **k):
        return self._answer("duplicate_row_clusters", a, k, [[0, 3], [1, 2, 4]], [])

    def neighbor_graph(self, *a, **k):
        g = st.NeighborGraph([IDS[0], IDS[2], IDS[3]], np.array([0, 0, 2], np.int64), np.array([1, 2, 0], np.int64),
                             np.array([0.875, 0.5, 0.25], np.float32))
        none = st.NeighborGraph([], np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
        return self._answer("neighbor_graph", a, k, g, none)

    def themes(self, *a, **k):
        themes = [st.Theme(4, [IDS[0], IDS[1], IDS[4], IDS[5]], IDS[4], 0.9375, PAYLOADS[4]),
                  st.Theme(2, [IDS[2], IDS[3]], IDS[2], 0.5, PAYLOADS[2])]
        return self._answer("themes", a, k, themes, [])

    def delete(self, *a, **k):
        return self._answer("delete", a, k, 2, 0)

    def save(self, *a, **k):
        return self._answer("save", a, k, None, None)


QUERY = [torch.tensor([0.5, 0.5, 0.5, 0.5]), torch.tensor([1.0, 0.0, 0.0, 0.0])]


def bare_facade(store, query, text_fails=False):
    """A ``SimpleReverso`` without a device: only its host-side methods work (tests/test_host_logic.py builds it so)."""
    r = object.__new__(SimpleReverso)
    r._lock = threading.RLock()
    r.vector_db = store
    r.current_database = None if store is None else store.collection
    r.region_embeddings = query
    r._decode_pool = ThreadPoolExecutor(max_workers=2)

    def embed_text(texts):
        if text_fails:
            raise RuntimeError("no tokenizer")
        return torch.stack([torch.full((4,), 0.125 * (n + 1)) for n in range(len(texts))])

    def embed_pils(pils):
        return torch.stack([torch.full((4,), 0.25 * (n + 1)) for n in range(len(pils))])

    r.embed_text = embed_text
    r._embed_pils = embed_pils
    return r


VEC = torch.tensor([0.0, 1.0, 0.0, 0.0])
ARR = np.array([0.0, 0.0, 1.0, 0.0], dtype=np.float32)
FLT = {"must": [{"key": "video", "match": {"value": "v1"}}]}


def _picture():
    return Image.new("RGB", (8, 6), (10, 20, 30))


# method -> the returns the table reaches, by name; the test counts the cases against this list
RETURNS = {
    "search_similar": ["no_query", "no_database", "no_hits", "hits"],
    "search_by_text": ["no_database", "text_error", "no_hits", "hits"],
    "search_by_text_and_image": ["no_query", "no_database", "text_error", "no_hits", "hits"],
    "label_database": ["no_database", "no_labels", "no_points", "error", "hits"],
    "search_similar_all_regions": ["no_query", "no_database", "too_many", "no_hits", "hits"],
    "search_all_similar": ["no_query", "no_database", "no_hits", "hits"],
    "search_by_examples": ["no_database", "no_positive", "key_error", "no_hits", "hits"],
    "search_by_context": ["no_database", "bad_pair", "nothing_given", "key_error", "no_hits", "hits"],
    "search_similar_diverse": ["no_query", "no_database", "no_hits", "hits"],
    "find_duplicates": ["no_database", "no_hits", "hits"],
    "find_duplicate_clusters": ["no_database", "no_hits", "hits"],
    "similarity_graph": ["no_database", "error", "no_hits", "hits"],
    "summarize_database": ["no_database", "no_points", "error", "no_hits", "hits"],
    "delete_images": ["no_database", "nothing_given", "error", "no_hits", "hits"],
}


def _case(method, outcome, *args, store="hits", query=True, text_fails=False, **kwargs):
    return {"method": method, "outcome": outcome, "store": store, "query": query, "text_fails": text_fails,
            "args": args, "kwargs": kwargs}


def cases():
    """The table: built anew for every run (a case's arguments hold tensors and images)."""
    c = _case
    many = [torch.tensor([float(n), 1.0, 0.0, 0.0]) for n in range(65)]
    out = [
        c("search_similar", "no_query", query=False),
        c("search_similar", "no_query", query=False, store=None),
        c("search_similar", "no_database", store=None),
        c("search_similar", "no_hits", store="empty"),
        c("search_similar", "no_hits", None, 7, store="empty"),
        c("search_similar", "hits"),
        c("search_similar", "hits", 0.5, 1),
        c("search_similar", "hits", similarity_threshold=0.25, max_results=3, query_filter=FLT),
        c("search_similar", "hits", group_by="video"),
        c("search_similar", "hits", 0.6, 2, query_filter=FLT, group_by="video"),
        c("search_similar", "no_hits", group_by="video", store="empty"),

        c("search_by_text", "no_database", "a dog", store=None),
        c("search_by_text", "text_error", "a dog", text_fails=True),
        c("search_by_text", "no_hits", "a dog", store="empty"),
        c("search_by_text", "no_hits", "a dog", 0.2, store="empty"),
        c("search_by_text", "hits", "a dog", query=False),
        c("search_by_text", "hits", ["a dog", "a cat"], 0.1, 2, query_filter=FLT, group_by="video"),

        c("search_by_text_and_image", "no_query", "a dog", query=False),
        c("search_by_text_and_image", "no_database", "a dog", store=None),
        c("search_by_text_and_image", "text_error", "a dog", text_fails=True),
        c("search_by_text_and_image", "no_hits", "a dog", store="empty"),
        c("search_by_text_and_image", "hits", "a dog"),
        c("search_by_text_and_image", "hits", ["a dog", "a cat"], max_results=2, candidates=50, fusion="dbsf", text_weight=0.5,
          image_weight=2.0, image_threshold=0.3, query_filter=FLT),

        c("label_database", "no_database", ["dog"], store=None),
        c("label_database", "no_labels", []),
        c("label_database", "no_points", ["dog"], store="no_points"),
        c("label_database", "error", ["dog"], store="error"),
        c("label_database", "hits", ["dog", "cat", "bird"]),
        c("label_database", "hits", "dog", query_filter=FLT, members=1),

        c("search_similar_all_regions", "no_query", query=False),
        c("search_similar_all_regions", "no_database", store=None),
        c("search_similar_all_regions", "too_many", query=many),
        c("search_similar_all_regions", "no_hits", store="empty"),
        c("search_similar_all_regions", "no_hits", 1.5, store="empty"),
        c("search_similar_all_regions", "hits"),
        c("search_similar_all_regions", "hits", 0.0, 2, query_filter=FLT, group_by="video"),

        c("search_all_similar", "no_query", query=False),
        c("search_all_similar", "no_database", store=None),
        c("search_all_similar", "no_hits", store="empty"),
        c("search_all_similar", "hits"),
        c("search_all_similar", "hits", 0.0, query_filter=FLT),

        c("search_by_examples", "no_database", ["id-1"], store=None),
        c("search_by_examples", "no_positive", []),
        c("search_by_examples", "no_positive", None, ["id-1"]),
        c("search_by_examples", "key_error", ["nope"], store="key_error"),
        c("search_by_examples", "no_hits", ["id-1"], store="empty"),
        c("search_by_examples", "no_hits", ["id-1"], similarity_threshold=0.0, store="empty"),
        c("search_by_examples", "hits", "id-2"),
        c("search_by_examples", "hits", VEC, ARR),
        c("search_by_examples", "hits", _picture()),
        c("search_by_examples", "hits", ["id-1", VEC, _picture(), ARR, _picture()], ["id-3", _picture()],
          similarity_threshold=0.5, max_results=2, query_filter=FLT),

        c("search_by_context", "no_database", None, [("id-1", "id-2")], store=None),
        c("search_by_context", "bad_pair", None, [("id-1",)]),
        c("search_by_context", "bad_pair", "id-0", ["id-1"]),
        c("search_by_context", "nothing_given", None, []),
        c("search_by_context", "nothing_given", None, None),
        c("search_by_context", "key_error", "nope", [], store="key_error"),
        c("search_by_context", "no_hits", "id-0", [], store="empty"),
        c("search_by_context", "no_hits", None, [("id-1", "id-2")], 0.0, store="empty"),
        c("search_by_context", "hits", None, [("id-1", "id-2")]),
        c("search_by_context", "hits", VEC, None),
        c("search_by_context", "hits", _picture(), [("id-1", _picture()), [ARR, VEC]], similarity_threshold=-1.0,
          max_results=3, query_filter=FLT),

        c("search_similar_diverse", "no_query", query=False),
        c("search_similar_diverse", "no_database", store=None),
        c("search_similar_diverse", "no_hits", store="empty"),
        c("search_similar_diverse", "hits"),
        c("search_similar_diverse", "hits", 0.0, 2, 1, candidates_limit=10, query_filter=FLT),

        c("find_duplicates", "no_database", store=None),
        c("find_duplicates", "no_hits", store="empty"),
        c("find_duplicates", "hits"),
        c("find_duplicates", "hits", 0.9, query_filter=FLT),

        c("find_duplicate_clusters", "no_database", store=None),
        c("find_duplicate_clusters", "no_hits", 0.99, store="empty"),
        c("find_duplicate_clusters", "hits"),
        c("find_duplicate_clusters", "hits", 0.9, query_filter=FLT, largest_first=False),

        c("similarity_graph", "no_database", store=None),
        c("similarity_graph", "error", store="error"),
        c("similarity_graph", "no_hits", store="empty"),
        c("similarity_graph", "hits"),
        c("similarity_graph", "hits", 2, 0.25, query_filter=FLT),

        c("summarize_database", "no_database", store=None),
        c("summarize_database", "no_points", store="no_points"),
        c("summarize_database", "error", store="error"),
        c("summarize_database", "no_hits", store="empty"),
        c("summarize_database", "hits"),
        c("summarize_database", "hits", 2, max_iter=3, seed=7, query_filter=FLT),

        c("delete_images", "no_database", "/nowhere/a.jpg", store=None),
        c("delete_images", "nothing_given"),
        c("delete_images", "error", "/nowhere/a.jpg", store="error"),
        c("delete_images", "no_hits", ["/nowhere/a.jpg"], store="empty"),
        c("delete_images", "hits", ["/nowhere/a.jpg", "/nowhere/b.jpg"], query_filter=FLT),
    ]
    return out


def run_case(case):
    """What the facade returns for one case and what it asked the store: ``{"text", "items", "calls"}``, JSON-clean."""
    store = None if case["store"] is None else StubStore(case["store"])
    query = case["query"] if isinstance(case["query"], list) else (list(QUERY) if case["query"] else None)
    r = bare_facade(store, query, case["text_fails"])
    try:
        res = getattr(r, case["method"])(*case["args"], **case["kwargs"])
    finally:
        r._decode_pool.shutdown()
    text, items = res if isinstance(res, tuple) else (res, None)
    return {"text": text, "items": _plain(_undataclass(items)), "calls": [] if store is None else store.calls}


def _undataclass(x):
    return dataclasses.asdict(x) if dataclasses.is_dataclass(x) and not isinstance(x, type) else x


def run_table():
    """``[{"method", "outcome", "text", "items", "calls"}]`` in table order."""
    return [dict(method=c["method"], outcome=c["outcome"], **run_case(c)) for c in cases()]
