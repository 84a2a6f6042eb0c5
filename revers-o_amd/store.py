"""Gallery store: device-resident vectors + host-side ids/payloads + persistence.

Stands where the reference keeps a ``QdrantClient(path=...)`` with one COSINE
collection (``core_system.py:100``, ``:521``, ``:600-603``, ``:608-622``, ``:659-664``).
Qdrant's sqlite format is not a compatibility target (third-party, un-pinned;
SURVEY.md §8(f) row 2).  A database directory here is append-only:

    manifest.jsonl          line 1: {"format": 2, "collection", "dim"}; then one line per DELTA SHARD, in order:
                            {"shard": i, "file", "rows", "ids": [...], "payloads": [...], "files_done": [...]};
                            one line per later change of flushed points:
                            {"op": "delete", "ids": [...]}
                            {"op": "update", "file": <new vectors or null>, "rows": n, "ids": [...], "payloads": [...]};
                            a last line {"complete": true, "rows": N} once a build has finished
    vectors.00000.f32.npy   the shard's normalised fp32 rows (the gallery's master copy)
    .lock                   present while a process has the database open

A save / checkpoint writes only the rows added since the last one (one .npy + one manifest line, the .npy first and
under a temporary name: a crash leaves at worst an orphan file no line points to) -- never the whole set: building a
1 M-vector gallery writes 4 GB once, not 4 GB per checkpoint.  The manifest of an unfinished build (no "complete"
line) IS its checkpoint: ``files_done`` says which source files the shards' rows cover (``create_database`` resumes
from there; the reference's own checkpoint is inoperative, ``core_system.py:480-489``, ``:524-538``).
Round-1/2 directories (one ``vectors.f32.npy`` + ``meta.json``) still load.
"""
import json
import os
import shutil
from dataclasses import dataclass

import numpy as np
import torch

from . import boost as _boost
from . import filters as _filters
from .engine import Gallery

MANIFEST = "manifest.jsonl"


def _fsync_dir(path):
    """Make a rename / create inside `path` durable (no-op where directories cannot be opened)."""
    try:
        fd = os.open(path, os.O_RDONLY)
    except OSError:
        return
    try:
        os.fsync(fd)
    except OSError:
        pass
    finally:
        os.close(fd)


OLD = ".revo-old"          # the set-aside previous database during a swap (a suffix no user database name is likely to end in)
OLD_LEGACY = ".old"        # what earlier builds called it: a crash under one of those may have left <db>.old behind -- recover(),
                           # list_databases and delete_database recognise it for one release (only next to a database name that
                           # is missing or was made by this package: a user database that happens to be called "x.old" and has
                           # no sibling "x" story is left alone, see is_legacy_set_aside)


def is_legacy_set_aside(root, name):
    """True if directory ``name`` = "<db>.old" under ``root`` is a previous build's set-aside copy rather than a user's
    database: it carries this package's manifest and either <db> is missing (the crash it was left by) or <db> is one of
    this package's databases too (a swap that died before the set-aside copy was removed)."""
    if not name.endswith(OLD_LEGACY) or name.endswith(OLD):
        return False
    base = os.path.join(root, name[: -len(OLD_LEGACY)])
    if not os.path.isfile(os.path.join(root, name, MANIFEST)):
        return False
    return (not os.path.isdir(base)) or os.path.isfile(os.path.join(base, MANIFEST))


def _is_complete(path):
    man = os.path.join(path, MANIFEST)
    try:
        return os.path.isfile(man) and bool(read_manifest(man)[2])
    except (OSError, ValueError):
        return False


def swap_in(build_path, db_path):
    """Replace the database directory by the finished build without a moment in which neither exists under a name
    list_databases / load_database look at: old -> <db>.revo-old, build -> <db>, then the old one is removed.  A crash in
    between leaves <db>.revo-old (complete) and possibly <db>.building (complete): recover() puts things right.
    If another process's recover() has already adopted the (complete) build under the database's name -- it can, between
    this build's last manifest line and this call -- there is nothing left to do."""
    old = db_path + OLD
    if not os.path.isdir(build_path) and _is_complete(db_path):
        return
    if os.path.isdir(old):
        shutil.rmtree(old)
    had = os.path.isdir(db_path)
    if had:
        os.replace(db_path, old)
    os.replace(build_path, db_path)
    _fsync_dir(os.path.dirname(db_path) or ".")
    if had:
        shutil.rmtree(old, ignore_errors=True)


def recover(db_path, building_suffix=".building"):
    """After a crash inside swap_in: a database that is missing while a COMPLETE build (or the set-aside old one) sits
    next to it is put back under its name.  Returns what was adopted, or None."""
    if os.path.isdir(db_path):
        return None
    for cand, what in ((db_path + building_suffix, "build"), (db_path + OLD, "old"), (db_path + OLD_LEGACY, "old")):
        man = os.path.join(cand, MANIFEST)
        if os.path.isfile(man):
            try:
                complete = read_manifest(man)[2]
            except (OSError, ValueError):
                complete = False
            if complete:
                os.replace(cand, db_path)
                return what
    return None


def read_manifest(man):
    """Parse a manifest.  Returns (header, records in order, complete, bytes of the file that are whole lines).  The
    records are the shard lines and, between them, the ``"op"`` lines of deletes and updates (:func:`replay_manifest` turns
    them into the points they leave).  A torn last line -- the process died while appending -- ends the parse: everything
    before it stands."""
    header, shards, complete, good = None, [], False, 0
    with open(man, "rb") as f:
        for raw in f:
            if not raw.endswith(b"\n"):
                break
            ln = raw.strip()
            if ln:
                try:
                    rec = json.loads(ln)
                except ValueError:
                    break
                if header is None:
                    header = rec
                elif rec.get("complete"):
                    complete = True
                else:
                    complete = False                   # rows appended after a save: complete again at the next save
                    shards.append(rec)
            good += len(raw)
    if header is None:
        raise ValueError(f"{man}: empty manifest")
    return header, shards, complete, good


def replay_manifest(records):
    """The points a manifest's records (the second value of :func:`read_manifest`) leave, in the order of the store's rows:
    a list of ``(id, payload, (vectors file, row in that file))``.  Pure host code: no device, no arrays.

    A shard line appends its points.  ``{"op": "delete", "ids"}`` takes out every point with one of the ids (unknown ids
    are ignored); the rest keep their order.  ``{"op": "update", "file", "rows", "ids", "payloads"}`` gives the point of
    ``ids[i]`` (the last one, should the id occur twice) the payload ``payloads[i]`` and, unless ``file`` is null, the
    vector in row i of ``file``; the point keeps its place.  An id deleted and upserted again is a new point at the end."""
    points = []
    last = None                      # id -> its last place in points, built when an update needs it, dropped when places move
    for rec in records:
        op = rec.get("op")
        if op is None:
            if rec["rows"] != len(rec["ids"]) or rec["rows"] != len(rec["payloads"]):
                raise ValueError(f"manifest: shard line {rec.get('shard')} names {rec['rows']} rows but lists "
                                 f"{len(rec['ids'])} ids and {len(rec['payloads'])} payloads")
            for i, (pid, pl) in enumerate(zip(rec["ids"], rec["payloads"])):
                if last is not None:
                    last[pid] = len(points)
                points.append((pid, pl, (rec["file"], i)))
        elif op == "delete":
            gone = set(rec["ids"])
            points = [p for p in points if p[0] not in gone]
            last = None
        elif op == "update":
            if last is None:
                last = {p[0]: r for r, p in enumerate(points)}
            for i, (pid, pl) in enumerate(zip(rec["ids"], rec["payloads"])):
                r = last[pid]        # KeyError: the manifest updates a point it never held
                points[r] = (pid, pl, (rec["file"], i) if rec["file"] is not None else points[r][2])
        else:
            raise ValueError(f"manifest: unknown op {op!r} (written by a newer version?)")
    return points


@dataclass
class ScoredPoint:
    """Shape of a qdrant search hit as the reference consumes it (core_system.py:671-676)."""
    id: str
    score: float
    payload: dict


@dataclass
class BoostedPoint(ScoredPoint):
    """One hit of :meth:`GalleryStore.search_boosted`: ``score`` is the boosted score, ``similarity`` the plain search score."""
    similarity: float = 0.0


@dataclass
class FusedPoint:
    """One hit of a hybrid query (:meth:`GalleryStore.query_fusion`): the fused ``score``, and per fused list the point's
    1-based rank in it (0: not in the list) and its score against that list's query."""
    id: str
    score: float
    payload: dict
    ranks: list
    scores: list


@dataclass
class PointGroup:
    """One group of a grouped search (Qdrant's ``PointGroup``): the payload value ``id`` and its best hits."""
    id: object
    hits: list


@dataclass
class MultiVectorResult:
    """One group of a multi-vector search: the payload value ``value``, its MaxSim ``score`` and, per query vector, the
    point of the group that matched it best (``hits[i].score`` is query vector i's share of ``score``)."""
    value: object
    score: float
    hits: list


@dataclass
class GroupsResult:
    """Qdrant's ``GroupsResult``: the groups best first."""
    groups: list


@dataclass
class DuplicatePair:
    """Two points whose vectors score at least the threshold of :meth:`GalleryStore.duplicate_pairs`."""
    id_a: str
    id_b: str
    score: float


@dataclass
class NeighborGraph:
    """What :meth:`GalleryStore.neighbor_graph` returns, in the shape of the database's matrix-offsets response: ``ids`` are
    the points of the graph in storage order; edge e goes from ``ids[offsets_row[e]]`` to its neighbour
    ``ids[offsets_col[e]]`` with ``scores[e]``.  Edges are ordered by source point, each point's neighbours best first."""
    ids: list
    offsets_row: np.ndarray
    offsets_col: np.ndarray
    scores: np.ndarray

    def pairs(self):
        """The edges as ``(id_a, id_b, score)`` tuples, in edge order (the matrix-pairs response)."""
        return [(self.ids[a], self.ids[b], float(s))
                for a, b, s in zip(self.offsets_row.tolist(), self.offsets_col.tolist(), self.scores.tolist())]


@dataclass
class Theme:
    """One theme of :meth:`GalleryStore.themes`: its ``size``, its members' point ids in storage order, and its
    representative -- the member that scores highest against the theme's centre (ties: the first in storage order)."""
    size: int
    ids: list
    representative_id: str
    representative_score: float
    representative_payload: dict


def seed_rows(mask, n, seed=0):
    """``n`` distinct rows of those ``mask`` (bool [len]) selects, drawn without replacement by a generator seeded with
    ``seed``, in ascending order: the initial centroids of :meth:`GalleryStore.themes`.  Raises if fewer are selected."""
    rows = np.flatnonzero(np.asarray(mask, dtype=bool))
    n = int(n)
    if n < 1:
        raise ValueError("n_themes must be at least 1")
    if rows.size < n:
        raise ValueError(f"{n} themes asked of {rows.size} selected points")
    return np.sort(np.random.default_rng(seed).choice(rows, size=n, replace=False)).astype(np.int64)


def assemble_themes(ids, payloads, labels, sizes, representatives, scores):
    """``Gallery.kmeans``'s host arrays as :class:`Theme` entries, largest first (equal sizes: the lower centroid first);
    centroids without members are left out.  ``labels`` [len] (-1: not a participant), ``sizes`` [C], ``representatives`` [C]
    the row of each centroid's representative (-1: none), ``scores`` [len]."""
    labels = np.asarray(labels, dtype=np.int64)
    sizes = np.asarray(sizes, dtype=np.int64)
    order = np.argsort(labels, kind="stable")                         # members of a centroid stay in storage order
    order = order[labels[order] >= 0]
    ends = np.cumsum(sizes)
    if order.size != (int(ends[-1]) if ends.size else 0):
        raise ValueError("assemble_themes: the sizes do not add up to the labelled rows")
    out = []
    for c in sorted(range(sizes.size), key=lambda c: (-int(sizes[c]), c)):
        if sizes[c] == 0:
            continue
        members = order[int(ends[c] - sizes[c]):int(ends[c])]
        r = int(representatives[c])
        if r < 0 or labels[r] != c:
            raise ValueError("assemble_themes: a representative outside its theme")
        out.append(Theme(int(sizes[c]), [ids[m] for m in members.tolist()], ids[r], float(scores[r]), payloads[r]))
    return out


def sample_mask(mask, sample, seed=0):
    """``mask`` (bool [n]) restricted to ``sample`` of its set entries, drawn without replacement by a generator seeded with
    ``seed`` (all of them when ``sample`` is None or not smaller than their number).  A new array."""
    mask = np.asarray(mask, dtype=bool)
    rows = np.flatnonzero(mask)
    if sample is None or int(sample) >= rows.size:
        return mask.copy()
    if int(sample) < 0:
        raise ValueError("sample must not be negative")
    out = np.zeros_like(mask)
    out[np.random.default_rng(seed).choice(rows, size=int(sample), replace=False)] = True
    return out


def knn_to_graph(ids, mask, scores, idx, counts):
    """``Gallery.knn``'s arrays (host copies: scores / idx [n, k], counts [n]) over the rows ``mask`` selects, as a
    :class:`NeighborGraph` over those rows' ids."""
    mask = np.asarray(mask, dtype=bool)
    rows = np.flatnonzero(mask)
    place = np.full(mask.shape[0], -1, dtype=np.int64)
    place[rows] = np.arange(rows.size)
    counts = np.asarray(counts, dtype=np.int64)[rows]
    k = scores.shape[1] if scores.ndim == 2 else 0
    take = np.arange(k)[None, :] < counts[:, None]                    # [rows, k]: the entries that are results
    cols = np.asarray(idx)[rows][take]
    if cols.size and (place[cols] < 0).any():
        raise ValueError("knn_to_graph: a neighbour outside the selected rows")
    return NeighborGraph([ids[r] for r in rows.tolist()], np.repeat(np.arange(rows.size, dtype=np.int64), counts),
                         place[cols].astype(np.int64), np.asarray(scores)[rows][take].astype(np.float32))


def connected_groups(pairs, n):
    """The connected components with at least two members of the graph on rows ``0 .. n - 1`` whose edges are ``pairs``
    (int array [m, 2]): lists of rows, each in ascending order, the lists ordered by their first row.  Union-find on numpy."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b in pairs.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)        # the smaller row is the root: a component's root is its first row
    rows = np.unique(pairs)
    roots = np.array([find(r) for r in rows.tolist()], dtype=np.int64)
    groups = {}
    for r, root in zip(rows.tolist(), roots.tolist()):
        groups.setdefault(root, []).append(r)
    return [groups[root] for root in sorted(groups) if len(groups[root]) >= 2]


def split_clusters(offsets, members):
    """The CSR ``(offsets [n + 1], members)`` of ``Gallery.clusters`` as a list of lists of rows."""
    offsets = np.asarray(offsets, dtype=np.int64).tolist()
    members = np.asarray(members, dtype=np.int64).tolist()
    return [members[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


def largest_first(groups):
    """``groups`` (lists of rows, each ascending) ordered by (size descending, first row ascending)."""
    return sorted(groups, key=lambda g: (-len(g), g[0]))


def average_vector_query(positive, negative=None):
    """The query vector of Qdrant's ``average_vector`` recommendation strategy (host, numpy): with the examples normalised,
    ``mean(positive) + (mean(positive) - mean(negative))``, or ``mean(positive)`` alone without negatives.  fp32 ``[dim]``."""
    def unit_rows(a):
        a = np.asarray(a, dtype=np.float32)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        return a / np.linalg.norm(a, axis=1, keepdims=True)
    pos = unit_rows(positive).mean(axis=0)
    if negative is None or np.asarray(negative).size == 0:
        return pos.astype(np.float32)
    return (pos + (pos - unit_rows(negative).mean(axis=0))).astype(np.float32)


class GalleryStore:
    _mutations = 0           # counts every upsert, delete, update and set_payload (the key of search_boosted's cache)
    _boost_cache = None      # ((formula key, filter key, _mutations), device mult, device bias) of the last boosted search

    def __init__(self, dim, device=0, capacity=65536, collection="simple_reverso", path=None, _fresh=True, build_info=None):
        """``build_info``: what the vectors were made from and how (source folder, model, region mode, ...), written into
        the manifest header; a resume compares it (core_system.create_database) so that rows of different builds never mix."""
        self.build_info = dict(build_info or {})
        self.dim = int(dim)
        self.device = device
        self.collection = collection
        self.path = path
        self.ids = []
        self.payloads = []
        self.gallery = Gallery(self.dim, max(int(capacity), 1), device=device)
        self.complete = False
        self._flushed = 0            # rows already in shards on disk
        self._shards = 0
        self._files_pending = []     # source files whose rows were added since the last flush
        self.files_done = set()      # source files covered by the shards on disk
        self._pindex = _filters.PayloadIndex()   # columnar payload index of query_filter, caught up lazily
        self._filter_cache = None                # (filter key, len(store), device allow-bitmap) of the last filtered search
        self._group_cache = None                 # ((group_by, len(store)), device group ids, values) of the last grouped search
        self._id_rows = None                     # (len(store), {point id: row}) of the last recommend by id
        if path:
            os.makedirs(path, exist_ok=True)
            open(os.path.join(path, ".lock"), "a").close()
            if _fresh:
                with open(os.path.join(path, MANIFEST), "w") as f:
                    f.write(json.dumps({"format": 2, "collection": collection, "dim": self.dim, "build": self.build_info}) + "\n")

    def __len__(self):
        return len(self.ids)

    def _grow(self, need):
        if need <= self.gallery.capacity:
            return
        cap = max(need, 2 * self.gallery.capacity)         # geometric: a build of N rows copies < 2 N rows in all
        old = self.gallery
        new = Gallery(self.dim, cap, device=self.device)
        n = len(old)
        step = max(1, (128 << 20) // (self.dim * 4))       # 128 MB of fp32 rows at a time: the peak is old + new + one chunk,
        for s0 in range(0, n, step):                       # not old + new + a full fp32 copy of old
            new.add(old.read(s0, min(step, n - s0)), normalize=False)       # device to device
        old.close()
        self.gallery = new

    def upsert(self, vectors, ids, payloads, files=None, replace_existing=False, skip_duplicates=None):
        """vectors: [n, dim] fp32 tensor, host or DEVICE (an ingest appends its embeddings where they are: they never
        visit the host); rows are normalised at insert.  ``files``: source files these rows complete (resume bookkeeping).
        ``replace_existing=True`` is the database's own upsert: a point whose id is already in the store gets the new vector
        and payload in place, the others are appended (of an id given twice in one call the last entry counts).  The
        default appends every row, whatever its id.
        ``skip_duplicates=t`` (a float) is the insert-time dedup (include/revo.h, DEDUP): in order, a point whose vector
        scores >= t against a stored point or an earlier kept point of this call is not stored.  Only kept points enter the
        ids, the payloads and the shards; ``files`` is recorded as ever (a file whose rows were all dropped is done).  The call
        then returns ``{"kept": n, "dropped": [(id, representative id, score), ...]}``.  Not with ``replace_existing``."""
        if skip_duplicates is not None:
            if replace_existing:
                raise ValueError("upsert: skip_duplicates and replace_existing exclude each other (a replaced point keeps its row)")
            skip_duplicates = float(skip_duplicates)
            if skip_duplicates != skip_duplicates:
                raise ValueError("upsert: skip_duplicates is NaN")
        vectors = torch.as_tensor(vectors, dtype=torch.float32)
        assert vectors.shape[0] == len(ids) == len(payloads)
        report = None if skip_duplicates is None else {"kept": 0, "dropped": []}
        if replace_existing and vectors.shape[0]:
            last = {pid: i for i, pid in enumerate(ids)}
            have = self._id_row_map()
            old = [i for i in sorted(last.values()) if ids[i] in have]
            new = [i for i in sorted(last.values()) if ids[i] not in have]
            if old:
                self._update([ids[i] for i in old], vectors[old], [payloads[i] for i in old])
            vectors, ids, payloads = vectors[new], [ids[i] for i in new], [payloads[i] for i in new]
        if vectors.shape[0]:
            self._grow(len(self) + vectors.shape[0])           # (room for every row of the call, kept or not)
            if skip_duplicates is None:
                self.gallery.add(vectors, normalize=True)
            else:
                rows, scores, kept = (a.cpu().tolist() for a in self.gallery.add_unique(vectors, skip_duplicates))
                base = len(self.ids)
                kept_ids = [pid for pid, k in zip(ids, kept) if k]
                report["kept"] = len(kept_ids)
                report["dropped"] = [(pid, self.ids[r] if r < base else kept_ids[r - base], s)
                                     for pid, r, s, k in zip(ids, rows, scores, kept) if not k]
                ids, payloads = kept_ids, [p for p, k in zip(payloads, kept) if k]
            self.ids.extend(ids)
            self.payloads.extend(payloads)
        if files:
            self._files_pending.extend(files)
        self.complete = False
        self._mutations += 1
        self._boost_cache = None
        return report

    # -- changes of stored points (include/revo.h, EDIT): on the device in place, on disk one manifest line each ------
    def _id_row_map(self):
        if self._id_rows is None or self._id_rows[0] != len(self):
            self._id_rows = (len(self), {pid: r for r, pid in enumerate(self.ids)})
        return self._id_rows[1]

    def _points_changed(self):
        """ids / payloads changed under the caches built from them"""
        self._pindex = _filters.PayloadIndex()
        self._filter_cache = self._group_cache = self._id_rows = self._boost_cache = None
        self._mutations += 1
        self.complete = False

    def _log_op(self, line):
        """one fsynced manifest line: a crash before it leaves the database as it was"""
        with open(os.path.join(self.path, MANIFEST), "a") as f:
            f.write(json.dumps(line) + "\n")
            f.flush()
            os.fsync(f.fileno())
        self._shards += 1
        self._flushed = len(self)

    def delete(self, points):
        """Remove points: ``points`` is a list of ids (unknown ones are ignored) or a filter (``filters.Filter`` or its dict
        form).  Every row that carries the id of a selected point goes (a store filled without ``replace_existing`` may
        hold an id twice).  The rows move on the device (``Gallery.remove``); ``ids`` and ``payloads`` close up the same
        way.  Returns the number of points removed.  A store with a directory first flushes, then appends a ``delete``
        line to the manifest: the shards are not rewritten -- ``save(path=<other directory>)`` writes a compact copy.
        A ``ShardedSearch`` over the gallery is to be refreshed afterwards."""
        if isinstance(points, (_filters.Filter, dict)):
            gone = {self.ids[r] for r in np.flatnonzero(self.filter_mask(points)).tolist()}
        else:
            gone = set(points)
        mask = np.fromiter((pid in gone for pid in self.ids), dtype=bool, count=len(self.ids))
        n = int(mask.sum())
        if n == 0:
            return 0
        if self.path:
            self.flush()
        removed = self.gallery.remove(torch.from_numpy(mask))
        assert removed == n, (removed, n)
        dead = list(dict.fromkeys(self.ids[r] for r in np.flatnonzero(mask).tolist()))
        self.ids = [pid for pid, m in zip(self.ids, mask.tolist()) if not m]
        self.payloads = [pl for pl, m in zip(self.payloads, mask.tolist()) if not m]
        self._points_changed()
        if self.path:
            self._log_op({"op": "delete", "ids": dead})
        return n

    def _update(self, ids, vectors, payloads):
        """the points ``ids`` (each once, all present) get ``vectors`` (None: kept) and ``payloads`` (None: kept)"""
        have = self._id_row_map()
        missing = [pid for pid in ids if pid not in have]
        if missing:
            raise KeyError(f"no point with id {missing[0]!r} in the store")
        if len(set(ids)) != len(ids):
            raise ValueError("an id is given twice")
        if not ids:
            return
        rows = [have[pid] for pid in ids]
        if self.path:
            self.flush()
        if vectors is not None:
            vectors = torch.as_tensor(vectors, dtype=torch.float32)
            self.gallery.update(rows, vectors, normalize=True)
        if payloads is not None:
            for r, pl in zip(rows, payloads):
                self.payloads[r] = pl
        id_rows = self._id_rows
        self._points_changed()
        self._id_rows = id_rows                              # no row moved
        if self.path:
            name = None
            if vectors is not None:
                name = f"vectors.{self._shards:05d}.f32.npy"
                vec = torch.cat([self.gallery.read(r, 1) for r in rows]).cpu().numpy()      # the rows as stored: normalised
                tmp = os.path.join(self.path, name + ".tmp.npy")
                with open(tmp, "wb") as f:
                    np.save(f, vec)
                    f.flush()
                    os.fsync(f.fileno())
                os.replace(tmp, os.path.join(self.path, name))
                _fsync_dir(self.path)
            self._log_op({"op": "update", "file": name, "rows": len(rows), "ids": list(ids),
                          "payloads": [self.payloads[r] for r in rows]})

    def update_vectors(self, ids, vectors):
        """New vectors (normalised at insert, like an upsert's) for the points ``ids``; payloads and places stay.  An
        unknown id raises ``KeyError``.  With a directory: flush, then one ``update`` manifest line naming a new vectors file."""
        vectors = torch.as_tensor(vectors, dtype=torch.float32)
        assert vectors.shape[0] == len(ids)
        self._update(list(ids), vectors, None)

    def set_payload(self, ids, payload):
        """Replace the payload of the points ``ids`` by ``payload`` (one dict for all of them, or a list with one per id).
        Host only: no vector is touched.  An unknown id raises ``KeyError``."""
        ids = list(ids)
        payloads = [payload] * len(ids) if isinstance(payload, dict) else list(payload)
        assert len(payloads) == len(ids)
        self._update(ids, None, payloads)

    def filter_mask(self, query_filter):
        """bool numpy [len(self)]: the points a Qdrant-style filter (filters.Filter or its dict form) selects."""
        return self._pindex.sync(self.ids, self.payloads).evaluate(query_filter)

    def _allow_bits(self, query_filter):
        key = (_filters.filter_key(query_filter), len(self))
        if self._filter_cache is None or self._filter_cache[0] != key:
            bits = torch.from_numpy(_filters.pack_bits(self.filter_mask(query_filter))).to(self.gallery.device)
            self._filter_cache = (key, bits)
        return self._filter_cache[1]

    def _points(self, scores, rows):
        """The hits of a result: host lists of scores and of the rows that have them."""
        return [ScoredPoint(self.ids[j], float(sc), self.payloads[j]) for sc, j in zip(scores, rows)]

    def search(self, query_vector, limit, score_threshold=None, query_filter=None):
        """One query, qdrant-style result list (core_system.py:659-664).  ``query_filter`` (Qdrant's ``Filter`` shape, see
        filters.py, or its dict form): only points it selects are searched -- exactly, in the kernels, not by dropping hits."""
        q = torch.as_tensor(query_vector, dtype=torch.float32).reshape(1, -1)
        dev = self.gallery.device
        allow = self._allow_bits(query_filter) if query_filter is not None else None
        s, i, c = self.gallery.search(q.to(dev), k=int(limit), score_threshold=score_threshold, allow=allow)
        n = int(c[0])
        s, i = s[0, :n].tolist(), i[0, :n].tolist()
        return self._points(s, i)

    def search_mmr(self, query_vector, limit, diversity=0.5, candidates_limit=None, score_threshold=None, query_filter=None):
        """One query, diverse results (Qdrant's ``Mmr(diversity, candidates_limit)`` re-ranking of a nearest-neighbour query):
        of the best ``candidates_limit`` points (default ``min(1024, max(limit, 100))``; selected by ``query_filter``, cut at
        ``score_threshold``) ``limit`` are picked greedily, each pick trading its score against its similarity to the points
        already picked.  Returns the :class:`ScoredPoint` list in pick order, ``score`` = the point's plain search score.
        Exact (include/revo.h, MMR); ``diversity=0`` is :meth:`search`."""
        q = torch.as_tensor(query_vector, dtype=torch.float32).reshape(1, -1)
        allow = self._allow_bits(query_filter) if query_filter is not None else None
        s, _, i, c = self.gallery.search_mmr(q.to(self.gallery.device), k=int(limit), candidates=candidates_limit,
                                             diversity=float(diversity), score_threshold=score_threshold, allow=allow)
        n = int(c[0])
        s, i = s[0, :n].tolist(), i[0, :n].tolist()
        return self._points(s, i)

    def search_range_batch(self, query_vectors, score_threshold, query_filter=None):
        """Every point (selected by ``query_filter``, if given) whose vector scores at least ``score_threshold`` against each
        query: one :class:`ScoredPoint` list per query, best first, with no cap on its length -- e.g. "which of these new
        vectors are already in the database".  Exact (include/revo.h, RANGE)."""
        q = torch.as_tensor(query_vectors, dtype=torch.float32)
        q = q.reshape(-1, q.shape[-1]) if q.dim() != 2 else q
        if q.shape[0] == 0:
            return []
        allow = self._allow_bits(query_filter) if query_filter is not None else None
        off, idx, sc = self.gallery.search_range(q.to(self.gallery.device), float(score_threshold), allow=allow)
        off, idx, sc = off.tolist(), idx.tolist(), sc.tolist()
        return [self._points(sc[off[r]:off[r + 1]], idx[off[r]:off[r + 1]]) for r in range(len(off) - 1)]

    def search_range(self, query_vector, score_threshold, query_filter=None):
        """One query: every point (selected by ``query_filter``, if given) scoring at least ``score_threshold``, best first --
        :meth:`search` without ``limit``."""
        q = torch.as_tensor(query_vector, dtype=torch.float32).reshape(1, -1)
        return self.search_range_batch(q, score_threshold, query_filter=query_filter)[0]

    def _row_of_id(self, point_id):
        if self._id_rows is None or self._id_rows[0] != len(self):
            self._id_rows = (len(self), {pid: r for r, pid in enumerate(self.ids)})
        try:
            return self._id_rows[1][point_id]
        except (KeyError, TypeError):
            raise KeyError(f"recommend: no point with id {point_id!r} in the store") from None

    def _example_vectors(self, examples):
        """(fp32 [n, dim] device tensor, rows of the examples given by id) of a list of point ids and / or vectors"""
        if examples is None:
            examples = []
        elif isinstance(examples, (str, bytes, int)) or (torch.is_tensor(examples) and examples.dim() == 1) or \
                (isinstance(examples, np.ndarray) and examples.ndim == 1):
            examples = [examples]
        dev = self.gallery.device
        vecs, rows = [], []
        for e in examples:
            if isinstance(e, (str, bytes, int)):
                r = self._row_of_id(e)
                rows.append(r)
                vecs.append(self.gallery.read(r, 1)[0])
            else:
                vecs.append(torch.as_tensor(e, dtype=torch.float32).reshape(-1).to(dev))
        out = torch.stack(vecs) if vecs else torch.empty((0, self.dim), dtype=torch.float32, device=dev)
        if out.shape[1] != self.dim:
            raise ValueError(f"recommend: example vectors must have {self.dim} elements")
        return out, rows

    def recommend(self, positive, negative=None, limit=5, score_threshold=None, query_filter=None, strategy="best_score"):
        """Search by examples in Qdrant's shape: each example is a point id of the store or a vector.  Points given by id
        are never part of the result.  ``strategy="best_score"``: a point's score is its best score against a positive if
        that beats its best score against a negative, else minus the square of the latter -- exact (include/revo.h,
        RECOMMEND), up to 128 examples, ``limit <= 1024``.  ``strategy="average_vector"``: :meth:`search` of
        :func:`average_vector_query`.  An unknown id raises ``KeyError``."""
        if strategy not in ("best_score", "average_vector"):
            raise ValueError(f"recommend: unknown strategy {strategy!r} (best_score, average_vector)")
        pos, prow = self._example_vectors(positive)
        neg, nrow = self._example_vectors(negative)
        if pos.shape[0] < 1:
            raise ValueError("recommend: needs at least one positive example")
        allow = None
        if prow or nrow or query_filter is not None:
            mask = self.filter_mask(query_filter).copy() if query_filter is not None else np.ones(len(self), dtype=bool)
            mask[prow + nrow] = False
            allow = torch.from_numpy(_filters.pack_bits(mask)).to(self.gallery.device)
        if strategy == "average_vector":
            q = torch.from_numpy(average_vector_query(pos.cpu().numpy(), neg.cpu().numpy())).to(self.gallery.device)
            s, i, c = self.gallery.search(q[None], k=int(limit), score_threshold=score_threshold, allow=allow)
            s, i, n = s[0], i[0], int(c[0])
        else:
            s, i, c = self.gallery.recommend(pos, neg if neg.shape[0] else None, k=int(limit), score_threshold=score_threshold,
                                             allow=allow)
            n = int(c)
        return self._points(s[:n].tolist(), i[:n].tolist())

    def discover(self, target=None, context=(), limit=5, score_threshold=None, query_filter=None):
        """Discovery search in Qdrant's shape: ``context`` is a list of ``(positive, negative)`` pairs and ``target`` the
        vector to find matches for; ``target`` and every member of a pair is a point id of the store or a vector.  A point
        is ranked first by the number of pairs it lies on the positive side of, then by its similarity to the target.
        ``target=None`` is the context search: the points that satisfy the pairs, scored 0 when they satisfy all of them
        and below 0 otherwise (1 to 64 pairs; with a target 0 to 63).  Points given by id are never part of the result; an
        unknown id raises ``KeyError``.  Exact (include/revo.h, DISCOVER), ``limit <= 1024``."""
        context = list(context or ())
        if any(not isinstance(pair, (tuple, list)) or len(pair) != 2 for pair in context):
            raise ValueError("discover: every context entry must be a (positive, negative) pair")
        if target is None and not context:
            raise ValueError("discover: needs a target or at least one context pair")
        pos, prow = self._example_vectors([p for p, _ in context])
        neg, nrow = self._example_vectors([n for _, n in context])
        tgt, trow = (None, []) if target is None else self._example_vectors([target])
        allow = None
        if prow or nrow or trow or query_filter is not None:
            mask = self.filter_mask(query_filter).copy() if query_filter is not None else np.ones(len(self), dtype=bool)
            mask[prow + nrow + trow] = False
            allow = torch.from_numpy(_filters.pack_bits(mask)).to(self.gallery.device)
        s, i, c = self.gallery.discover(None if tgt is None else tgt[0], pos, neg, k=int(limit), score_threshold=score_threshold,
                                        allow=allow)
        n = int(c)
        return self._points(s[:n].tolist(), i[:n].tolist())

    def search_boosted(self, query_vector, limit, formula, score_threshold=None, min_similarity=None, query_filter=None,
                       defaults=None):
        """One query rescored by a formula over ``$score`` and the points' payloads (the database's score-boosting query;
        boost.py has the formula's shape): "like this, but prefer the ones taken near this date".  The formula must be
        affine in ``$score`` with a coefficient >= 0 on every point searched; it then is ``M * $score + B`` per point, and
        the device search (include/revo.h, BOOSTED) ranks EVERY point ``query_filter`` selects by it -- no prefetched
        candidate list a late winner could be missing from.  ``min_similarity`` cuts on the plain score, ``score_threshold``
        on the boosted one; ``defaults`` gives payload keys a value where a point lacks them.  Returns
        :class:`BoostedPoint` s, best boosted score first, ``limit <= 1024``.  The per-point arrays are cached on the device
        per (formula, filter, state of the store): any upsert, delete, update or ``set_payload`` drops them."""
        q = torch.as_tensor(query_vector, dtype=torch.float32).reshape(-1)
        dev = self.gallery.device
        allow = self._allow_bits(query_filter) if query_filter is not None else None
        key = (_boost.formula_key(formula, defaults), _filters.filter_key(query_filter) if query_filter is not None else None,
               self._mutations)
        if self._boost_cache is None or self._boost_cache[0] != key:
            mask = self.filter_mask(query_filter) if query_filter is not None else None
            m, b = _boost.compile_formula(formula, self.payloads, defaults=defaults, allowed=mask)
            self._boost_cache = (key, torch.from_numpy(m).to(dev), torch.from_numpy(b).to(dev))
        _, m, b = self._boost_cache
        s, sim, i, c = self.gallery.search_boosted(q.to(dev), m, b, k=int(limit), score_threshold=score_threshold,
                                                   min_similarity=min_similarity, allow=allow)
        n = int(c)
        return [BoostedPoint(self.ids[j], float(sc), self.payloads[j], float(sm))
                for sc, sm, j in zip(s[:n].tolist(), sim[:n].tolist(), i[:n].tolist())]

    def query_fusion(self, prefetch, limit=5, prefetch_limit=100, fusion="rrf", rrf_k=60.0, weights=None, prefetch_thresholds=None,
                     score_threshold=None, query_filter=None):
        """Hybrid query in Qdrant's shape (``prefetch`` + ``fusion``): every entry of ``prefetch`` is a point id of the store or
        a vector -- an image embedding and a text embedding, say -- and is searched for its best ``prefetch_limit`` points
        (selected by ``query_filter``); the lists are fused by ``fusion``: ``"rrf"`` (reciprocal rank fusion with the constant
        ``rrf_k``) or ``"dbsf"`` (each list's scores standardised by its own mean and deviation, then added).  ``weights``
        and ``prefetch_thresholds`` hold one entry per prefetch (a threshold drops that list's points below it; the ranks
        behind them stay).  Returns :class:`FusedPoint` objects, best first: ``score`` is the fused score, ``ranks[j]`` the
        point's 1-based rank in list j (0: not in it), ``scores[j]`` its exact score against prefetch j, in the list or not.
        Points given by id are never part of the result; an unknown id raises ``KeyError``.  Exact (include/revo.h, FUSION):
        1 to 64 prefetches, ``prefetch_limit <= 1024`` and ``len(prefetch) * prefetch_limit <= 8192``, ``limit <= 1024``."""
        if isinstance(prefetch, (str, bytes, int)) or (torch.is_tensor(prefetch) and prefetch.dim() == 1) or \
                (isinstance(prefetch, np.ndarray) and prefetch.ndim == 1):
            prefetch = [prefetch]
        q, rows = self._example_vectors(list(prefetch))
        if q.shape[0] < 1:
            raise ValueError("query_fusion: needs at least one prefetch")
        allow = None
        if rows or query_filter is not None:
            mask = self.filter_mask(query_filter).copy() if query_filter is not None else np.ones(len(self), dtype=bool)
            mask[rows] = False
            allow = torch.from_numpy(_filters.pack_bits(mask)).to(self.gallery.device)
        s, i, c, r, ls = self.gallery.search_fusion(q[None], k=int(limit), limit=int(prefetch_limit), method=fusion, rrf_k=rrf_k,
                                                    weights=weights, list_thresholds=prefetch_thresholds,
                                                    score_threshold=score_threshold, allow=allow, with_list_scores=True)
        n = int(c[0])
        return [FusedPoint(self.ids[j], float(sc), self.payloads[j], ranks, scores)
                for sc, j, ranks, scores in zip(s[0, :n].tolist(), i[0, :n].tolist(), r[0, :n].tolist(), ls[0, :n].tolist())]

    def _group_ids(self, group_by):
        key = (group_by, len(self))
        if self._group_cache is None or self._group_cache[0] != key:
            ids, values = self._pindex.sync(self.ids, self.payloads).group_ids(group_by)
            self._group_cache = (key, torch.from_numpy(ids).to(self.gallery.device), values)
        return self._group_cache[1], self._group_cache[2]

    def search_groups(self, query_vector, group_by, limit, group_size=1, score_threshold=None, query_filter=None):
        """One query, Qdrant's ``search_groups`` shape: the best ``limit`` values of payload key ``group_by``, each with its
        best ``group_size`` hits (``limit * group_size <= 50``).  Points without a str / int value under the key are in no
        group; a list value raises ValueError.  Exact, in the kernels (include/revo.h, GROUPED)."""
        q = torch.as_tensor(query_vector, dtype=torch.float32).reshape(1, -1)
        dev = self.gallery.device
        groups, values = self._group_ids(group_by)
        allow = self._allow_bits(query_filter) if query_filter is not None else None
        s, i, hc, gid, gc = self.gallery.search_groups(q.to(dev), groups, limit=int(limit), group_size=int(group_size),
                                                       score_threshold=score_threshold, allow=allow)
        s, i, hc, gid = s[0].tolist(), i[0].tolist(), hc[0].tolist(), gid[0].tolist()
        out = []
        for r in range(int(gc[0])):
            out.append(PointGroup(values[gid[r]], self._points(s[r][:hc[r]], i[r][:hc[r]])))
        return GroupsResult(out)

    def search_multivector(self, query_vectors, group_by, limit=5, score_threshold=None, query_filter=None):
        """A set of query vectors against the points grouped by payload key ``group_by`` (multi-vector points with the
        MaxSim comparator): a group's score is the sum over the query vectors of its best score among the group's points
        that ``query_filter`` selects.  Returns the best ``limit <= 1024`` groups as :class:`MultiVectorResult` entries
        (``value``: the group's payload value, ``score``, ``hits``: one :class:`ScoredPoint` per query vector, the point
        that matched it best with that score).  Up to 64 query vectors.  Exact (include/revo.h, MAXSIM)."""
        q = torch.as_tensor(query_vectors, dtype=torch.float32)
        q = q.reshape(-1, q.shape[-1]) if q.dim() != 2 else q
        if q.shape[0] < 1:
            raise ValueError("search_multivector: needs at least one query vector")
        groups, values = self._group_ids(group_by)
        allow = self._allow_bits(query_filter) if query_filter is not None else None
        s, gid, c, ps, pr = self.gallery.search_maxsim(q.to(self.gallery.device), groups, k=int(limit),
                                                       score_threshold=score_threshold, allow=allow, with_parts=True)
        n = int(c)
        s, gid, ps, pr = s[:n].tolist(), gid[:n].tolist(), ps[:n].tolist(), pr[:n].tolist()
        return [MultiVectorResult(values[gid[r]], float(s[r]), self._points(ps[r], pr[r])) for r in range(n)]

    def _pairs(self, score_threshold, query_filter):
        allow = self._allow_bits(query_filter) if query_filter is not None else None
        pairs, scores = self.gallery.pairs(float(score_threshold), allow=allow)
        return pairs.cpu().numpy(), scores.cpu().numpy()

    def duplicate_pairs(self, score_threshold, query_filter=None):
        """Every pair of points (both selected by ``query_filter``, if given) whose vectors score at least
        ``score_threshold``: :class:`DuplicatePair` entries in row order (first point, then second).  Exact (include/revo.h,
        PAIRS)."""
        pairs, scores = self._pairs(score_threshold, query_filter)
        return [DuplicatePair(self.ids[a], self.ids[b], float(s)) for (a, b), s in zip(pairs.tolist(), scores.tolist())]

    def duplicate_groups(self, score_threshold, query_filter=None):
        """The groups of near-duplicates: connected components (at least two points) of the graph whose edges are the
        pairs of :meth:`duplicate_pairs`, as lists of point ids.  Members in row order; groups ordered by their first row."""
        return [[self.ids[r] for r in grp] for grp in self.duplicate_row_groups(score_threshold, query_filter)]

    def duplicate_row_groups(self, score_threshold, query_filter=None):
        """:meth:`duplicate_groups` as lists of row indices (the places of the points in ``ids`` / ``payloads``)."""
        pairs, _ = self._pairs(score_threshold, query_filter)
        return connected_groups(pairs, len(self))

    def duplicate_row_clusters(self, score_threshold, query_filter=None):
        """The lists :meth:`duplicate_row_groups` returns, from the device route (include/revo.h, CLUSTERS): the components
        are found on the device without materialising the pairs, so a group may be of any size (a static shot of 30 000
        frames is one group; its 4.5e8 pairs are more than :meth:`duplicate_pairs` will return)."""
        allow = self._allow_bits(query_filter) if query_filter is not None else None
        _, offsets, members = self.gallery.clusters(float(score_threshold), allow=allow)
        return split_clusters(offsets.cpu().numpy(), members.cpu().numpy())

    def duplicate_clusters(self, score_threshold, query_filter=None):
        """The lists :meth:`duplicate_groups` returns (point ids; members in row order, groups ordered by their first row),
        from the device route of :meth:`duplicate_row_clusters`."""
        return [[self.ids[r] for r in grp] for grp in self.duplicate_row_clusters(score_threshold, query_filter)]

    def neighbor_graph(self, limit=3, score_threshold=None, query_filter=None, sample=None, seed=0):
        """The database's distance-matrix query: for every point ``query_filter`` selects (all points without one) -- or for
        ``sample`` of them, drawn on the host with a generator seeded by ``seed`` -- its ``limit <= 64`` nearest other
        points of that same set, cut at ``score_threshold`` if given.  Returns a :class:`NeighborGraph` (CSR arrays over the
        set's ids, or ``.pairs()``).  Exact (include/revo.h, KNN): a point is never its own neighbour, identical vectors at
        other points are."""
        mask = self.filter_mask(query_filter) if query_filter is not None else np.ones(len(self), dtype=bool)
        mask = sample_mask(mask, sample, seed)
        restricted = query_filter is not None or sample is not None
        if len(self) == 0 or not mask.any():
            return NeighborGraph([], np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
        allow = torch.from_numpy(_filters.pack_bits(mask)).to(self.gallery.device) if restricted else None
        scores, idx, counts = self.gallery.knn(int(limit), score_threshold=score_threshold, allow=allow)
        return knn_to_graph(self.ids, mask, scores.cpu().numpy(), idx.cpu().numpy(), counts.cpu().numpy())

    def themes(self, n_themes, max_iter=10, seed=0, query_filter=None):
        """What is in this collection: the points ``query_filter`` selects (all points without one) partitioned into
        ``n_themes`` themes by exact spherical k-means (include/revo.h, KMEANS), started from ``n_themes`` distinct selected
        points drawn by :func:`seed_rows` with ``seed``.  Returns :class:`Theme` entries, largest first; themes that end
        without members are left out.  Raises if fewer points are selected than themes asked."""
        mask = self.filter_mask(query_filter) if query_filter is not None else np.ones(len(self), dtype=bool)
        rows = seed_rows(mask, n_themes, seed)
        dev = self.gallery.device
        allow = torch.from_numpy(_filters.pack_bits(mask)).to(dev) if query_filter is not None else None
        init = self.gallery.read()[torch.from_numpy(rows).to(dev)]
        _, labels, scores, sizes, _, _ = self.gallery.kmeans(init, max_iter=int(max_iter), normalize=True, allow=allow)
        # each theme's representative on the device: the best score of the theme, then the lowest row that has it
        n_c = int(sizes.shape[0])
        lab = labels.to(torch.int64)
        ok = lab >= 0
        best = torch.full((n_c,), float("-inf"), dtype=torch.float32, device=dev)
        best.scatter_reduce_(0, lab[ok], scores[ok], reduce="amax", include_self=True)
        is_best = ok.clone()
        is_best[ok] = scores[ok] == best[lab[ok]]
        rep = torch.full((n_c,), len(self), dtype=torch.int64, device=dev)
        at = torch.arange(len(self), dtype=torch.int64, device=dev)
        rep.scatter_reduce_(0, lab[is_best], at[is_best], reduce="amin", include_self=True)
        rep = torch.where(rep >= len(self), torch.full_like(rep, -1), rep)
        return assemble_themes(self.ids, self.payloads, labels.cpu().numpy(), sizes.cpu().numpy(), rep.cpu().numpy(),
                               scores.cpu().numpy())

    def assign(self, vectors, query_filter=None):
        """The best of ``vectors`` (fp32 ``[C, dim]``, normalised like stored rows) for every point: the exact assignment of
        ``Gallery.kmeans(max_iter=0)``.  Returns ``(labels [len] int32, scores [len] fp32)`` device tensors, label -1 and
        score -inf for a point ``query_filter`` leaves out -- what ``search(k=1)`` over a gallery of ``vectors`` gives for
        each stored row, ties to the lowest index."""
        dev = self.gallery.device
        allow = self._allow_bits(query_filter) if query_filter is not None else None
        c = torch.as_tensor(vectors, dtype=torch.float32).to(dev)
        _, labels, scores, _, _, _ = self.gallery.kmeans(c, max_iter=0, normalize=True, allow=allow)
        return labels, scores

    # -- persistence ----------------------------------------------------------
    def flush(self, path=None):
        """Write the rows (and finished source files) added since the last flush as one delta shard.  Returns the rows written."""
        path = path or self.path
        if not path:
            raise ValueError("this store has no directory to flush to")
        n = len(self)
        new = n - self._flushed
        if new <= 0 and not self._files_pending:
            return 0
        name = None
        if new > 0:
            name = f"vectors.{self._shards:05d}.f32.npy"
            vec = self.gallery.read(self._flushed, new).cpu().numpy()
            tmp = os.path.join(path, name + ".tmp.npy")
            with open(tmp, "wb") as f:                     # the shard's bytes and its name are on disk BEFORE the manifest
                np.save(f, vec)                            # line that points to them is appended: after a power loss the
                f.flush()                                  # manifest never names a shard that is not there
                os.fsync(f.fileno())
            os.replace(tmp, os.path.join(path, name))
            _fsync_dir(path)
        line = {"shard": self._shards, "file": name, "rows": new, "ids": self.ids[self._flushed:n],
                "payloads": self.payloads[self._flushed:n], "files_done": self._files_pending}
        with open(os.path.join(path, MANIFEST), "a") as f:
            f.write(json.dumps(line) + "\n")
            f.flush()
            os.fsync(f.fileno())
        self.files_done.update(self._files_pending)
        self._files_pending = []
        self._flushed = n
        self._shards += 1
        return new

    def save(self, path=None):
        """Flush what is new and mark the collection complete.  Deletes and updates only add manifest lines: the vectors of
        removed and replaced points stay in the old shard files.  ``save(path=<other directory>)`` writes everything anew,
        the current points only -- that is the way to compact a database."""
        path = path or self.path
        if not path:
            raise ValueError("this store has no directory (created without one, or loaded from the one-file format of "
                             "rounds 1-2): save(path=<new directory>) writes it out in the delta-shard format")
        os.makedirs(path, exist_ok=True)
        if path != self.path:                              # saving somewhere else: write everything there
            other = os.path.join(path, MANIFEST)
            with open(other, "w") as f:
                f.write(json.dumps({"format": 2, "collection": self.collection, "dim": self.dim, "build": self.build_info}) + "\n")
            keep = (self._flushed, self._shards, self._files_pending, self.path)
            self._flushed, self._shards, self._files_pending = 0, 0, sorted(self.files_done) + self._files_pending
            try:
                self.flush(path)
                with open(other, "a") as f:
                    f.write(json.dumps({"complete": True, "rows": len(self)}) + "\n")
            finally:
                self._flushed, self._shards, self._files_pending, self.path = keep
            return
        self.flush(path)
        if not self.complete:
            with open(os.path.join(path, MANIFEST), "a") as f:
                f.write(json.dumps({"complete": True, "rows": len(self)}) + "\n")
                f.flush()
                os.fsync(f.fileno())
            self.complete = True

    @classmethod
    def load(cls, path, device=0, allow_partial=False, capacity=0):
        """Open a database directory.  An unfinished build (no "complete" line) raises unless ``allow_partial``
        (``create_database(resume_from_checkpoint=True)`` continues it)."""
        man = os.path.join(path, MANIFEST)
        if not os.path.exists(man):
            return cls._load_v1(path, device)
        header, shards, complete, good_bytes = read_manifest(man)
        if not complete and not allow_partial:
            raise ValueError(f"{path}: unfinished build (resume it with create_database(resume_from_checkpoint=True))")
        if good_bytes < os.path.getsize(man):
            # a torn last line (the process died while appending): cut it off before anything is appended behind it
            with open(man, "r+b") as f:
                f.truncate(good_bytes)
        points = replay_manifest(shards)                   # what the shard, delete and update lines leave, in row order
        rows = len(points)
        st = cls(header["dim"], device=device, capacity=max(rows, capacity, 1), collection=header["collection"], path=path,
                 _fresh=False, build_info=header.get("build"))
        file_rows = {s["file"]: s["rows"] for s in shards if s.get("file") is not None}
        opened = {}

        def vectors_of(name):
            if name not in opened:
                vec = np.load(os.path.join(path, name), mmap_mode="r")
                if vec.shape != (file_rows[name], st.dim):
                    raise ValueError(f"{path}/{name}: {vec.shape} does not match its manifest line")
                opened[name] = vec
            return opened[name]

        step = max(1, (128 << 20) // (st.dim * 4))          # the surviving rows in order, 128 MB at a time
        for s0 in range(0, rows, step):
            src = [p[2] for p in points[s0:s0 + step]]
            vec = np.empty((len(src), st.dim), np.float32)
            names = np.array([f for f, _ in src], dtype=object)
            at = np.array([r for _, r in src], dtype=np.int64)
            for name in dict.fromkeys(f for f, _ in src):
                sel = np.flatnonzero(names == name)
                vec[sel] = vectors_of(name)[at[sel]]
            st.gallery.add(torch.from_numpy(vec), normalize=False)          # stored rows are already normalised
        st.ids = [p[0] for p in points]
        st.payloads = [p[1] for p in points]
        for s in shards:
            st.files_done.update(s.get("files_done", []))
        st._flushed, st._shards, st.complete = rows, len(shards), complete
        return st

    @classmethod
    def _load_v1(cls, path, device):
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        vec = np.load(os.path.join(path, "vectors.f32.npy"))
        st = cls(meta["dim"], device=device, capacity=max(len(meta["ids"]), 1), collection=meta["collection"], path=None)
        if len(meta["ids"]):
            st.gallery.add(torch.from_numpy(vec), normalize=False)
        st.ids, st.payloads = list(meta["ids"]), list(meta["payloads"])
        st.complete = True
        return st

    def close(self):
        if self.path:
            try:
                os.remove(os.path.join(self.path, ".lock"))
            except OSError:
                pass
        self.gallery.close()


# -- the small JSON at the reference's checkpoint path (core_system.py:474-476); the vectors live in the build's shards
def remove_checkpoint(ckpt_base):
    for ext in (".json", ".npy"):
        try:
            os.remove(ckpt_base + ext)
        except OSError:
            pass
