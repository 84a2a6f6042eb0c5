"""Every stream-taking entry point of include/revo.h on a side stream whose inputs arrive late.

The ABI's promise is "work is enqueued asynchronously on `stream` and the caller owns ordering".  On the default stream that
promise cannot fail: whatever the library puts on stream 0 by mistake is ordered with everything else by accident.  Here a
case runs twice:

* ``run_default``: inputs hold their real values, the library is called on the default stream;
* ``run_late``: the same input buffers are filled with poison (NaN, 0x5A5A5A5A), and the side stream first sleeps
  ``SLEEP_MS``, then receives the copies that bring the real values in, then the library's calls.  Whatever the library does
  off that stream runs during the sleep: it reads poison or a stale workspace, or overtakes a step that precedes it in program
  order, and the outputs differ.  Equality of the two runs is on BYTES.

While the sleep runs the stream cannot be idle, so ``not stream.query()`` right after an entry point returns proves two things
at once: the sleep outlasted the host side of the enqueue, and the entry point did not synchronise behind the caller's back.
Entries documented SYNCHRONOUS are held to the opposite.

A case is a function of one argument, the run's :class:`Run`; it is written once and knows no mode.  It is registered with
the ABI names it reaches (tests/test_stream_cases_host.py holds the header to that list).  Not a conftest: plain helpers,
imported by tests/test_gpu_streams.py.
"""
import contextlib
import ctypes as C
import functools
import json
import time

import numpy as np
import torch

SLEEP_MS = 50.0            # about 50 x the host time of a few hundred launches; checked per call, never trusted
POISON_WORD = 0x5A5A5A5A
DEV = torch.device("cuda", 0)


# ---- the clock and the side streams -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cycles_per_ms():
    """Cycles of torch.cuda._sleep per millisecond, measured once per process with two events on the default stream."""
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(20_000_000)
    b.record()
    b.synchronize()
    return 20_000_000 / a.elapsed_time(b)


def _sleep(ms):
    torch.cuda._sleep(int(ms * cycles_per_ms()))


def _independent_of_default(s):
    """True if work on the default stream runs while ``s`` sleeps (streams that share a hardware queue are served in
    submission order, and a late-input run on such a stream could not see anything)."""
    flag = torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _sleep(10.0)
    flag.add_(1.0)                                   # default stream
    torch.cuda.default_stream().synchronize()
    free = not s.query()
    s.synchronize()
    return free


@functools.lru_cache(maxsize=None)
def side_streams():
    """The two side streams of every late run in this process: each shown to run beside the default stream and beside the
    other.  The fake cases of tests/test_gpu_streams.py run on the same objects, so what they prove holds for the real ones."""
    found = []
    for _ in range(16):
        s = torch.cuda.Stream(device=DEV)
        if not _independent_of_default(s):
            continue
        if found:
            with torch.cuda.stream(found[0]):
                _sleep(10.0)
            with torch.cuda.stream(s):
                torch.zeros(1, device=DEV)
            s.synchronize()
            free = not found[0].query()
            found[0].synchronize()
            if not free:
                continue
        found.append(s)
        if len(found) == 2:
            return tuple(found)
    raise RuntimeError("no two side streams that run beside the default stream: a late-input run would prove nothing")


# ---- one run of a case --------------------------------------------------------------------------------------------------------
def _poison_(t):
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.view(-1).view(torch.uint8).fill_(POISON_WORD & 0xFF)       # every byte 0x5A: words of 0x5A5A5A5A
    return t


def _as_bytes(v):
    if isinstance(v, torch.Tensor):
        return v.detach().contiguous().cpu().numpy().tobytes()
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v).tobytes()
    return json.dumps(v, sort_keys=True, default=repr).encode()


class Run:
    """What a case sees.  ``late`` is False on the default stream.  The order inside a case: handles (``closing``), inputs
    (``dev`` / ``host``), ``arm()``, the library's calls with ``asynchronous`` / ``synchronous`` / ``noted`` after each, and
    ``out`` for everything that must have the default run's bytes."""

    def __init__(self, late, sleep_ms=SLEEP_MS):
        self.late = bool(late)
        self.sleep_ms = float(sleep_ms)
        self.stream = self.stream2 = None
        if self.late:
            self.stream, self.stream2 = side_streams()
        self.outputs = {}            # name -> value (tensors stay on the device until finish())
        self.order = []
        self.failed = []             # checks that did not hold: strings
        self.calls = []              # (label, what was expected, ms since arm(), stream idle?)
        self.taps = {}               # ABI name -> (ms since arm(), stream idle?) when its last call returned
        self._pending = []           # (buffer, real values) still to be copied on the side stream
        self._stack = contextlib.ExitStack()
        self._armed_at = None
        self._hosts = []

    # -- handles
    def closing(self, handle):
        """A handle created before the inputs (creation is synchronous by contract); closed when the run ends.  Every entry
        point the engine calls on it is tapped: the stream's state is recorded the moment the LIBRARY returns, before the
        wrapper's own torch work (which would make a drained stream look busy)."""
        self._stack.callback(handle.close)
        inner = getattr(handle, "_call", None)
        if inner is not None:
            def tapped(name, *args):
                inner(name, *args)
                if self.late and self._armed_at is not None:
                    self.taps[name] = (self._elapsed_ms(), bool(torch.cuda.current_stream().query()))
            handle._call = tapped
        return handle

    # -- inputs
    def dev(self, value):
        """A device input holding ``value`` (host tensor or array).  Late: the buffer holds poison until the side stream's
        copy, which ``arm()`` enqueues behind the sleep."""
        real = torch.as_tensor(value).contiguous().to(DEV)
        if not self.late:
            return real
        buf = _poison_(torch.empty_like(real))
        self._pending.append((buf, real))
        return buf

    def host(self, value):
        """A host input: a private copy the case overwrites with ``scribble`` as soon as the call has returned (the header
        lets the caller free a host source on return)."""
        a = np.array(value, copy=True)
        self._hosts.append(a)
        return a

    @staticmethod
    def scribble(a):
        a.view(np.uint8).reshape(-1)[:] = 0xA5

    def arm(self):
        """Late: everything so far is complete; then, on the side stream, the sleep and the copies that bring the inputs'
        real values.  From here to the end of the case the side stream is torch's current stream."""
        if not self.late:
            return
        torch.cuda.synchronize()
        self._stack.enter_context(torch.cuda.stream(self.stream))
        self._armed_at = time.perf_counter()                 # before the sleep is enqueued: it cannot end sooner than
        _sleep(self.sleep_ms)                                # sleep_ms after this
        self.feed()

    def feed(self):
        """The copies of inputs declared since the last ``arm`` / ``feed``, on the current stream."""
        for buf, real in self._pending:
            buf.copy_(real, non_blocking=True)
        self._pending = []

    # -- what an entry point did to the stream
    def _elapsed_ms(self):
        return (time.perf_counter() - self._armed_at) * 1e3

    def _note(self, label, expect, abi):
        """(ms since arm(), stream idle?) right now, or when the library last returned from the entry point ``abi``"""
        if not self.late:
            return None
        ms, idle = self.taps[abi] if abi is not None else (self._elapsed_ms(), bool(torch.cuda.current_stream().query()))
        self.calls.append((label, expect, ms, idle))
        return ms, idle

    def asynchronous(self, label, abi=None):
        """The entry point that just returned is documented asynchronous.  It must have returned while the sleep was
        running: the stream busy, and the host no further than half the sleep from its start -- the sleep is to be at least
        twice what the enqueue needs, and a call that waits for the stream returns only when the whole sleep is over (a
        busy stream alone does not show that: a call that waits and THEN enqueues a kernel leaves the stream busy too)."""
        got = self._note(label, "async", abi)
        if got is None:
            return
        ms, idle = got
        if idle or ms >= self.sleep_ms / 2:
            self.failed.append(f"{label}: returned {ms:.2f} ms after the sleep of {self.sleep_ms:.0f} ms was enqueued with the "
                               f"stream {'idle' if idle else 'busy'} -- the call synchronised, or the sleep did not outlast "
                               "the enqueue twice over")

    def synchronous(self, label, abi=None):
        """The entry point that just returned is documented SYNCHRONOUS on `stream`: nothing may be pending."""
        got = self._note(label, "sync", abi)
        if got is not None and not got[1]:
            self.failed.append(f"{label}: documented synchronous, but work was pending on the stream on return")

    def noted(self, label, abi=None):
        """Recorded only: a call that is documented to wait (for a host source, a workspace that grows, a pinned buffer's
        previous copy), or one that follows such a call, when the sleep is over and nothing can be told."""
        self._note(label, "either", abi)

    # -- outputs
    def out(self, name, value):
        assert name not in self.outputs, name
        if isinstance(value, (tuple, list)) and any(isinstance(v, torch.Tensor) for v in value):
            for i, v in enumerate(value):
                self.out(f"{name}[{i}]", v)
            return
        self.outputs[name] = value
        self.order.append(name)

    @property
    def enqueue_ms(self):
        """Host time from the start of the sleep to the return of the last call checked to be asynchronous."""
        t = [ms for _, expect, ms, _ in self.calls if expect == "async"]
        return max(t) if t else 0.0

    def finish(self):
        """Outputs as bytes: read the way a caller on that stream reads them -- after synchronising it, nothing else."""
        try:
            torch.cuda.current_stream().synchronize()
            return {k: _as_bytes(self.outputs[k]) for k in self.order}
        finally:
            self.close()

    def close(self):
        try:
            torch.cuda.synchronize()
        finally:
            self._stack.close()


class Report:
    def __init__(self, name, mismatches, failed, late, default):
        self.name, self.mismatches, self.failed = name, mismatches, failed
        self.late, self.default = late, default          # the two Run objects (calls, enqueue_ms)

    @property
    def ok(self):
        return not self.mismatches and not self.failed

    def __str__(self):
        lines = [f"{self.name}: host enqueue {self.late.enqueue_ms:.2f} ms under a sleep of {self.late.sleep_ms:.0f} ms"]
        lines += [f"  call {label}: expected {expect}, {ms:.2f} ms, stream {'idle' if idle else 'busy'}"
                  for label, expect, ms, idle in self.late.calls]
        lines += [f"  MISMATCH {m}" for m in self.mismatches] + [f"  FAILED {f}" for f in self.failed]
        return "\n".join(lines)


def run_default(fn):
    r = Run(late=False)
    try:
        fn(r)
        return r, r.finish()
    except BaseException:
        r.close()
        raise


def run_late(fn, sleep_ms=SLEEP_MS):
    r = Run(late=True, sleep_ms=sleep_ms)
    try:
        fn(r)
        return r, r.finish()
    except BaseException:
        r.close()
        raise


def compare(name, fn, sleep_ms=SLEEP_MS):
    """Both runs of ``fn``; the outputs whose bytes differ and the stream checks that failed."""
    d, want = run_default(fn)
    l, got = run_late(fn, sleep_ms)
    mism = []
    if list(want) != list(got):
        mism.append(f"outputs {list(got)} instead of {list(want)}")
    for k in want:
        if k in got and want[k] != got[k]:
            a, b = np.frombuffer(want[k], np.uint8), np.frombuffer(got[k], np.uint8)
            where = "sizes %d / %d" % (a.size, b.size) if a.size != b.size else "%d of %d bytes, first at %d" % (
                int((a != b).sum()), a.size, int(np.flatnonzero(a != b)[0]))
            if len(want[k]) <= 400 and not isinstance(l.outputs[k], torch.Tensor):
                where += f": {got[k].decode()} instead of {want[k].decode()}"
            mism.append(f"{k}: late run differs from the default stream's ({where})")
    return Report(name, mism, list(l.failed) + list(d.failed), l, d)


# ---- the registry -------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, fn, abi):
        self.name, self.fn, self.abi = name, fn, tuple(abi)


CASES = {}


def case(*abi):
    """Registers a case under its function's name with the ABI names (include/revo.h) its calls reach."""
    def deco(fn):
        name = fn.__name__
        assert name not in CASES
        CASES[name] = Case(name, fn, abi)
        return fn
    return deco


# Stream-taking launchers that the product reaches only inside another entry point: claimed through the entry point that calls
# the SAME launcher (csrc: api.hip's revo_op_* wrappers are one call each), which a case above runs.
VIA = {
    "revo_op_gemm": "revo_vit_forward",                  # revo::launch_gemm, every form of it
    "revo_op_gemm_rope": "revo_vit_forward",
    "revo_op_gemm_resid_ln": "revo_vit_forward",
    "revo_op_gemm_ln_in": "revo_vit_forward",
    "revo_op_gemm_ln_in_rope": "revo_vit_forward",
    "revo_op_gemm_resid_norm": "revo_vit_forward",
    "revo_op_layernorm": "revo_vit_forward",             # launch_layernorm (ln_pre)
    "revo_op_layernorm_logits": "revo_vit_forward",      # launch_layernorm with the pool's logits (ln_post)
    "revo_op_linear_f32": "revo_vit_forward",            # launch_gemm_f32_skinny (the head)
    "revo_op_linear_f32_grouped": "revo_vit_forward",
    "revo_op_pool_rows": "revo_vit_forward",             # launch_pool_head_rows
    "revo_op_attention": "revo_vit_forward",             # launch_attention -> launch_attention_ex
    "revo_op_pool_rows_masked": "revo_vit_forward_regions",
    "revo_op_detect_scores": "revo_vit_detect",
    "revo_op_detect_regions": "revo_vit_detect",
    "revo_op_attention_causal": "revo_text_forward",
    "revo_op_embed_tokens": "revo_text_forward",
    "revo_op_pool_eot": "revo_text_forward",
    "revo_op_l2norm_rows": "revo_gallery_append",        # launch_l2norm_rows: every row and every query
}

# Stream-taking declarations no case runs, and why.
NOT_RUN = {
    "revo_probe_mfma": "calibration probe of bench.py: one fixed kernel, no state, not on the product's path",
    "revo_probe_copy": "calibration probe of bench.py: one fixed kernel, no state, not on the product's path",
    "revo_probe_gridbar": "experiment probe of the experiments library (scripts/gridbar_probe.py); spins on a grid barrier",
}


# ---- fixtures (host side, made once, never written to) ------------------------------------------------------------------------
D = 64


@functools.lru_cache(maxsize=None)
def rows(n, seed, dim=D):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def bitmap(n, seed, keep=0.6):
    """A packed allow- or remove-bitmap over n rows: int32 [ceil(n / 32)], bit r & 31 of word r >> 5."""
    from reverso_amd.filters import pack_bits
    m = np.random.default_rng(seed).random(n) < keep
    return torch.from_numpy(pack_bits(m).copy())


@functools.lru_cache(maxsize=None)
def group_ids(n, seed, n_groups=300):
    g = np.random.default_rng(seed).integers(0, n_groups, n).astype(np.int32)
    g[::17] = -1
    return torch.from_numpy(g)


@functools.lru_cache(maxsize=None)
def tied_rows(n_random, n_ties, seed):
    """n_random random rows with n_ties copies of one more row spread among them, and that row (the query that ties)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(D).astype(np.float32)
    x = np.concatenate([rng.standard_normal((n_random, D)).astype(np.float32), np.repeat(v[None], n_ties, 0)])
    x = x[rng.permutation(x.shape[0])]
    return torch.from_numpy(x), torch.from_numpy(v[None].copy())


@functools.lru_cache(maxsize=None)
def between_two_centroids(N=2048, n_c=5):
    """tests/test_gpu_kmeans.py's fixture: rows between two centroids, where bf16 and fp32 disagree about the nearer one."""
    g = torch.Generator().manual_seed(7)
    cents = torch.nn.functional.normalize(torch.randn(n_c, D, generator=g), dim=1)
    a = torch.randint(0, n_c, (N,), generator=g)
    b = (a + torch.randint(1, n_c, (N,), generator=g)) % n_c
    x = torch.nn.functional.normalize(cents[a] + cents[b] + 1e-3 * torch.randn(N, D, generator=g), dim=1)
    return x, cents


def _engine():
    from reverso_amd import engine
    return engine


def _lib():
    from reverso_amd import _lib as lib
    return lib


def gallery(r, x=None, capacity=None, normalize=True, experiments=False, keep_f32=True):
    """A gallery handle of this run holding ``x`` (host rows), complete before anything else happens."""
    cap = capacity if capacity is not None else max(1, 0 if x is None else x.shape[0])
    G = r.closing(_engine().Gallery(D, cap, device=0, keep_f32=keep_f32, experiments=experiments))
    if x is not None and x.shape[0]:
        G.add(x.to(DEV), normalize=normalize)
    torch.cuda.synchronize()
    return G


def _stats(r, G, name):
    r.out(name, G.search_stats())
    r.synchronous(name)


N_ROWS = 3000          # more than one 256-row tile column, no multiple of 256 or of 32
N_Q = 5


# ---- rows -------------------------------------------------------------------------------------------------------------------------
def _rows_after(r, G, tag=""):
    """What the gallery now holds: its fp32 rows, the certificate's maxima, and a search over the bf16 copy."""
    q = rows(3, 901).to(DEV)                                  # (complete: allocated and filled on the stream that uses it)
    r.out(tag + "search", G.search(q, k=10))
    r.out(tag + "master rows", G.read())
    r.out(tag + "cert", list(G.cert_stats()))
    r.synchronous(tag + "cert_stats")
    r.out(tag + "size", len(G))


@case("revo_gallery_append", "revo_search_topk", "revo_op_gallery_cert_stats")
def add_from_device(r):
    G = gallery(r, capacity=N_ROWS)
    x = r.dev(rows(N_ROWS, 1))
    r.arm()
    G.add(x)
    r.asynchronous("add(device rows)")
    _rows_after(r, G)


@case("revo_gallery_append")
def add_from_host(r):
    G = gallery(r, capacity=N_ROWS)
    x = r.host(rows(N_ROWS, 2).numpy())
    r.arm()
    G.add(torch.from_numpy(x))
    r.synchronous("add(host rows)")
    r.scribble(x)
    _rows_after(r, G)


@case("revo_gallery_append")
def add_unnormalized(r):
    G = gallery(r, capacity=N_ROWS)
    x = r.dev(rows(N_ROWS, 3) * 3.5)
    r.arm()
    G.add(x, normalize=False)
    r.asynchronous("add(normalize=False)")
    _rows_after(r, G)


@case("revo_gallery_update")
def update_rows(r):
    G = gallery(r, rows(N_ROWS, 4))
    perm = np.random.default_rng(5).permutation(N_ROWS)[:700].astype(np.int64)
    idx, idx2 = r.host(perm), r.host(perm[:300])
    v = r.dev(rows(700, 6))
    vh = r.host(rows(300, 7).numpy())
    r.arm()
    G.update(torch.from_numpy(idx), v)
    r.noted("update(device rows)")                           # waits for its copy of the host indices, then enqueues
    r.scribble(idx)                                          # (read when the call returns: the row kernel is still pending)
    G.update(torch.from_numpy(idx2), torch.from_numpy(vh), normalize=False)
    r.synchronous("update(host rows)")
    r.scribble(idx2)
    r.scribble(vh)
    _rows_after(r, G)


@case("revo_gallery_remove")
def remove_rows(r):
    G = gallery(r, rows(N_ROWS, 8))
    bits = r.dev(bitmap(N_ROWS, 9, keep=0.3))
    r.arm()
    r.out("removed (device bitmap)", G.remove(bits))
    r.synchronous("remove(device bitmap)")
    hb = r.host(bitmap(len(G), 10, keep=0.5).numpy())
    r.out("removed (host bitmap)", G.remove(torch.from_numpy(hb)))
    r.synchronous("remove(host bitmap)")
    r.scribble(hb)
    _rows_after(r, G)


@case("revo_gallery_append_unique")
def append_unique(r):
    base = rows(2000, 11)
    G = gallery(r, base, capacity=2000 + 600 + 400)
    near = torch.nn.functional.normalize(base[:300], dim=1) + 1e-3 * rows(300, 12)
    x = r.dev(torch.cat([near, rows(300, 13)])[torch.from_numpy(np.random.default_rng(14).permutation(600))])
    xh = r.host(torch.cat([rows(200, 15), near[:200] + 1e-3 * rows(200, 16)]).numpy())
    r.arm()
    r.out("add_unique(device rows)", G.add_unique(x, 0.98))
    r.synchronous("add_unique(device rows)", abi="revo_gallery_append_unique")
    r.out("add_unique(host rows)", G.add_unique(torch.from_numpy(xh), 0.98))
    r.synchronous("add_unique(host rows)", abi="revo_gallery_append_unique")
    r.scribble(xh)
    _stats(r, G, "stats")
    _rows_after(r, G)


@case("revo_search_set_filter", "revo_search_topk")
def filter_from_device_and_host(r):
    G = gallery(r, rows(N_ROWS, 17))
    q = r.dev(rows(N_Q, 18))
    bits = r.dev(bitmap(N_ROWS, 19))
    hb = r.host(bitmap(N_ROWS, 20, keep=0.01).numpy())
    r.arm()
    r.out("search(allow: device bitmap)", G.search(q, k=10, allow=bits))
    r.asynchronous("set_filter(device) + search")
    _stats(r, G, "stats (device)")
    lib = _lib()
    with G._frame():
        G._call("revo_search_set_filter", C.c_void_p(hb.ctypes.data), N_ROWS, 0, lib.current_stream())
        r.synchronous("set_filter(host bitmap)")
        r.scribble(hb)
    try:
        r.out("search(allow: host bitmap)", G.search(q, k=50))
    finally:
        G._lib.revo_search_set_filter(G._h, None, 0, 0, None)
    _stats(r, G, "stats (host)")


@case("revo_search_set_groups", "revo_search_groups")
def groups_from_device_and_host(r):
    G = gallery(r, rows(N_ROWS, 21))
    q = r.dev(rows(N_Q, 22))
    gid = r.dev(group_ids(N_ROWS, 23))
    hg = r.host(group_ids(N_ROWS, 24, n_groups=7).numpy())
    bits = r.dev(bitmap(N_ROWS, 25))
    r.arm()
    r.out("search_groups(device ids)", G.search_groups(q, gid, limit=5, group_size=3))
    r.asynchronous("set_groups(device) + search_groups")
    _stats(r, G, "stats (device)")
    r.out("search_groups(device ids, filtered)", G.search_groups(q, gid, limit=10, group_size=5, allow=bits))
    lib = _lib()
    Q = q.shape[0]
    outs = [torch.empty((Q, 10, 5), dtype=torch.float32, device=DEV), torch.empty((Q, 10, 5), dtype=torch.int64, device=DEV),
            torch.empty((Q, 10), dtype=torch.int32, device=DEV), torch.empty((Q, 10), dtype=torch.int32, device=DEV),
            torch.empty((Q,), dtype=torch.int32, device=DEV)]
    with G._frame():
        try:
            G._call("revo_search_set_groups", C.c_void_p(hg.ctypes.data), N_ROWS, 0, lib.current_stream())
            r.synchronous("set_groups(host ids)")
            r.scribble(hg)
            # seven groups of hundreds of rows, ten wanted with five rows each: the top-50 cannot decide it (fp32 passes)
            G._call("revo_search_groups", lib.ptr(q), Q, 10, 5, 0, 0.0, 0, *[lib.ptr(t) for t in outs], lib.current_stream())
        finally:
            G._lib.revo_search_set_groups(G._h, None, 0, 0, None)
    r.out("search_groups(host ids)", outs)
    _stats(r, G, "stats (host)")


# ---- top-k ------------------------------------------------------------------------------------------------------------------------
@case("revo_search_topk", "revo_search_stats", "revo_sync")
def search_k10(r):
    G = gallery(r, rows(N_ROWS, 30))
    q = r.dev(rows(N_Q, 31))
    r.arm()
    r.out("k=10", G.search(q, k=10))
    r.asynchronous("search(k=10)")
    r.out("k=10, offset and threshold", G.search(q, k=10, score_threshold=0.2, index_offset=(1 << 40) + 7))
    r.asynchronous("search(k=10, index_offset, threshold)")
    lib = _lib()
    lib.check(lib.load().revo_sync(lib.current_stream()), "revo_sync")
    r.synchronous("revo_sync")
    _stats(r, G, "stats")


@case("revo_search_topk", "revo_search_stats")
def search_k50_ties_wider_than_the_candidates(r):
    x, v = tied_rows(N_ROWS, 200, 32)                        # 200 equal scores: the scan keeps 64 candidates per query
    G = gallery(r, x)
    q = r.dev(torch.cat([v, rows(2, 33)]))
    r.arm()
    r.out("k=50", G.search(q, k=50))
    r.asynchronous("search(k=50, ties)")
    st = G.search_stats()
    r.out("stats", st)
    assert st["uncertified"] >= 1, st                        # (the fixture: the certificate fails and the exact round runs)


@case("revo_search_topk_large", "revo_search_stats")
def search_k200(r):
    G = gallery(r, rows(N_ROWS, 34))
    q = r.dev(rows(7, 35))
    bits = r.dev(bitmap(N_ROWS, 36))
    r.arm()
    r.out("k=200", G.search(q, k=200))
    r.asynchronous("search(k=200)")
    _stats(r, G, "stats")
    r.out("k=200 filtered", G.search(q, k=200, allow=bits, index_offset=5))
    _stats(r, G, "stats (filtered)")


@case("revo_search_topk_large", "revo_search_stats")
def search_k200_exhaustive_fallback(r):
    x, v = tied_rows(N_ROWS, 8192 + 1000, 37)                # more copies than a band holds (8192): the exhaustive fallback
    G = gallery(r, x)
    q = r.dev(torch.cat([v, v + 0.01 * rows(1, 38), rows(1, 39)]))
    r.arm()
    r.out("k=200", G.search(q, k=200))
    r.asynchronous("search(k=200, band overflow)")
    st = G.search_stats()
    r.out("stats", st)
    assert st["large_k_fallback"] >= 1, st


# ---- the candidate pipeline -----------------------------------------------------------------------------------------------------
def _late_gallery(r, x, **kw):
    """A gallery whose rows are the late input: the append is pending on the stream when the search is enqueued."""
    G = gallery(r, capacity=x.shape[0], **kw)
    xd = r.dev(x)
    return G, xd


@functools.lru_cache(maxsize=None)
def near_duplicates(n=N_ROWS, seed=40):
    """rows of which a third are noisy copies of others: pairs, clusters and kNN lists that are not empty"""
    rng = np.random.default_rng(seed)
    x = torch.nn.functional.normalize(rows(n, seed), dim=1)
    src = torch.from_numpy(rng.integers(0, n, n // 3))
    dst = torch.from_numpy(rng.permutation(n)[: n // 3])
    x = x.clone()
    x[dst] = x[src] + 0.02 * rows(n // 3, seed + 1)
    return x


@functools.lru_cache(maxsize=None)
def identical_rows(n=2000, seed=41):
    return torch.from_numpy(np.repeat(np.random.default_rng(seed).standard_normal((1, D)).astype(np.float32), n, 0))


@case("revo_gallery_pairs", "revo_gallery_append")
def pairs(r):
    G, x = _late_gallery(r, near_duplicates())
    bits = r.dev(bitmap(N_ROWS, 42, keep=0.8))
    r.arm()
    G.add(x)
    r.asynchronous("add")
    r.out("pairs", G.pairs(0.9))
    r.synchronous("pairs")
    _stats(r, G, "stats")
    r.out("pairs (filtered)", G.pairs(0.9, allow=bits))


@case("revo_gallery_pairs")
def pairs_workspace_regrow(r):
    G, x = _late_gallery(r, identical_rows())
    r.arm()
    G.add(x)
    p, s = G.pairs(0.99)
    r.synchronous("pairs")
    st = G.search_stats()
    assert st["join_passes"] == 2, st                        # 1 999 000 pairs: the join ran again in a grown workspace
    r.out("stats", st)
    r.out("pairs", (p, s))


@case("revo_gallery_clusters")
def clusters(r):
    G, x = _late_gallery(r, near_duplicates())
    bits = r.dev(bitmap(N_ROWS, 43, keep=0.8))
    r.arm()
    G.add(x)
    r.out("clusters", G.clusters(0.9))
    r.synchronous("clusters")
    _stats(r, G, "stats")
    r.out("clusters (filtered)", G.clusters(0.9, allow=bits))


@case("revo_gallery_clusters")
def clusters_workspace_regrow(r):
    """tests/test_gpu_clusters.py's fixture: the threshold ON the exact score of 2 000 identical rows, so that no pair is
    certain and merged in place -- all 1 999 000 are stored for the fp32 re-score and outgrow the first workspace, while the
    union-find and the error word have to survive the regrow"""
    P = gallery(r, identical_rows()[:2])                     # (a handle of its own: the exact fp32 score of any two of the rows)
    thr = float(P.pairs(0.5)[1][0].cpu())
    G, x = _late_gallery(r, identical_rows())
    r.arm()
    G.add(x)
    res = G.clusters(thr)
    r.synchronous("clusters")
    st = G.search_stats()
    assert st["collected_rows"] == 1_999_000 and st["join_passes"] == 2, st
    r.out("stats", st)
    r.out("clusters", res)


@case("revo_gallery_knn")
def knn(r):
    G, x = _late_gallery(r, near_duplicates())
    bits = r.dev(bitmap(N_ROWS, 44, keep=0.8))
    r.arm()
    G.add(x)
    r.out("knn", G.knn(10))
    r.synchronous("knn")
    _stats(r, G, "stats")
    r.out("knn (filtered, threshold)", G.knn(10, score_threshold=0.5, allow=bits))


@case("revo_gallery_knn")
def knn_small_workspace(r):
    lib = _lib().load_exp()
    G, x = _late_gallery(r, near_duplicates(), experiments=True)
    r.arm()
    G.add(x)
    try:
        assert lib.revo_debug_set_knn(1000, 0) == 0          # keys are lost: their rows take the exhaustive fallback
        r.out("knn", G.knn(10))
    finally:
        lib.revo_debug_set_knn(0, 0)
    r.synchronous("knn")
    st = G.search_stats()
    assert st["large_k_fallback"] > 0, st
    r.out("stats", st)


def _kmeans(r, G, cents, label):
    res = G.kmeans(cents, max_iter=2, normalize=False)
    r.synchronous(label)
    r.out(label, list(res[:4]))
    r.out(label + " iterations", [res[4], res[5]])


@case("revo_gallery_kmeans")
def kmeans(r):
    x, c = between_two_centroids()
    G, xd = _late_gallery(r, x)
    cents = r.dev(c)
    r.arm()
    G.add(xd)
    _kmeans(r, G, cents, "kmeans")
    _stats(r, G, "stats")


@case("revo_gallery_kmeans")
def kmeans_workspace_regrow(r):
    lib = _lib().load_exp()
    x, c = between_two_centroids()
    G, xd = _late_gallery(r, x, experiments=True)
    cents = r.dev(c)
    r.arm()
    G.add(xd)
    _kmeans(r, G, cents, "kmeans")
    base = G.search_stats()
    try:
        assert lib.revo_debug_set_kmeans(64) == 0            # 64 candidate keys: a step's join runs again in a grown workspace
        _kmeans(r, G, cents, "kmeans, small workspace")
    finally:
        lib.revo_debug_set_kmeans(0)
    st = G.search_stats()
    assert st["join_passes"] > base["join_passes"], (base, st)
    r.out("stats", [base, st])


@case("revo_search_range")
def search_range(r):
    G = gallery(r, near_duplicates())
    q = r.dev(near_duplicates()[:N_Q] + 0.01 * rows(N_Q, 45))
    r.arm()
    r.out("range", G.search_range(q, 0.5, index_offset=11))
    r.synchronous("search_range")
    _stats(r, G, "stats")


@case("revo_search_range")
def search_range_workspace_regrow(r):
    G, x = _late_gallery(r, identical_rows())
    q = r.dev(identical_rows()[:1])
    r.arm()
    G.add(x)
    r.out("range", G.search_range(q, 0.99))
    r.synchronous("search_range")
    st = G.search_stats()
    assert st["join_passes"] == 2, st
    r.out("stats", st)


@case("revo_search_recommend")
def recommend(r):
    G = gallery(r, rows(N_ROWS, 46))
    pos, neg = r.dev(rows(3, 47)), r.dev(rows(2, 48))
    r.arm()
    r.out("recommend", G.recommend(pos, neg, k=50))
    r.synchronous("recommend")
    _stats(r, G, "stats")


@case("revo_search_discover")
def discover(r):
    G = gallery(r, rows(N_ROWS, 49))
    t, pos, neg = r.dev(rows(1, 50)[0]), r.dev(rows(4, 51)), r.dev(rows(4, 52))
    r.arm()
    r.out("discover", G.discover(t, pos, neg, k=50))
    r.synchronous("discover")
    _stats(r, G, "stats")
    r.out("context", G.discover(None, pos, neg, k=10))


@case("revo_search_maxsim", "revo_search_set_groups")
def maxsim(r):
    G = gallery(r, rows(N_ROWS, 53))
    q, gid = r.dev(rows(4, 54)), r.dev(group_ids(N_ROWS, 55))
    r.arm()
    r.out("maxsim", G.search_maxsim(q, gid, k=50, with_parts=True))
    r.synchronous("maxsim")
    _stats(r, G, "stats")


@case("revo_search_mmr")
def mmr(r):
    G = gallery(r, near_duplicates())
    q = r.dev(rows(N_Q, 56))
    r.arm()
    r.out("mmr", G.search_mmr(q, k=10, candidates=100, diversity=0.5))
    r.asynchronous("search_mmr")
    _stats(r, G, "stats")


@case("revo_search_fusion", "revo_topk_fuse")
def fusion(r):
    G = gallery(r, rows(N_ROWS, 57))
    q = r.dev(rows(6, 58).reshape(3, 2, D))
    r.arm()
    r.out("rrf", G.search_fusion(q, k=10, limit=50, with_list_scores=True))
    r.asynchronous("search_fusion(rrf)")
    r.out("dbsf", G.search_fusion(q, k=10, limit=50, method="dbsf", weights=[1.0, 0.5]))
    s, i, c = G.search(q.reshape(6, D), k=50)
    fused = _engine().fuse_topk(s.reshape(3, 2, 50), i.reshape(3, 2, 50), c.reshape(3, 2), k=10)
    r.asynchronous("search + fuse_topk")
    r.out("fuse_topk", fused)
    _stats(r, G, "stats")


# ---- the two-phase shard protocol ---------------------------------------------------------------------------------------------
@case("revo_search_candidates", "revo_search_finish", "revo_topk_merge_packed", "revo_search_exact", "revo_topk_merge",
      "revo_search_topk")
def two_shards(r):
    from reverso_amd import sharded
    x, v = tied_rows(4300, 200, 59)                          # ties across both shards: the cross-shard certificate fails
    A, B = gallery(r, x[:2000]), gallery(r, x[2000:])
    q = r.dev(torch.cat([v, rows(4, 60)]))
    r.arm()
    sh = sharded.LocalShards.from_galleries([A, B])
    try:
        bounds = A.search_candidates(q, k=10, top_m=8)
        r.asynchronous("search_candidates")
        r.out("bounds", bounds)
        r.out("sharded k=10", sh.search(q, 10))
        r.out("second rounds k=10", sh.last_uncertified)
        r.out("sharded k=50", sh.search(q, 50))
        n50 = sh.last_uncertified
        r.out("second rounds k=50", n50)
        assert n50 >= 1, n50                                 # (the fixture: revo_search_exact ran)
    finally:
        sh.close()
    ra, rb = A.search(q, k=10), B.search(q, k=10, index_offset=2000)
    merged = _engine().merge_topk(torch.stack([ra[0], rb[0]]), torch.stack([ra[1], rb[1]]), 10)
    r.noted("search x 2 + merge_topk")                       # (behind the sharded searches, which read counts on the host)
    r.out("merge_topk", merged)


# ---- towers -------------------------------------------------------------------------------------------------------------------------
TOWER = "PE-Tiny-T14-56"
TEXT_TOWER = "PE-Tiny-Text-16"      # the miniature text tower of the same output width


def _vit(r, max_batch=8):
    eng = r.closing(_engine().VitEngine.synthetic(TOWER, seed=3, device=0, max_batch=max_batch, randomize_affine=True))
    torch.cuda.synchronize()
    return eng


@functools.lru_cache(maxsize=None)
def images_u8(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, 3, 56, 56), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def region_bits(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(1, 1 << 17, (n, 1)).astype(np.int32))


@case("revo_vit_forward")
def embed_images(r):
    eng = _vit(r)
    u8 = r.dev(images_u8(6, 70))
    f32 = r.dev((images_u8(5, 71).to(torch.float32) / 255.0 - 0.5) / 0.5)
    one = r.dev(images_u8(1, 72))
    r.arm()
    r.out("u8", eng.embed(u8))
    r.asynchronous("embed(u8)")
    r.out("fp32", eng.embed(f32, normalize=False))
    r.asynchronous("embed(fp32)")
    r.out("one image", eng.embed(one))
    r.asynchronous("embed(one image)")


@case("revo_vit_forward_regions")
def embed_regions(r):
    eng = _vit(r)
    u8 = r.dev(images_u8(4, 73))
    ri, ri2 = r.host(np.array([0, 3, 3, 1, 2, 0, 1], dtype=np.int64)), r.host(np.array([2, 2, 0, 1, 3, 3, 0], dtype=np.int64))
    hb = r.host(region_bits(7, 74).numpy())
    db = r.dev(region_bits(7, 75))
    r.arm()
    g, rg = eng.embed_regions(u8, ri, torch.from_numpy(hb))
    r.asynchronous("embed_regions(host bitmaps)")
    r.scribble(hb)
    r.scribble(ri)
    r.out("host bitmaps", (g, rg))
    r.out("device bitmaps", eng.embed_regions(u8, ri2, db))
    r.noted("embed_regions(device bitmaps)")                 # its host image indices wait for the pinned buffer's last copy
    r.scribble(ri2)


@case("revo_vit_forward_regions")
def embed_regions_more_than_4096(r):
    eng = _vit(r)
    u8 = r.dev(images_u8(4, 76))
    n = 4096 + 37
    ri = r.host(np.random.default_rng(77).integers(0, 4, n).astype(np.int64))
    hb = r.host(region_bits(n, 78).numpy())
    r.arm()
    g, rg = eng.embed_regions(u8, ri, torch.from_numpy(hb))
    r.noted("embed_regions(4133 regions)")                   # documented: waits for its own earlier copies in between
    r.scribble(hb)
    r.scribble(ri)
    r.out("regions", (g, rg))


@case("revo_vit_forward_tokens")
def embed_tokens(r):
    eng = _vit(r)
    u8 = r.dev(images_u8(3, 79))
    r.arm()
    r.out("tokens", eng.embed_tokens(u8))
    r.asynchronous("embed_tokens")


@case("revo_vit_detect")
def detect(r):
    eng = _vit(r)
    u8 = r.dev(images_u8(4, 80))
    prompts = r.dev(rows(5, 81))
    r.arm()
    d = eng.detect(u8, prompts, thresholds=None, n_background=1, max_regions=16, with_maps=True, with_global=True)
    r.synchronous("detect", abi="revo_vit_detect")
    r.out("regions", len(d))
    r.out("detections", [d.image, d.prompt, d.boxes, d.cells, d.confidence, d.bits, d.vectors, d.scores, d.labels,
                         d.global_vectors])


@case("revo_vit_stats", "revo_vit_forward")
def ln_fold_stats_between_two_forwards(r):
    eng = _vit(r)
    a, b = r.dev(images_u8(8, 82)), r.dev(images_u8(8, 83))
    r.arm()
    r.out("first", eng.embed(a))
    r.asynchronous("embed")
    r.out("stats after the first (reset)", eng.ln_fold_stats(reset=True))
    r.synchronous("ln_fold_stats(reset)")
    r.out("second", eng.embed(b))
    r.out("stats after the second", eng.ln_fold_stats())
    r.out("third", eng.embed(a[:5]))
    r.out("stats after the third (not reset in between)", eng.ln_fold_stats(reset=True))
    r.out("stats after the reset", eng.ln_fold_stats())


@case("revo_text_forward")
def embed_text_twice(r):
    eng = r.closing(_engine().TextEngine.synthetic(TEXT_TOWER, seed=5, device=0, max_batch=8))
    torch.cuda.synchronize()
    rng = np.random.default_rng(84)
    cfg = eng.cfg

    def prompts(n):
        t = rng.integers(1, cfg.vocab_size - 1, (n, cfg.context_length)).astype(np.int32)
        for i in range(n):
            e = int(rng.integers(2, cfg.context_length))
            t[i, e] = cfg.vocab_size - 1                      # the end token: the largest id
            t[i, e + 1:] = 0
        return t
    ta, tb = r.host(prompts(6)), r.host(prompts(8))
    r.arm()
    a = eng.embed_tokens(ta)
    r.asynchronous("text embed, first")
    r.scribble(ta)
    b = eng.embed_tokens(tb, normalize=False)                # the pinned staging buffer still has the first copy pending
    r.noted("text embed, second")
    r.scribble(tb)
    r.out("first", a)
    r.out("second", b)


@case("revo_vit_read_residual", "revo_vit_read_tap", "revo_vit_forward")
def parity_hooks_of_the_image_tower(r):
    eng = r.closing(_engine().VitEngine.synthetic(TOWER, seed=3, device=0, max_batch=8, experiments=True, randomize_affine=True))
    torch.cuda.synchronize()
    u8 = r.dev(images_u8(3, 86))
    r.arm()
    x = eng.residual_after(u8, 1)
    r.asynchronous("residual_after")
    taps = eng.taps(u8)
    r.asynchronous("taps")
    r.out("residual after one block", x)
    for k in sorted(taps):
        r.out("tap " + k, taps[k])


@case("revo_text_read_residual", "revo_text_forward")
def parity_hook_of_the_text_tower(r):
    eng = r.closing(_engine().TextEngine.synthetic(TEXT_TOWER, seed=5, device=0, max_batch=8, experiments=True))
    torch.cuda.synchronize()
    cfg = eng.cfg
    t = np.random.default_rng(87).integers(1, cfg.vocab_size - 1, (5, cfg.context_length)).astype(np.int32)
    t[:, -1] = cfg.vocab_size - 1
    th = r.host(t)
    r.arm()
    x = eng.residual_after(th, 1)
    r.asynchronous("text residual_after")
    r.scribble(th)
    r.out("residual after one block", x)


# ---- preprocess -------------------------------------------------------------------------------------------------------------------
@case("revo_preprocess_crop_resize")
def crop_resize_on_two_streams(r):
    from reverso_amd import preprocess as pp
    rng = np.random.default_rng(85)
    frames = [r.dev(torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))) for h, w in ((97, 131), (240, 135))]
    boxes = []
    for i in range(40):
        f = i % 2
        h, w = frames[f].shape[:2]
        x0, y0 = int(rng.integers(0, w - 8)), int(rng.integers(0, h - 8))
        boxes.append((f, x0, y0, int(rng.integers(x0 + 4, w + 1)), int(rng.integers(y0 + 4, h + 1))))
    r.arm()
    a = pp.crop_resize_device(frames, boxes, 56)
    r.asynchronous("crop_resize, first stream")
    first = torch.cuda.current_stream()
    second = r.stream2 if r.late else first
    second.wait_stream(first)
    with torch.cuda.stream(second):
        b = pp.crop_resize_device(frames, boxes[:17], 28)   # another stream: the documented wait for the previous call's
    first.wait_stream(second)
    c = pp.crop_resize_device(frames, boxes[5:], 56)         # and back
    b.record_stream(first)
    r.out("first stream", a)
    r.out("second stream", b)
    r.out("first stream again", c)


# ---- launchers no engine call reaches: through _lib ----------------------------------------------------------------------------
@case("revo_op_rope", "revo_op_f32_to_bf16", "revo_op_probe_qk")
def stand_alone_ops(r):
    lib = _lib()
    L = lib.load()
    seq, W, heads, n = 17, 128, 2, 34
    qkv = r.dev(rows(n, 90, 3 * W).to(torch.bfloat16))
    ang = rows(seq, 91, W // heads // 2)
    cs = r.dev(torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1))
    src = r.dev(rows(37, 92, 100))
    qp, wk, bk = r.dev(rows(1, 93, W)[0]), r.dev(rows(W, 94, W)), r.dev(rows(1, 95, W)[0])
    r.arm()
    st = lib.current_stream()
    lib.check(L.revo_op_rope(lib.ptr(qkv), 3 * W, lib.ptr(cs), n, seq, W, heads, st), "revo_op_rope")
    r.asynchronous("op_rope")
    dst = torch.empty((37, 104), dtype=torch.bfloat16, device=DEV)
    lib.check(L.revo_op_f32_to_bf16(lib.ptr(src), 100, lib.ptr(dst), 104, 37, 100, st), "revo_op_f32_to_bf16")
    r.asynchronous("op_f32_to_bf16")
    qk = torch.empty((heads, W), dtype=torch.float32, device=DEV)
    ck = torch.empty((heads,), dtype=torch.float32, device=DEV)
    lib.check(L.revo_op_probe_qk(lib.ptr(qp), lib.ptr(wk), lib.ptr(bk), W, heads, lib.ptr(qk), lib.ptr(ck), st), "revo_op_probe_qk")
    r.asynchronous("op_probe_qk")
    r.out("rope", qkv.view(torch.int16))
    r.out("bf16", dst.view(torch.int16))
    r.out("probe", (qk, ck))


# ---- sequences: several calls behind ONE sleep ------------------------------------------------------------------------------
@case("revo_search_topk")
def sequence_search_k10_then_k50(r):
    G = gallery(r, rows(N_ROWS, 100))
    G.search(rows(7, 113).to(DEV), k=50)                     # the handle's workspaces at their size: neither call below grows one
    torch.cuda.synchronize()
    qa, qb = r.dev(rows(N_Q, 101)), r.dev(rows(7, 102))
    r.arm()
    a = G.search(qa, k=10)
    r.asynchronous("search(k=10)")
    b = G.search(qb, k=50)                                   # its set-up is enqueued while the first call has not started
    r.asynchronous("search(k=50)")
    r.out("k=10", a)
    r.out("k=50", b)


@case("revo_search_mmr")
def sequence_mmr_twice(r):
    G = gallery(r, near_duplicates())
    qa, qb = r.dev(rows(N_Q, 103)), r.dev(rows(N_Q, 104))
    r.arm()
    a = G.search_mmr(qa, k=10, candidates=100, diversity=0.5)
    r.asynchronous("search_mmr, first")
    b = G.search_mmr(qb, k=10, candidates=100, diversity=0.3)
    r.asynchronous("search_mmr, second")                     # same sizes: nothing grows, both calls are pending at once
    r.out("first", a)
    r.out("second", b)


@case("revo_search_fusion")
def sequence_fusion_twice(r):
    G = gallery(r, rows(N_ROWS, 105))
    qa, qb = r.dev(rows(6, 106).reshape(3, 2, D)), r.dev(rows(6, 107).reshape(3, 2, D))
    r.arm()
    a = G.search_fusion(qa, k=10, limit=50)
    r.asynchronous("search_fusion, first")
    b = G.search_fusion(qb, k=10, limit=50, method="dbsf")
    r.asynchronous("search_fusion, second")                  # same sizes: nothing grows, both calls are pending at once
    r.out("first", a)
    r.out("second", b)


@case("revo_search_topk", "revo_search_topk_large")
def sequence_workspace_grows_between_two_calls(r):
    G = gallery(r, rows(N_ROWS, 108))
    qa, qb = r.dev(rows(3, 109)), r.dev(rows(300, 110))
    r.arm()
    a = G.search(qa, k=10)
    r.asynchronous("search(3 queries)")
    b = G.search(qb, k=10)                                   # the per-query arrays grow: waits for the stream, then frees
    r.noted("search(300 queries)")
    c = G.search(qa, k=200)
    d = G.search(qb, k=200)
    r.noted("search(300 queries, k=200)")
    r.out("3 queries", a)
    r.out("300 queries", b)
    r.out("3 queries, k=200", c)
    r.out("300 queries, k=200", d)


def unit_rows():
    return torch.nn.functional.normalize(rows(N_ROWS, 111), dim=1)


@case("revo_gallery_append", "revo_search_topk", "revo_op_gallery_cert_stats")
def sequence_clear_between_two_appends(r):
    """rows of norm 2^20 as given -> clear() -> unit rows -> search -> cert_stats: the maxima of the rows that left must not
    survive the clear (and the clear must not land on the maxima of the rows that came after it)."""
    G = gallery(r, capacity=N_ROWS)
    big = r.dev(unit_rows() * float(2 ** 20))
    unit = r.dev(unit_rows())
    q = r.dev(rows(N_Q, 112))
    r.arm()
    G.add(big, normalize=False)
    r.asynchronous("add(rows of norm 2^20)")
    G.clear()
    r.asynchronous("clear")
    G.add(unit, normalize=False)
    r.asynchronous("add(unit rows)")
    r.out("search", G.search(q, k=10))
    r.asynchronous("search")
    r.out("cert", list(G.cert_stats()))
    r.synchronous("cert_stats")
    _stats(r, G, "stats")


def fresh_unit_gallery_cert_stats():
    """What a gallery that never held anything but the unit rows reports (default stream)."""
    G = _engine().Gallery(D, N_ROWS, device=0)
    try:
        G.add(unit_rows().to(DEV), normalize=False)
        return list(G.cert_stats())
    finally:
        G.close()


# ---- stand-ins for a library that breaks the contract (torch only): the harness must catch each ----------------------------
class _FakeHandle:
    """A 'library' with a counter and a workspace in its handle, written in torch."""

    def __init__(self):
        self.counter = torch.zeros(64, device=DEV)
        self.work = torch.zeros(64, device=DEV)

    def close(self):
        pass


def fake_zeroes_a_counter_on_the_default_stream(r):
    h = r.closing(_FakeHandle())
    x = r.dev(rows(1, 200)[0])
    r.arm()
    h.counter.add_(x)                                        # step 1, on the caller's stream
    with torch.cuda.stream(torch.cuda.default_stream()):
        h.counter.zero_()                                    # the reset between the steps: on stream 0
    out = h.counter + x                                      # step 2
    r.asynchronous("fake call")
    r.out("out", out)


def fake_launches_its_middle_step_on_the_default_stream(r):
    h = r.closing(_FakeHandle())
    x = r.dev(rows(1, 201)[0])
    r.arm()
    torch.mul(x, 2.0, out=h.work)
    with torch.cuda.stream(torch.cuda.default_stream()):
        mid = h.work + 1.0
    out = mid * 3.0
    r.asynchronous("fake call")
    r.out("out", out)


def fake_synchronises_inside_an_asynchronous_call(r):
    h = r.closing(_FakeHandle())
    x = r.dev(rows(1, 202)[0])
    r.arm()
    torch.mul(x, 2.0, out=h.work)
    torch.cuda.current_stream().synchronize()
    out = h.work + 1.0
    r.asynchronous("fake call")
    r.out("out", out)


def fake_that_keeps_the_contract(r):
    h = r.closing(_FakeHandle())
    x = r.dev(rows(1, 203)[0])
    r.arm()
    torch.mul(x, 2.0, out=h.work)
    out = h.work + 1.0
    r.asynchronous("fake call")
    r.out("out", out)
