"""Many shards in one process: a thread-per-rank world, the shard layouts of
the many-shard tests and the checks both of their files share.

``tests/test_many_shards_cpu.py`` runs everything here on the host backend
(which proves the harness, the layouts and the expected-value code without a
GPU) and ``tests/test_gpu_many_shards.py`` runs it against the kernels. The
expected value is always built on the CPU from the concatenation of the
shards that were handed to ``add`` / ``add_csr``.

The world: ``VirtualWorld(W, device, register)`` starts W threads, each builds
``DDStore(comm=ThreadComm, device=device)`` and calls ``register(store,
rank)``. ``ThreadComm`` carries ``same_process = True``, so GPU stores exchange
``(pid, device pointer)`` entries instead of IPC handles (a process cannot
open its own). The fetch calls are one-sided and touch no comm, so
``world.stores[r]`` is then used from the calling thread; a collective
(``column_stats``) goes through ``world.run(fn)``.
"""
import functools
import hashlib
import threading

import numpy as np
import torch

from tests import cast_ref, graph_ref
from tests import csr_fast_ref as ref

SENTINEL = 0xA5
HEAD_BYTES = 4096   # sentinel in front of an output (keeps it 16-B aligned)
TAIL_BYTES = 4096   # sentinel behind it
_CTRS = ("oob_skipped", "cap_skipped")


# ---------------------------------------------------------------------------
# the thread communicator and the world
# ---------------------------------------------------------------------------
class _Shared:
    def __init__(self, size, timeout):
        self.size = size
        self.barrier = threading.Barrier(size, timeout=timeout)
        self.slots = [None] * size
        self.closed = False


class ThreadComm:
    """The mpi4py surface ``as_comm`` duck-types, for ranks that are threads
    of one process, and the explicit opt-in to same-process peer entries."""

    same_process = True

    def __init__(self, shared, rank):
        self._sh, self._rank = shared, rank

    def Get_rank(self):  # noqa: N802
        return self._rank

    def Get_size(self):  # noqa: N802
        return self._sh.size

    def Barrier(self):  # noqa: N802
        # a closed world is torn down by one thread: nobody else would come
        if not self._sh.closed and self._sh.size > 1:
            self._sh.barrier.wait()

    def allgather(self, obj):
        sh = self._sh
        sh.slots[self._rank] = obj
        if sh.size > 1:
            sh.barrier.wait()   # every slot written
        out = list(sh.slots)
        if sh.size > 1:
            sh.barrier.wait()   # every slot read before the next call reuses it
        return out

    def bcast(self, obj, root=0):
        return self.allgather(obj)[root]


class VirtualWorld:
    """W ranks as threads of this process. Use as a context manager (or call
    ``close()``): teardown frees every store, also after a failure."""

    def __init__(self, size, device, register=None, timeout=120.0):
        self.size, self.device = size, device
        self._sh = _Shared(size, timeout)
        self.comms = [ThreadComm(self._sh, r) for r in range(size)]
        self.stores = [None] * size

        def build(store_unused, rank):
            from ddstore_amd import DDStore

            s = DDStore(comm=self.comms[rank], device=device)
            self.stores[rank] = s
            if register is not None:
                register(s, rank)

        try:
            self._spmd(build, with_store=False)
        except BaseException:
            self.close()
            raise

    def _spmd(self, fn, with_store=True):
        """fn(store, rank) on every rank in its own thread; any rank's
        exception aborts the barrier (so no other rank waits for it) and is
        raised here."""
        results = [None] * self.size
        errors = [None] * self.size

        def body(rank):
            try:
                results[rank] = fn(self.stores[rank] if with_store else None, rank)
            except BaseException as e:  # noqa: BLE001
                errors[rank] = e
                self._sh.barrier.abort()

        threads = [threading.Thread(target=body, args=(r,), daemon=True)
                   for r in range(self.size)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        real = [e for e in errors
                if e is not None and not isinstance(e, threading.BrokenBarrierError)]
        if real:
            raise real[0]
        broken = [e for e in errors if e is not None]
        if broken:
            raise broken[0]
        return results

    def run(self, fn):
        """``[fn(store, rank) for every rank]``, each in its own thread:
        for the collective calls."""
        return self._spmd(fn)

    def close(self):
        """Free every store from this thread. Nothing of the world is in use
        any more, so the barrier inside ``DDStore.free`` is switched off
        first: no thread is left waiting in it, and no shard goes while
        another store could still read it."""
        self._sh.closed = True
        for s in self.stores:
            if s is not None:
                s.free()
        self.stores = [None] * self.size

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ---------------------------------------------------------------------------
# the layout table: rows per shard (CSR: samples per shard)
# ---------------------------------------------------------------------------
def _w128_rows():
    rows = [0 if r % 3 == 1 else r % 4 for r in range(128)]
    rows[64], rows[127] = 70, 3
    return rows


_ROWS = {
    # leading empty shard, isolated empty shards
    "w4": [0, 5, 0, 3],
    # kernel-argument directory with no padding slot; consecutive and trailing
    # empties; a shard larger than one 64-row tile
    "w8": [3, 0, 0, 70, 1, 0, 2, 0],
    # only slot 7 owns anything
    "w8_last": [0, 0, 0, 0, 0, 0, 0, 9],
    # first world that takes the LDS directory without the env knob
    "w9": [1, 0, 4, 0, 0, 65, 2, 0, 1],
    # the limit
    "w128": _w128_rows(),
    # binary search to the far end, and to the near one
    "w128_last": [0] * 127 + [5],
    "w128_first": [5] + [0] * 127,
}


class Layout:
    def __init__(self, lid):
        self.id = lid
        self.rows = list(_ROWS[lid])
        self.W = len(self.rows)
        self.prefix = np.concatenate([[0], np.cumsum(self.rows)]).astype(np.int64)
        self.total = int(self.prefix[-1])
        self.nonempty = [r for r, n in enumerate(self.rows) if n]
        self.last = self.nonempty[-1]          # last non-empty shard
        # the non-empty shard whose samples are all empty (CSR) and whose
        # graphs have nodes and no edges; a layout with one non-empty shard
        # has none
        self.zero = self.nonempty[0] if len(self.nonempty) > 1 else None
        big = int(np.argmax(self.rows))
        self.big = big if big not in (self.last, self.zero) else None

    def span(self, r):
        return int(self.prefix[r]), int(self.prefix[r + 1])

    def owner(self, g):
        return int(np.searchsorted(self.prefix, g, side="right")) - 1

    def readers(self):
        """Rank 0, the last rank and one rank whose own shard is empty."""
        empty = [r for r in range(1, self.W - 1) if self.rows[r] == 0]
        return sorted({0, self.W - 1, empty[0]})

    def describe(self, g):
        if not 0 <= g < self.total:
            return f"index {g} (out of range)"
        p = self.owner(g)
        return f"index {g} (shard {p}, local row {g - int(self.prefix[p])})"


LAYOUT_IDS = list(_ROWS)
LAYOUTS = {lid: Layout(lid) for lid in LAYOUT_IDS}


@functools.lru_cache(maxsize=None)
def index_set(lid, bad=False):
    """Every global row in order, the same reversed, the first and last row of
    every non-empty shard twice, and seeded random indices with duplicates
    (100, or as many as bring the request to 300: tiles of 64 rows need that
    many). ``bad=True`` puts -1, ``total`` and 2**40 into three different
    64-row tiles; the kernels are specified to skip and count those."""
    lay = LAYOUTS[lid]
    fwd = np.arange(lay.total, dtype=np.int64)
    edges = []
    for r in lay.nonempty:
        lo, hi = lay.span(r)
        edges += [lo, lo, hi - 1, hi - 1]
    n_fixed = 2 * lay.total + len(edges)
    rnd = np.random.default_rng(1000 + lay.W + lay.total).integers(
        0, lay.total, max(100, 300 - n_fixed))
    idx = np.concatenate([fwd, fwd[::-1], np.asarray(edges, dtype=np.int64), rnd])
    if bad:
        idx = np.insert(idx, [10, 150, idx.size - 5], [-1, lay.total, 2 ** 40])
        at = np.nonzero((idx < 0) | (idx >= lay.total))[0]
        assert len({int(a) // 64 for a in at}) == 3
    return torch.from_numpy(idx.astype(np.int64))


# ---------------------------------------------------------------------------
# the variables: global data, cut into shards by the layout
# ---------------------------------------------------------------------------
def _encoded(lay, disp, kind):
    """Rows whose every element encodes (owner, local row, column) uniquely:
    a wrong owner, a wrong local offset or a wrong column each change the
    bits."""
    g = np.arange(lay.total, dtype=np.int64)
    owner = np.searchsorted(lay.prefix, g, side="right") - 1
    local = g - lay.prefix[owner]
    col = np.arange(disp, dtype=np.int64)
    if kind == "f32":      # as bits; owner 127 stays below the NaN exponents
        bits = (owner[:, None] << 24) | (local[:, None] << 12) | col[None, :]
        return torch.from_numpy(bits.astype(np.int32)).view(torch.float32)
    if kind == "i64":
        bits = (owner[:, None] << 40) | (local[:, None] << 16) | col[None, :]
        return torch.from_numpy(bits)
    assert kind == "u8" and disp >= 3
    a = np.broadcast_to(0xF0 + col[None, :], (lay.total, disp)).copy()
    a[:, 0], a[:, 1] = owner, local
    return torch.from_numpy(a.astype(np.uint8))


def _exact(n, disp):
    """(row * 7 + column) % 251 as f32: exact in f32, f16 and bf16, so a cast
    of them is a plain ``.to()`` and no rounding question enters."""
    v = (torch.arange(n, dtype=torch.int64)[:, None] * 7
         + torch.arange(disp, dtype=torch.int64)[None, :]) % 251
    return v.to(torch.float32)


FIXED = {   # name: (how, disp)
    "enc128": ("f32", 128), "enc_i64": ("i64", 2), "u8x7": ("u8", 7),
    "val128": ("exact", 128), "val8": ("exact", 8), "val5": ("exact", 5),
    "st": ("stats", 3),
}
CSR = {     # name: (dtype, disp); None: exact values instead of random bits
    "c_f32x4": (torch.float32, 4), "c_f32x1": (torch.float32, 1),
    "c_u8x3": (torch.uint8, 3), "c_val4": (None, 4),
}
GRAPH = {"g_x": None, "g_ei64": torch.int64, "g_ei32": torch.int32}


def stats_array(lid):
    """(total, 3) f32 for column_stats: column 0 constant, the rest random."""
    lay = LAYOUTS[lid]
    a = (np.random.default_rng(77 + lay.total).standard_normal((lay.total, 3)) * 3
         + 100).astype(np.float32)
    a[:, 0] = a[0, 0]
    return a


@functools.lru_cache(maxsize=None)
def csr_lens(lid):
    """Stored sample lengths: (5 g) % 11 of the global sample id g, 0 where
    g % 4 == 0; all 0 in the layout's ``zero`` shard (sample_prefix advances,
    elem_prefix does not). Placed on top, for f32 x 1 elements (work items of
    256): 600 (three items) as the last sample of the last non-empty shard,
    so that shard's owner goes into a descriptor, 300 (two items) as its
    first, 256 (exactly one) as its second and 0 as its third where it has
    that many, and the three long ones again in the largest shard."""
    lay = LAYOUTS[lid]
    g = np.arange(lay.total, dtype=np.int64)
    lens = (5 * g) % 11
    lens[g % 4 == 0] = 0
    if lay.zero is not None:
        lo, hi = lay.span(lay.zero)
        lens[lo:hi] = 0
    lo, hi = lay.span(lay.last)
    if hi - lo >= 2:
        lens[lo] = 300
    if hi - lo >= 3:
        lens[lo + 1] = 256
    if hi - lo >= 4:
        lens[lo + 2] = 0       # an empty sample between the long ones
    lens[hi - 1] = 600
    if lay.big is not None:
        lo, _ = lay.span(lay.big)
        lens[lo + 1], lens[lo + 2], lens[lo + 3] = 300, 256, 600
    return [int(x) for x in lens]


@functools.lru_cache(maxsize=None)
def graphs(lid):
    """(x, node lens, pairs, edge lens) of the layout's graphs, one per
    sample: node and edge counts differ in every shard, the ``zero`` shard
    has nodes and no edges, and the last sample of the last non-empty shard
    has more edges than the 64 lanes that work on a graph."""
    lay = LAYOUTS[lid]
    g = np.arange(lay.total, dtype=np.int64)
    nl = 1 + (3 * g) % 5
    nl[g % 7 == 3] = 0
    el = np.where(nl > 0, (7 * g) % 9, 0)
    if lay.zero is not None:
        lo, hi = lay.span(lay.zero)
        nl[lo:hi] = np.maximum(nl[lo:hi], 1)
        el[lo:hi] = 0
    _, hi = lay.span(lay.last)
    nl[hi - 1], el[hi - 1] = 70, 130
    return graph_ref.make_graphs(nl, el, seed=21 + lay.total, disp=3)


@functools.lru_cache(maxsize=None)
def var_data(lid, name):
    """("fixed", full) or ("csr", values, lengths): the variable as ONE array
    over all shards, which is what every expected value is built from."""
    lay = LAYOUTS[lid]
    if name in FIXED:
        how, disp = FIXED[name]
        if how == "exact":
            return "fixed", _exact(lay.total, disp)
        if how == "stats":
            return "fixed", torch.from_numpy(stats_array(lid))
        return "fixed", _encoded(lay, disp, how)
    if name in CSR:
        dtype, disp = CSR[name]
        lens = csr_lens(lid)
        n = sum(lens)
        vals = (_exact(n, disp) if dtype is None
                else ref.random_values(n, dtype, disp, 500 + lay.total + disp))
        return "csr", vals, lens
    x, nl, pairs, el = graphs(lid)
    if name == "g_x":
        return "csr", torch.from_numpy(x), [int(v) for v in nl]
    return "csr", torch.from_numpy(pairs).to(GRAPH[name]), [int(v) for v in el]


def shard_of(lid, name, rank):
    """What rank ``rank`` hands to add (a tensor) or add_csr (values, lens)."""
    lay = LAYOUTS[lid]
    lo, hi = lay.span(rank)
    d = var_data(lid, name)
    if d[0] == "fixed":
        return (d[1][lo:hi],)
    goff = np.concatenate([[0], np.cumsum(d[2])]).astype(np.int64)
    return (d[1][int(goff[lo]):int(goff[hi])],
            torch.tensor(d[2][lo:hi], dtype=torch.int64))


def register(lid, names):
    """The ``register(store, rank)`` of a world holding ``names``."""
    def reg(store, rank):
        for name in names:
            sh = shard_of(lid, name, rank)
            if len(sh) == 1:
                store.add(name, sh[0])
            else:
                store.add_csr(name, sh[0], sh[1])
    return reg


def world(lid, device, names, **kw):
    return VirtualWorld(LAYOUTS[lid].W, device, register(lid, names), **kw)


# ---------------------------------------------------------------------------
# checks (host and GPU backend alike)
# ---------------------------------------------------------------------------
def _sync(store):
    if store.mode == "hip":
        torch.cuda.synchronize()


def _counters(store, name):
    q = store.query(name)
    return tuple(q[k] for k in _CTRS)


class Guarded:
    """An output cut out of a sentinel-filled backing buffer."""

    def __init__(self, shape, dtype, device, byte_offset=0):
        esz = torch.empty(0, dtype=dtype).element_size()
        self.nbytes = int(np.prod(shape)) * esz
        self.head = HEAD_BYTES + byte_offset
        self.backing = torch.full((self.head + self.nbytes + TAIL_BYTES,), SENTINEL,
                                  dtype=torch.uint8, device=device)
        self.out = self.backing[self.head: self.head + self.nbytes].view(dtype).view(shape)

    def region(self, row_bytes):
        """(rows, row_bytes) uint8 of the output on the CPU, after asserting
        that the guard bytes still hold the sentinel."""
        b = self.backing.cpu()
        assert bool((b[: self.head] == SENTINEL).all()), "wrote in front of the output"
        assert bool((b[self.head + self.nbytes:] == SENTINEL).all()), \
            "wrote behind the output"
        return b[self.head: self.head + self.nbytes].view(-1, row_bytes)


def _as_bytes(t):
    t = t.contiguous()
    return t.view(torch.uint8).view(t.shape[0], -1)


def check_batch(store, lid, name, idx, out_dtype=None, byte_offset=0, affine=None,
                expect_full=None, digest=None):
    """One ``get_batch`` into a guarded buffer against ``full[idx]`` (cast by
    ``.to()``, or ``expect_full``: the model's output for EVERY stored row).
    Bad indices leave their rows and the counters say how many there were."""
    lay = LAYOUTS[lid]
    full = var_data(lid, name)[1]
    out_dtype = out_dtype or full.dtype
    want_full = expect_full if expect_full is not None else full.to(out_dtype)
    assert want_full.dtype == out_dtype and want_full.shape == full.shape
    idx = torch.as_tensor(idx, dtype=torch.int64)
    n, disp = idx.numel(), full.shape[1]
    good = (idx >= 0) & (idx < lay.total)
    g = Guarded((n, disp), out_dtype, store.device, byte_offset)
    before = _counters(store, name)
    got = store.get_batch(name, idx.to(store.device), out=g.out, affine=affine)
    _sync(store)
    assert got.data_ptr() == g.out.data_ptr()
    region = g.region(disp * g.out.element_size())
    want = _as_bytes(want_full[idx[good]])
    same = (region[good] == want).all(dim=1)
    if not bool(same.all()):
        at = int(torch.nonzero(good)[int(torch.nonzero(~same)[0])])
        raise AssertionError(
            f"{lid} rank {store.rank} {name} -> {out_dtype}: request {at}, "
            f"{lay.describe(int(idx[at]))} differs")
    assert bool((region[~good] == SENTINEL).all()), \
        f"{lid} rank {store.rank} {name}: the row of a bad index was written"
    delta = tuple(a - b for a, b in zip(_counters(store, name), before))
    assert delta == (int((~good).sum()), 0), \
        f"{lid} rank {store.rank} {name}: (oob, cap) grew by {delta}"
    if digest is not None:
        digest.update(region.numpy().tobytes())


def affine_model(vals, out_kind, scale, shift, fused):
    """cast_ref's affine model of every element of ``vals`` (f32, 2-D), one
    call per column; ``fused`` is the kernels' fma, otherwise the host's two
    roundings. scale / shift: numbers or vectors of disp."""
    bits = cast_ref.from_torch(vals, "f32")
    disp = bits.shape[1]
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float32), (disp,))
    sh = np.broadcast_to(np.asarray(shift, dtype=np.float32), (disp,))
    f = cast_ref.model_affine if fused else cast_ref.model_affine_unfused
    out = np.empty(bits.shape, dtype=cast_ref.BITS[out_kind])
    for c in range(disp):
        out[:, c], _ = f(bits[:, c], "f32", out_kind, float(sc[c]), float(sh[c]))
    return cast_ref.to_torch(out, out_kind)


def check_csr_alloc(store, lid, name, idx):
    """``get_csr`` without ``out``: offsets and the whole packed payload
    against the model; a bad index has length 0 and is counted."""
    _, vals, lens = var_data(lid, name)
    idx = torch.as_tensor(idx, dtype=torch.int64)
    off, keep, packed = ref.expected(vals, lens, idx, cap=2 ** 62)
    nbad = int(((idx < 0) | (idx >= len(lens))).sum())
    before = _counters(store, name)
    got, got_off = store.get_csr(name, idx.to(store.device))
    _sync(store)
    tag = f"{lid} rank {store.rank} {name}"
    assert torch.equal(got_off.cpu(), off), f"{tag}: offsets differ"
    assert tuple(got.shape) == tuple(packed.shape) and got.dtype == vals.dtype
    same = (_as_bytes(got.cpu()) == _as_bytes(packed)).all(dim=1)
    if not bool(same.all()):
        e = int(torch.nonzero(~same)[0])
        s = int(torch.searchsorted(off, torch.tensor(e), right=True)) - 1
        raise AssertionError(
            f"{tag}: element {e} differs (request {s}, sample "
            f"{LAYOUTS[lid].describe(int(idx[s]))})")
    delta = tuple(a - b for a, b in zip(_counters(store, name), before))
    assert delta == (nbad, 0), f"{tag}: (oob, cap) grew by {delta}"


def check_csr_out(store, lid, name, idx, cut=False):
    """``get_csr(out=)`` by csr_fast_ref's model, at the exact capacity or,
    with ``cut``, at a capacity that ends in the middle of the last shard's
    three-item sample."""
    lay = LAYOUTS[lid]
    _, vals, lens = var_data(lid, name)
    idx = torch.as_tensor(idx, dtype=torch.int64)
    off, _, _ = ref.expected(vals, lens, idx, cap=0)
    cap = int(off[-1])
    if cut:
        s = lay.span(lay.last)[1] - 1
        assert lens[s] == 600
        at = int(torch.nonzero(idx == s)[0])
        cap = int(off[at]) + 300
    return ref.check(store, name, vals, lens, idx, cap)


def check_padded(store, lid, name, idx, max_len, out_dtype, pad, affine=None,
                 expect_vals=None):
    """``get_csr_padded`` into a guarded buffer: ``dense[i, j]`` is element j
    of sample idx[i] (``.to(out_dtype)``, or ``expect_vals``: the model's
    output for every stored element), pad slots hold the pad, ``lengths`` the
    true stored lengths; a bad index is an all-pad row of length 0."""
    _, vals, lens = var_data(lid, name)
    conv = expect_vals if expect_vals is not None else vals.to(out_dtype)
    assert conv.dtype == out_dtype and conv.shape == vals.shape
    idx = torch.as_tensor(idx, dtype=torch.int64)
    n, disp = idx.numel(), vals.shape[1]
    goff = np.concatenate([[0], np.cumsum(lens)])
    want = torch.tensor([pad], dtype=out_dtype).repeat(n, max_len, disp)
    want_len = torch.zeros(n, dtype=torch.int64)
    nbad = 0
    for i, s in enumerate(idx.tolist()):
        if not 0 <= s < len(lens):
            nbad += 1
            continue
        want_len[i] = lens[s]
        k = min(lens[s], max_len)
        want[i, :k] = conv[goff[s]: goff[s] + k]
    g = Guarded((n, max_len, disp), out_dtype, store.device)
    before = _counters(store, name)
    dense, lengths = store.get_csr_padded(name, idx.to(store.device), max_len,
                                          out=g.out.view(-1), affine=affine,
                                          pad_value=pad)
    _sync(store)
    tag = f"{lid} rank {store.rank} {name} padded"
    assert dense.data_ptr() == g.out.data_ptr() and tuple(dense.shape) == (n, max_len, disp)
    assert torch.equal(lengths.cpu(), want_len), f"{tag}: lengths differ"
    row_bytes = max_len * disp * g.out.element_size()
    same = (g.region(row_bytes) == _as_bytes(want.view(n, -1))).all(dim=1)
    if not bool(same.all()):
        at = int(torch.nonzero(~same)[0])
        raise AssertionError(
            f"{tag}: row {at}, sample {LAYOUTS[lid].describe(int(idx[at]))} differs")
    delta = tuple(a - b for a, b in zip(_counters(store, name), before))
    assert delta == (nbad, 0), f"{tag}: (oob, cap) grew by {delta}"


def check_graph(store, lid, stored_dtype, out_dtype, idx, coo):
    """``get_graph_batch`` by graph_ref's model at the exact capacities."""
    gr = graphs(lid)
    names = ("g_x", "g_ei64" if stored_dtype == torch.int64 else "g_ei32")
    idx = np.asarray(idx, dtype=np.int64)
    ncap, ecap = graph_ref.exact_caps(gr, idx)
    return graph_ref.check(store, names, gr, stored_dtype, out_dtype, idx, ncap, ecap,
                           coo=coo)


def check_ranges(store, lid, name):
    """``get`` (get_range): every non-empty shard's whole range comes back,
    also when ``start`` is the prefix of a run of empty shards in front of
    it; a range that crosses into the next non-empty shard raises."""
    lay = LAYOUTS[lid]
    full = var_data(lid, name)[1]
    for k, r in enumerate(lay.nonempty):
        lo, hi = lay.span(r)
        if r > 0 and lay.rows[r - 1] == 0:
            assert int(lay.prefix[r - 1]) == lo   # the empty run starts here too
        out = torch.full((hi - lo, full.shape[1]), 0, dtype=full.dtype).to(store.device)
        store.get(name, out, start=lo)
        _sync(store)
        assert torch.equal(_as_bytes(out.cpu()), _as_bytes(full[lo:hi])), \
            f"{lid} rank {store.rank} {name}: range of shard {r} differs"
        if k + 1 < len(lay.nonempty):
            over = torch.empty((hi - lo + 1, full.shape[1]), dtype=full.dtype).to(store.device)
            try:
                store.get(name, over, start=lo)
            except RuntimeError as e:
                assert "Invalid count on target" in str(e)
            else:
                raise AssertionError(
                    f"{lid} {name}: a range crossing from shard {r} into shard "
                    f"{lay.nonempty[k + 1]} was not refused")
    try:
        store.get(name, torch.empty((1, full.shape[1]), dtype=full.dtype).to(store.device),
                  start=lay.total)
    except RuntimeError as e:
        assert "Invalid start on target" in str(e)
    else:
        raise AssertionError(f"{lid} {name}: start == total was not refused")


def tiled_digest(w, lid, bad):
    """SHA-256 over the outputs of the two tiled fetches (f32 -> bf16 and the
    f32 byte move, rows of 128) from every reader rank, each checked on the
    way. Two runs that differ only in the directory must give the same."""
    h = hashlib.sha256()
    idx = index_set(lid, bad)
    for r in LAYOUTS[lid].readers():
        check_batch(w.stores[r], lid, "val128", idx, torch.bfloat16, digest=h)
        check_batch(w.stores[r], lid, "enc128", idx, digest=h)
    return h.hexdigest()
