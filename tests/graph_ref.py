"""Reference model, checker and shared inputs for the fused graph-batch
fetch, ``DDStore.get_graph_batch``.

The model is plain NumPy, written from the documented semantics and
independent of ``store.py``'s host path: ``tests/test_graph_batch_cpu.py``
runs that host path against it, ``tests/test_gpu_graph_batch.py`` the
kernels (k_csr_scan3, k_gather_csr_relabel, k_graph_fill).

For a request ``idx`` of ``n`` graphs into buffers of ``Ncap`` nodes and
``Ecap`` edges:

* a bad index (outside ``[0, nsamples)``) is a graph of 0 nodes and 0 edges
  and counts once in ``oob_skipped`` of the node and of the edge variable;
* ``ptr`` / ``edge_ptr`` are the exclusive cumsums of the requested node /
  edge counts, never clamped;
* graph ``i``'s nodes are kept iff ``nodes_i > 0 and ptr[i+1] <= Ncap``
  (the rule of ``get_csr``); ``batch[ptr[i]:ptr[i+1]] = i`` for them and
  ``batch = n`` everywhere else;
* graph ``i``'s edges are kept iff ``edges_i > 0 and ptr[i+1] <= Ncap and
  edge_ptr[i+1] <= Ecap``; edge ``e`` of a kept graph is ``stored + ptr[i]``
  at position ``edge_ptr[i] + e``; every other slot holds ``edge_fill``;
* a graph with ``edges_i > 0`` whose edges are not kept counts once in the
  edge variable's ``cap_skipped``; its ``bytes_gathered`` grows by the kept
  edges times 2 times the stored itemsize. The node variable's counters move
  as under ``get_csr(out=)``.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

SENTINEL = 0x5A
GUARD = 4096  # sentinel bytes in front of and behind every buffer

G = 64  # lanes per graph of the relabel and fill kernels

Expected = namedtuple(
    "Expected", "ptr edge_ptr batch edge_index node_keep edge_keep "
                "node_counts edge_counts")

# (stored dtype, output dtype): the three widenings the kernels have
DTYPE_PAIRS = [(torch.int64, torch.int64), (torch.int32, torch.int64),
               (torch.int32, torch.int32)]


def expected(node_vals, node_lens, edge_pairs, edge_lens, idx, Ncap, Ecap, coo,
             edge_fill, out_dtype=np.int64):
    """The model of the module docstring. ``node_vals`` (nodes, disp) and
    ``edge_pairs`` (edges, 2) are the stored values of all graphs in order;
    counts are ``(oob_skipped, cap_skipped, bytes_gathered)`` deltas."""
    node_vals = np.asarray(node_vals)
    edge_pairs = np.asarray(edge_pairs)
    nl = np.asarray(node_lens, dtype=np.int64)
    el = np.asarray(edge_lens, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    ns, n = nl.size, idx.size
    e_start = np.concatenate([[0], np.cumsum(el)])
    ptr = np.zeros(n + 1, dtype=np.int64)
    edge_ptr = np.zeros(n + 1, dtype=np.int64)
    batch = np.full(Ncap, n, dtype=np.int64)
    flat = np.full((Ecap, 2), edge_fill, dtype=out_dtype)
    node_keep = np.zeros(n, dtype=bool)
    edge_keep = np.zeros(n, dtype=bool)
    oob = ncap_skip = ecap_skip = nkept = ekept = 0
    for i, g in enumerate(idx.tolist()):
        bad = g < 0 or g >= ns
        nn = 0 if bad else int(nl[g])
        ne = 0 if bad else int(el[g])
        oob += bad
        ptr[i + 1] = ptr[i] + nn
        edge_ptr[i + 1] = edge_ptr[i] + ne
        fits = ptr[i + 1] <= Ncap
        if nn > 0:
            if fits:
                node_keep[i] = True
                batch[ptr[i]:ptr[i + 1]] = i
                nkept += nn
            else:
                ncap_skip += 1
        if ne > 0:
            if fits and edge_ptr[i + 1] <= Ecap:
                edge_keep[i] = True
                stored = edge_pairs[e_start[g]:e_start[g] + ne].astype(np.int64)
                flat[edge_ptr[i]:edge_ptr[i + 1]] = (stored + ptr[i]).astype(out_dtype)
                ekept += ne
            else:
                ecap_skip += 1
    nb = node_vals.shape[1] * node_vals.dtype.itemsize if node_vals.ndim == 2 else 0
    return Expected(
        ptr, edge_ptr, batch, np.ascontiguousarray(flat.T) if coo else flat,
        node_keep, edge_keep, (int(oob), ncap_skip, nkept * nb),
        (int(oob), ecap_skip, ekept * 2 * edge_pairs.dtype.itemsize))


# ---------------------------------------------------------------------------
# shared inputs
# ---------------------------------------------------------------------------
def make_graphs(node_lens, edge_lens, seed, disp=3):
    """Stored data of a set of graphs: f32 node features of random bits'
    worth of values, and (src, dst) pairs local to each graph whose first
    edge names node 0 and whose last names node ``nodes - 1`` (both ends of
    the id range). A graph without nodes has no edges."""
    rng = np.random.default_rng(seed)
    nl = np.asarray(node_lens, dtype=np.int64)
    el = np.asarray(edge_lens, dtype=np.int64)
    assert not np.any((nl == 0) & (el > 0))
    x = rng.standard_normal((int(nl.sum()), disp)).astype(np.float32)
    pairs = np.zeros((int(el.sum()), 2), dtype=np.int64)
    o = 0
    for n_i, e_i in zip(nl.tolist(), el.tolist()):
        if e_i:
            p = rng.integers(0, n_i, (e_i, 2))
            p[0] = (0, 0)
            p[-1] = (n_i - 1, n_i - 1) if e_i > 1 else p[-1]
            pairs[o:o + e_i] = p
            o += e_i
    return x, nl, pairs, el


# The shapes at which the kernels can go wrong, in one request: no nodes;
# one node with a self-loop; nodes without edges; edge counts around the lane
# group; node and edge counts 1, 2, 3 in a row, which walk ptr through both
# residues mod 2 and edge_ptr through all four mod 4.
SHAPE_NODES = [0, 1, 5, 7, 70, 66, 3, 130, 1, 2, 3, 1, 2, 3, 9, 4]
SHAPE_EDGES = [0, 1, 0, G - 1, G, G + 1, 2, 2 * G + 1, 1, 2, 3, 1, 1, 1, 5, 0]


@functools.lru_cache(maxsize=None)
def shape_graphs():
    x, nl, pairs, el = make_graphs(SHAPE_NODES, SHAPE_EDGES, seed=11)
    assert pairs[0].tolist() == [0, 0]  # the self-loop of the one-node graph
    return x, nl, pairs, el


@functools.lru_cache(maxsize=None)
def tile_graphs():
    """64 small graphs for the request-size sweep."""
    nl = [(3 * i) % 7 for i in range(64)]
    el = [0 if n == 0 else (5 * i) % 9 for i, n in enumerate(nl)]
    return make_graphs(nl, el, seed=12, disp=1)


def register(store, tag, graphs, stored_dtype):
    """add_csr the node and edge variables of ``graphs``; returns names."""
    x, nl, pairs, el = graphs
    names = (f"{tag}_x", f"{tag}_ei")
    store.add_csr(names[0], torch.from_numpy(x), torch.from_numpy(nl))
    store.add_csr(names[1], torch.from_numpy(pairs).to(stored_dtype),
                  torch.from_numpy(el))
    return names


def exact_caps(graphs, idx):
    _, nl, _, el = graphs
    idx = np.asarray(idx)
    ok = idx[(idx >= 0) & (idx < nl.size)]
    return int(nl[ok].sum()), int(el[ok].sum())


def cut_caps(graphs, idx):
    """{label: (Ncap, Ecap)} for an in-range request: cuts on a graph
    boundary, inside a graph, with nothing kept, and on Ecap alone."""
    _, nl, _, el = graphs
    idx = np.asarray(idx)
    ptr = np.concatenate([[0], np.cumsum(nl[idx])])
    eptr = np.concatenate([[0], np.cumsum(el[idx])])
    N, E = int(ptr[-1]), int(eptr[-1])
    mid = [i for i in range(idx.size // 2, idx.size) if nl[idx[i]] > 1 and el[idx[i]] > 1][0]
    first_n = int(nl[idx][np.nonzero(nl[idx])[0][0]])
    return {
        "exact": (N, E),
        "nodes_on_boundary": (int(ptr[mid + 1]), E),
        "nodes_inside_graph": (int(ptr[mid + 1]) - 1, E),
        "edges_on_boundary": (N, int(eptr[mid + 1])),
        "edges_inside_graph": (N, int(eptr[mid + 1]) - 1),
        "edges_only": (N, 0),
        "nothing_kept": (first_n - 1, E),
        "zero": (0, 0),
        "both_cut": (int(ptr[mid]) + 1, int(eptr[mid // 2 + 1])),
    }


# ---------------------------------------------------------------------------
# checker
# ---------------------------------------------------------------------------
def _guarded(nbytes, dtype, device, fill=SENTINEL):
    """A ``dtype`` view of ``nbytes`` bytes cut out of a sentinel-filled
    backing buffer; returns (backing, view). GUARD keeps 16-B alignment."""
    backing = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8,
                         device=device)
    return backing, backing[GUARD:GUARD + nbytes].view(dtype)


def _guards_intact(backing, nbytes, fill=SENTINEL):
    b = backing.cpu()
    return bool((b[:GUARD] == fill).all()) and bool((b[GUARD + nbytes:] == fill).all())


_CTRS = ("oob_skipped", "cap_skipped", "bytes_gathered")


class Fetch:
    """One checked ``get_graph_batch`` call into sentinel-guarded buffers."""

    def __init__(self, store, names, graphs, stored_dtype, out_dtype, idx, Ncap,
                 Ecap, coo=True, edge_fill=-1, garbage=SENTINEL):
        self.store, self.names, self.graphs = store, names, graphs
        self.stored_dtype, self.out_dtype = stored_dtype, out_dtype
        self.idx = np.asarray(idx, dtype=np.int64)
        self.Ncap, self.Ecap, self.coo, self.edge_fill = int(Ncap), int(Ecap), coo, edge_fill
        self.garbage = garbage
        x = graphs[0]
        dev = store.device
        esz = torch.empty(0, dtype=out_dtype).element_size()
        self.nbytes = (self.Ncap * x.shape[1] * 4, 2 * self.Ecap * esz, self.Ncap * 8)
        self.bx, self.x_out = _guarded(self.nbytes[0], torch.float32, dev, garbage)
        self.be, self.edge_out = _guarded(self.nbytes[1], out_dtype, dev, garbage)
        self.bb, self.batch_out = _guarded(self.nbytes[2], torch.int64, dev, garbage)
        self.x_out = self.x_out.view(self.Ncap, x.shape[1])
        # the second buffer get_csr(out=) fills, for the bit-for-bit check of x
        self.bx2, self.x_ref = _guarded(self.nbytes[0], torch.float32, dev, garbage)
        self.x_ref = self.x_ref.view(self.Ncap, x.shape[1])
        self.idx_dev = torch.from_numpy(self.idx).to(dev)

    def _counters(self):
        return [tuple(self.store.query(nm)[k] for k in _CTRS) for nm in self.names]

    def run(self):
        before = self._counters()
        self.got = self.store.get_graph_batch(
            self.names[0], self.names[1], self.idx_dev, x_out=self.x_out,
            edge_out=self.edge_out, batch_out=self.batch_out, coo=self.coo,
            edge_dtype=self.out_dtype, edge_fill=self.edge_fill)
        after = self._counters()
        self.delta = [tuple(a - b for a, b in zip(aa, bb)) for aa, bb in zip(after, before)]
        return self

    def verify(self):
        x, nl, pairs, el = self.graphs
        np_out = np.int32 if self.out_dtype == torch.int32 else np.int64
        stored = pairs.astype(np.int32 if self.stored_dtype == torch.int32 else np.int64)
        m = expected(x, nl, stored, el, self.idx, self.Ncap, self.Ecap, self.coo,
                     self.edge_fill, np_out)
        tag = f"{self.names[1]} n={self.idx.size} Ncap={self.Ncap} Ecap={self.Ecap} coo={self.coo}"
        g = self.got
        assert g.x is self.x_out
        assert g.edge_index.dtype == self.out_dtype and g.batch.dtype == torch.int64
        assert tuple(g.edge_index.shape) == ((2, self.Ecap) if self.coo else (self.Ecap, 2))
        assert tuple(g.batch.shape) == (self.Ncap,)
        assert g.edge_index.data_ptr() == self.edge_out.data_ptr()
        assert g.batch.data_ptr() == self.batch_out.data_ptr()
        assert np.array_equal(g.ptr.cpu().numpy(), m.ptr), f"{tag}: ptr differs"
        assert np.array_equal(g.edge_ptr.cpu().numpy(), m.edge_ptr), f"{tag}: edge_ptr differs"
        got_b = g.batch.cpu().numpy()
        bad = np.nonzero(got_b != m.batch)[0]
        assert bad.size == 0, (
            f"{tag}: batch differs at {bad.size} slots, first {int(bad[0])}: "
            f"{int(got_b[bad[0]])} != {int(m.batch[bad[0]])}")
        got_e = g.edge_index.cpu().numpy()
        bad = np.argwhere(got_e != m.edge_index)
        assert bad.shape[0] == 0, (
            f"{tag}: edge_index differs at {bad.shape[0]} slots, first {bad[0].tolist()}: "
            f"{int(got_e[tuple(bad[0])])} != {int(m.edge_index[tuple(bad[0])])}")
        # a written edge never names a node that was not written
        kept_nodes = int((m.ptr[1:] - m.ptr[:-1])[m.node_keep].sum())
        named = got_e[got_e != np_out(self.edge_fill)]
        assert named.size == 0 or int(named.max()) < kept_nodes, (
            f"{tag}: an edge names node {int(named.max())} of {kept_nodes} kept")
        # x: bit for bit what get_csr(out=) writes into a second buffer,
        # its slack untouched, and the same offsets
        ref_before = tuple(self.store.query(self.names[0])[k] for k in _CTRS)
        if self.store.mode == "hip":
            _, off = self.store.get_csr(self.names[0], self.idx_dev, out=self.x_ref)
        else:
            # the host get_csr takes no bad index; its gather primitive does
            off = torch.from_numpy(m.ptr)
            self.store._backend.gather_csr(self.names[0], self.idx_dev, off,
                                           self.x_ref, self.Ncap)
        ref_after = tuple(self.store.query(self.names[0])[k] for k in _CTRS)
        assert torch.equal(off.cpu(), g.ptr.cpu())
        assert torch.equal(self.bx.cpu(), self.bx2.cpu()), f"{tag}: x differs from get_csr"
        # and the model's own word on x: every kept node row is the stored one
        L = m.ptr[1:] - m.ptr[:-1]
        kept = np.nonzero(m.node_keep)[0]
        goff = np.concatenate([[0], np.cumsum(nl)])
        rows = np.repeat(m.ptr[:-1][kept], L[kept]) + _ramp(L[kept])
        src = np.repeat(goff[self.idx[kept]], L[kept]) + _ramp(L[kept])
        assert np.array_equal(g.x.cpu().numpy()[rows].view(np.uint32),
                              x[src].view(np.uint32)), f"{tag}: x differs from the model"
        for backing, nb, what in ((self.bx, self.nbytes[0], "x"),
                                  (self.be, self.nbytes[1], "edge_index"),
                                  (self.bb, self.nbytes[2], "batch")):
            assert _guards_intact(backing, nb, self.garbage), f"{tag}: wrote around {what}"
        assert self.delta[0] == m.node_counts, f"{tag}: node counters grew by {self.delta[0]}"
        assert self.delta[0] == tuple(a - b for a, b in zip(ref_after, ref_before)), (
            f"{tag}: node counters differ from get_csr's")
        assert self.delta[1] == m.edge_counts, f"{tag}: edge counters grew by {self.delta[1]}"
        return m


def _ramp(lens):
    """0..L-1 for every L in ``lens``, concatenated."""
    lens = np.asarray(lens, dtype=np.int64)
    ends = np.cumsum(lens)
    return np.arange(int(lens.sum())) - np.repeat(ends - lens, lens)


def check(store, names, graphs, stored_dtype, out_dtype, idx, Ncap, Ecap, **kw):
    return Fetch(store, names, graphs, stored_dtype, out_dtype, idx, Ncap, Ecap,
                 **kw).run().verify()
