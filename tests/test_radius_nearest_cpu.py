"""The nearest-``K`` cap of both radius-graph fetches on the host backend;
tests/test_gpu_radius_nearest.py runs the same cases on the kernels.

The reference is the float64 brute force of tests/radius_ref.py and
tests/test_radius_pbc_cpu.py at exact capacities, thinned by the documented
rule: per dst, rank the run's edges by (d2, position in the run), keep the K
smallest, emit them in the old order. d2 comes from the model's edge vectors in
float64 and is exact (all fixtures sit on a 1/8 grid), so every element and
every edge_vec bit must be equal; the grid makes ties abundant."""
import functools

import numpy as np
import pytest
import torch

from ddstore_amd import _C
from tests import radius_ref as ref
from tests import test_radius_graph_cpu as open_cases
from tests import test_radius_pbc_cpu as pbc

KMAX = _C.RADIUS_NEAREST_MAX


def thin(dst, vec, edge_ptr, K):
    """(keep mask, thinned edge_ptr) of an edge list in run order."""
    d2 = (vec.astype(np.float64) ** 2).sum(1)
    cuts = np.flatnonzero(np.diff(dst, prepend=-1, append=-1))  # run boundaries
    keep = np.zeros(len(dst), dtype=bool)
    for a, b in zip(cuts[:-1], cuts[1:]):
        keep[a + np.argsort(d2[a:b], kind="stable")[:K]] = True
    return keep, np.concatenate([[0], np.cumsum(keep)])[edge_ptr], np.diff(cuts)


class Nearest:
    """The store with ``nearest=True`` on the open call, for ref.check."""

    def __init__(self, store):
        self._store = store

    def __getattr__(self, name):
        return getattr(self._store, name)

    def get_radius_graph_batch(self, *a, **kw):
        return self._store.get_radius_graph_batch(*a, nearest=True, **kw)


@functools.lru_cache(maxsize=None)
def dense():
    """One graph of T+1 nodes on the 1/8 grid of a unit box: nearly every pair
    is within R = 1.3 and most distances tie."""
    pos = np.random.default_rng(17).integers(0, 9, (ref.T + 1, 3)) / 8.0
    return pos, np.array([ref.T + 1], dtype=np.int64), np.array([0], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def open_model(which, extra_empty=0):
    """The uncapped model at exact capacities. Shared: do not modify."""
    pos, lens, idx = (dense() if which == "dense" else
                      open_cases.grid() + (ref.request(extra_empty),))
    m = ref.expected(pos, lens, idx, ref.R, int(lens.sum()) * 2, int((lens ** 2).sum()) * 2)
    E = int(m.edge_ptr[-1])
    return pos, lens, idx, int(m.ptr[-1]), m._replace(
        batch=m.batch[:m.ptr[-1]], edge_index=m.edge_index[:, :E], vec=m.vec[:E])


def run_open(store, which="grid", K=1, stored=np.float32, extra_empty=0, coo=True,
             edge_dtype=torch.int64):
    pos, lens, idx, N, m = open_model(which, extra_empty)
    keep, edge_ptr, runs = thin(m.edge_index[1], m.vec, m.edge_ptr, K)
    if which == "dense":  # several queue flushes per dst
        assert runs.min() > KMAX + 64
    e = m.edge_index[:, keep].astype(np.int32 if edge_dtype == torch.int32 else np.int64)
    want = m._replace(edge_ptr=edge_ptr, edge_index=e if coo else np.ascontiguousarray(e.T),
                      vec=m.vec[keep], vec_rows=np.ones(int(keep.sum()), dtype=bool),
                      counts=m.counts[:2] + (m.counts[2] // 8 * np.dtype(stored).itemsize,))
    store.add_csr("pos", torch.from_numpy(pos.astype(stored)), torch.from_numpy(lens))
    ref.check(Nearest(store), "pos", pos.astype(stored), lens, idx, ref.R, N,
              int(keep.sum()), K=K, coo=coo, edge_dtype=edge_dtype, m=want)


def check_pbc(store, K, Ncap=None, Ecap=None, edge_fill=-1, **rule):
    """One periodic call with max_neighbors=K into sentinel-guarded buffers
    against the thinned model; Ncap / Ecap default to the exact ones."""
    idx = tuple(pbc.REQUEST)
    m = pbc.expected(idx, Ncap, None, **rule)  # the node cut, every edge
    keep, edge_ptr, _ = thin(m.edge_index[1], m.vec, m.edge_ptr, K)
    N = int(m.ptr[-1]) if Ncap is None else Ncap
    E = int(edge_ptr[-1]) if Ecap is None else Ecap
    rows = int(edge_ptr[int((edge_ptr[1:] <= E).sum())])  # a prefix keeps its edges
    dev = store.device
    nbytes = (N * 12, E * 16, N * 8, E * 12, E * 12)
    dts = (torch.float32, torch.int64, torch.int64, torch.int32, torch.float32)
    (bp, po), (be, eo), (bb, bo), (bs, so), (bv, vo) = (
        ref._guarded(nb, dt, dev) for nb, dt in zip(nbytes, dts))
    before = store.query("pos")["cap_skipped"]
    g = store.get_radius_graph_pbc_batch(
        "pos", "cell", torch.tensor(idx, device=dev), pbc.R, max_neighbors=K,
        pos_out=po.view(N, 3), edge_out=eo, batch_out=bo, shift_out=so, vec_out=vo,
        edge_vec=True, edge_fill=edge_fill, **rule)
    assert store.query("pos")["cap_skipped"] - before == m.counts[1]
    assert np.array_equal(g.ptr.cpu().numpy(), m.ptr)
    assert np.array_equal(g.edge_ptr.cpu().numpy(), edge_ptr)
    assert np.array_equal(g.batch.cpu().numpy(), m.batch)
    assert np.array_equal(g.shifts_needed.cpu().numpy(), m.needed)
    sentinel = np.frombuffer(bytes([ref.SENTINEL]) * 4, np.int32)[0]
    for got, model, rest in ((g.edge_index.cpu().numpy().T, m.edge_index.T, edge_fill),
                             (g.edge_shift.cpu().numpy(), m.shift, sentinel),
                             (g.edge_vec.cpu().numpy().view(np.int32),
                              m.vec.view(np.int32), sentinel)):
        assert np.array_equal(got[:rows], model[keep][:rows]) and (got[rows:] == rest).all()
    for backing, nb in zip((bp, be, bb, bs, bv), nbytes):
        assert ref._intact(backing, nb)
    return g, edge_ptr, m


PBC_RULES = {"base": {}, "loop": {"loop": True}, "max_shift_1": {"max_shift": 1},
             "pbc_FFF": {"pbc": (False,) * 3}}


def run_pbc(store, rule, K):
    pbc.fill_store(store)
    g, edge_ptr, m = check_pbc(store, K, **PBC_RULES[rule])
    if rule == "base":  # the cube's atom: 18 self-images within R, all ties
        assert m.edge_ptr[3] - m.edge_ptr[2] == 18 and edge_ptr[3] - edge_ptr[2] == K
    if rule == "pbc_FFF":
        h = store.get_radius_graph_batch("pos", list(pbc.REQUEST), pbc.R, max_neighbors=K,
                                         nearest=True, edge_vec=True)
        assert torch.equal(h.edge_ptr, g.edge_ptr) and torch.equal(h.edge_index, g.edge_index)
        assert torch.equal(h.edge_vec.view(torch.int32), g.edge_vec.view(torch.int32))


def run_noop(store):
    """K above every degree: exactly the uncapped calls."""
    pbc.fill_store(store)
    idx = list(pbc.REQUEST)
    a = store.get_radius_graph_pbc_batch("pos", "cell", idx, pbc.R, edge_vec=True)
    b = store.get_radius_graph_pbc_batch("pos", "cell", idx, pbc.R, edge_vec=True,
                                         max_neighbors=KMAX)
    c = store.get_radius_graph_batch("pos", idx, pbc.R, edge_vec=True)
    d = store.get_radius_graph_batch("pos", idx, pbc.R, edge_vec=True, max_neighbors=KMAX,
                                     nearest=True)
    for u, v in ((a, b), (c, d)):
        degree = torch.unique_consecutive(u.edge_index[1], return_counts=True)[1]
        assert 6 < int(degree.max()) < KMAX
        assert torch.equal(u.edge_ptr, v.edge_ptr) and torch.equal(u.edge_index, v.edge_index)
        assert torch.equal(u.edge_vec.view(torch.int32), v.edge_vec.view(torch.int32))
    assert torch.equal(a.edge_shift, b.edge_shift)


def run_capacity_cuts(store):
    pbc.fill_store(store)
    K = 6
    _, full, _ = check_pbc(store, K)
    N, E = int(pbc.sizes()[1]), int(full[-1])
    _, cut, _ = check_pbc(store, K, Ncap=N - 1, edge_fill=-7)  # the last node does not fit
    assert cut[-1] == cut[-2] == full[-2] < E
    _, cut, _ = check_pbc(store, K, Ecap=int(full[pbc.MID + 1]) - 1)  # nor these edges
    assert cut[-1] == E and full[pbc.MID] > 0
    ok = [i for i in pbc.REQUEST if i < len(pbc.GRAPHS)]  # sized by the call
    g = store.get_radius_graph_pbc_batch("pos", "cell", ok, pbc.R, max_neighbors=K)
    assert g.edge_index.shape[1] == g.edge_shift.shape[0] == int(g.edge_ptr[-1]) == E
    assert E <= N * K


def run_refusals(store):
    store.add_csr("pos", torch.zeros(5, 3), torch.tensor([2, 3]))
    store.add("cell", torch.eye(3).reshape(1, 9).repeat(2, 1))
    with pytest.raises(ValueError, match="nearest"):
        store.get_radius_graph_batch("pos", [0], 1.0, nearest=True)
    for k in (0, KMAX + 1, 1.5):
        with pytest.raises(ValueError):
            store.get_radius_graph_batch("pos", [0], 1.0, max_neighbors=k, nearest=True)
        with pytest.raises(ValueError):
            store.get_radius_graph_pbc_batch("pos", "cell", [0], 1.0, max_neighbors=k)


OPEN = {
    "K1": {"K": 1}, "K4": {"K": 4}, "K1_f64": {"K": 1, "stored": np.float64},
    "K4_pairs_int32": {"K": 4, "coo": False, "edge_dtype": torch.int32},
    "K4_small_mean": {"K": 4, "extra_empty": 40},
    **{f"dense_K{k}": {"which": "dense", "K": k} for k in (63, 64, 65, KMAX)},
}


@pytest.fixture
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    yield s
    s.free()


@pytest.mark.parametrize("case", list(OPEN))
def test_open(store, case):
    run_open(store, **OPEN[case])


@pytest.mark.parametrize("K", [1, 6])
@pytest.mark.parametrize("rule", list(PBC_RULES))
def test_pbc(store, rule, K):
    run_pbc(store, rule, K)


@pytest.mark.parametrize("run", [run_noop, run_capacity_cuts, run_refusals])
def test_properties(store, run):
    run(store)
