"""``get_radius_graph_batch(..., algorithm="cells")`` on the host backend (which
checks the argument and ignores it) against the model of tests/radius_ref.py;
tests/test_gpu_radius_cells.py runs the same cases on the cell-list kernels.
The result must equal the brute-force one bit for bit, so the cases of
tests/test_radius_graph_cpu.py run again with the argument bound, next to
graphs aimed at the binning: pairs at exactly r, shifted origins, flat and
single-bin boxes, a box that must be coarsened, nodes without a bin, and more
coincident nodes than a dst orders in LDS."""
import functools

import numpy as np
import pytest
import torch

from ddstore_amd import _C
from tests import radius_ref as ref
from tests import test_radius_graph_cpu as brute
from tests.test_radius_graph_cpu import store  # noqa: F401  (the fixture)

GRID_CASES = ["base", "f64", "pairs", "int32", "loop", "K1", "K4", "no_vec"]


def bind_cells(store, monkeypatch):  # noqa: F811
    monkeypatch.setattr(store, "get_radius_graph_batch", functools.partial(
        store.get_radius_graph_batch, algorithm="cells"))


def run_grid_case(store, monkeypatch, case):  # noqa: F811
    assert 2 * ref.T + 3 > 2 * 256  # the largest graph spans three blocks of dst
    bind_cells(store, monkeypatch)
    brute.run_grid_case(store, **brute.CASES[case])


def run_capacity_cuts(store, monkeypatch):  # noqa: F811
    bind_cells(store, monkeypatch)
    brute.run_capacity_cuts(store)


@functools.lru_cache(maxsize=None)
def boundary_graphs():
    """Hand-made graphs for r = 1.0, every coordinate a multiple of 1/8 (or
    huge), so d2 is exact in float32 where it is finite."""
    rng = np.random.default_rng(5)
    ax = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1.125, 0, 0],
                   [0, 1.125, 0], [0, 0, 1.125], [-1, 0, 0], [-1.125, 0, 0]])
    flat = rng.integers(0, 33, (40, 3)) / 8.0
    flat[:, 2] = 0.5
    one_bin = rng.integers(0, 5, (10, 3)) / 8.0
    far = rng.integers(0, 17, (16, 3)) / 8.0
    far[8:, 0] += 1e30
    odd = rng.integers(0, 17, (12, 3)) / 8.0
    odd[2, 0], odd[5, 1], odd[9, 2] = np.nan, np.inf, -np.inf
    n = _C.RADIUS_CELLS_SORT_MAX + 5
    heap = np.full((n + 7, 3), 2.0)  # n nodes at one point
    heap[[3, 15, 27, 39, 51, 63]] += [0.5, 0.0, 0.0]  # six apart, spread over the ids
    heap[7] += 5.0
    graphs = [ax, ax - 37.5, ax + 2.0 ** 20, flat, one_bin, far, odd, heap]
    lens = np.array([len(g) for g in graphs], dtype=np.int64)
    return np.concatenate(graphs).astype(np.float32), lens


def run_boundary(store, monkeypatch, K):  # noqa: F811
    bind_cells(store, monkeypatch)
    pos, lens = boundary_graphs()
    idx = np.arange(len(lens))
    with np.errstate(all="ignore"):  # the model squares 1e30 and subtracts inf
        m = ref.expected(pos, lens, idx, 1.0, 10 ** 6, 10 ** 6, K, f32=True)
        first = m.degrees[:9]  # the axis graph: node 0 reaches the four at exactly r
        assert first[0] == (4 if K is None else min(K, 4)) and first[4] == 1
        assert K is not None or m.degrees.max() > _C.RADIUS_CELLS_SORT_MAX
        store.add_csr("pos", torch.from_numpy(pos), torch.from_numpy(lens))
        ref.check(store, "pos", pos, lens, idx, 1.0, int(m.ptr[-1]), int(m.edge_ptr[-1]),
                  K, f32=True)


def run_random_f32(store, monkeypatch):  # noqa: F811
    bind_cells(store, monkeypatch)
    rng = np.random.default_rng(13)
    lens = np.array([1, 17, 601], dtype=np.int64)
    pos = (rng.random((int(lens.sum()), 3)) * 5.0 - 1.5).astype(np.float32)
    store.add_csr("pos", torch.from_numpy(pos), torch.from_numpy(lens))
    idx = np.array([2, 0, 1, 2])
    m = ref.expected(pos, lens, idx, 0.9, 10 ** 6, 10 ** 6, f32=True)
    assert m.degrees.mean() > 8
    ref.check(store, "pos", pos, lens, idx, 0.9, int(m.ptr[-1]), int(m.edge_ptr[-1]),
              f32=True)


def run_refusals_and_dispatch(store):  # noqa: F811
    pos, lens = brute.grid()
    idx = ref.request()
    store.add_csr("pos", torch.from_numpy(pos.astype(np.float32)), torch.from_numpy(lens))
    with pytest.raises(ValueError, match="algorithm"):
        store.get_radius_graph_batch("pos", idx, ref.R, algorithm="grid")
    with pytest.raises(ValueError, match="nearest"):
        store.get_radius_graph_batch("pos", idx, ref.R, max_neighbors=4, nearest=True,
                                     algorithm="cells")
    a, b = (store.get_radius_graph_batch("pos", idx, ref.R, edge_vec=True, algorithm=alg)
            for alg in ("brute", "auto"))
    for x, y in zip((a.pos, a.ptr, a.batch, a.edge_ptr, a.edge_index, a.edge_vec),
                    (b.pos, b.ptr, b.batch, b.edge_ptr, b.edge_index, b.edge_vec)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("case", GRID_CASES)
def test_grid(store, monkeypatch, case):  # noqa: F811
    run_grid_case(store, monkeypatch, case)


def test_capacity_cuts(store, monkeypatch):  # noqa: F811
    run_capacity_cuts(store, monkeypatch)


@pytest.mark.parametrize("K", [None, 3])
def test_boundary(store, monkeypatch, K):  # noqa: F811
    run_boundary(store, monkeypatch, K)


def test_random_f32(store, monkeypatch):  # noqa: F811
    run_random_f32(store, monkeypatch)


def test_refusals_and_dispatch(store):  # noqa: F811
    run_refusals_and_dispatch(store)
