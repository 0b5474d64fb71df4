"""``get_radius_graph_pbc_batch(..., algorithm="cells")`` on the host backend
(which checks the argument and ignores it); tests/test_gpu_radius_pbc_cells.py
runs the same cases on the cell-list kernels. The result must equal the
brute-force one bit for bit, so the cases of tests/test_radius_pbc_cpu.py run
again with the argument bound, next to graphs aimed at the binning, with a
float64 model of their own (the shared one is cached over its own data).

Those graphs keep the dyadic grid of the shared data: integer cell entries
(times a power of two), coordinates and translations multiples of 1/8 below
2**20 and R = 1.5, so every dx of the rule is exact in float32, every d2 up to
4 R*R as well (the model asserts it), and a larger d2 stays above R*R after its
float32 roundings of 2**-22 in all."""
import functools
import itertools
from collections import namedtuple

import numpy as np
import pytest
import torch

from ddstore_amd import _C
from tests import test_radius_pbc_cpu as brute
from tests.test_radius_pbc_cpu import store  # noqa: F401  (the fixture)

R = brute.R
WIDE = np.array([[6, 0, 0], [2, 6, 0], [2, 2, 8]], dtype=np.float64)  # wider than 2R
PILE = _C.RADIUS_CELLS_SORT_MAX + 5
Model = namedtuple("Model", "ptr edge_ptr edge_index shift vec needed image_hits")


def bind_cells(store, monkeypatch):  # noqa: F811
    monkeypatch.setattr(store, "get_radius_graph_pbc_batch", functools.partial(
        store.get_radius_graph_pbc_batch, algorithm="cells"))


def run_case(store, monkeypatch, case):  # noqa: F811
    bind_cells(store, monkeypatch)
    brute.run_case(store, **brute.CASES[case])


def run_capacity_cuts(store, monkeypatch):  # noqa: F811
    bind_cells(store, monkeypatch)
    brute.run_capacity_cuts(store)


@functools.lru_cache(maxsize=None)
def binning_graphs(scale=1.0):
    """(positions, cell) of every graph; `scale` multiplies the lattice vectors
    of the two wide cells and not their atoms' places inside the first cell."""
    rng = np.random.default_rng(11)

    def atoms(n, cell):
        return rng.integers(0, 8, (n, 3)) / 8.0 @ np.asarray(cell, dtype=np.float64)

    wide = atoms(600, WIDE)
    moved = wide.copy()  # a third of the atoms whole lattice vectors away
    moved[::3] += rng.integers(-1, 2, (200, 3)) @ (WIDE * scale)
    if scale != 1.0:
        return ((wide, WIDE * scale), (moved, WIDE * scale))
    outlier = atoms(40, np.eye(3) * 4)
    outlier[7, 2] += 2.0 ** 18  # far away on the axis pbc switches off: a coarsened grid
    odd = atoms(12, np.eye(3) * 3)
    odd[2, 0], odd[5, 1] = np.nan, np.inf
    return ((wide, WIDE), (moved, WIDE),
            (atoms(96, np.diag([1, 8, 8])), np.diag([1.0, 8, 8])),  # two layers on x
            (outlier, np.eye(3) * 4),
            (np.tile([[0.5, 0.25, 0.75]], (PILE, 1)), np.eye(3)),   # every image overflows
            (odd, np.eye(3) * 3),
            (atoms(6, np.eye(3) * 2), np.array([[2.0, 0, 0], [0, 2, 0], [2, 2, 0]])))


@functools.lru_cache(maxsize=None)
def model(pbc, scale=1.0, max_shift=3):
    """Float64 brute force over the box the call searches (atoms outside their
    cell have neighbours beyond it, which the contract leaves out; that the box
    suffices inside the cell is the shared model's business). Shared: do not
    modify."""
    ptr, edge_ptr, pairs, shifts, vecs, needed, image_hits = [0], [0], [], [], [], [], []
    for p, a in binning_graphs(scale):
        det = abs(a[0] @ np.cross(a[1], a[2]))
        nd, box = [], []
        for k in range(3):
            q = R * np.linalg.norm(np.cross(a[(k + 1) % 3], a[(k + 2) % 3])) / det if det else None
            nk = (2 ** 31 - 1 if q is None else int(np.floor(q * (1 + 2.0 ** -10))) + 1) * pbc[k]
            nd.append(nk)
            box.append(min(nk, max_shift))
        S = np.array(list(itertools.product(*(range(-b, b + 1) for b in box))))
        t = S @ a
        assert max(np.abs(p[np.isfinite(p)]).max(), np.abs(t).max()) < 2 ** 20
        zero = int(np.nonzero((S == 0).all(1))[0][0])
        n, most = len(p), 0
        with np.errstate(invalid="ignore"):
            for dst in range(n):
                d = (p - p[dst])[None] + t[:, None]  # [image, src]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                near = d2[d2 <= 4 * R * R]
                assert np.array_equal(near, near.astype(np.float32)), "a d2 is not exact"
                m = d2 <= R * R
                m[zero, dst] = False
                im, src = np.nonzero(m)
                pairs.append(np.stack([src, np.full_like(src, dst)]) + ptr[-1])
                shifts.append(S[im])
                vecs.append(d[im, src])
                most = max(most, int(m.sum(1).max()))
        needed.append(nd)
        image_hits.append(most)
        ptr.append(ptr[-1] + n)
        edge_ptr.append(sum(x.shape[1] for x in pairs))
    return Model(np.array(ptr), np.array(edge_ptr), np.concatenate(pairs, 1),
                 np.concatenate(shifts).astype(np.int32),
                 np.concatenate(vecs).astype(np.float32), np.array(needed, dtype=np.int32),
                 image_hits)


def run_binning(store, pbc, scale=1.0):  # noqa: F811
    m = model(pbc, scale)
    graphs = binning_graphs(scale)
    lens = torch.tensor([len(p) for p, _ in graphs])
    pos = np.concatenate([p for p, _ in graphs]).astype(np.float32)
    store.add_csr("pos", torch.from_numpy(pos), lens)
    store.add("cell", torch.tensor(np.array([a.reshape(9) for _, a in graphs]),
                                   dtype=torch.float32))
    deg = np.bincount(m.edge_index[1, :m.edge_ptr[1]], minlength=600)
    assert deg.mean() > 8  # the wide cell
    if scale == 1.0:
        assert m.image_hits[4] > _C.RADIUS_CELLS_SORT_MAX  # the pile ranks every image
        assert m.edge_ptr[6] > m.edge_ptr[5] and m.edge_ptr[7] > m.edge_ptr[6]
    else:
        assert np.abs(m.shift[m.edge_ptr[1]:]).any() and 6 * scale / R > 2 ** 14
    g = store.get_radius_graph_pbc_batch("pos", "cell", list(range(len(graphs))), R, pbc=pbc,
                                         edge_vec=True, algorithm="cells")
    assert np.array_equal(g.ptr.cpu().numpy(), m.ptr)
    assert np.array_equal(g.shifts_needed.cpu().numpy(), m.needed)
    assert np.array_equal(g.edge_ptr.cpu().numpy(), m.edge_ptr)
    assert np.array_equal(g.edge_index.cpu().numpy(), m.edge_index)
    assert np.array_equal(g.edge_shift.cpu().numpy(), m.shift)
    assert np.array_equal(g.edge_vec.cpu().numpy().view(np.uint32), m.vec.view(np.uint32))


def run_refusals_and_dispatch(store):  # noqa: F811
    brute.fill_store(store)
    idx = [i for i in brute.REQUEST if i < len(brute.GRAPHS)]  # a bad index: no cell row
    call = functools.partial(store.get_radius_graph_pbc_batch, "pos", "cell", idx, R)
    with pytest.raises(ValueError, match="algorithm"):
        call(algorithm="grid")
    with pytest.raises(ValueError, match="nearest cap"):
        call(max_neighbors=4, algorithm="cells")
    nodes = 2 ** 32 // 17 ** 3 + 1  # nodes * (2 * 8 + 1)**3 >= 2**32
    store.add_csr("big", torch.zeros(nodes, 3), torch.tensor([nodes]))
    store.add("bigcell", torch.eye(3).reshape(1, 9))
    with pytest.raises(ValueError, match="nodes x images"):
        store.get_radius_graph_pbc_batch("big", "bigcell", [0], R, max_shift=8,
                                         algorithm="cells")
    a, b = (call(edge_vec=True, algorithm=alg) for alg in ("brute", "auto"))
    for x, y in zip(a[:-1], b[:-1]):  # node_extras is empty
        assert torch.equal(x, y)


@pytest.mark.parametrize("case", list(brute.CASES))
def test_case(store, monkeypatch, case):  # noqa: F811
    run_case(store, monkeypatch, case)


def test_capacity_cuts(store, monkeypatch):  # noqa: F811
    run_capacity_cuts(store, monkeypatch)


@pytest.mark.parametrize("pbc", [(True, True, True), (True, True, False)])
def test_binning(store, pbc):  # noqa: F811
    run_binning(store, pbc)


def test_large_translation(store):  # noqa: F811
    run_binning(store, (True, True, True), scale=2.0 ** 14)


def test_refusals_and_dispatch(store):  # noqa: F811
    run_refusals_and_dispatch(store)
