"""``DDStore.get_radius_graph_pbc_batch`` on the host backend against a float64
brute force written from the contract; tests/test_gpu_radius_pbc.py runs the
same cases on the kernels.

Cells have integer entries and fractional coordinates are multiples of 1/8 in
[0, 1), so positions and r*r = 2.25 lie on a 1/8 grid: every operation of the
rule is exact in float32 (the model asserts that every d2 is representable) and
the float64 model decides the same edges with the same edge_vec bits. The model
searches one image layer more than the call does on every periodic axis and
discards nothing, so equality also shows that the searched box was sufficient;
only a search clamped by max_shift is modelled with the clamped box itself."""
import functools
import itertools
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import radius_ref as ref

R = 1.5
TRI = [[3, 0, 0], [1, 3, 0], [1, 1, 4]]
# nodes and cell of every stored graph: the side-1 cube needs two layers at R
# and its atom sees only its own images; the last two cells are wider than 2R
GRAPHS = [(1, np.eye(3)), (2, TRI), (3, np.diag([1, 2, 3])), (17, TRI), (63, TRI),
          (65, np.eye(3) * 8), (ref.T + 1, [[6, 0, 0], [2, 6, 0], [2, 2, 8]])]
REQUEST = [3, 6, 0, 99, 1, 4, 2, 5, 0]  # shuffled, one bad index, graph 0 twice
MID = 5                                 # the 63-node graph's place in it

Expected = namedtuple("Expected", "ptr edge_ptr batch edge_index shift vec rows needed "
                                  "layers counts")


@functools.lru_cache(maxsize=None)
def data():
    rng = np.random.default_rng(5)
    cells = np.array([np.asarray(c, dtype=np.float64) for _, c in GRAPHS])
    lens = np.array([n for n, _ in GRAPHS], dtype=np.int64)
    pos = np.concatenate([rng.integers(0, 8, (n, 3)) / 8.0 @ c for n, c in zip(lens, cells)])
    return pos, cells, lens


@functools.lru_cache(maxsize=None)
def expected(idx, Ncap=None, Ecap=None, pbc=(True,) * 3, max_shift=3, loop=False, coo=True,
             edge_fill=-1, out_dtype=np.int64, itemsize=4):
    """The model; without capacities, the exact ones. Shared: do not modify."""
    pos, cells, lens = data()
    start = np.concatenate([[0], np.cumsum(lens)])
    n = len(idx)
    ptr, edge_ptr = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    needed, layers = np.zeros((n, 3), dtype=np.int64), np.zeros((n, 3), dtype=np.int64)
    oob = cap_skip = kept_nodes = 0
    kept, edges = [], []
    for i, g in enumerate(idx):
        bad = g < 0 or g >= len(lens)
        nn = 0 if bad else int(lens[g])
        oob += bad
        ptr[i + 1], edge_ptr[i + 1] = ptr[i] + nn, edge_ptr[i]
        if bad:
            continue
        if Ncap is not None and ptr[i + 1] > Ncap:
            cap_skip += 1
            continue
        kept.append(i)
        kept_nodes += nn
        a, p = cells[g], pos[start[g]:start[g] + nn]
        box = []
        for k in range(3):
            q = R * np.linalg.norm(np.cross(a[(k + 1) % 3], a[(k + 2) % 3])) / abs(np.linalg.det(a))
            if pbc[k]:  # q = R / h_k, the cell's height along axis k
                layers[i, k] = np.ceil(q)
                needed[i, k] = np.floor(q * (1 + 2.0 ** -10)) + 1
            box.append(needed[i, k] + 1 if needed[i, k] <= max_shift else max_shift)
            box[k] *= bool(pbc[k])
        S = np.array(list(itertools.product(*(range(-b, b + 1) for b in box))))
        t = S @ a
        zero = int(np.nonzero((S == 0).all(1))[0][0])
        for dst in range(nn):
            d = (p - p[dst])[None] + t[:, None]  # [image, src]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert np.array_equal(d2, d2.astype(np.float32)), "a d2 is not exact in float32"
            m = d2 <= R * R
            m[zero, dst] &= loop
            edges += [(i, s, dst, S[im], d[im, s]) for im, s in zip(*np.nonzero(m))]
            edge_ptr[i + 1] += int(m.sum())
    Ncap = int(ptr[-1]) if Ncap is None else Ncap
    Ecap = int(edge_ptr[-1]) if Ecap is None else Ecap
    batch = np.full(Ncap, n, dtype=np.int64)
    for i in kept:
        batch[ptr[i]:ptr[i + 1]] = i
    flat = np.full((Ecap, 2), edge_fill, dtype=out_dtype)
    shift = np.zeros((Ecap, 3), dtype=np.int32)
    vec = np.zeros((Ecap, 3), dtype=np.float32)
    rows = np.zeros(Ecap, dtype=bool)
    ke = int((edge_ptr[1:] <= Ecap).sum())  # a prefix of the request keeps its edges
    for e, (i, s, dst, sh, d) in enumerate(edges[:int(edge_ptr[ke])]):
        flat[e], shift[e], vec[e], rows[e] = (s + ptr[i], dst + ptr[i]), sh, d, True
    return Expected(ptr, edge_ptr, batch, np.ascontiguousarray(flat.T) if coo else flat,
                    shift, vec, rows, needed, layers,
                    (oob, cap_skip, kept_nodes * 3 * itemsize))


@functools.lru_cache(maxsize=None)
def sizes(extra=0, **kw):
    """The request with `extra` more 1-atom graphs, and its exact capacities."""
    idx = tuple(REQUEST + [0] * extra)
    m = expected(idx, **kw)
    return idx, int(m.ptr[-1]), int(m.edge_ptr[-1])


def fill_store(store, pos_dtype=np.float32, cell_dtype=np.float32):
    pos, cells, lens = data()
    store.add_csr("pos", torch.from_numpy(pos.astype(pos_dtype)), torch.from_numpy(lens))
    store.add("cell", torch.from_numpy(cells.reshape(-1, 9).astype(cell_dtype)))


def check(store, idx, Ncap, Ecap, pos_dtype=np.float32, cell_dtype=np.float32, coo=True,
          edge_dtype=torch.int64, edge_vec=True, edge_fill=-1, **rule):
    """One call into sentinel-guarded capacity buffers, compared element by
    element with the model."""
    np_out = np.int32 if edge_dtype == torch.int32 else np.int64
    m = expected(idx, Ncap, Ecap, coo=coo, edge_fill=edge_fill, out_dtype=np_out,
                 itemsize=np.dtype(pos_dtype).itemsize, **rule)
    dev = store.device
    nbytes = (Ncap * 3 * np.dtype(pos_dtype).itemsize, 2 * Ecap * np_out().itemsize,
              Ncap * 8, Ecap * 12, Ecap * 12)
    dts = (torch.from_numpy(np.zeros(0, pos_dtype)).dtype, edge_dtype, torch.int64,
           torch.int32, torch.float32)
    (bp, po), (be, eo), (bb, bo), (bs, so), (bv, vo) = (
        ref._guarded(nb, dt, dev) for nb, dt in zip(nbytes, dts))
    keys = ("oob_skipped", "cap_skipped", "bytes_gathered")
    before = [store.query("pos")[k] for k in keys] + [store.query("cell")["oob_skipped"]]
    g = store.get_radius_graph_pbc_batch(
        "pos", "cell", torch.tensor(idx, dtype=torch.int64, device=dev), R,
        pos_out=po.view(Ncap, 3), edge_out=eo, batch_out=bo, shift_out=so,
        vec_out=vo if edge_vec else None, coo=coo, edge_dtype=edge_dtype,
        edge_fill=edge_fill, edge_vec=edge_vec, **rule)
    after = [store.query("pos")[k] for k in keys] + [store.query("cell")["oob_skipped"]]
    assert np.array_equal(g.ptr.cpu().numpy(), m.ptr)
    assert np.array_equal(g.edge_ptr.cpu().numpy(), m.edge_ptr)
    assert np.array_equal(g.batch.cpu().numpy(), m.batch)
    got_e = g.edge_index.cpu().numpy()
    assert got_e.dtype == np_out and np.array_equal(got_e, m.edge_index)
    sentinel = np.frombuffer(bytes([ref.SENTINEL]) * 4, np.int32)[0]
    assert np.array_equal(g.edge_shift.cpu().numpy(),
                          np.where(m.rows[:, None], m.shift, sentinel))
    if edge_vec:
        want_v = np.where(m.rows[:, None], m.vec.view(np.uint32), sentinel.view(np.uint32))
        assert np.array_equal(g.edge_vec.cpu().numpy().view(np.uint32), want_v)
    else:
        assert g.edge_vec is None and (bv.cpu() == ref.SENTINEL).all()
    for backing, nb in zip((bp, be, bb, bs, bv), nbytes):
        assert ref._intact(backing, nb)
    pos, cells, lens = data()
    got_p, got_c = g.pos.cpu().numpy(), g.cell.cpu().numpy()
    got_n = g.shifts_needed.cpu().numpy()
    assert got_c.dtype == cell_dtype and got_n.dtype == np.int32
    start = np.concatenate([[0], np.cumsum(lens)])
    for i, gi in enumerate(idx):
        if gi < len(lens):
            assert np.array_equal(got_c[i], cells[gi])
            if m.ptr[i + 1] <= Ncap:
                assert np.array_equal(got_p[m.ptr[i]:m.ptr[i + 1]], pos[start[gi]:start[gi + 1]])
    assert (got_p[m.ptr[int((m.ptr <= Ncap).sum()) - 1]:].view(np.uint8) == ref.SENTINEL).all()
    assert np.array_equal(got_n, m.needed)
    assert (m.layers <= got_n).all() and (got_n <= m.layers + 1).all()
    assert [a - b for a, b in zip(after, before)] == list(m.counts) + [m.counts[0] * (store.mode == "hip")]
    return g, m


# every switch once against the first row
CASES = {
    "base": {},
    "pbc_TTF": {"pbc": (True, True, False)},
    "pbc_FFF": {"pbc": (False, False, False)},
    "max_shift_1": {"max_shift": 1},
    "f64_pos": {"pos_dtype": np.float64},
    "f64_cell": {"cell_dtype": np.float64},
    "pairs": {"coo": False},
    "int32": {"edge_dtype": torch.int32},
    "loop": {"loop": True},
    "no_vec": {"edge_vec": False},
    "small_group": {"extra": 160},  # under 96 items per graph: 16 lanes per graph
}


def run_case(store, extra=0, **kw):
    rule = {k: kw[k] for k in ("pbc", "max_shift", "loop") if k in kw}
    idx, ncap, ecap = sizes(extra, **rule)
    fill_store(store, kw.get("pos_dtype", np.float32), kw.get("cell_dtype", np.float32))
    g, m = check(store, idx, ncap, ecap, **kw)
    if rule.get("max_shift") == 1:  # the cube and the 1 x 2 x 3 cell are truncated
        assert (m.needed > 1).any(1).tolist() == [gi in (0, 2) for gi in idx]
    elif "pbc" not in rule:
        one = m.edge_ptr[3] - m.edge_ptr[2]  # the cube's atom: 18 self-images within R
        assert one == 18 + bool(rule.get("loop")) and (m.needed <= 3).all()
    if rule.get("pbc") == (False,) * 3:
        h = store.get_radius_graph_batch("pos", list(idx), R, edge_vec=True)
        assert torch.equal(h.edge_ptr, g.edge_ptr) and torch.equal(h.edge_index, g.edge_index)
        assert torch.equal(h.edge_vec.view(torch.int32), g.edge_vec.view(torch.int32))
        assert not g.edge_shift.any()


def run_capacity_cuts(store):
    fill_store(store)
    idx, N, E = sizes()
    full = expected(idx, N, E)
    _, m = check(store, idx, N - 1, E, edge_fill=-7)  # the last graph's node does not fit
    assert m.edge_ptr[-1] == m.edge_ptr[-2] < E and not m.needed[-1].any()
    cut = int(full.edge_ptr[MID + 1]) - 1         # nor do the 63-node graph's edges
    _, m = check(store, idx, N, cut, coo=False)
    assert m.edge_ptr[-1] == E and m.rows.sum() == full.edge_ptr[MID] > 0


def run_sized_by_the_call(store):
    fill_store(store)
    store.add_csr("z", torch.arange(int(data()[2].sum())).unsqueeze(1),
                  torch.from_numpy(data()[2]))
    ok = tuple(i for i in REQUEST if i < len(GRAPHS))  # the host get_csr takes no bad index
    m = expected(ok)
    N, E = int(m.ptr[-1]), int(m.edge_ptr[-1])
    g = store.get_radius_graph_pbc_batch("pos", "cell", list(ok), R, edge_vec=True,
                                         node_extras=("z",))
    assert tuple(g.pos.shape) == (N, 3) and tuple(g.edge_vec.shape) == (E, 3)
    assert np.array_equal(g.edge_index.cpu().numpy(), m.edge_index)
    assert np.array_equal(g.edge_shift.cpu().numpy(), m.shift)
    assert np.array_equal(g.edge_vec.cpu().numpy(), m.vec)
    assert torch.equal(g.node_extras[0][1].cpu(), g.ptr.cpu())


def run_refusals(store):
    lens = torch.tensor([2, 3])
    store.add_csr("pos", torch.zeros(5, 3), lens)
    store.add("cell", torch.eye(3).reshape(1, 9).repeat(2, 1))
    store.add("wide", torch.zeros(2, 12))
    store.add("rows3", torch.zeros(3, 9))
    store.add_csr("csr", torch.zeros(5, 9), lens)
    store.init_mx("mx", 2, 9)
    call = store.get_radius_graph_pbc_batch
    for name in ("wide", "csr", "mx"):
        with pytest.raises(TypeError):
            call("pos", name, [0], 1.0)
    with pytest.raises(ValueError, match="one row per graph"):
        call("pos", "rows3", [0], 1.0)
    for ms in (0, 9):
        with pytest.raises(ValueError, match="max_shift"):
            call("pos", "cell", [0], 1.0, max_shift=ms)
    dev = store.device
    bufs = dict(pos_out=torch.zeros(5, 3, device=dev),
                edge_out=torch.zeros(8, dtype=torch.int64, device=dev),
                batch_out=torch.zeros(5, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="together"):
        call("pos", "cell", [0], 1.0, **bufs)  # no shift_out
    bufs["shift_out"] = torch.zeros(12, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="together"):
        call("pos", "cell", [0], 1.0, edge_vec=True, **bufs)
    with pytest.raises(ValueError, match="edge_vec=True"):
        call("pos", "cell", [0], 1.0, vec_out=torch.zeros(12, device=dev), **bufs)


@pytest.fixture
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    yield s
    s.free()


@pytest.mark.parametrize("case", list(CASES))
def test_case(store, case):
    run_case(store, **CASES[case])


def test_capacity_cuts(store):
    run_capacity_cuts(store)


def test_sized_by_the_call(store):
    run_sized_by_the_call(store)


def test_refusals(store):
    run_refusals(store)
