"""``DDStore.get_triplets`` on the host backend; tests/test_gpu_triplets.py
runs the same cases on the kernels.

The reference is a brute force over the batch the store returned: per kept
graph, for every edge ``e`` the columns ``e'`` of the graph whose dst is the
src of ``e``, in column order, without the one that leads back to the dst of
``e`` through the negated shift. Every comparison is exact: ``trip_ptr``, the
written prefix of ``triplets`` and ``trip_fill`` everywhere else."""
import numpy as np
import pytest
import torch

from ddstore_amd import _C, GraphBatch

R = 1.0
DTYPES = [torch.int32, torch.int64]
MODES = ["sized", "capacity"]


def reference(ei, shift, ptr, edge_ptr, ncap, tcap, fill):
    """(trip_ptr, triplets of shape (2, tcap)); tcap None: exactly the total."""
    n, ecap = len(ptr) - 1, ei.shape[1]
    per_graph = []
    for g in range(n):
        rows = []
        if ptr[g + 1] <= ncap and edge_ptr[g + 1] <= ecap:
            cols = np.arange(edge_ptr[g], edge_ptr[g + 1])
            for e in cols:
                run = cols[ei[1, cols] == ei[0, e]]
                back = (ei[0, run] == ei[1, e]) & ~(shift[run] + shift[e]).any(1)
                rows += [(f, e) for f in run[~back]]
        per_graph.append(np.array(rows, dtype=np.int64).reshape(-1, 2))
    trip_ptr = np.concatenate([[0], np.cumsum([len(t) for t in per_graph])])
    tcap = int(trip_ptr[-1]) if tcap is None else tcap
    out = np.full((2, tcap), fill, dtype=np.int64)
    for g, t in enumerate(per_graph):  # a prefix: trip_ptr is monotone
        if len(t) and trip_ptr[g + 1] <= tcap:
            out[:, trip_ptr[g]:trip_ptr[g + 1]] = t.T
    return trip_ptr, out


def fetch(store, sizes, idx, dtype, cells=None, ncap=None, ecap=None, seed=0, side=None,
          **kw):
    """Graphs of `sizes` nodes at random places in a box (`side`; by default
    under 8 nodes all within R, else 2 nodes per unit volume), registered under
    fresh names and fetched: open, or periodic with one cubic cell per graph.
    ncap / ecap: the capacity call."""
    rng = np.random.default_rng(seed)
    box = [side or (0.5 if n < 8 else (n / 2.0) ** (1 / 3)) for n in sizes]
    pos = np.concatenate([rng.random((n, 3)) * b for n, b in zip(sizes, box)])
    name, cname = (f"{v}{len(store.variables())}" for v in ("pos", "cell"))
    store.add_csr(name, torch.from_numpy(pos.astype(np.float32)), torch.tensor(sizes))
    bufs = {}
    if ncap is not None:
        dev = store.device
        bufs = dict(pos_out=torch.empty(ncap, 3, device=dev),
                    batch_out=torch.empty(ncap, dtype=torch.int64, device=dev),
                    edge_out=torch.empty(2 * ecap, dtype=dtype, device=dev))
        if cells is not None:
            bufs["shift_out"] = torch.empty(3 * ecap, dtype=torch.int32, device=dev)
    if cells is None:
        return store.get_radius_graph_batch(name, idx, R, edge_dtype=dtype, **bufs, **kw)
    cell = torch.eye(3).reshape(1, 9) * torch.tensor(cells, dtype=torch.float32)[:, None]
    store.add(cname, cell)
    return store.get_radius_graph_pbc_batch(name, cname, idx, R, edge_dtype=dtype,
                                            **bufs, **kw)


def check(store, batch, mode, tcap=None, fill=-1, skew=0):
    """One get_triplets call against the reference; returns trip_ptr. skew:
    trip_out starts that many elements into its allocation."""
    ei = batch.edge_index.cpu().numpy().astype(np.int64)
    shift = (batch.edge_shift.cpu().numpy().astype(np.int64) if hasattr(batch, "edge_shift")
             else np.zeros((ei.shape[1], 3), dtype=np.int64))
    args = (ei, shift, batch.ptr.cpu().numpy(), batch.edge_ptr.cpu().numpy(),
            batch.batch.numel())
    if mode == "sized":
        want_ptr, want = reference(*args, None, fill)
        got = store.get_triplets(batch, trip_fill=fill)
    else:
        if tcap is None:  # three slots of slack: an odd tail to fill
            tcap = int(reference(*args, None, fill)[0][-1]) + 3
        want_ptr, want = reference(*args, tcap, fill)
        out = torch.full((2 * tcap + skew,), 77, dtype=batch.edge_index.dtype,
                         device=store.device)[skew:]
        got = store.get_triplets(batch, trip_out=out, trip_fill=fill)
        assert got.triplets.data_ptr() == out.data_ptr()
    assert got.triplets.dtype == batch.edge_index.dtype and got.trip_ptr.dtype == torch.int64
    assert np.array_equal(got.trip_ptr.cpu().numpy(), want_ptr)
    assert got.triplets.shape == want.shape
    assert np.array_equal(got.triplets.cpu().numpy(), want)
    return want_ptr


# sizes of the stored graphs, the request (99 is a bad index), fetch options
MIXED = dict(sizes=[0, 1, 2, 40], idx=[3, 0, 1, 99, 2, 3])
SLICE = _C.TRIPLET_SLICE
CASES = {
    "open": dict(MIXED),
    "open_loop": dict(MIXED, loop=True),
    "open_first3": dict(MIXED, max_neighbors=3),
    "open_nearest3": dict(MIXED, max_neighbors=3, nearest=True),
    # cells of side 1 with 1..4 atoms: self-images, pairs differing only in shift
    "pbc_shift1": dict(sizes=[1, 2, 3, 4], idx=[3, 0, 99, 2, 1], cells=[1.0] * 4,
                       max_shift=1),
    "pbc_shift2": dict(sizes=[1, 2, 3, 4], idx=[0, 1, 2, 3], cells=[1.0, 0.6, 1.0, 0.7],
                       max_shift=2),
    "pbc_nearest6": dict(sizes=[1, 2, 3, 4], idx=[3, 2, 1, 0], cells=[1.0] * 4,
                         max_shift=2, max_neighbors=6),
    # 70 nodes within range of each other: 4830 edges of 68 triplets each
    "tiles": dict(sizes=[70], idx=[0], side=0.5),
    # a tile that starts in a small graph and ends in a dense one, more dimer
    # edges than the slice between them: no edge of a dimer has a triplet
    "zero_span": dict(sizes=[5] + [2] * (SLICE // 2 + 20) + [12],
                      idx=list(range(SLICE // 2 + 22)), side=0.5),
}


def run_case(store, case, dtype, mode):
    batch = fetch(store, dtype=dtype, **CASES[case])
    trip_ptr = check(store, batch, mode)
    edges = int(batch.edge_ptr[-1])
    if case == "tiles":
        assert edges == 70 * 69 and trip_ptr[-1] == edges * 68
    if case == "zero_span":
        assert edges == 20 + 2 * (SLICE // 2 + 20) + 132 and trip_ptr[-1] == 60 + 1320
    if case.startswith("pbc"):  # some pair is joined through more than one image
        e = torch.cat([batch.edge_index.T.cpu().long(), batch.edge_shift.cpu().long()], 1)
        assert len(torch.unique(e[:, :2], dim=0)) < len(e)
        assert (e[:, 0] == e[:, 1]).any()


def run_capacity(store, dtype):
    batch = fetch(store, dtype=dtype, **MIXED)
    total = int(check(store, batch, "sized")[-1])
    for tcap in (total // 2, (total - 2) | 1, 8, 0):  # cut, odd, small, none
        assert check(store, batch, "capacity", tcap=tcap, fill=-7)[-1] == total > tcap
    # 16-B stores with the cut inside the buffer: a multiple of 4 behind the
    # first graph, whose end is not one, so a lane holds triplets and fill;
    # then the same buffer 8 bytes off a 16-B boundary: element stores
    trip_ptr = check(store, batch, "sized")
    tend = int(trip_ptr[1])
    tcap = (tend // 4 + 3) * 4
    assert tend % 4 and 0 < tend < tcap < total
    check(store, batch, "capacity", tcap=tcap, fill=-7)
    check(store, batch, "capacity", tcap=tcap, fill=-7, skew=8 // batch.edge_index.element_size())


def run_many_tiles(store, case, dtype):
    """A capacity of 3 Mi slots, 3072 tiles of the fill: more than the blocks
    of its grid (8 per CU), so a block owns consecutive tiles and finds the
    first edge of the second from the first. `tiles`: a step of a few edges;
    `zero_span`: a step over more edges than one round looks at."""
    check(store, fetch(store, dtype=dtype, **CASES[case]), "capacity", tcap=3 << 20)


def run_cut_batches(store, dtype):
    """Batches whose Ecap, then Ncap, cut graphs: those count no triplets."""
    full = fetch(store, dtype=dtype, **MIXED)
    N, E = int(full.ptr[-1]), int(full.edge_ptr[-1])
    for ncap, ecap in ((N, E - 1), (N - 1, E)):
        batch = fetch(store, dtype=dtype, ncap=ncap, ecap=ecap, **MIXED)
        for mode in MODES:
            trip_ptr = check(store, batch, mode)
            assert trip_ptr[-1] == trip_ptr[-2] > 0  # the last graph is cut


def run_refusals(store):
    batch = fetch(store, dtype=torch.int64, **MIXED)
    with pytest.raises(TypeError):
        store.get_triplets(GraphBatch(batch.pos, batch.edge_index, batch.ptr,
                                      batch.edge_ptr, batch.batch, (), ()))
    with pytest.raises(ValueError):
        store.get_triplets(fetch(store, dtype=torch.int64, coo=False, **MIXED))
    dev = store.device
    for bad in (torch.empty(8, dtype=torch.int32, device=dev),   # dtype
                torch.empty(7, dtype=torch.int64, device=dev),   # odd element count
                torch.empty(16, dtype=torch.int64, device=dev)[::2]):  # not contiguous
        with pytest.raises(ValueError):
            store.get_triplets(batch, trip_out=bad)
    with pytest.raises(ValueError):
        store.get_triplets(batch, trip_fill=2 ** 70)


@pytest.fixture
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    yield s
    s.free()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["int32", "int64"])
@pytest.mark.parametrize("case", list(CASES))
def test_cases(store, case, dtype, mode):
    run_case(store, case, dtype, mode)


@pytest.mark.parametrize("dtype", DTYPES, ids=["int32", "int64"])
@pytest.mark.parametrize("run", [run_capacity, run_cut_batches])
def test_capacity(store, run, dtype):
    run(store, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["int32", "int64"])
@pytest.mark.parametrize("case", ["tiles", "zero_span"])
def test_many_tiles(store, case, dtype):
    run_many_tiles(store, case, dtype)


def test_refusals(store):
    run_refusals(store)
