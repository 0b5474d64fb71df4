"""``DDStore.get_graph_batch`` and ``GraphPrefetchLoader`` without a GPU: the
host path (``device="cpu"``) against the NumPy model of tests/graph_ref.py,
through the same checker the GPU tests use, plus every refusal."""
import numpy as np
import pytest
import torch

from tests import graph_ref as ref
from tests.dist_utils import run_dist


@pytest.fixture
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    yield s
    s.free()


def shape_request():
    """Every shape graph once, shuffled, then duplicates: 40 graphs."""
    ns = len(ref.SHAPE_NODES)
    rng = np.random.default_rng(5)
    return np.concatenate([rng.permutation(ns), rng.integers(0, ns, 40 - ns)])


def test_model_on_a_hand_case():
    """The model itself, on a request small enough to write down."""
    x = np.arange(12, dtype=np.float32).reshape(6, 2)
    nl, el = [2, 0, 3, 1], [1, 0, 2, 1]
    pairs = np.array([[0, 1], [2, 0], [1, 2], [0, 0]], dtype=np.int32)
    m = ref.expected(x, nl, pairs, el, [2, 9, 0, 3, 1], 5, 3, True, -1)
    assert m.ptr.tolist() == [0, 3, 3, 5, 6, 6]
    assert m.edge_ptr.tolist() == [0, 2, 2, 3, 4, 4]
    assert m.batch.tolist() == [0, 0, 0, 2, 2]
    assert m.edge_index.tolist() == [[2, 1, 3], [0, 2, 4]]
    assert m.node_keep.tolist() == [True, False, True, False, False]
    assert m.edge_keep.tolist() == [True, False, True, False, False]
    assert m.node_counts == (1, 1, 5 * 8) and m.edge_counts == (1, 1, 3 * 2 * 4)
    # nodes fit, edges do not: graph 0 (request slot 2) keeps its nodes only
    m = ref.expected(x, nl, pairs, el, [2, 9, 0, 3, 1], 6, 2, False, 7)
    assert m.batch.tolist() == [0, 0, 0, 2, 2, 3]
    assert m.edge_index.tolist() == [[2, 0], [1, 2]]
    assert m.edge_keep.tolist() == [True, False, False, False, False]
    assert m.edge_counts == (1, 2, 2 * 2 * 4)
    m = ref.expected(x, nl, pairs, el, [], 2, 1, True, -1)
    assert m.ptr.tolist() == [0] and m.batch.tolist() == [0, 0]
    assert m.edge_index.tolist() == [[-1], [-1]]


@pytest.mark.parametrize("coo", [True, False], ids=["coo", "pairs"])
@pytest.mark.parametrize("stored,out", ref.DTYPE_PAIRS,
                         ids=["i64_i64", "i32_i64", "i32_i32"])
def test_shapes_exact_capacity(store, stored, out, coo):
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, stored)
    idx = shape_request()
    m = ref.check(store, names, graphs, stored, out, idx,
                  *ref.exact_caps(graphs, idx), coo=coo)
    assert m.edge_counts[1] == 0 and bool(m.edge_keep.any())


@pytest.mark.parametrize("coo", [True, False], ids=["coo", "pairs"])
def test_capacity_cuts(store, coo):
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, torch.int32)
    idx = shape_request()
    caps = ref.cut_caps(graphs, idx)
    assert len(set(caps.values())) == len(caps)
    for label, (ncap, ecap) in caps.items():
        m = ref.check(store, names, graphs, torch.int32, torch.int64, idx, ncap,
                      ecap, coo=coo, edge_fill=-7)
        if label == "exact":
            assert m.node_counts[1] == 0 and m.edge_counts[1] == 0
        elif label in ("nothing_kept", "zero"):
            assert not m.node_keep.any() and not m.edge_keep.any(), label
        elif label == "edges_only":
            assert m.node_counts[1] == 0 and not m.edge_keep.any()
            assert m.edge_counts[1] == int((graphs[3][idx] > 0).sum())
        elif label.startswith("edges"):
            assert m.node_counts[1] == 0 and m.edge_counts[1] > 0 and m.edge_keep.any()
            # nodes kept, edges dropped: the caller sees it in edge_ptr
            assert int(m.edge_ptr[-1]) > ecap
        else:
            assert m.node_counts[1] > 0 and m.node_keep.any(), label


def test_bad_indices(store):
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, torch.int64)
    idx = shape_request()
    ns = len(ref.SHAPE_NODES)
    idx[[0, 3, 17, 39]] = [-1, ns, 2 ** 40, -2 ** 63]
    m = ref.check(store, names, graphs, torch.int64, torch.int64, idx,
                  *ref.exact_caps(graphs, idx))
    assert m.node_counts[0] == 4 and m.edge_counts[0] == 4
    # (the checker's own get_csr reference call counts on the node variable too)
    assert store.query(names[1])["oob_skipped"] == 4
    assert (m.ptr[1:] - m.ptr[:-1])[[0, 3, 17, 39]].tolist() == [0] * 4
    assert (m.edge_ptr[1:] - m.edge_ptr[:-1])[[0, 3, 17, 39]].tolist() == [0] * 4


def test_empty_request(store):
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, torch.int32)
    g = store.get_graph_batch(*names, [])
    assert g.ptr.tolist() == [0] and g.edge_ptr.tolist() == [0]
    assert tuple(g.x.shape) == (0, 3) and tuple(g.edge_index.shape) == (2, 0)
    assert tuple(g.batch.shape) == (0,) and g.edge_index.dtype == torch.int64
    g = store.get_graph_batch(*names, [], coo=False, edge_dtype=torch.int32)
    assert tuple(g.edge_index.shape) == (0, 2) and g.edge_index.dtype == torch.int32
    # into buffers: everything is tail
    m = ref.check(store, names, graphs, torch.int32, torch.int32, [], 3, 2)
    assert m.batch.tolist() == [0, 0, 0]


def test_buffers_sized_by_the_call(store):
    graphs = ref.shape_graphs()
    x, nl, pairs, el = graphs
    names = ref.register(store, "g", graphs, torch.int32)
    idx = shape_request()
    idx[5] = 99  # a bad index takes no room
    ncap, ecap = ref.exact_caps(graphs, idx)
    g = store.get_graph_batch(*names, idx)
    m = ref.expected(x, nl, pairs.astype(np.int32), el, idx, ncap, ecap, True, -1)
    assert tuple(g.x.shape) == (ncap, 3) and tuple(g.edge_index.shape) == (2, ecap)
    assert np.array_equal(g.edge_index.numpy(), m.edge_index)
    assert np.array_equal(g.batch.numpy(), m.batch)
    assert np.array_equal(g.ptr.numpy(), m.ptr)
    assert np.array_equal(g.edge_ptr.numpy(), m.edge_ptr)
    assert g.node_extras == () and g.edge_extras == ()


def test_extras(store):
    graphs = ref.shape_graphs()
    x, nl, pairs, el = graphs
    names = ref.register(store, "g", graphs, torch.int64)
    pos = torch.arange(int(nl.sum()), dtype=torch.float32).unsqueeze(1)
    w = torch.arange(int(el.sum()), dtype=torch.float32).unsqueeze(1)
    store.add_csr("pos", pos, torch.from_numpy(nl))
    store.add_csr("w", w, torch.from_numpy(el))
    idx = shape_request()
    g = store.get_graph_batch(*names, idx, node_extras=("pos",), edge_extras=("w",))
    (pv, po), = g.node_extras
    (wv, wo), = g.edge_extras
    assert torch.equal(po, g.ptr) and torch.equal(wo, g.edge_ptr)
    want_p, _ = store.get_csr("pos", idx)
    want_w, _ = store.get_csr("w", idx)
    assert torch.equal(pv, want_p) and torch.equal(wv, want_w)
    # the lengths of the other group: refused, and the verdict is kept
    for _ in range(2):
        with pytest.raises(ValueError, match="sample lengths"):
            store.get_graph_batch(*names, idx, node_extras=("w",))
        with pytest.raises(ValueError, match="sample lengths"):
            store.get_graph_batch(*names, idx, edge_extras=("pos",))
    assert store._graph_extras_ok[("w", names[0])] is False
    assert store._graph_extras_ok[("pos", names[0])] is True


def test_refusals(store):
    graphs = ref.shape_graphs()
    x, nl, pairs, el = graphs
    names = ref.register(store, "g", graphs, torch.int64)
    ne = int(el.sum())
    store.add("fixed", torch.zeros(len(nl), 2, dtype=torch.int64))
    store.add_csr("ei3", torch.zeros(ne, 3, dtype=torch.int64), torch.from_numpy(el))
    store.add_csr("eif", torch.zeros(ne, 2, dtype=torch.float32), torch.from_numpy(el))
    store.add_csr("short", torch.from_numpy(pairs[: int(el[:-1].sum())]),
                  torch.from_numpy(el[:-1]))
    idx = shape_request()
    with pytest.raises(ValueError, match="not a CSR variable"):
        store.get_graph_batch(names[0], "fixed", idx)
    with pytest.raises(ValueError, match="not a CSR variable"):
        store.get_graph_batch("fixed", names[1], idx)
    with pytest.raises(ValueError, match="disp == 2"):
        store.get_graph_batch(names[0], "ei3", idx)
    with pytest.raises(TypeError, match="int32 or int64"):
        store.get_graph_batch(names[0], "eif", idx)
    with pytest.raises(ValueError, match="samples per rank"):
        store.get_graph_batch(names[0], "short", idx)
    with pytest.raises(TypeError, match="not narrowed"):
        store.get_graph_batch(*names, idx, edge_dtype=torch.int32)
    with pytest.raises(TypeError, match="edge_dtype"):
        store.get_graph_batch(*names, idx, edge_dtype=torch.float32)
    with pytest.raises(KeyError):
        store.get_graph_batch(names[0], "nope", idx)

    ncap, ecap = ref.exact_caps(graphs, idx)
    xo = torch.empty(ncap, 3)
    eo = torch.empty(2 * ecap, dtype=torch.int64)
    bo = torch.empty(ncap, dtype=torch.int64)
    for partial in ({"x_out": xo}, {"edge_out": eo, "batch_out": bo},
                    {"x_out": xo, "edge_out": eo}):
        with pytest.raises(ValueError, match="together"):
            store.get_graph_batch(*names, idx, **partial)
    wrong = [
        {"batch_out": torch.empty(ncap + 1, dtype=torch.int64)},
        {"batch_out": torch.empty(ncap - 1, dtype=torch.int64)},
        {"batch_out": torch.empty(ncap, dtype=torch.int32)},
        {"batch_out": torch.empty(2 * ncap, dtype=torch.int64)[::2]},
        {"edge_out": torch.empty(2 * ecap + 1, dtype=torch.int64)},
        {"edge_out": torch.empty(2 * ecap, dtype=torch.int32)},
        {"edge_out": torch.empty(4 * ecap, dtype=torch.int64)[::2]},
    ]
    for kw in wrong:
        args = {"x_out": xo, "edge_out": eo, "batch_out": bo, **kw}
        with pytest.raises(ValueError, match="must be a contiguous"):
            store.get_graph_batch(*names, idx, **args)
    store.get_graph_batch(*names, idx, x_out=xo, edge_out=eo, batch_out=bo)


def _w_two_ranks(rank, world):
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    x, nl, pairs, el = graphs = ref.shape_graphs()
    half = len(nl) // 2
    lo, hi = (0, half) if rank == 0 else (half, len(nl))
    n0, n1 = int(nl[:lo].sum()), int(nl[:hi].sum())
    e0, e1 = int(el[:lo].sum()), int(el[:hi].sum())
    s.add_csr("g_x", torch.from_numpy(x[n0:n1]), torch.from_numpy(nl[lo:hi]))
    s.add_csr("g_ei", torch.from_numpy(pairs[e0:e1]).to(torch.int32),
              torch.from_numpy(el[lo:hi]))
    idx = shape_request()
    assert ((idx < half).sum() > 10) and ((idx >= half).sum() > 10)
    ref.check(s, ("g_x", "g_ei"), graphs, torch.int32, torch.int64, idx,
              *ref.exact_caps(graphs, idx))
    ncap, ecap = ref.cut_caps(graphs, idx)["both_cut"]
    ref.check(s, ("g_x", "g_ei"), graphs, torch.int32, torch.int32, idx, ncap, ecap,
              coo=False)
    s.comm.barrier()
    s.free()


def test_two_ranks():
    """Half the graphs live on the other rank: same result as on one."""
    run_dist(_w_two_ranks, 2)


def check_loader(store, names, graphs, **kw):
    """GraphPrefetchLoader against one get_graph_batch call per batch into
    buffers of the loader's sizes; a ragged last batch and a label."""
    from ddstore_amd import GraphBatch, GraphPrefetchLoader

    x, nl, pairs, el = graphs
    labels = torch.arange(len(nl), dtype=torch.int64).unsqueeze(1) * 3
    store.add("y", labels)
    order = torch.from_numpy(np.random.default_rng(8).permutation(len(nl)))[:14]
    dev = store.device
    for with_label in (False, True):
        loader = GraphPrefetchLoader(store, names[0], names[1], order, 4,
                                     label_name="y" if with_label else None, **kw)
        assert len(loader) == 4
        seen = 0
        for item, b in zip(loader, order.split(4)):
            g, y = item if with_label else (item, None)
            assert isinstance(g, GraphBatch)
            ncap, ecap = b.numel() * int(nl.max()), b.numel() * int(el.max())
            edt = kw.get("edge_dtype") or torch.int64
            want = store.get_graph_batch(
                names[0], names[1], b,
                x_out=torch.zeros(ncap, x.shape[1], device=dev),
                edge_out=torch.empty(2 * ecap, dtype=edt, device=dev),
                batch_out=torch.empty(ncap, dtype=torch.int64, device=dev),
                coo=kw.get("coo", True), edge_dtype=kw.get("edge_dtype"),
                edge_fill=kw.get("edge_fill", -1))
            nn = int(want.ptr[-1])
            assert torch.equal(g.ptr, want.ptr) and torch.equal(g.edge_ptr, want.edge_ptr)
            assert torch.equal(g.x[:nn], want.x[:nn])
            assert torch.equal(g.edge_index, want.edge_index)
            assert torch.equal(g.batch, want.batch)
            if with_label:
                assert torch.equal(y.cpu(), labels[b])
            seen += 1
        assert seen == 4 and b.numel() == 2  # the last batch was ragged
    loader = GraphPrefetchLoader(store, names[0], names[1], order, 4, drop_last=True)
    assert len(loader) == 3 and len(list(loader)) == 3


def test_loader_host(store):
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, torch.int32)
    check_loader(store, names, graphs, coo=False, edge_dtype=torch.int32, edge_fill=-2)
    from ddstore_amd import GraphPrefetchLoader

    with pytest.raises(ValueError, match="not a CSR variable"):
        GraphPrefetchLoader(store, names[0], "y", [0, 1], 2)
