"""The fused graph-batch fetch on the GPU, ``get_graph_batch``: the offsets
kernel (k_csr_scan3 behind the unchanged k_csr_plan1/2), the relabelling
edge gather (k_gather_csr_relabel) and the fill (k_graph_fill) against the
NumPy model of tests/graph_ref.py.

Every buffer is cut out of a sentinel-filled backing tensor: around it the
sentinel must survive, inside it every ``batch`` and ``edge_index`` element
equals the model, tails included; ``x`` equals what ``get_csr(out=)`` writes
into a second buffer; offsets and counter deltas equal the model. Run with
``pytest -m gpu``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import graph_ref as ref
from tests.dist_utils import run_dist
from tests.test_gpu_csr_padded import store  # noqa: F401  (the fixture)
from tests.test_graph_batch_cpu import check_loader, shape_request

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("coo", [True, False], ids=["coo", "pairs"])
@pytest.mark.parametrize("stored,out", ref.DTYPE_PAIRS,
                         ids=["i64_i64", "i32_i64", "i32_i32"])
def test_shapes_all_kernel_instances(store, stored, out, coo):  # noqa: F811
    """The six instances of the relabelling gather over the shape table: no
    nodes, a self-loop on one node, nodes without edges, edge counts G-1, G,
    G+1 and 2G+1, every residue of edge_ptr mod 4 and of ptr mod 2, stored
    ids 0 and nodes-1."""
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, stored)
    idx = shape_request()
    m = ref.check(store, names, graphs, stored, out, idx,
                  *ref.exact_caps(graphs, idx), coo=coo)
    starts = m.edge_ptr[:-1][m.edge_keep]
    assert set((starts % 4).tolist()) == {0, 1, 2, 3}
    assert set((m.ptr[:-1][m.edge_keep] % 2).tolist()) == {0, 1}
    lens = set((m.edge_ptr[1:] - m.edge_ptr[:-1]).tolist())
    assert {0, 1, ref.G - 1, ref.G, ref.G + 1, 2 * ref.G + 1} <= lens


@pytest.mark.parametrize("nidx", [1, 255, 256, 257, 513, 66000])
def test_request_sizes(store, nidx):  # noqa: F811
    """Plan tile edges; 66000 requests are 258 tiles, the second chunk of
    tile aggregates in k_csr_plan2. The whole output is checked."""
    graphs = ref.tile_graphs()
    names = ref.register(store, "t", graphs, torch.int32)
    idx = np.random.default_rng(nidx).integers(0, 64, nidx)
    ref.check(store, names, graphs, torch.int32, torch.int64, idx,
              *ref.exact_caps(graphs, idx))


@pytest.mark.parametrize("coo", [True, False], ids=["coo", "pairs"])
@pytest.mark.parametrize("stored,out", [ref.DTYPE_PAIRS[0], ref.DTYPE_PAIRS[2]],
                         ids=["i64_i64", "i32_i32"])
def test_capacity_cuts(store, stored, out, coo):  # noqa: F811
    """Cuts on a graph boundary, inside a graph, with nothing kept, on Ecap
    alone and on both. The checker asserts after each that no written edge
    names a node at or behind the kept ones."""
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, stored)
    idx = shape_request()
    for label, (ncap, ecap) in ref.cut_caps(graphs, idx).items():
        m = ref.check(store, names, graphs, stored, out, idx, ncap, ecap, coo=coo,
                      edge_fill=-7)
        if label == "edges_only":
            assert m.node_counts[1] == 0 and not m.edge_keep.any()
        if label in ("edges_on_boundary", "edges_inside_graph"):
            assert m.node_counts[1] == 0 and m.edge_counts[1] > 0


def test_slack_capacity(store):  # noqa: F811
    """Buffers larger than the batch, as the loader passes them: the dummy
    segment and the edge tail are long, of odd lengths, and start at odd
    offsets."""
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, torch.int32)
    idx = shape_request()
    ncap, ecap = ref.exact_caps(graphs, idx)
    for out, coo in ((torch.int32, True), (torch.int64, False)):
        ref.check(store, names, graphs, torch.int32, out, idx, ncap + 4099,
                  ecap + 70001, coo=coo, edge_fill=-3)


def test_bad_indices(store):  # noqa: F811
    graphs = ref.tile_graphs()
    names = ref.register(store, "t", graphs, torch.int64)
    ns = 64
    idx = np.random.default_rng(3).integers(0, ns, 300)
    bad_at = [0, 3, 17, 100, 255, 256, 257, 299]
    idx[bad_at] = [-1, ns, 2 ** 40, -2 ** 63, ns, -1, 2 ** 40, ns + 1]
    m = ref.check(store, names, graphs, torch.int64, torch.int64, idx,
                  *ref.exact_caps(graphs, idx))
    assert m.node_counts[0] == len(bad_at) and m.edge_counts[0] == len(bad_at)
    assert store.query(names[1])["oob_skipped"] == len(bad_at)


def test_empty_request(store):  # noqa: F811
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, torch.int32)
    g = store.get_graph_batch(*names, [])
    assert g.ptr.tolist() == [0] and g.edge_ptr.tolist() == [0]
    assert tuple(g.x.shape) == (0, 3) and tuple(g.edge_index.shape) == (2, 0)
    ref.check(store, names, graphs, torch.int32, torch.int32, [], 5, 3)


@pytest.mark.parametrize("cut", [False, True], ids=["exact", "cut"])
def test_uninitialised_outputs(store, cut):  # noqa: F811
    """The same call into buffers pre-filled with different garbage gives
    identical results: no element is left unwritten."""
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, torch.int32)
    idx = shape_request()
    ncap, ecap = ref.cut_caps(graphs, idx)["both_cut"] if cut else \
        tuple(c + 37 for c in ref.exact_caps(graphs, idx))
    for coo in (True, False):
        runs = [ref.Fetch(store, names, graphs, torch.int32, torch.int32, idx, ncap,
                          ecap, coo=coo, garbage=garbage).run()
                for garbage in (0x00, 0xFF)]
        torch.cuda.synchronize()
        a, b = runs
        assert torch.equal(a.got.edge_index, b.got.edge_index)
        assert torch.equal(a.got.batch, b.got.batch)
        assert torch.equal(a.got.ptr, b.got.ptr) and torch.equal(a.got.edge_ptr, b.got.edge_ptr)
        b.verify()


def test_buffers_sized_by_the_call_and_extras(store):  # noqa: F811
    graphs = ref.shape_graphs()
    x, nl, pairs, el = graphs
    names = ref.register(store, "g", graphs, torch.int32)
    w = torch.arange(int(el.sum()), dtype=torch.float32).unsqueeze(1)
    store.add_csr("w", w, torch.from_numpy(el))
    idx = shape_request()
    ncap, ecap = ref.exact_caps(graphs, idx)
    g = store.get_graph_batch(*names, torch.from_numpy(idx).to(store.device),
                              edge_extras=("w",))
    m = ref.expected(x, nl, pairs.astype(np.int32), el, idx, ncap, ecap, True, -1)
    assert tuple(g.x.shape) == (ncap, 3) and tuple(g.edge_index.shape) == (2, ecap)
    assert np.array_equal(g.edge_index.cpu().numpy(), m.edge_index)
    assert np.array_equal(g.batch.cpu().numpy(), m.batch)
    (wv, wo), = g.edge_extras
    assert torch.equal(wo, g.edge_ptr)
    want = torch.cat([w[int(s):int(s) + int(n)] for s, n in
                      zip(np.concatenate([[0], np.cumsum(el)])[idx], el[idx])])
    assert torch.equal(wv.cpu(), want)
    with pytest.raises(ValueError, match="sample lengths"):
        store.get_graph_batch(*names, idx, node_extras=("w",))
    store.add_csr("ei64", torch.from_numpy(pairs), torch.from_numpy(el))
    with pytest.raises(TypeError, match="not narrowed"):
        store.get_graph_batch(names[0], "ei64", idx, edge_dtype=torch.int32)


def _w_two_ranks(rank, world):
    from ddstore_amd import DDStore

    s = DDStore(device=f"cuda:{rank % max(torch.cuda.device_count(), 1)}")
    assert s.mode == "hip"
    x, nl, pairs, el = graphs = ref.shape_graphs()
    half = len(nl) // 2
    lo, hi = (0, half) if rank == 0 else (half, len(nl))
    n0, n1 = int(nl[:lo].sum()), int(nl[:hi].sum())
    e0, e1 = int(el[:lo].sum()), int(el[:hi].sum())
    s.add_csr("g_x", torch.from_numpy(x[n0:n1]), torch.from_numpy(nl[lo:hi]))
    s.add_csr("g_ei", torch.from_numpy(pairs[e0:e1]).to(torch.int32),
              torch.from_numpy(el[lo:hi]))
    idx = shape_request()
    # the model is the single-rank result: the sharding must not show
    ref.check(s, ("g_x", "g_ei"), graphs, torch.int32, torch.int64, idx,
              *ref.exact_caps(graphs, idx))
    ncap, ecap = ref.cut_caps(graphs, idx)["both_cut"]
    ref.check(s, ("g_x", "g_ei"), graphs, torch.int32, torch.int32, idx, ncap, ecap,
              coo=False)
    s.comm.barrier()  # no rank frees its shard while another still reads it
    s.free()


def test_two_ranks_one_gpu():
    """Half of the graphs are remote; the result is the single-rank one."""
    idx = shape_request()
    half = len(ref.SHAPE_NODES) // 2
    assert 0.3 < float((idx >= half).mean()) < 0.7
    run_dist(_w_two_ranks, 2)


def test_loader_gpu(store):  # noqa: F811
    """GraphPrefetchLoader on the side streams: batches equal direct calls."""
    graphs = ref.shape_graphs()
    names = ref.register(store, "g", graphs, torch.int32)
    check_loader(store, names, graphs, edge_dtype=torch.int32)
    torch.cuda.synchronize()


def test_gnn_example_edges():
    """One epoch of the message-passing example in a child process."""
    r = subprocess.run(
        [sys.executable, "examples/gnn_csr_train.py", "--edges", "--epochs", "1",
         "--graphs-per-rank", "1500", "--batch-size", "256"],
        cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "acc" in r.stdout and "mode=hip" in r.stdout
