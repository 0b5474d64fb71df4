"""``DDStore.get_radius_graph_batch`` on the host backend against the model of
tests/radius_ref.py; tests/test_gpu_radius_graph.py runs the same cases on the
kernels. Grid positions (multiples of 1/8, r = 1.3) make every d2 exact in
float32 and keep it 0.0025 away from r*r, so the float64 model is exact and
every element must be equal."""
import functools

import numpy as np
import pytest
import torch

from tests import radius_ref as ref


@pytest.fixture
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    yield s
    s.free()


@functools.lru_cache(maxsize=None)
def grid():
    return ref.grid_graphs(ref.SHAPE_NODES)


@functools.lru_cache(maxsize=None)
def grid_model(K=None, loop=False, extra_empty=0):
    """The exact-capacity model of the shape request, computed once."""
    pos, lens = grid()
    idx = ref.request(extra_empty)
    big = 10 ** 7
    m = ref.expected(pos, lens, idx, ref.R, big, big, K, loop)
    return idx, int(m.ptr[-1]), int(m.edge_ptr[-1]), m


# each switch once against the first row: stored dtype, layout, id width,
# loop, K, edge vectors, and the small-graph lane group (many empty requests)
CASES = {
    "base": {},
    "f64": {"stored": np.float64},
    "pairs": {"coo": False},
    "int32": {"edge_dtype": torch.int32},
    "loop": {"loop": True},
    "K1": {"K": 1},
    "K4": {"K": 4},
    "no_vec": {"edge_vec": False},
    "small_mean": {"extra_empty": 40},
}


def run_grid_case(store, stored=np.float32, extra_empty=0, **kw):
    pos, lens = grid()
    idx, ncap, ecap, m = grid_model(kw.get("K"), kw.get("loop", False), extra_empty)
    assert m.gap > 1e-3, "the grid keeps d2 away from r*r"
    base = grid_model()[3].degrees  # without loops and without a K cap
    assert (base > 4).any() and (base == 0).any() and 6 < base.mean() < 11
    store.add_csr("pos", torch.from_numpy(pos.astype(stored)), torch.from_numpy(lens))
    ref.check(store, "pos", pos.astype(stored), lens, idx, ref.R, ncap, ecap, **kw)


def run_capacity_cuts(store):
    pos, lens = grid()
    pos = pos.astype(np.float32)
    idx, N, E, m = grid_model()
    store.add_csr("pos", torch.from_numpy(pos), torch.from_numpy(lens))
    mid = int(np.argmax(lens[np.clip(idx, 0, len(lens) - 1)] == ref.T))  # a full-slice graph
    p, e = m.ptr, m.edge_ptr
    cuts = {"nodes_on_boundary": (int(p[mid + 1]), E), "nodes_inside": (int(p[mid + 1]) - 1, E),
            "edges_inside": (N, int(e[mid + 1]) - 1), "nothing": (0, 0), "slack": (N + 37, E + 101)}
    for label, (ncap, ecap) in cuts.items():
        c = ref.check(store, "pos", pos, lens, idx, ref.R, ncap, ecap, edge_fill=-7,
                      coo=label != "edges_inside")
        if label.startswith("nodes"):
            assert (np.diff(c.edge_ptr)[mid + 1:] == 0).all() and c.edge_ptr[-1] > 0
        if label == "edges_inside":
            assert c.edge_ptr[-1] == E and not c.vec_rows[int(e[mid]):].any()


def run_random_f32(store):
    """Random float32 positions in small graphs against the float32 model."""
    rng = np.random.default_rng(11)
    lens = np.array([0, 1, 2, 15, 16, 17, 33, 40], dtype=np.int64)
    pos = (rng.random((int(lens.sum()), 3)) * 3.0).astype(np.float32)
    store.add_csr("pos", torch.from_numpy(pos), torch.from_numpy(lens))
    idx = rng.permutation(len(lens))
    m = ref.expected(pos, lens, idx, 0.9, 10 ** 6, 10 ** 6, f32=True)
    ref.check(store, "pos", pos, lens, idx, 0.9, int(m.ptr[-1]), int(m.edge_ptr[-1]),
              f32=True)


def run_sized_by_the_call(store):
    pos, lens = grid()
    idx, N, E, m = grid_model()
    store.add_csr("pos", torch.from_numpy(pos), torch.from_numpy(lens))
    store.add_csr("z", torch.arange(int(lens.sum())).unsqueeze(1), torch.from_numpy(lens))
    ok = idx[idx < len(lens)]  # the host get_csr (the extras) takes no bad index
    m = ref.expected(pos, lens, ok, ref.R, N, E)
    g = store.get_radius_graph_batch("pos", ok, ref.R, edge_vec=True, node_extras=("z",))
    assert tuple(g.pos.shape) == (N, 3) and tuple(g.edge_vec.shape) == (E, 3)
    assert np.array_equal(g.edge_index.cpu().numpy(), m.edge_index)
    assert np.array_equal(g.edge_vec.cpu().numpy(), m.vec)
    assert torch.equal(g.node_extras[0][1].cpu(), g.ptr.cpu())


@pytest.mark.parametrize("case", list(CASES))
def test_grid(store, case):
    run_grid_case(store, **CASES[case])


def test_capacity_cuts(store):
    run_capacity_cuts(store)


def test_random_f32(store):
    run_random_f32(store)


def test_sized_by_the_call(store):
    run_sized_by_the_call(store)


def test_refusals(store):
    lens = torch.tensor([2, 3])
    store.add_csr("pos", torch.zeros(5, 3), lens)
    store.add_csr("wide", torch.zeros(5, 4), lens)
    store.add_csr("ints", torch.zeros(5, 3, dtype=torch.int32), lens)
    store.add("rows", torch.zeros(5, 3))
    store.init_csr_mx("mx", lens, 3)
    for name in ("wide", "ints", "rows", "mx"):
        with pytest.raises(TypeError):
            store.get_radius_graph_batch(name, [0], 1.0)
    for r in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            store.get_radius_graph_batch("pos", [0], r)
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError):
            store.get_radius_graph_batch("pos", [0], 1.0, max_neighbors=k)
    with pytest.raises(ValueError, match="together"):
        store.get_radius_graph_batch("pos", [0], 1.0, pos_out=torch.zeros(5, 3))
    bufs = dict(pos_out=torch.zeros(5, 3), edge_out=torch.zeros(8, dtype=torch.int64),
                batch_out=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="together"):
        store.get_radius_graph_batch("pos", [0], 1.0, edge_vec=True, **bufs)
