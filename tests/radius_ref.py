"""Brute-force model, inputs and checker for ``DDStore.get_radius_graph_batch``.

The model is float64 NumPy written from the documented contract: a bad index
is a graph of 0 nodes; ``ptr`` is the unclamped scan of the node counts; a
graph's nodes are kept iff ``ptr[i+1] <= Ncap``; a kept graph's edges are the
pairs ``(src, dst)`` with ``d2 <= r*r`` (``src != dst`` unless ``loop``),
ordered by ``dst`` then ``src``, each ``dst`` cut at its first ``K`` sources;
``edge_ptr`` scans those counts (0 for an unkept graph) and a graph's edges
are written iff ``edge_ptr[i+1] <= Ecap`` as well. With ``f32=True`` the same
model runs in NumPy float32 in the contract's operation order.
"""
from collections import namedtuple

import numpy as np
import torch

from ddstore_amd import _C

T = _C.RADIUS_TILE  # nodes per LDS slice of the kernels
R = 1.3
SENTINEL = 0x5A
GUARD = 4096
SHAPE_NODES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]

Expected = namedtuple("Expected", "ptr edge_ptr batch edge_index vec vec_rows "
                                  "degrees gap counts")


def expected(pos, lens, idx, r, Ncap, Ecap, K=None, loop=False, coo=True,
             edge_fill=-1, out_dtype=np.int64, f32=False):
    ft = np.float32 if f32 else np.float64
    p_all = np.asarray(pos).astype(np.float32).astype(ft)  # the store's cast rule
    r2 = ft(r) * ft(r) if f32 else float(r) ** 2
    start = np.concatenate([[0], np.cumsum(lens)])
    n = len(idx)
    ptr = np.zeros(n + 1, dtype=np.int64)
    edge_ptr = np.zeros(n + 1, dtype=np.int64)
    batch = np.full(Ncap, n, dtype=np.int64)
    flat = np.full((Ecap, 2), edge_fill, dtype=out_dtype)
    vec = np.zeros((Ecap, 3), dtype=np.float32)
    vec_rows = np.zeros(Ecap, dtype=bool)
    degrees, gap, oob, cap_skip, kept_nodes = [], np.inf, 0, 0, 0
    for i, g in enumerate(np.asarray(idx, dtype=np.int64).tolist()):
        bad = g < 0 or g >= len(lens)
        nn = 0 if bad else int(lens[g])
        oob += bad
        ptr[i + 1] = ptr[i] + nn
        edge_ptr[i + 1] = edge_ptr[i]
        if nn == 0:
            continue
        if ptr[i + 1] > Ncap:
            cap_skip += 1
            continue
        kept_nodes += nn
        batch[ptr[i]:ptr[i + 1]] = i
        p = p_all[start[g]:start[g] + nn]
        edges = []
        for dst in range(nn):
            d = p - p[dst]  # pos[src] - pos[dst], every src
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            gap = min(gap, float(np.abs(d2.astype(np.float64) - float(r2)).min()))
            srcs = [s for s in np.nonzero(d2 <= r2)[0].tolist() if loop or s != dst]
            srcs = srcs[:K] if K else srcs
            degrees.append(len(srcs))
            edges += [(s, dst, d[s]) for s in srcs]
        edge_ptr[i + 1] += len(edges)
        if edge_ptr[i + 1] <= Ecap:
            for e, (s, dst, d) in enumerate(edges, start=int(edge_ptr[i])):
                flat[e] = (s + ptr[i], dst + ptr[i])
                vec[e], vec_rows[e] = d, True
    nb = kept_nodes * 3 * np.asarray(pos).dtype.itemsize
    return Expected(ptr, edge_ptr, batch, np.ascontiguousarray(flat.T) if coo else flat,
                    vec, vec_rows, np.array(degrees), gap, (oob, cap_skip, nb))


def grid_graphs(node_lens, seed=7, density=1.1):
    """Positions on a 1/8 grid, each graph in a box sized for about 8
    neighbours within R = 1.3 (surface included); two coincident nodes in the
    first graph of more than 64."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(node_lens, dtype=np.int64)
    parts = []
    for n in lens.tolist():
        side = max(8, int(round(8 * (n / density) ** (1 / 3))))
        parts.append(rng.integers(0, side + 1, (n, 3)) / 8.0)
    big = int(np.nonzero(lens > 64)[0][0])
    parts[big][1] = parts[big][0]
    return np.concatenate(parts), lens


def request(extra_empty=0):
    """Every shape graph in a shuffled order, one of them twice, one bad index;
    `extra_empty` more requests of the empty graph pull the mean graph size
    under the kernels' small-graph threshold."""
    idx = np.random.default_rng(3).permutation(len(SHAPE_NODES)).tolist()
    idx = idx[:4] + [len(SHAPE_NODES) + 5] + idx[4:] + [idx[2]]
    return np.array(idx + [0] * extra_empty, dtype=np.int64)


def _guarded(nbytes, dtype, device):
    backing = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8,
                         device=device)
    return backing, backing[GUARD:GUARD + nbytes].view(dtype)


def _intact(backing, nbytes):
    b = backing.cpu()
    return bool((b[:GUARD] == SENTINEL).all() and (b[GUARD + nbytes:] == SENTINEL).all())


def check(store, name, pos, lens, idx, r, Ncap, Ecap, K=None, loop=False, coo=True,
          edge_dtype=torch.int64, edge_vec=True, edge_fill=-1, f32=False, m=None):
    """One call into sentinel-guarded capacity buffers, compared element by
    element with the model (`m`, or computed here); returns the model."""
    np_out = np.int32 if edge_dtype == torch.int32 else np.int64
    m = m or expected(pos, lens, idx, r, Ncap, Ecap, K, loop, coo, edge_fill, np_out, f32)
    dev, pdt = store.device, torch.from_numpy(pos[:0]).dtype
    sizes = (Ncap * 3 * pos.dtype.itemsize, 2 * Ecap * np_out().itemsize, Ncap * 8,
             Ecap * 12)
    (bp, po), (be, eo), (bb, bo), (bv, vo) = (
        _guarded(nb, dt, dev) for nb, dt in zip(sizes, (pdt, edge_dtype, torch.int64,
                                                        torch.float32)))
    keys = ("oob_skipped", "cap_skipped", "bytes_gathered")
    before = [store.query(name)[k] for k in keys]
    g = store.get_radius_graph_batch(
        name, torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev), r,
        max_neighbors=K, loop=loop, pos_out=po.view(Ncap, 3), edge_out=eo, batch_out=bo,
        vec_out=vo if edge_vec else None, coo=coo, edge_dtype=edge_dtype,
        edge_fill=edge_fill, edge_vec=edge_vec)
    delta = tuple(store.query(name)[k] - b for k, b in zip(keys, before))
    assert np.array_equal(g.ptr.cpu().numpy(), m.ptr)
    assert np.array_equal(g.edge_ptr.cpu().numpy(), m.edge_ptr)
    assert np.array_equal(g.batch.cpu().numpy(), m.batch)
    got_e = g.edge_index.cpu().numpy()
    assert got_e.dtype == np_out and got_e.shape == m.edge_index.shape
    bad = np.argwhere(got_e != m.edge_index)
    assert bad.shape[0] == 0, f"edge_index differs at {bad.shape[0]} slots, first {bad[0]}"
    assert g.edge_index.data_ptr() == eo.data_ptr() and g.batch.data_ptr() == bo.data_ptr()
    # positions: kept rows are the stored ones, the slack still the sentinel
    want_p = np.full((Ncap, 3), np.frombuffer(bytes([SENTINEL]) * 8, pos.dtype)[0], dtype=pos.dtype)
    start = np.concatenate([[0], np.cumsum(lens)])
    for i, gi in enumerate(np.asarray(idx).tolist()):
        if m.ptr[i + 1] > m.ptr[i] and m.ptr[i + 1] <= Ncap:
            want_p[m.ptr[i]:m.ptr[i + 1]] = pos[start[gi]:start[gi + 1]]
    assert np.array_equal(g.pos.cpu().numpy().view(np.uint8), want_p.view(np.uint8))
    if edge_vec:
        want_v = np.where(m.vec_rows[:, None], m.vec,
                          np.frombuffer(bytes([SENTINEL]) * 4, np.float32)[0])
        assert np.array_equal(g.edge_vec.cpu().numpy().view(np.uint32),
                              want_v.astype(np.float32).view(np.uint32))
    else:
        assert g.edge_vec is None
    for backing, nb in zip((bp, be, bb, bv), sizes):
        assert _intact(backing, nb)
    assert (bv.cpu() == SENTINEL).all() or edge_vec
    assert delta == m.counts, f"position counters grew by {delta}, model {m.counts}"
    return m
