#!/usr/bin/env python3
"""A/B of the two algorithms of DDStore.get_radius_graph_pbc_batch, "brute"
(every (dst, image, src) triple of a graph, one lane group per graph) and
"cells" (a spatial grid per graph, every node probing its images), in one
process per shape on one GPU.

A shape is `--graphs` G cubic cells of `--nodes` N atoms each at `--density`
atoms per unit volume, random f32 positions inside the cell, periodic on all
three axes, all G requested in one call into capacity buffers of exactly the
counted nodes and edges (int64 ids, no host sync in the timed call), without
and with edge vectors. `--nodes 0` is the shape of tools/radius_pbc_bench.py:
structures of 2..64 atoms, orthorhombic and triclinic. Where both algorithms
run, their results must be equal before anything is timed. Sides alternate
inside every repetition, device events around a number of calls chosen from
the first call's time (about `--budget` seconds per repetition).

`--all` runs the shapes the dispatch rule rests on, each in a fresh child
process under its own time limit, and stops at the first that fails: "brute"
and "cells" on one cell of 256, 1 k and 4 k atoms and on 64 cells of 2 k,
"cells" alone on one cell of 16 k and 64 k ("brute" would run for many seconds
per call there), and 8,192 small structures under "auto" and "brute".

  python tools/radius_pbc_cells_bench.py --all > profiles/radius_pbc_cells_ab.txt
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

# (graphs, nodes, algorithms, seconds allowed)
SHAPES = [(1, 256, "brute,cells", 120), (1, 1024, "brute,cells", 120),
          (1, 4096, "brute,cells", 120), (1, 16384, "cells", 120),
          (64, 2048, "brute,cells", 180), (1, 65536, "cells", 120),
          (8192, 0, "auto,brute", 180)]


def run_all(args):
    for graphs, nodes, algs, limit in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--graphs", str(graphs),
               "--nodes", str(nodes), "--algorithms", algs, "--r", str(args.r),
               "--density", str(args.density), "--reps", str(args.reps)]
        sys.stdout.flush()
        rc = subprocess.run(cmd, timeout=limit).returncode
        if rc != 0:
            sys.exit(f"radius_pbc_cells_bench: {graphs} x {nodes} ended with {rc}; stopping")


def structures(args, g):
    import torch

    G = args.graphs
    nl = (torch.full((G,), args.nodes) if args.nodes
          else torch.randint(2, 65, (G,), generator=g))
    side = (nl.double() / args.density) ** (1.0 / 3.0)
    cell = torch.diag_embed(side[:, None].expand(G, 3))
    if not args.nodes:  # sides of ratio 0.8..1.25, odd graphs skewed; the volume stays
        ratio = 0.8 + 0.45 * torch.rand(G, 3, generator=g, dtype=torch.float64)
        ratio /= ratio.prod(1, keepdim=True) ** (1.0 / 3.0)
        skew = (torch.rand(G, 3, 3, generator=g, dtype=torch.float64) - 0.5) * 0.6
        skew = torch.tril(skew, -1) * side[:, None, None] * (torch.arange(G) % 2)[:, None, None]
        cell = torch.diag_embed(side[:, None] * ratio) + skew
    cell = cell.float()
    frac = torch.rand(int(nl.sum()), 3, generator=g)
    pos = torch.einsum("nk,nkc->nc", frac, torch.repeat_interleave(cell, nl, 0))
    return pos, cell, nl


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--all", action="store_true")
    p.add_argument("--graphs", type=int, default=1)
    p.add_argument("--nodes", type=int, default=4096,
                   help="atoms per cell; 0: structures of 2..64 atoms")
    p.add_argument("--algorithms", default="brute,cells")
    p.add_argument("--r", type=float, default=1.0)
    p.add_argument("--density", type=float, default=4.5)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--budget", type=float, default=0.25)
    args = p.parse_args()
    if args.all:
        return run_all(args)

    import torch

    sys.path.insert(0, ROOT)
    from ddstore_amd import DDStore, _C

    if not torch.cuda.is_available():
        sys.exit("radius_pbc_cells_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    store = DDStore(device=dev)
    g = torch.Generator().manual_seed(4321)
    pos, cell, nl = structures(args, g)
    G, ncap = args.graphs, int(nl.sum())
    store.add_csr("pos", pos, nl)
    store.add("cell", cell.reshape(G, 9))
    idx = torch.randperm(G, generator=g).to(dev)
    algs = args.algorithms.split(",")
    etot = int(store.get_radius_graph_pbc_batch("pos", "cell", idx, args.r,
                                                algorithm=algs[0]).edge_ptr[-1])
    bufs = dict(pos_out=torch.empty(ncap, 3, device=dev),
                edge_out=torch.empty(2 * etot, dtype=torch.int64, device=dev),
                batch_out=torch.empty(ncap, dtype=torch.int64, device=dev),
                shift_out=torch.empty(3 * etot, dtype=torch.int32, device=dev))
    vec = torch.empty(3 * etot, device=dev)

    def call(alg, with_vec):
        extra = dict(vec_out=vec, edge_vec=True) if with_vec else {}
        return store.get_radius_graph_pbc_batch("pos", "cell", idx, args.r, algorithm=alg,
                                                **bufs, **extra)

    def timed(fn, n):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n * 1e3  # us per call

    print(f"# radius_pbc_cells_bench on {torch.cuda.get_device_name(0)}: {G} cells of "
          f"{args.nodes or '2..64'} atoms, {ncap} atoms, f32, density {args.density}, "
          f"r={args.r}, max_shift=3, pbc on three axes: {etot} edges ({etot / ncap:.2f} per "
          f"atom); int64 ids, exact capacities, 1 rank; RADIUS_CELLS_MIN_NODES = "
          f"{_C.RADIUS_CELLS_MIN_NODES}")
    want = None
    for alg in algs:  # equal results first; this is also the warm-up
        b = call(alg, True)
        got = (b.edge_ptr.clone(), b.edge_index.clone(), b.edge_shift.clone(),
               b.edge_vec.clone(), b.shifts_needed.clone())
        assert want is None or all(torch.equal(x, y) for x, y in zip(want, got)), alg
        want = want or got
    print(f"# the sides ({', '.join(algs)}) give equal edge_ptr, edge_index, edge_shift, "
          "edge_vec and shifts_needed"
          if len(algs) > 1 else "# one side only: nothing to compare it with here")
    print("# call time in us: median of the repetitions, min..max, spread = max - min; "
          f"{args.reps} repetitions, sides alternating, device events")
    for with_vec in (False, True):
        iters = {}
        for alg in algs:
            call(alg, with_vec)
            first = timed(lambda: call(alg, with_vec), 1)
            iters[alg] = max(2, min(200, int(args.budget * 1e6 / max(first, 1.0))))
        times = {alg: [] for alg in algs}
        for _ in range(args.reps):
            for alg in algs:
                times[alg].append(timed(lambda: call(alg, with_vec), iters[alg]))
        for alg, t in times.items():
            print(f"{G:5d} x {args.nodes:6d} {'vec' if with_vec else 'ids':3s} {alg:6s} "
                  f"median {statistics.median(t):12.1f}   {min(t):12.1f} .. {max(t):12.1f}"
                  f"   spread {max(t) - min(t):10.1f}   ({iters[alg]} calls per repetition)")
    store.free()


if __name__ == "__main__":
    main()
