#!/usr/bin/env python3
"""A/B of the two algorithms of DDStore.get_radius_graph_batch, "brute" (every
pair of a graph, one lane group per graph) and "cells" (a spatial grid per
graph), on large graphs, in one process per shape on one GPU.

A shape is `--graphs` G graphs of `--nodes` N nodes each, random f32 positions
in a cube of `--density` nodes per unit volume, all G requested in one call
into capacity buffers of exactly the counted nodes and edges (int64 ids, no
host sync in the timed call), without and with edge vectors. Where both
algorithms run, their results must be equal before anything is timed. Sides
alternate inside every repetition, device events around a number of calls
chosen from the first call's time (about `--budget` seconds per repetition).

`--all` runs the shapes the "auto" threshold rests on, each in a fresh child
process under its own time limit, and stops at the first that fails:
"brute" and "cells" on one graph of 256, 1 k, 4 k and 16 k nodes and on 64
graphs of 2 k, "cells" alone on one graph of 64 k and 256 k ("brute" would run
for seconds per call there), and the benchmark shape (8,192 graphs of 16..239
nodes) under "auto" and "brute".

  python tools/radius_cells_bench.py --all > profiles/radius_cells_ab.txt
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

# (graphs, nodes, algorithms, seconds allowed)
SHAPES = [(1, 256, "brute,cells", 120), (1, 1024, "brute,cells", 120),
          (1, 4096, "brute,cells", 120), (1, 16384, "brute,cells", 240),
          (64, 2048, "brute,cells", 180), (1, 65536, "cells", 120),
          (1, 262144, "cells", 180), (8192, 0, "auto,brute", 180)]


def run_all(args):
    for graphs, nodes, algs, limit in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--graphs", str(graphs),
               "--nodes", str(nodes), "--algorithms", algs, "--r", str(args.r),
               "--density", str(args.density), "--reps", str(args.reps)]
        sys.stdout.flush()
        rc = subprocess.run(cmd, timeout=limit).returncode
        if rc != 0:
            sys.exit(f"radius_cells_bench: {graphs} x {nodes} ended with {rc}; stopping")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--all", action="store_true")
    p.add_argument("--graphs", type=int, default=1)
    p.add_argument("--nodes", type=int, default=4096,
                   help="nodes per graph; 0: the benchmark's 16..239")
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
        sys.exit("radius_cells_bench needs a GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    store = DDStore(device=dev)
    g = torch.Generator().manual_seed(4321)
    G = args.graphs
    nl = (torch.full((G,), args.nodes) if args.nodes
          else torch.randint(16, 240, (G,), generator=g))
    side = (nl.double() / args.density) ** (1.0 / 3.0)
    pos = torch.rand(int(nl.sum()), 3, generator=g) * \
        torch.repeat_interleave(side.float(), nl)[:, None]
    store.add_csr("pos", pos, nl)
    ncap = int(nl.sum())
    idx = torch.randperm(G, generator=g).to(dev)
    algs = args.algorithms.split(",")
    etot = int(store.get_radius_graph_batch("pos", idx, args.r,
                                            algorithm=algs[-1]).edge_ptr[-1])
    bufs = dict(pos_out=torch.empty(ncap, 3, device=dev),
                edge_out=torch.empty(2 * etot, dtype=torch.int64, device=dev),
                batch_out=torch.empty(ncap, dtype=torch.int64, device=dev))
    vec = torch.empty(3 * etot, device=dev)

    def call(alg, with_vec):
        extra = dict(vec_out=vec, edge_vec=True) if with_vec else {}
        return store.get_radius_graph_batch("pos", idx, args.r, algorithm=alg, **bufs,
                                            **extra)

    def timed(fn, n):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n * 1e3  # us per call

    print(f"# radius_cells_bench on {torch.cuda.get_device_name(0)}: {G} graphs of "
          f"{args.nodes or '16..239'} nodes, {ncap} nodes, f32, density {args.density}, "
          f"r={args.r}: {etot} edges ({etot / ncap:.2f} per node); int64 ids, exact "
          f"capacities, 1 rank; RADIUS_CELLS_MIN_NODES = {_C.RADIUS_CELLS_MIN_NODES}")
    want = None
    for alg in algs:  # equal results first; this is also the warm-up
        b = call(alg, True)
        got = (b.edge_ptr.clone(), b.edge_index.clone(), b.edge_vec.clone())
        assert want is None or all(torch.equal(x, y) for x, y in zip(want, got)), alg
        want = want or got
    print(f"# the sides ({', '.join(algs)}) give equal edge_ptr, edge_index and edge_vec"
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
