#!/usr/bin/env python3
"""A/B of the fused graph-batch fetch against the composition it replaces,
in one process on one GPU.

  fused    get_graph_batch into preallocated buffers (one native call)
  compose  what the same batch costs without it: two get_csr(out=) calls,
           repeat_interleave for the graph id of every edge and of every
           node, an add, and .t().contiguous(). Only int64 storage: nothing
           widens the ids on the way out of get_csr.

The fused path also runs on int32 storage (int32 and int64 output). Shape:
the CSR config of bench.py -- B graphs per batch, 16..2*dim-16 nodes per
graph -- with 4 edges per node. Sides alternate inside every repetition;
each is timed with device events around `--iters` back-to-back calls after a
warm-up, and the spread between repetitions is printed next to the median:
two medians closer than that spread count as equal. Outputs of the two sides
are compared before anything is timed.

  python tools/graph_bench.py > profiles/graph_batch_ab.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from ddstore_amd import DDStore  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=262144)
    p.add_argument("--dim", type=int, default=128, help="mean nodes per graph")
    p.add_argument("--graphs", type=int, default=262144, help="stored graphs")
    p.add_argument("--edges-per-node", type=int, default=4)
    p.add_argument("--feat", type=int, default=1, help="f32 features per node")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("graph_bench needs a GPU: nothing is measured without one")

    dev = torch.device("cuda", 0)
    store = DDStore(device=dev)
    g = torch.Generator().manual_seed(4321)
    nl = torch.randint(16, 2 * args.dim - 16, (args.graphs,), generator=g)
    el = nl * args.edges_per_node
    nl_d, el_d = nl.to(dev), el.to(dev)
    x = torch.randn(int(nl.sum()), args.feat, device=dev)
    gid = torch.repeat_interleave(torch.arange(args.graphs, device=dev), el_d)
    n_of_edge = nl_d[gid].unsqueeze(1)
    pairs = torch.randint(0, 1 << 30, (gid.numel(), 2), device=dev) % n_of_edge
    del gid, n_of_edge
    store.add_csr("x", x, nl)
    store.add_csr("ei64", pairs, el)
    store.add_csr("ei32", pairs.to(torch.int32), el)
    del pairs, x

    B = args.batch
    idx = torch.randperm(args.graphs, generator=g)[:B].to(dev)
    ncap, ecap = int(nl[idx.cpu()].sum()), int(el[idx.cpu()].sum())
    xbuf = torch.empty(ncap, args.feat, device=dev)
    bbuf = torch.empty(ncap, dtype=torch.int64, device=dev)
    e64 = torch.empty(2 * ecap, dtype=torch.int64, device=dev)
    e32 = torch.empty(2 * ecap, dtype=torch.int32, device=dev)
    raw = torch.empty(ecap, 2, dtype=torch.int64, device=dev)
    ar = torch.arange(B, device=dev)

    def fused(name, ebuf, dt):
        return store.get_graph_batch("x", name, idx, x_out=xbuf, edge_out=ebuf,
                                     batch_out=bbuf, edge_dtype=dt)

    def compose():
        xv, ptr = store.get_csr("x", idx, out=xbuf)
        ev, eptr = store.get_csr("ei64", idx, out=raw)
        egid = torch.repeat_interleave(ar, eptr[1:] - eptr[:-1])
        ei = (ev + ptr[egid].unsqueeze(1)).t().contiguous()
        batch = torch.repeat_interleave(ar, ptr[1:] - ptr[:-1])
        return xv, ei, ptr, eptr, batch

    sides = {
        "compose i64->i64": compose,
        "fused   i64->i64": lambda: fused("ei64", e64, torch.int64),
        "fused   i32->i64": lambda: fused("ei32", e64, torch.int64),
        "fused   i32->i32": lambda: fused("ei32", e32, torch.int32),
    }

    # same answer first
    want = compose()
    for name, fn in sides.items():
        got = fn()
        torch.cuda.synchronize()
        assert torch.equal(got[1].long(), want[1]), name
        assert torch.equal(got[4], want[4]) and torch.equal(got[2], want[2]), name
    del want, got

    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(args.reps):
        for name, fn in sides.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / args.iters * 1e3)  # us per call

    print(f"# graph_bench on {torch.cuda.get_device_name(0)}")
    print(f"# B={B} graphs per batch, {ncap} nodes ({args.feat} f32 each), {ecap} edges, "
          f"{args.graphs} stored graphs, 1 rank")
    print(f"# {args.reps} repetitions x {args.iters} calls per side, sides alternating; "
          f"{args.warmup} warm-up calls each; device events")
    print("# call time in us: median of the repetitions, min..max, spread = max - min")
    for name, t in times.items():
        med = statistics.median(t)
        print(f"{name}   median {med:10.1f}   {min(t):10.1f} .. {max(t):10.1f}   "
              f"spread {max(t) - min(t):8.1f}")
    mc = statistics.median(times["compose i64->i64"])
    mf = statistics.median(times["fused   i64->i64"])
    spread = max(max(t) - min(t) for k, t in times.items() if "i64->i64" in k)
    verdict = "equal within the spread" if abs(mc - mf) < spread else (
        "fused faster" if mf < mc else "fused SLOWER")
    print(f"# same storage (i64->i64): compose / fused = {mc / mf:.2f}x  ({verdict})")
    store.free()


if __name__ == "__main__":
    main()
