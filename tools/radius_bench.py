#!/usr/bin/env python3
"""A/B of the radius-graph fetch against storing the edges and against
building them in torch, in one process on one GPU.

  radius   get_radius_graph_batch into preallocated buffers: positions are
           fetched, the edges built from them (with and without edge vectors)
  stored   get_graph_batch on the same graphs with those same edges kept as an
           int64 CSR variable: what the store offers without this fetch
  torch    get_csr of the positions, then the same edges from torch ops on the
           device: positions padded per graph, pairwise d2 in the contract's
           operation order, mask, nonzero, relabel

Shape: B graphs of 16..239 nodes, f32 positions uniform in a box per graph
sized for a given density, one cutoff. All three sides must produce the same
edge_index before anything is timed. Sides alternate inside every repetition,
device events around `--iters` calls after a warm-up; the spread between
repetitions is printed next to the median. `--only radius` runs that side
alone, for a kernel trace (count / scan / fill split).

  python tools/radius_bench.py > profiles/radius_graph_ab.txt
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
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--r", type=float, default=1.0)
    p.add_argument("--density", type=float, default=4.5, help="nodes per unit volume")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--only", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("radius_bench needs a GPU: nothing is measured without one")

    dev = torch.device("cuda", 0)
    store = DDStore(device=dev)
    g = torch.Generator().manual_seed(4321)
    B = args.batch
    nl = torch.randint(16, 240, (B,), generator=g)
    side = (nl.double() / args.density) ** (1.0 / 3.0)
    pos = torch.rand(int(nl.sum()), 3, generator=g) * torch.repeat_interleave(
        side, nl).unsqueeze(1).float()
    store.add_csr("pos", pos, nl)
    ncap = int(nl.sum())

    # the edges, once, in storage order: local ids per graph
    ar = torch.arange(B, device=dev)
    built = store.get_radius_graph_batch("pos", ar, args.r, coo=False)
    el = (built.edge_ptr[1:] - built.edge_ptr[:-1])
    local = built.edge_index - torch.repeat_interleave(built.ptr[:-1], el).unsqueeze(1)
    store.add_csr("ei64", local, el.cpu())
    ecap = int(built.edge_ptr[-1])
    del built, local

    idx = torch.randperm(B, generator=g).to(dev)
    pbuf = torch.empty(ncap, 3, device=dev)
    bbuf = torch.empty(ncap, dtype=torch.int64, device=dev)
    ebuf = torch.empty(2 * ecap, dtype=torch.int64, device=dev)
    vbuf = torch.empty(3 * ecap, device=dev)
    nmax = int(nl.max())
    lane = torch.arange(nmax, device=dev)
    r2 = torch.tensor(args.r, dtype=torch.float32, device=dev) ** 2

    def radius(vec):
        return store.get_radius_graph_batch(
            "pos", idx, args.r, pos_out=pbuf, edge_out=ebuf, batch_out=bbuf,
            vec_out=vbuf if vec else None, edge_vec=vec)

    def stored():
        return store.get_graph_batch("pos", "ei64", idx, x_out=pbuf, edge_out=ebuf,
                                     batch_out=bbuf)

    def in_torch():
        pv, ptr = store.get_csr("pos", idx, out=pbuf)
        n = ptr[1:] - ptr[:-1]
        valid = lane.unsqueeze(0) < n.unsqueeze(1)                     # (B, nmax)
        rows = (ptr[:-1].unsqueeze(1) + lane.unsqueeze(0)).clamp_(max=ncap - 1)
        pp = pv[rows]                                                  # (B, nmax, 3)
        d2 = None
        for c in (0, 1, 2):  # d[b, dst, src] = pos[src] - pos[dst]
            d = pp[:, None, :, c] - pp[:, :, None, c]
            d2 = d * d if d2 is None else d2 + d * d
        m = (d2 <= r2) & valid.unsqueeze(1) & valid.unsqueeze(2)
        m &= ~torch.eye(nmax, dtype=torch.bool, device=dev)
        b, dst, src = m.nonzero(as_tuple=True)
        ei = torch.stack([src + ptr[b], dst + ptr[b]])
        batch = torch.repeat_interleave(ar, n)
        return pv, ei, ptr, None, batch

    sides = {
        "radius            ": lambda: radius(False),
        "radius + edge_vec ": lambda: radius(True),
        "stored i64 edges  ": stored,
        "torch construction": in_torch,
    }
    if args.only:
        sides = {k: v for k, v in sides.items() if k.strip() == args.only}

    want = radius(False).edge_index.clone()
    for name, fn in sides.items():
        got = fn()
        torch.cuda.synchronize()
        assert torch.equal(got[1], want), name
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

    pairs = int((nl.double() ** 2).sum())
    print(f"# radius_bench on {torch.cuda.get_device_name(0)}")
    print(f"# B={B} graphs of 16..239 nodes, {ncap} nodes, f32 positions, density "
          f"{args.density}, r={args.r}: {ecap} edges ({ecap / ncap:.2f} per node), "
          f"{pairs} pair tests per pass; int64 ids, exact capacities, 1 rank")
    print(f"# stored bytes: positions {ncap * 12}, int64 edge variable {ecap * 16} "
          f"({ecap * 16 / (ncap * 12):.1f}x)")
    print(f"# {args.reps} repetitions x {args.iters} calls per side, sides alternating; "
          f"{args.warmup} warm-up calls each; device events")
    print("# call time in us: median of the repetitions, min..max, spread = max - min")
    for name, t in times.items():
        print(f"{name}   median {statistics.median(t):10.1f}   {min(t):10.1f} .. "
              f"{max(t):10.1f}   spread {max(t) - min(t):8.1f}")
    store.free()


if __name__ == "__main__":
    main()
