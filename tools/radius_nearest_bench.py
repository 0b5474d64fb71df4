#!/usr/bin/env python3
"""A/B of the nearest-K cap of both radius-graph fetches against thinning the
uncapped fetch in torch, in one process on one GPU.

  nearest   get_radius_graph_batch(nearest=True) / get_radius_graph_pbc_batch
            with max_neighbors=K into preallocated buffers of Ncap * K edges
  thinned   what a user does without it: the uncapped fetch with edge_vec into
            preallocated buffers, then d2 from the vectors in the contract's
            operation order, a stable sort by d2 and one by dst, the first K of
            every dst, edge_ptr rebuilt
  uncapped  the uncapped fetch alone (and, open shape, the first-K cap): the
            existing calls, to compare with the numbers of the parent commit in
            profiles/radius_graph_ab.txt and profiles/radius_pbc_ab.txt

Shapes: `--shape open`, B graphs of 16..239 nodes in a box of `--density` nodes
per unit volume; `--shape pbc`, B periodic structures of 2..64 atoms as in
tools/radius_pbc_bench.py. Both sides must give the same edge_ptr and
edge_index before anything is timed. Sides alternate inside every repetition,
device events around `--iters` calls after a warm-up. `--only nearest` runs
that side alone, for a kernel trace.

  python tools/radius_nearest_bench.py --shape open > profiles/radius_nearest_ab.txt
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
    p.add_argument("--shape", choices=("open", "pbc"), default="open")
    p.add_argument("--batch", type=int, default=8192)
    p.add_argument("--r", type=float, default=1.0)
    p.add_argument("--density", type=float, default=4.5)
    p.add_argument("--k", type=int, nargs="+", default=[12, 32])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--only", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("radius_nearest_bench needs a GPU: nothing is measured without one")

    dev = torch.device("cuda", 0)
    store = DDStore(device=dev)
    g = torch.Generator().manual_seed(4321)
    B, periodic = args.batch, args.shape == "pbc"
    if periodic:
        nl = torch.randint(2, 65, (B,), generator=g)
        side = (nl.double() / args.density) ** (1.0 / 3.0)
        cell = torch.diag_embed(side[:, None].expand(B, 3)).float()
        frac = torch.rand(int(nl.sum()), 3, generator=g)
        pos = frac * torch.repeat_interleave(side.float(), nl)[:, None]
        store.add("cell", cell.reshape(B, 9))
    else:
        nl = torch.randint(16, 240, (B,), generator=g)
        side = (nl.double() / args.density) ** (1.0 / 3.0)
        pos = torch.rand(int(nl.sum()), 3, generator=g) * \
            torch.repeat_interleave(side.float(), nl)[:, None]
    store.add_csr("pos", pos, nl)
    ncap = int(nl.sum())
    idx = torch.randperm(B, generator=g).to(dev)

    def fetch(ecap, bufs, **kw):
        e, s, v = bufs
        common = dict(pos_out=pbuf, batch_out=bbuf, edge_out=e[:2 * ecap], **kw)
        if v is not None:
            common.update(vec_out=v[:3 * ecap], edge_vec=True)
        if periodic:
            return store.get_radius_graph_pbc_batch("pos", "cell", idx, args.r,
                                                    shift_out=s[:3 * ecap], **common)
        return store.get_radius_graph_batch("pos", idx, args.r, **common)

    pbuf = torch.empty(ncap, 3, device=dev)
    bbuf = torch.empty(ncap, dtype=torch.int64, device=dev)
    full = (store.get_radius_graph_pbc_batch("pos", "cell", idx, args.r) if periodic
            else store.get_radius_graph_batch("pos", idx, args.r))
    etot = int(full.edge_ptr[-1])
    del full
    big = (torch.empty(2 * etot, dtype=torch.int64, device=dev),
           torch.empty(3 * etot, dtype=torch.int32, device=dev),
           torch.empty(3 * etot, device=dev))
    kmax = max(args.k)
    small = (torch.empty(2 * ncap * kmax, dtype=torch.int64, device=dev),
             torch.empty(3 * ncap * kmax, dtype=torch.int32, device=dev), None)
    near_kw = (lambda k: {"max_neighbors": k}) if periodic else \
        (lambda k: {"max_neighbors": k, "nearest": True})

    def thinned(k):
        u = fetch(etot, big)
        v, dst = u.edge_vec, u.edge_index[1]
        d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        o1 = torch.sort(d2, stable=True).indices
        perm = o1[torch.sort(dst[o1], stable=True).indices]  # by dst, d2, position
        deg = torch.bincount(dst, minlength=ncap)
        rank = torch.arange(etot, device=dev) - (torch.cumsum(deg, 0) - deg)[dst[perm]]
        keep = torch.zeros(etot, dtype=torch.bool, device=dev)
        keep[perm] = rank < k
        csum = torch.cat([keep.new_zeros(1, dtype=torch.int64), torch.cumsum(keep, 0)])
        return u.edge_index[:, keep], csum[u.edge_ptr]

    sides = {}
    for k in args.k:
        sides[f"nearest K={k}"] = lambda k=k: fetch(ncap * k, small, **near_kw(k))
        sides[f"thinned K={k}"] = lambda k=k: thinned(k)
    sides["uncapped"] = lambda: fetch(etot, (big[0], big[1], None))
    sides["uncapped + edge_vec"] = lambda: fetch(etot, big)
    if not periodic:
        sides["first K=12"] = lambda: fetch(ncap * 12, small, max_neighbors=12)
    if args.only:
        sides = {k: v for k, v in sides.items() if k.split()[0] == args.only}

    kept = {}
    for k in args.k:  # the same edges on both sides before anything is timed
        a = fetch(ncap * k, small, **near_kw(k))
        kept[k] = int(a.edge_ptr[-1])
        ei, ep = thinned(k)
        assert torch.equal(ep, a.edge_ptr) and torch.equal(ei, a.edge_index[:, :kept[k]]), k
    del a, ei, ep

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

    print(f"# radius_nearest_bench --shape {args.shape} on {torch.cuda.get_device_name(0)}")
    print(f"# B={B}, {ncap} nodes, f32, density {args.density}, r={args.r}: {etot} uncapped "
          f"edges ({etot / ncap:.2f} per node); kept " +
          ", ".join(f"K={k}: {e}" for k, e in kept.items()) +
          "; int64 ids, nearest into Ncap * K slots, 1 rank")
    print(f"# {args.reps} repetitions x {args.iters} calls per side, sides alternating; "
          f"{args.warmup} warm-up calls each; device events")
    print("# call time in us: median of the repetitions, min..max, spread = max - min")
    for name, t in times.items():
        print(f"{name:20s} median {statistics.median(t):10.1f}   {min(t):10.1f} .. "
              f"{max(t):10.1f}   spread {max(t) - min(t):8.1f}")
    store.free()


if __name__ == "__main__":
    main()
