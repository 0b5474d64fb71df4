#!/usr/bin/env python3
"""A/B of DDStore.get_triplets against building the same index in torch, in one
process on one GPU.

  native   get_triplets(batch, trip_out=...) into a preallocated buffer of
           exactly the counted triplets: no host sync
  torch    what a user does without it, on the same batch: in-degree by
           bincount, every edge paired with the whole run into its source by
           repeat_interleave and a rank, then the way back masked out (with
           shifts: OCP's mask); the sizes in the middle are host-visible

Shapes: `--shape open`, B graphs of 16..239 nodes in a box of `--density` nodes
per unit volume; `--shape pbc`, B periodic structures of 2..64 atoms as in
tools/radius_pbc_bench.py. The batch is fetched once, at exact capacities, with
int64 ids, and is not part of either time. Both sides must give the same
triplets before anything is timed. Sides alternate inside every repetition,
device events around `--iters` calls after a warm-up.

  python tools/triplet_bench.py --shape open > profiles/triplet_ab.txt
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
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--warmup", type=int, default=2)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("triplet_bench needs a GPU: nothing is measured without one")

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
    batch = (store.get_radius_graph_pbc_batch("pos", "cell", idx, args.r) if periodic
             else store.get_radius_graph_batch("pos", idx, args.r))
    etot = int(batch.edge_ptr[-1])
    src, dst = batch.edge_index
    shift = batch.edge_shift if periodic else None

    def in_torch():
        deg = torch.bincount(dst, minlength=ncap)
        start = torch.cumsum(deg, 0) - deg
        cnt = deg[src]
        ji = torch.repeat_interleave(torch.arange(etot, device=dev), cnt)
        first = torch.cumsum(cnt, 0) - cnt
        kj = start[src][ji] + (torch.arange(ji.numel(), device=dev) - first[ji])
        mask = src[kj] != dst[ji]
        if periodic:
            mask |= ((shift[kj] + shift[ji]) != 0).any(1)
        return torch.stack([kj[mask], ji[mask]])

    ttot = int(store.get_triplets(batch).trip_ptr[-1])
    out = torch.empty(2 * ttot, dtype=torch.int64, device=dev)
    sides = {"native": lambda: store.get_triplets(batch, trip_out=out),
             "torch": in_torch}
    assert torch.equal(sides["native"]().triplets, in_torch())

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

    print(f"# triplet_bench --shape {args.shape} on {torch.cuda.get_device_name(0)}")
    print(f"# B={B}, {ncap} nodes, f32, density {args.density}, r={args.r}: {etot} edges "
          f"({etot / ncap:.2f} per node), {ttot} triplets ({ttot / max(etot, 1):.2f} per "
          "edge); int64 ids, exact capacities, 1 rank; both sides give the same triplets")
    print(f"# bytes written by the native side: {16 * ttot} of triplets, "
          f"{8 * (B + 1)} of trip_ptr")
    print(f"# {args.reps} repetitions x {args.iters} calls per side, sides alternating; "
          f"{args.warmup} warm-up calls each; device events")
    print("# call time in us: median of the repetitions, min..max, spread = max - min")
    for name, t in times.items():
        print(f"{name:8s} median {statistics.median(t):10.1f}   {min(t):10.1f} .. "
              f"{max(t):10.1f}   spread {max(t) - min(t):8.1f}")
    med = statistics.median(times["native"])
    print(f"# native: {16 * ttot / med / 1e3:.1f} GB/s of triplets written per call time "
          "(the whole call, five launches); the per-kernel split was not measured")
    store.free()


if __name__ == "__main__":
    main()
