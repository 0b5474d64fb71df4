#!/usr/bin/env python3
"""Measurements for per-column normalization, in one process on one GPU.

  (a) fetch   flagship shape, --batch rows x --dim f32 -> bf16, per call:
        percol   get_batch(affine=(scale_vec, shift_vec))   the fused fetch
        scalar   get_batch(affine=(scale, shift))
        twopass  what users do without it: get_batch(dtype=f32), then the
                 torch broadcast x * scale + shift, then .to(bf16)
        plain    get_batch(dtype=f32) alone: the gather's own read rate
      Sides alternate inside every repetition; outputs and index sets rotate
      (4 of each) so that no side finds its data in the cache; each side is
      timed with device events around --iters back-to-back calls after a
      warm-up; the spread between repetitions is printed beside the median.
  (b) stats   column_stats on a --stats-gib GiB f32 shard of --dim columns and
      on a CSR variable of the same size, beside torch.var_mean + torch.aminmax
      over local_shard(name).double() with that path's peak extra memory.

--tree DIR imports ddstore_amd from DIR instead of this repository (another
build of the package); sides that build lacks are left out and named.

  python tools/colnorm_bench.py > profiles/colnorm_ab.txt
"""
import argparse
import os
import statistics
import sys

import torch


def timed(sides, reps, iters, warmup):
    """{name: [us per call, one per repetition]}; fn(i) gets a call counter."""
    for fn in sides.values():
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(iters):
                fn(i)
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / iters * 1e3)
    return times


def report(times, nbytes=None):
    for name, t in times.items():
        med = statistics.median(t)
        rate = f"   {nbytes[name] / med / 1e3:8.1f} GB/s" if nbytes and name in nbytes else ""
        print(f"{name:<28} median {med:10.1f} us   {min(t):10.1f} .. {max(t):10.1f}   "
              f"spread {max(t) - min(t):8.1f}{rate}")


def part_fetch(store, args, dev):
    rows, dim, B = args.rows, args.dim, args.batch
    g = torch.Generator().manual_seed(1234)
    store.add("x", torch.randn(rows, dim, device=dev))
    have_cols = hasattr(store, "column_stats")
    idxs = [torch.randint(0, rows, (B,), generator=g).to(dev) for _ in range(4)]
    outs = [torch.empty(B, dim, dtype=torch.bfloat16, device=dev) for _ in range(4)]
    f32s = [torch.empty(B, dim, dtype=torch.float32, device=dev) for _ in range(4)]
    scale = (torch.rand(dim, generator=g) + 0.5).to(dev)
    shift = torch.randn(dim, generator=g).to(dev)

    def percol(i):
        return store.get_batch("x", idxs[i % 4], out=outs[i % 4], affine=(scale, shift))

    def scalar(i):
        return store.get_batch("x", idxs[i % 4], out=outs[i % 4], affine=(0.5, -1.0))

    def plain(i):
        return store.get_batch("x", idxs[i % 4], out=f32s[i % 4])

    def twopass(i):
        x = store.get_batch("x", idxs[i % 4], out=f32s[i % 4])
        return (x * scale + shift).to(torch.bfloat16)

    sides = {"twopass f32, torch, bf16": twopass, "scalar affine": scalar,
             "plain f32 gather": plain}
    if have_cols:
        sides = {"percol affine": percol, **sides}
        # the fused form rounds once, the two-pass form three times: compare loosely
        a, b = percol(0).float(), twopass(0).float()
        torch.cuda.synchronize()
        assert torch.allclose(a, b, rtol=2 ** -6, atol=2 ** -6)
    times = timed(sides, args.reps, args.iters, args.warmup)
    rd = B * dim * 4
    print(f"## (a) fetch: {B} rows x {dim} f32 -> bf16 from a {rows}-row shard")
    print("# rate = bytes read + written by the fetch itself (twopass: the gather's "
          "alone) over the call time")
    report(times, {"percol affine": rd + rd // 2, "scalar affine": rd + rd // 2,
                   "plain f32 gather": 2 * rd, "twopass f32, torch, bf16": 2 * rd})
    med = {k: statistics.median(t) for k, t in times.items()}
    if have_cols:
        print(f"# twopass / percol = {med['twopass f32, torch, bf16'] / med['percol affine']:.2f}x"
              f"   percol / scalar = {med['percol affine'] / med['scalar affine']:.3f}")
    else:
        print("# this build has no per-column affine: percol left out")
    print(f"# plain f32 gather reads {rd / med['plain f32 gather'] / 1e3:.1f} GB/s "
          "(payload bytes read over the call time)")
    store._backend.free_var("x")
    return rd / med["plain f32 gather"] / 1e3


def part_stats(store, args, dev, gather_read_gbs):
    dim = args.dim
    rows = int(args.stats_gib * 2 ** 30) // (4 * dim)
    nbytes = rows * dim * 4
    g = torch.Generator(device=dev).manual_seed(99)
    x = torch.randn(rows, dim, device=dev, generator=g) + 100.0
    store.add("s", x)
    lens = torch.full((rows // 64,), 64, dtype=torch.int64)
    store.add_csr("c", x.view(-1, dim), lens)
    del x
    have = hasattr(store, "column_stats")

    def torch_stats(i, name="s"):
        d = store.local_shard(name).double()
        var, mean = torch.var_mean(d, 0, unbiased=False)
        mn, mx = torch.aminmax(d, dim=0)
        return mean, var, mn, mx

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ref = torch_stats(0)
    torch.cuda.synchronize()
    peak_extra = torch.cuda.max_memory_allocated() - base
    sides = {"torch .double() var_mean+aminmax": torch_stats}
    if have:
        sides = {"column_stats fixed-stride": lambda i: store.column_stats("s", local=True),
                 "column_stats CSR": lambda i: store.column_stats("c", local=True), **sides}
        cs = store.column_stats("s", local=True)
        assert torch.allclose(cs.mean, ref[0].cpu(), rtol=1e-12)
        assert torch.allclose(cs.std, ref[1].sqrt().cpu(), rtol=1e-9)
        assert torch.equal(cs.min, ref[2].cpu()) and torch.equal(cs.max, ref[3].cpu())
    del ref
    times = timed(sides, args.reps, max(1, args.iters // 4), 1)
    print(f"## (b) column_stats: {rows} rows x {dim} f32 = {nbytes / 2 ** 30:.2f} GiB, "
          "and the same values as a CSR variable (64-element samples)")
    print("# call time includes the read-back of 5 * dim doubles and its sync; "
          "rate = shard bytes over the call time")
    report(times, {k: nbytes for k in times})
    print(f"# torch path: peak extra device memory {peak_extra / 2 ** 30:.2f} GiB "
          f"({peak_extra / nbytes:.2f}x the shard)")
    if have:
        med = statistics.median(times["column_stats fixed-stride"])
        gbs = nbytes / med / 1e3
        print(f"# column_stats reads {gbs:.1f} GB/s = {gbs / gather_read_gbs:.2f} of the "
              f"{gather_read_gbs:.1f} GB/s the plain f32 gather reads in (a)")
    else:
        print("# this build has no column_stats: left out")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tree", default=os.path.join(os.path.dirname(__file__), ".."))
    p.add_argument("--part", choices=["fetch", "stats", "both"], default="both")
    p.add_argument("--rows", type=int, default=2 * 1024 * 1024)
    p.add_argument("--batch", type=int, default=262144)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--stats-gib", type=float, default=4.0)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("colnorm_bench needs a GPU: nothing is measured without one")
    sys.path.insert(0, os.path.abspath(args.tree))
    from ddstore_amd import DDStore

    dev = torch.device("cuda", 0)
    store = DDStore(device=dev)
    print(f"# colnorm_bench on {torch.cuda.get_device_name(0)}; package from "
          f"{'this tree' if args.tree == p.get_default('tree') else 'another build (--tree)'}")
    print(f"# {args.reps} repetitions x {args.iters} calls per side, sides alternating, "
          f"{args.warmup} warm-up calls; device events; median, min..max, spread = max - min")
    gather = part_fetch(store, args, dev) if args.part != "stats" else float("nan")
    if args.part != "fetch":
        part_stats(store, args, dev, gather)
    store.free()


if __name__ == "__main__":
    main()
