#!/usr/bin/env python3
"""A/B of the periodic radius-graph fetch against building the image edges in
torch, in one process on one GPU.

  pbc      get_radius_graph_pbc_batch into preallocated buffers: positions and
           cells are fetched, the edges and their shifts built from them (with
           and without edge vectors)
  torch    what a user of the store does without it: get_csr of the positions,
           get_batch of the cells, then the same edges from torch ops on the
           device: positions padded per graph, the image box of the batch,
           d2 in the contract's operation order, mask, nonzero, relabel; in
           chunks of `--chunk` graphs, which bounds the (graph, dst, image,
           src) temporaries
  open     get_radius_graph_batch on the same positions: other edges (no
           images), here only as the cost per pair test of the non-periodic
           kernels, next to the periodic call's cost per (pair x image) test

Shape: B periodic structures of 2..64 atoms, f32, half orthorhombic and half
triclinic cells of `--density` atoms per unit volume, fractional coordinates
uniform in [0, 1), one cutoff: the small-cell regime, where an axis needs one
or two image layers. The torch side must produce the same edge_index and
shifts before anything is timed. Sides alternate inside every repetition,
device events around `--iters` calls after a warm-up; the spread between
repetitions is printed next to the median. `--only pbc` runs that side alone,
for a kernel trace (count / scan / fill split).

  python tools/radius_pbc_bench.py > profiles/radius_pbc_ab.txt
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
    p.add_argument("--density", type=float, default=4.5, help="atoms per unit volume")
    p.add_argument("--max-shift", type=int, default=3)
    p.add_argument("--chunk", type=int, default=256)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--only", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("radius_pbc_bench needs a GPU: nothing is measured without one")

    dev = torch.device("cuda", 0)
    store = DDStore(device=dev)
    g = torch.Generator().manual_seed(4321)
    B, ms = args.batch, args.max_shift
    nl = torch.randint(2, 65, (B,), generator=g)
    side = (nl.double() / args.density) ** (1.0 / 3.0)
    # sides of ratio 0.8..1.25 at the cell's volume; odd graphs get a skew of
    # up to 0.3 of a side below the diagonal (the volume stays)
    ratio = 0.8 + 0.45 * torch.rand(B, 3, generator=g, dtype=torch.float64)
    ratio /= ratio.prod(1, keepdim=True) ** (1.0 / 3.0)
    cell = torch.diag_embed(side[:, None] * ratio)
    skew = (torch.rand(B, 3, 3, generator=g, dtype=torch.float64) - 0.5) * 0.6
    skew = torch.tril(skew, -1) * side[:, None, None] * (torch.arange(B) % 2)[:, None, None]
    cell = (cell + skew).float()
    frac = torch.rand(int(nl.sum()), 3, generator=g)
    pos = torch.einsum("nk,nkc->nc", frac, torch.repeat_interleave(cell, nl, 0))
    store.add_csr("pos", pos, nl)
    store.add("cell", cell.reshape(B, 9))
    ncap = int(nl.sum())

    ar = torch.arange(B, device=dev)
    built = store.get_radius_graph_pbc_batch("pos", "cell", ar, args.r, max_shift=ms)
    ecap = int(built.edge_ptr[-1])
    need = built.shifts_needed.cpu()
    nimg = (2 * need.clamp(max=ms) + 1).prod(1)
    oecap = int(store.get_radius_graph_batch("pos", ar, args.r).edge_ptr[-1])
    del built

    idx = torch.randperm(B, generator=g).to(dev)
    pbuf = torch.empty(ncap, 3, device=dev)
    bbuf = torch.empty(ncap, dtype=torch.int64, device=dev)
    ebuf = torch.empty(2 * ecap, dtype=torch.int64, device=dev)
    sbuf = torch.empty(3 * ecap, dtype=torch.int32, device=dev)
    vbuf = torch.empty(3 * ecap, device=dev)
    nmax = int(nl.max())
    lane = torch.arange(nmax, device=dev)
    r2 = torch.tensor(args.r, dtype=torch.float32, device=dev) ** 2
    bmax = int(need.clamp(max=ms).max())
    S = torch.cartesian_prod(*(torch.arange(-bmax, bmax + 1, device=dev),) * 3)
    Sf = S.float()
    zero = int((S == 0).all(1).nonzero())
    eye = torch.eye(nmax, dtype=torch.bool, device=dev)

    def pbc(vec):
        return store.get_radius_graph_pbc_batch(
            "pos", "cell", idx, args.r, max_shift=ms, pos_out=pbuf, edge_out=ebuf,
            batch_out=bbuf, shift_out=sbuf, vec_out=vbuf if vec else None, edge_vec=vec)

    def open_graph():
        return store.get_radius_graph_batch("pos", idx, args.r, pos_out=pbuf,
                                            edge_out=ebuf[:2 * oecap], batch_out=bbuf)

    def in_torch():
        pv, ptr = store.get_csr("pos", idx, out=pbuf)
        a = store.get_batch("cell", idx).view(B, 3, 3)
        n = ptr[1:] - ptr[:-1]
        ad = a.double()
        cr = torch.stack([torch.linalg.cross(ad[:, (k + 1) % 3], ad[:, (k + 2) % 3])
                          for k in range(3)], 1)
        q = args.r * cr.norm(dim=2) / (ad[:, 0] * cr[:, 0]).sum(1).abs().unsqueeze(1)
        b = (torch.floor(q * (1 + 2.0 ** -10)) + 1).clamp(max=ms)
        ei, sh = [], []
        for g0 in range(0, B, args.chunk):
            sl = slice(g0, min(g0 + args.chunk, B))
            valid = lane.unsqueeze(0) < n[sl].unsqueeze(1)                  # (G, nmax)
            rows = (ptr[sl].unsqueeze(1) + lane.unsqueeze(0)).clamp_(max=ncap - 1)
            pp = pv[rows]                                                   # (G, nmax, 3)
            inbox = (S.abs().unsqueeze(0) <= b[sl].unsqueeze(1)).all(2)     # (G, nimg)
            ac = a[sl]
            d2 = None
            for c in (0, 1, 2):  # d[g, dst, image, src] = pos[src] - pos[dst] + t
                t = (Sf[:, 0] * ac[:, 0, c, None] + Sf[:, 1] * ac[:, 1, c, None]) \
                    + Sf[:, 2] * ac[:, 2, c, None]                          # (G, nimg)
                d0 = (pp[:, None, :, c] - pp[:, :, None, c]).unsqueeze(2)
                d = d0 + t[:, None, :, None]
                d[:, :, zero] = d0[:, :, 0]
                d2 = d * d if d2 is None else d2 + d * d
            m = (d2 <= r2) & valid[:, :, None, None] & valid[:, None, None, :]
            m &= inbox[:, None, :, None]
            m[:, :, zero] &= ~eye
            gg, dst, img, src = m.nonzero(as_tuple=True)
            ei.append(torch.stack([src, dst]) + ptr[sl][gg])
            sh.append(S[img])
        batch = torch.repeat_interleave(ar, n)
        return pv, torch.cat(ei, 1), torch.cat(sh).int(), ptr, batch

    sides = {
        "pbc               ": lambda: pbc(False),
        "pbc + edge_vec    ": lambda: pbc(True),
        "torch construction": in_torch,
        "open (no images)  ": open_graph,
    }
    if args.only:
        sides = {k: v for k, v in sides.items() if k.strip() == args.only}

    want = pbc(False)
    want_e, want_s = want.edge_index.clone(), want.edge_shift.clone()
    for name, fn in sides.items():
        got = fn()
        torch.cuda.synchronize()
        if not name.startswith("open"):
            assert torch.equal(got[1], want_e) and torch.equal(got[2], want_s), name
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
    tests = int((nl.double() ** 2 * nimg).sum())
    hist = torch.bincount(need.flatten().clamp(max=ms + 1)).tolist()
    print(f"# radius_pbc_bench on {torch.cuda.get_device_name(0)}")
    print(f"# B={B} structures of 2..64 atoms, {ncap} atoms, f32, density {args.density}, "
          f"r={args.r}, max_shift={ms}: {ecap} edges ({ecap / ncap:.2f} per atom); "
          f"int64 ids, exact capacities, 1 rank")
    print(f"# shifts_needed per axis, counts of 0, 1, ..., >{ms}: {hist}; "
          f"{int(nimg.sum())} images, {tests} (pair x image) tests per pass, "
          f"{pairs} pair tests per pass of the open call")
    print(f"# {args.reps} repetitions x {args.iters} calls per side, sides alternating; "
          f"{args.warmup} warm-up calls each; device events; torch in chunks of "
          f"{args.chunk} graphs")
    print("# call time in us: median of the repetitions, min..max, spread = max - min")
    for name, t in times.items():
        print(f"{name}   median {statistics.median(t):10.1f}   {min(t):10.1f} .. "
              f"{max(t):10.1f}   spread {max(t) - min(t):8.1f}")
    med = {k.strip(): statistics.median(t) for k, t in times.items()}
    if "pbc" in med and "open (no images)" in med:
        print(f"# per test: pbc {med['pbc'] * 1e3 / tests:.4f} ns per (pair x image), "
              f"open {med['open (no images)'] * 1e3 / pairs:.4f} ns per pair")
    store.free()


if __name__ == "__main__":
    main()
