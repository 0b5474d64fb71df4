#!/usr/bin/env python3
"""HydraGNN-style training loop over a CSR graph store (BASELINE config 3).

DDStore's purpose in its home project is feeding graph neural network
training from atomistic datasets too large for one node (reference
README.md:200-212). This example shows that loop MI355X-native: each rank
owns a shard of variable-length graphs (node-feature matrices) in HBM, every
epoch draws a DistributedSampler-style global shuffle, minibatches of whole
graphs are packed by the CSR gather kernel (remote graphs over xGMI), pooled
per-graph, and pushed through a bf16 classifier with DDP. With ``--edges``
every graph also stores an edge index, batches come from the fused
graph-batch fetch (GraphPrefetchLoader) and one message-passing layer runs
before the pooling.

Launch:
  python examples/gnn_csr_train.py --epochs 2
  python examples/gnn_csr_train.py --epochs 2 --edges
  torchrun --standalone --local-addr 127.0.0.1 --nproc-per-node 8 \
      examples/gnn_csr_train.py --epochs 2
"""
import argparse
import os
import sys

import torch
import torch.distributed as dist
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from ddstore_amd import DDStore, GraphPrefetchLoader, PrefetchLoader  # noqa: E402

FEAT = 16


def segment_mean(values: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """Mean-pool packed per-node features to per-graph vectors.
    values: (total_nodes, FEAT); offsets: (B+1,) element offsets."""
    B = offsets.numel() - 1
    lens = (offsets[1:] - offsets[:-1]).clamp(min=1)
    gid = torch.repeat_interleave(
        torch.arange(B, device=values.device), offsets[1:] - offsets[:-1]
    )
    pooled = torch.zeros(B, values.shape[1], device=values.device, dtype=values.dtype)
    pooled.index_add_(0, gid, values)
    return pooled / lens.unsqueeze(1).to(values.dtype)


def masked_mean(dense: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """Mean-pool a padded batch to per-graph vectors. dense: (B, L, FEAT),
    zero past each graph's nodes; lengths: (B,) true node counts."""
    n = lengths.clamp(min=1, max=dense.shape[1]).unsqueeze(1)
    return (dense.float().sum(1) / n).to(dense.dtype)


def synthetic_edges(lens: torch.Tensor, chords: int, g: torch.Generator):
    """A ring plus ``chords`` random chords per graph, node ids local to the
    graph: ``(pairs (E, 2) int32, edges per graph)``."""
    n_edges = lens + chords
    gid = torch.repeat_interleave(torch.arange(lens.numel()), n_edges)
    start = torch.cumsum(n_edges, 0) - n_edges
    k = torch.arange(int(n_edges.sum())) - start[gid]  # edge number in its graph
    n = lens[gid]
    ring = k < n
    rnd = torch.randint(0, 1 << 30, (k.numel(), 2), generator=g)
    src = torch.where(ring, k, rnd[:, 0] % n)
    dst = torch.where(ring, (k + 1) % n, rnd[:, 1] % n)
    return torch.stack([src, dst], 1).to(torch.int32), n_edges


def message_pass(gb) -> torch.Tensor:
    """One neighbour-mean layer then mean pooling, on a GraphBatch whose
    buffers carry slack: ``edge_index`` slots past the batch's edges hold -1
    and ``batch`` slots past its nodes hold the dummy segment ``n``."""
    x, (src, dst) = gb.x, gb.edge_index.long()
    live = (src >= 0).unsqueeze(1).to(x.dtype)
    src, dst = src.clamp(min=0), dst.clamp(min=0)
    agg = torch.zeros_like(x).index_add_(0, dst, x[src] * live)
    deg = torch.zeros(x.shape[0], 1, device=x.device, dtype=x.dtype).index_add_(0, dst, live)
    h = 0.5 * (x + agg / deg.clamp(min=1))
    n = gb.ptr.numel() - 1
    # slack rows of x are uninitialised: the dummy segment swallows them
    pooled = torch.zeros(n + 1, x.shape[1], device=x.device, dtype=x.dtype)
    pooled.index_add_(0, gb.batch, torch.where(gb.batch.unsqueeze(1) < n, h,
                                               torch.zeros_like(h)))
    nodes = (gb.ptr[1:] - gb.ptr[:-1]).clamp(min=1).unsqueeze(1)
    return pooled[:n] / nodes.to(x.dtype)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--edges", action="store_true",
                   help="store an edge index per graph, fetch whole graph "
                        "batches with GraphPrefetchLoader and run one "
                        "message-passing layer before the pooling")
    p.add_argument("--epochs", type=int, default=2)
    p.add_argument("--padded", action="store_true",
                   help="fetch fixed-shape (B, L, FEAT) bf16 batches with the "
                        "fused padded gather (no host sync, no cast pass)")
    p.add_argument("--graphs-per-rank", type=int, default=20000)
    p.add_argument("--batch-size", type=int, default=512)
    p.add_argument("--device", default=None)
    p.add_argument("--backend", default=None,
                   help="dist backend override (default nccl on GPU; use gloo "
                        "to oversubscribe ranks on one GPU)")
    args = p.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    use_cuda = torch.cuda.is_available() if args.device is None else str(
        args.device).startswith("cuda")
    if world > 1:
        backend = args.backend or ("nccl" if use_cuda else "gloo")
        dist.init_process_group(backend, rank=rank, world_size=world)
    if use_cuda:
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
        device = torch.device("cuda", local_rank)
        torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")

    store = DDStore(device=device if use_cuda else "cpu")

    # synthetic graphs: class c graphs have node features centered at c
    nloc = args.graphs_per_rank
    g = torch.Generator().manual_seed(rank)
    lens = torch.randint(4, 60, (nloc,), generator=g)
    labels_local = torch.randint(0, 4, (nloc,), generator=g)
    total_nodes = int(lens.sum())
    centers = labels_local.repeat_interleave(lens).to(torch.float32)
    feats = centers.unsqueeze(1) + 0.1 * torch.randn(total_nodes, FEAT, generator=g)
    store.add_csr("graphs", feats, lens)
    store.add("labels", labels_local.unsqueeze(1))
    if args.edges:
        pairs, n_edges = synthetic_edges(lens, 3, g)
        store.add_csr("edge_index", pairs, n_edges)

    model = nn.Sequential(
        nn.Linear(FEAT, 128), nn.GELU(), nn.Linear(128, 4)
    ).to(device=device, dtype=torch.bfloat16)
    if world > 1:
        model = nn.parallel.DistributedDataParallel(
            model, device_ids=[local_rank] if use_cuda else None)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    lossf = nn.CrossEntropyLoss()

    ntotal = nloc * world
    for epoch in range(args.epochs):
        gs = torch.Generator().manual_seed(100 + epoch)
        mine = torch.randperm(ntotal, generator=gs)[rank::world]
        correct, seen, tot_loss, nb = 0, 0, 0.0, 0
        store.epoch_begin()
        # CSR prefetch: next batch's variable-length gather runs on a side
        # HIP stream while this batch trains
        if args.edges:
            loader = GraphPrefetchLoader(store, "graphs", "edge_index", mine,
                                         args.batch_size, label_name="labels",
                                         drop_last=True, edge_dtype=torch.int32)
        elif args.padded:
            # graphs have at most 59 nodes: nothing is truncated at 60
            loader = PrefetchLoader(store, "graphs", mine, args.batch_size,
                                    label_name="labels", drop_last=True,
                                    pad_to=60, out_dtype=torch.bfloat16)
        else:
            loader = PrefetchLoader(store, "graphs", mine, args.batch_size,
                                    label_name="labels", drop_last=True)
        for data, y in loader:
            y = y.view(-1).long()
            values, offsets = (None, None) if args.edges else data
            if args.edges:  # no host sync: shapes come from the buffers
                x = message_pass(data).to(torch.bfloat16)
            elif args.padded:  # (dense, lengths): bf16 straight from the gather
                x = masked_mean(values, offsets)
            else:
                x = segment_mean(values[: int(offsets[-1])], offsets).to(torch.bfloat16)
            opt.zero_grad(set_to_none=True)
            logits = model(x)
            loss = lossf(logits.float(), y)
            loss.backward()
            opt.step()
            correct += (logits.argmax(1) == y).sum().item()
            seen += y.numel()
            tot_loss += loss.item()
            nb += 1
        store.epoch_end()
        if rank == 0:
            print(f"epoch {epoch}: loss {tot_loss/max(nb,1):.4f} "
                  f"acc {correct/max(seen,1):.3f} ({nb} batches, mode={store.mode})")
    store.free()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
