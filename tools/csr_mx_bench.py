"""A/B of the MX CSR fetches at the CSR bench shape widened to disp = 128
(lengths 16..239), bf16 output: the fused MX fetches against (a) the same data
stored as f32 and fetched with get_csr_padded(dtype=bf16) and (b) MX kept as a
raw uint8 CSR variable, get_csr(out=), then decoded in torch. All cases in one
process, alternating round by round; the two MX results are first compared
with (b)'s, bit for bit. Prints the table (profiles/csr_mx_ab.txt).

    python tools/csr_mx_bench.py"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ddstore_amd import DDStore, mx  # noqa: E402

DEV = os.environ.get("CSR_MX_BENCH_DEV", "cuda:0")   # "cpu": a tiny rehearsal, no timing
TINY = DEV == "cpu"
NS, B, DISP, MAXLEN = (64, 16, 128, 240) if TINY else (32768, 8192, 128, 240)
WARM, REPS, ROUNDS = (1, 1, 1) if TINY else (10, 300, 3)
bf16 = torch.bfloat16

torch.manual_seed(0)
g = torch.Generator().manual_seed(1)
lens = torch.randint(16, 240, (NS,), generator=g)
T = int(lens.sum())
vals = torch.randn((T, DISP), device=DEV) * 3.0
store = DDStore(device=DEV)
store.add_csr("f32", vals, lens)
for e in ("e4m3", "e2m1"):
    store.add_csr_mx(e, vals, lens, e)
    store.add_csr("raw_" + e, store.local_shard(e).clone(), lens)
del vals
idx_sets = [torch.randint(0, NS, (B,), generator=g).to(DEV) for _ in range(4)]
goff = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
cap = max(int((goff[i.cpu() + 1] - goff[i.cpu()]).sum()) for i in idx_sets)
lut = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], device=DEV)


def torch_decode(p, elem):
    n, nblk = p.shape[0], DISP // 32
    if elem == "e4m3":
        npay = DISP
        val = p[:, :npay].view(torch.float8_e4m3fn).to(torch.float32)
    else:
        npay = DISP // 2
        pay = p[:, :npay]
        val = lut[torch.stack([pay & 15, pay >> 4], -1).reshape(n, DISP).long()]
    sc = torch.exp2(p[:, npay:npay + nblk].to(torch.float32) - 127)
    return (val.view(n, nblk, 32) * sc.unsqueeze(-1)).view(n, DISP).to(bf16)


dense = [torch.empty((B, MAXLEN, DISP), dtype=bf16, device=DEV) for _ in range(2)]
packed = [torch.empty((cap, DISP), dtype=bf16, device=DEV) for _ in range(2)]
packed_f32 = [torch.empty((cap, DISP), dtype=torch.float32, device=DEV) for _ in range(2)]
raw = {e: [torch.empty((cap, mx.row_bytes(DISP, e)), dtype=torch.uint8, device=DEV)
           for _ in range(2)] for e in ("e4m3", "e2m1")}


def v_padded(name):
    return lambda k: store.get_csr_padded(name, idx_sets[k % 4], MAXLEN, out=dense[k % 2])


def v_packed(name):
    return lambda k: store.get_csr(name, idx_sets[k % 4], out=packed[k % 2], dtype=bf16)


def v_raw(e):
    def run(k):
        p, _ = store.get_csr("raw_" + e, idx_sets[k % 4], out=raw[e][k % 2])
        return torch_decode(p, e)
    return run


variants = {
    "padded  mx e4m3 -> bf16 (k_gather_csr_mx)": v_padded("e4m3"),
    "padded  mx e2m1 -> bf16 (k_gather_csr_mx)": v_padded("e2m1"),
    "padded  f32 -> bf16 (a, k_gather_csr_padded)": v_padded("f32"),
    "packed  mx e4m3 -> bf16 (k_gather_csr_mx)": v_packed("e4m3"),
    "packed  mx e2m1 -> bf16 (k_gather_csr_mx)": v_packed("e2m1"),
    "packed  raw u8 e4m3 get_csr + torch decode (b)": v_raw("e4m3"),
    "packed  raw u8 e2m1 get_csr + torch decode (b)": v_raw("e2m1"),
    "packed  f32 get_csr(out=), no cast (for scale)":
        lambda k: store.get_csr("f32", idx_sets[k % 4], out=packed_f32[k % 2]),
}

# the results at this size: fused fetch == byte fetch + torch decode
for e in ("e4m3", "e2m1"):
    a, off = store.get_csr(e, idx_sets[0], out=packed[0], dtype=bf16)
    b = v_raw(e)(0)
    n = int(off[-1])
    assert torch.equal(a[:n].view(torch.int16), b[:n].view(torch.int16)), e
    print("outputs equal", e, n, "elements", flush=True)

times = {k: [] for k in variants}
for r in range(ROUNDS):          # alternate the variants, round by round
    for name, fn in variants.items():
        for k in range(WARM):
            fn(k)
        if TINY:
            times[name].append(0.0)
            continue
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(REPS):
            fn(k)
        t1.record()
        torch.cuda.synchronize()
        times[name].append(t0.elapsed_time(t1) / REPS * 1e3)

mean_elems = T / NS * B
lines = [f"NS={NS} samples, lengths 16..239 (mean {T / NS:.1f}), disp={DISP}, B={B} per fetch, "
         f"max_len={MAXLEN}, cap={cap}; ~{mean_elems:.0f} elements per fetch",
         f"warm-up {WARM}, {REPS} fetches per window (device events), {ROUNDS} alternating rounds;"
         " us per fetch: median (min .. max)"]
for name, ts in times.items():
    lines.append(f"{name:52s} {statistics.median(ts):8.1f} ({min(ts):.1f} .. {max(ts):.1f})")
print("\n".join(lines))
store.free()
