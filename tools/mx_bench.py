"""A/B of the MX fetch at the flagship shape (262,144 rows x disp 128 -> bf16).

Per-fetch time, in one process and interleaved, of: (a) f32-stored, (b) plain
e4m3-stored, (c) MX e4m3, (d) MX e2m1, (e) MX e4m3 with a per-column affine,
and the ingest rate of the quantizer. Method of profiles/gather_tiled_ab.txt:
rotating outputs, a fresh index set per step, device events around windows
that end in a synchronise. Prints one line per case.
"""
import argparse
import statistics

import torch

from ddstore_amd import DDStore


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--disp", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    s = DDStore(device="cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((a.rows, a.disp), device=dev, generator=g)
    s.add("f32", x)
    s.add("fp8", x.to(torch.float8_e4m3fn))
    s.add_mx("mx8", x, "e4m3")
    s.add_mx("mx4", x, "e2m1")
    sc = torch.rand(a.disp, device=dev) + 0.5
    sh = torch.rand(a.disp, device=dev)
    outs = [torch.empty((a.batch, a.disp), dtype=torch.bfloat16, device=dev) for _ in range(4)]
    idxs = [torch.randint(0, a.rows, (a.batch,), device=dev, generator=g) for _ in range(8)]
    cases = {
        "a f32 -> bf16": ("f32", None, 4 * a.disp),
        "b e4m3 -> bf16": ("fp8", None, a.disp),
        "c mx e4m3 -> bf16": ("mx8", None, s.query("mx8")["row_bytes"]),
        "d mx e2m1 -> bf16": ("mx4", None, s.query("mx4")["row_bytes"]),
        "e mx e4m3 -> bf16, column affine": ("mx8", (sc, sh), s.query("mx8")["row_bytes"]),
    }

    def window(name, affine):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.steps):
            s.get_batch(name, idxs[k % 8], out=outs[k % 4], affine=affine)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.steps  # us per fetch

    times = {k: [] for k in cases}
    for k, (name, aff, _) in cases.items():
        window(name, aff)  # warm-up
    for _ in range(a.reps):  # interleaved
        for k, (name, aff, _) in cases.items():
            times[k].append(window(name, aff))
    for k, (_, _, rb) in cases.items():
        t = times[k]
        med = statistics.median(t)
        moved = a.batch * (rb + 2 * a.disp)
        print(f"{k:36s} median {med:7.2f} us  min {min(t):7.2f} max {max(t):7.2f}  "
              f"{rb + 2 * a.disp} B/row r+w  {moved / med / 1e6:6.2f} TB/s")
    # ingest: device-resident f32 source -> packed rows
    ing = []
    for _ in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            s._backend.update_mx("mx8", x, 0)
        e1.record()
        torch.cuda.synchronize()
        ing.append(e0.elapsed_time(e1) / 10)
    ing = ing[1:]
    print(f"quantize_rows_mx e4m3 ingest: median {x.numel() * 4 / statistics.median(ing) / 1e6:.1f} "
          f"GB/s of f32 source ({statistics.median(ing) * 1e3:.1f} us per {a.rows} rows, "
          f"includes one stream sync per call)")
    s.free()


if __name__ == "__main__":
    main()
