"""bench.py command-line contract: --steps sets the timed step count,
ms_per_step is consistent with the headline value, --dump-outputs is
repeatable and holds what the timed path returned, and the secondary
measurements appear only under --full. bench.main() is called in-process
with small shapes (no subprocess start-up per case)."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.timeout(120)


def _load_bench():
    spec = importlib.util.spec_from_file_location(
        "_bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(monkeypatch, capsys, argv):
    bench = _load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py"] + [str(a) for a in argv])
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return bench, json.loads(lines[0])


SMALL = ["--gpus", 1, "--rows", 4096, "--dim", 32, "--batch", 512,
         "--steps", 3, "--warmup", 2]


def _check_result_line(res, steps, batch):
    assert res["steps"] == steps
    assert res["unit"] == "samples/s" and res["higher_is_better"] is True
    assert res["dtype"] == "bf16"
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same timed interval
    assert res["value"] == pytest.approx(batch / (res["ms_per_step"] * 1e-3), rel=1e-9)


def test_plain_run_is_lean_and_full_adds_accounting_cpu(monkeypatch, capsys):
    _, plain = _run(monkeypatch, capsys, SMALL + ["--device", "cpu"])
    _check_result_line(plain, 3, 512)
    for k in ("remote_bytes_measured", "local_bytes_measured",
              "remote_read_GBps_aggregate", "store_stats_rank0"):
        assert k not in plain["extra"]
    _, full = _run(monkeypatch, capsys, SMALL + ["--device", "cpu", "--full"])
    _check_result_line(full, 3, 512)
    assert full["metric"] == plain["metric"]
    assert full["extra"]["remote_bytes_measured"] == 0
    assert full["extra"]["local_bytes_measured"] == 3 * 512 * 32 * 4
    assert "store_stats_rank0" in full["extra"]


@pytest.mark.parametrize("mode", ["fetch", "csr"])
def test_dump_outputs_repeatable_cpu(monkeypatch, capsys, tmp_path, mode):
    outs = []
    for tag in ("a", "b"):
        d = tmp_path / tag
        _run(monkeypatch, capsys,
             SMALL + ["--device", "cpu", "--mode", mode, "--dump-outputs", d])
        outs.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert outs[0].keys() == outs[1].keys() and outs[0]
    for name, a in outs[0].items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        assert a.size > 0
        assert np.array_equal(a, outs[1][name]), name
    if mode == "fetch":
        assert outs[0]["batch.npy"].shape == (512, 32)
    else:
        off = outs[0]["offsets.npy"]
        assert off.shape == (513,) and off[0] == 0
        assert outs[0]["values.npy"].shape[0] == int(off[-1])


def _expected_last_fetch(rows, dim, batch, steps, warmup, device):
    """Rebuild the seeded shard and index order and gather the rows of the
    last timed step with plain torch."""
    torch.manual_seed(1234)
    shard = torch.randn(rows, dim, dtype=torch.float32, device=device)
    g = torch.Generator().manual_seed(1234)
    need = max((steps + warmup) * batch, batch)
    order = []
    while sum(o.numel() for o in order) < need:
        order.append(torch.randperm(rows, generator=g))
    order = torch.cat(order)[:need]
    k = (warmup + steps - 1) % (need // batch)
    idx = order[k * batch:(k + 1) * batch].to(device)
    return shard[idx]


def test_dump_outputs_match_torch_gather_cpu(monkeypatch, capsys, tmp_path):
    _run(monkeypatch, capsys,
         SMALL + ["--device", "cpu", "--dump-outputs", tmp_path])
    want = _expected_last_fetch(4096, 32, 512, 3, 2, "cpu")
    got = np.load(tmp_path / "batch.npy")
    assert np.array_equal(got, want.numpy())


@pytest.mark.gpu
def test_dump_outputs_sampled_and_exact_gpu(monkeypatch, capsys, tmp_path):
    """65536 x 128 bf16 output is above the per-array cap, so the dump is the
    seeded row sample; it must equal the same rows of a plain torch gather
    (f32 -> bf16 is one rounding, identical in torch and in the fused cast)."""
    rows, dim, batch, steps, warmup = 131072, 128, 65536, 3, 2
    argv = ["--gpus", 1, "--rows", rows, "--dim", dim, "--batch", batch,
            "--steps", steps, "--warmup", warmup]
    bench, res = _run(monkeypatch, capsys, argv + ["--dump-outputs", tmp_path / "a"])
    _check_result_line(res, steps, batch)
    _run(monkeypatch, capsys, argv + ["--dump-outputs", tmp_path / "b"])
    a = np.load(tmp_path / "a" / "batch.npy")
    b = np.load(tmp_path / "b" / "batch.npy")
    keep = bench.DUMP_MAX_ELEMS // dim
    assert a.dtype == np.float32 and a.shape == (keep, dim)
    assert np.array_equal(a, b)
    want = _expected_last_fetch(rows, dim, batch, steps, warmup, "cuda")
    g = torch.Generator().manual_seed(bench.DUMP_SEED)
    sel = torch.randperm(batch, generator=g)[:keep].sort().values
    want = want[sel.cuda()].to(torch.bfloat16).to(torch.float32).cpu().numpy()
    assert np.array_equal(a, want)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 1000 * 1000


@pytest.mark.gpu
def test_dump_outputs_repeatable_csr_gpu(monkeypatch, capsys, tmp_path):
    argv = ["--gpus", 1, "--rows", 65536, "--dim", 64, "--batch", 8192,
            "--steps", 3, "--warmup", 2, "--mode", "csr"]
    outs = []
    for tag in ("a", "b"):
        _run(monkeypatch, capsys, argv + ["--dump-outputs", tmp_path / tag])
        outs.append({f: np.load(tmp_path / tag / f) for f in ("values.npy", "offsets.npy")})
    off = outs[0]["offsets.npy"]
    assert off.shape == (8193,) and np.all(np.diff(off) >= 16)
    assert outs[0]["values.npy"].shape[0] == int(off[-1])
    for name in outs[0]:
        assert np.array_equal(outs[0][name], outs[1][name]), name
