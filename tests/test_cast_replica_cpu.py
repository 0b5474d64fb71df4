"""The host backend has no fused cast and therefore no fetch replica: it
accepts the calls, reports none, and returns what it returned before."""
import torch

from ddstore_amd import DDStore


def test_host_backend_accepts_and_reports_none():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(256, 16, generator=g)
    idx = torch.randint(0, 256, (300,), generator=g)
    s = DDStore(device="cpu")
    s.add("x", x)
    before = s.get_batch("x", idx, dtype=torch.bfloat16)
    assert s.prepare_fetch("x", torch.bfloat16) is False
    s.epoch_begin()
    after = s.get_batch("x", idx, dtype=torch.bfloat16)
    s.epoch_end()
    q = s.query("x")
    assert q["replica_dtype"] == "" and q["replica_bytes"] == 0
    assert q["replica_gathers"] == 0
    st = s.stats()["x"]
    assert st["replica_dtype"] == "" and st["replica_gathers"] == 0
    s.drop_fetch_replica("x")
    s.drop_fetch_replica()
    assert torch.equal(before.view(torch.int16), after.view(torch.int16))
    assert torch.equal(after, x[idx].to(torch.bfloat16))
    assert torch.equal(s.get_batch("x", idx), x[idx])
    s.free()
