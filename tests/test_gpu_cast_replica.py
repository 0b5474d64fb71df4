"""Fetch replicas: a shard cast once to the dtype its fetches ask for, and
fetches served from it as same-dtype byte moves.

The yardstick throughout is the casting gather itself: a fetch served from a
replica must return the very bits the same fetch returns from a fresh store
with ``DDSTORE_CAST_REPLICA_MB=0`` (feature off). Shards have 4,096 rows;
widths 128 (tiled gather), 8 (one-shot gather, below the tiled boundary) and
136 (no power of two); row 0 and the last row carry the special values.
"""
import contextlib
import functools
import os

import pytest
import torch

from tests.dist_utils import run_dist

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

N = 4096
DEV = "cuda:0"
ENV = "DDSTORE_CAST_REPLICA_MB"
PAIRS = [
    (torch.float32, torch.bfloat16),
    (torch.float32, torch.float16),
    (torch.float64, torch.float32),
]
WIDTHS = [128, 8, 136]
NAME = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}

# +-0, f32 / bf16 / f16 subnormals, +-inf, NaN, exact bf16 ties (1 + 2^-8 is
# halfway between 1 and 1 + 2^-7; 1 + 3 * 2^-8 the next one up), the f16
# overflow tie 65520 and values beyond f16 range, values beyond f32 range, and
# 1 + 2^-8 + 2^-30: as f64 it lies above the bf16 tie, as f32 on it, so one
# rounding gives 1 + 2^-7 and the contract's two (f64 -> f32 -> bf16) give 1.
SPECIALS = [
    0.0, -0.0, 1e-40, -1e-40, 1e-39, 6e-8, -6e-8, 1e-45, 7e-46,
    float("inf"), float("-inf"), float("nan"),
    1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -30,
    65504.0, 65520.0, 65519.0, 1e5, -7e4, 3.3e38, 1e39, -1e39,
]


@contextlib.contextmanager
def env(value):
    old = os.environ.get(ENV)
    if value is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old


@functools.lru_cache(maxsize=None)
def shard(in_dt, width, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(N, width, generator=g, dtype=torch.float64) * 100
    sp = torch.tensor(SPECIALS, dtype=torch.float64)
    flat = x.view(-1)
    flat[: sp.numel()] = sp
    flat[-sp.numel():] = sp
    return x.to(in_dt)


@functools.lru_cache(maxsize=None)
def indices():
    """Seeded; duplicates, the first and last row, and -1, n, 2**40 mixed in."""
    g = torch.Generator().manual_seed(77)
    idx = torch.cat([
        torch.randint(0, N, (1500,), generator=g),
        torch.tensor([0, N - 1, 0, N - 1, 5, 5, 5, -1, N, 2 ** 40]),
    ])
    return idx[torch.randperm(idx.numel(), generator=g)]


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu()


def fetch(store, idx, out_dt, width, name="x", **kw):
    """Raw bits of one fetch into an output prefilled with 7: a skipped row
    keeps what was there."""
    out = torch.full((idx.numel(), width), 7, dtype=out_dt, device=DEV)
    store.get_batch(name, idx, out=out, **kw)
    torch.cuda.synchronize()
    return bits(out)


def cast_path(x, idx, out_dt, **kw):
    """(bits, oob_skipped) of the fetch from a fresh store with the feature
    off: the casting gather."""
    from ddstore_amd import DDStore

    with env(0):
        s = DDStore(device=DEV)
        s.add("x", x)
        b = fetch(s, idx, out_dt, x.shape[1], **kw)
        q = s.query("x")
        assert q["replica_dtype"] == "" and q["replica_gathers"] == 0
        s.free()
    return b, q["oob_skipped"]


@functools.lru_cache(maxsize=None)
def reference(in_dt, out_dt, width):
    return cast_path(shard(in_dt, width), indices(), out_dt)


def new_store(x, name="x"):
    from ddstore_amd import DDStore

    s = DDStore(device=DEV)
    s.add(name, x)
    return s


CASES = [(i, o, w) for i, o in PAIRS for w in WIDTHS] + [
    (torch.float64, torch.bfloat16, 128)]


@pytest.mark.parametrize("in_dt,out_dt,width", CASES)
def test_bit_equal_after_prepare_fetch(in_dt, out_dt, width):
    ref, ref_oob = reference(in_dt, out_dt, width)
    assert ref_oob == 3
    with env(None):
        s = new_store(shard(in_dt, width))
        assert s.prepare_fetch("x", out_dt) is True
        q = s.query("x")
        assert q["replica_dtype"] == NAME[out_dt]
        assert q["replica_bytes"] == N * width * torch.empty(0, dtype=out_dt).element_size()
        got = fetch(s, indices(), out_dt, width)
        empty = fetch(s, torch.empty(0, dtype=torch.int64), out_dt, width)
        q = s.query("x")
        s.free()
    assert torch.equal(got, ref)
    assert empty.numel() == 0
    assert q["oob_skipped"] == ref_oob
    assert q["replica_gathers"] == 2 and q["n_gather"] == 2
    assert q["rows_gathered"] == indices().numel()
    # stored-dtype bytes, as without a replica
    assert q["bytes_gathered"] == indices().numel() * width * shard(in_dt, width).element_size()


def test_trigger_is_one_shard_of_rows():
    x = shard(torch.float32, 128)
    g = torch.Generator().manual_seed(5)
    quarters = torch.randperm(N, generator=g).view(4, 1024)
    ref, _ = cast_path(x, quarters[3], torch.bfloat16)
    with env(None):
        s = new_store(x)
        for k in range(3):
            fetch(s, quarters[k], torch.bfloat16, 128)
            assert s.query("x")["replica_dtype"] == ""
        got = fetch(s, quarters[3], torch.bfloat16, 128)  # builds, and is served
        q = s.query("x")
        s.free()
    assert q["replica_dtype"] == "bfloat16" and q["replica_gathers"] == 1
    assert torch.equal(got, ref)


def test_f32_and_affine_fetches_bypass_the_replica():
    x = shard(torch.float32, 128)
    idx = indices()[:512]
    ref_aff, _ = cast_path(x, idx, torch.bfloat16, affine=(0.5, 3.0))
    ref_f32, _ = cast_path(x, idx, torch.float32)
    with env(None):
        s = new_store(x)
        assert s.prepare_fetch("x", torch.bfloat16)
        got_f32 = fetch(s, idx, torch.float32, 128)
        got_aff = fetch(s, idx, torch.bfloat16, 128, affine=(0.5, 3.0))
        q = s.query("x")
        s.free()
    assert q["replica_gathers"] == 0 and q["replica_dtype"] == "bfloat16"
    assert torch.equal(got_f32, ref_f32) and torch.equal(got_aff, ref_aff)


def test_second_dtype_takes_the_cast_path():
    x = shard(torch.float32, 128)
    idx = torch.arange(N)
    ref, _ = cast_path(x, idx, torch.float16)
    with env(None):
        s = new_store(x)
        assert s.prepare_fetch("x", torch.bfloat16)
        for _ in range(3):  # three shards' worth: past any trigger
            got = fetch(s, idx, torch.float16, 128)
        q = s.query("x")
        s.free()
    assert q["replica_dtype"] == "bfloat16" and q["replica_gathers"] == 0
    assert torch.equal(got, ref)


@pytest.mark.parametrize("width", [136, 3])  # 3: the written range starts and
def test_update_recasts_the_rows_written(width):  # ends off a 16-B boundary
    x = shard(torch.float32, width).clone()
    new = shard(torch.float32, width, seed=1)[:64].clone()
    new.view(-1)[: len(SPECIALS)] = torch.tensor(SPECIALS, dtype=torch.float64).to(torch.float32)
    idx = torch.arange(90, 175)
    with env(None):
        s = new_store(x)
        assert s.prepare_fetch("x", torch.bfloat16)
        before = fetch(s, idx, torch.bfloat16, width)
        s.update("x", new, 100)
        got = fetch(s, idx, torch.bfloat16, width)
        q = s.query("x")
        s.free()
    x[100:164] = new
    ref, _ = cast_path(x, idx, torch.bfloat16)
    assert q["replica_dtype"] == "bfloat16" and q["replica_gathers"] == 2
    assert torch.equal(got, ref)
    keep = torch.cat([torch.arange(0, 10), torch.arange(74, 85)])  # rows 90..99, 164..174
    assert torch.equal(got[keep], before[keep])


def _all_rows_match_cast_path(s, out_dt=torch.bfloat16):
    """Every row fetched as ``out_dt`` against the casting gather over what
    the store holds now."""
    idx = torch.arange(N)
    now = s.get_batch("x", idx, dtype=torch.float32).cpu()
    ref, _ = cast_path(now, idx, out_dt)
    assert torch.equal(fetch(s, idx, out_dt, now.shape[1]), ref)


def test_writers_drop_the_replica():
    x = shard(torch.float32, 128)
    with env(None):
        s = new_store(x)
        # local_shard hands out a writable view
        assert s.prepare_fetch("x", torch.bfloat16)
        view = s.local_shard("x")
        assert s.query("x")["replica_dtype"] == ""
        view[7] = 42.0
        torch.cuda.synchronize()
        got = fetch(s, torch.tensor([7, 8]), torch.bfloat16, 128)
        assert (got[0] == bits(torch.tensor([42.0], dtype=torch.bfloat16))[0]).all()
        _all_rows_match_cast_path(s)
        # the view stays valid, so a shard's worth of demand builds nothing now
        assert s.query("x")["replica_state"] == "none"
        # both reshuffle forms
        for kw in ({}, {"max_chunk_bytes": 64 * 1024}):
            assert s.prepare_fetch("x", torch.bfloat16)
            s.reshuffle("x", seed=11, **kw)
            assert s.query("x")["replica_dtype"] == ""
            _all_rows_match_cast_path(s)
        # drop_fetch_replica, and a free with a live replica
        assert s.prepare_fetch("x", torch.bfloat16)
        s.drop_fetch_replica("x")
        q = s.query("x")
        assert q["replica_dtype"] == "" and q["replica_bytes"] == 0
        assert s.prepare_fetch("x", torch.bfloat16)
        s.free()


def test_no_automatic_replica_behind_a_view():
    """A view handed out before any replica exists can be written at any
    time: the demand trigger must not freeze the rows behind it."""
    x = shard(torch.float32, 128)
    idx = torch.arange(N)
    with env(None):
        s = new_store(x)
        view = s.local_shard("x")
        for _ in range(2):
            fetch(s, idx, torch.bfloat16, 128)
        assert s.query("x")["replica_state"] == "none"
        view[9] = -3.0
        torch.cuda.synchronize()
        got = fetch(s, torch.tensor([9]), torch.bfloat16, 128)
        assert (got[0] == bits(torch.tensor([-3.0], dtype=torch.bfloat16))[0]).all()
        s.free()


def test_dump_keeps_the_replica(tmp_path):
    x = shard(torch.float32, 8)
    with env(None):
        s = new_store(x)
        assert s.prepare_fetch("x", torch.bfloat16)
        s.dump("x", str(tmp_path / "x.pt"))
        assert s.query("x")["replica_state"] == "complete"
        s.free()


def test_memory_returns_after_a_drop():
    width = 2048  # a 16 MiB replica: well above the 2 MiB allocation granule
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, width, generator=g)
    granule = 2 << 20
    with env(None):
        s = new_store(x)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        assert s.prepare_fetch("x", torch.bfloat16)
        assert s.query("x")["replica_bytes"] == N * width * 2
        s.drop_fetch_replica()
        free1 = torch.cuda.mem_get_info(0)[0]
        assert s.prepare_fetch("x", torch.bfloat16)
        s._backend.free_var("x")
        del s._vars["x"]
        s.add("x", x)  # re-registration starts without a replica
        assert s.query("x")["replica_dtype"] == ""
        s.free()
    assert abs(free0 - free1) <= granule, (free0, free1)


def test_budget_below_the_replica_size():
    width = 136  # replica: 4096 * 136 * 2 B = 1.06 MiB
    x = shard(torch.float32, width)
    idx = torch.arange(N)
    ref, _ = cast_path(x, idx, torch.bfloat16)
    with env(1):
        s = new_store(x)
        for _ in range(2):  # the first call crosses the trigger
            assert torch.equal(fetch(s, idx, torch.bfloat16, width), ref)
            q = s.query("x")
            assert q["replica_dtype"] == "" and q["replica_bytes"] == 0
        assert s.prepare_fetch("x", torch.bfloat16) is False
    with env(64):
        # the refusal is remembered: a budget that would fit is not asked
        assert torch.equal(fetch(s, idx, torch.bfloat16, width), ref)
        assert s.query("x")["replica_dtype"] == ""
        s.drop_fetch_replica("x")  # an invalidation forgets it
        assert torch.equal(fetch(s, idx, torch.bfloat16, width), ref)
        q = s.query("x")
        assert q["replica_dtype"] == "bfloat16" and q["replica_gathers"] == 1
        s.free()


def _w_two_ranks(rank, world):
    from ddstore_amd import DDStore

    os.environ.pop(ENV, None)
    dev = f"cuda:{rank % max(torch.cuda.device_count(), 1)}"
    s = DDStore(device=dev)
    s.add("x", shard(torch.float32, 128, seed=rank))
    idx = torch.arange(N * world)

    def fetch_all():
        out = s.get_batch("x", idx, dtype=torch.bfloat16)
        torch.cuda.synchronize()
        return out.view(torch.int16).cpu()

    def state():
        q = s.query("x")
        return q["replica_state"], q["replica_dtype"]

    # several ranks never build inside a fetch: these are the casting gather
    ref = fetch_all()
    assert torch.equal(fetch_all(), ref)
    assert state() == ("none", "")
    s.drop_fetch_replica()  # forget the demand of the reference fetches

    # the automatic route: rank 0 alone crosses the trigger
    s.epoch_begin()
    if rank == 0:
        assert torch.equal(fetch_all(), ref)
    assert state() == ("none", "")
    s.epoch_end()
    s.epoch_begin()
    assert state() == ("complete", "bfloat16")
    assert torch.equal(fetch_all(), ref)
    assert s.query("x")["replica_gathers"] == 1
    s.epoch_end()

    s.drop_fetch_replica()
    assert state() == ("none", "") and s.query("x")["replica_bytes"] == 0
    assert s.prepare_fetch("x", torch.bfloat16) is True
    assert torch.equal(fetch_all(), ref)
    assert s.query("x")["replica_gathers"] == 2

    # one rank gives its replica up and stops using it at once. The ranks
    # now differ, and prepare_fetch on all of them must still agree: every
    # rank drops and rebuilds
    if rank == 1:
        s.local_shard("x")
    assert state() == (("stale", "") if rank == 1 else ("complete", "bfloat16"))
    assert s.prepare_fetch("x", torch.bfloat16) is True
    assert state() == ("complete", "bfloat16")
    assert torch.equal(fetch_all(), ref)
    assert s.query("x")["replica_gathers"] == 3

    # ... and without prepare_fetch the next epoch_begin drops it everywhere
    if rank == 1:
        s.local_shard("x")
    s.epoch_begin()
    assert state() == ("none", "") and s.query("x")["replica_bytes"] == 0
    # rank 1 has handed out a view: rank 0's demand builds nothing any more
    if rank == 0:
        assert torch.equal(fetch_all(), ref)
    s.epoch_end()
    s.epoch_begin()
    assert state() == ("none", "")
    assert torch.equal(fetch_all(), ref)
    s.epoch_end()
    s.free()


def test_two_ranks_on_one_gpu():
    run_dist(_w_two_ranks, 2)
