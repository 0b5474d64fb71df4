"""Tiled fixed-stride gather kernel (persistent row tiles, directory in the
kernel arguments): tile edges, dtype pairs, special values, bad indices,
duplicates, many tiles per wave, the LDS-directory and legacy variants, two
parts, and the misaligned-output fallback.

The expected value is always ``arr[idx].to(out_dtype)`` computed by torch on
the device and compared bit for bit (NaNs only have to stay NaN).
"""
import os
import subprocess
import sys

import pytest
import torch

from tests.dist_utils import run_dist

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROWS = 3000
NIDX = [1, 3, 15, 16, 17, 63, 64, 65, 255, 1000, 4099]
F8 = torch.float8_e4m3fn

# (in dtype, out dtype, dim)
TRIPLES = [
    (torch.float32, torch.bfloat16, 128),   # the flagship shape
    (torch.float32, torch.float32, 128),    # same-dtype byte move
    (torch.float32, torch.bfloat16, 8),     # one chunk per row
    (torch.float32, torch.bfloat16, 24),    # three chunks per row
    (torch.float32, torch.float32, 4),      # 16-B rows
    (torch.float32, torch.float32, 36),     # 144-B rows, nine 16-B chunks
    (torch.bfloat16, torch.float32, 136),
    (torch.float16, torch.bfloat16, 128),
    (torch.uint8, torch.float32, 64),
    (F8, torch.bfloat16, 128),
]

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def make_shard(dtype, nrows, dim, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (nrows, dim), generator=g, dtype=torch.uint8)
    return torch.randn(nrows, dim, generator=g).to(dtype)


def assert_bits_equal(out, exp, what=""):
    """Bit-for-bit equality; a NaN only has to be a NaN."""
    assert out.dtype == exp.dtype and out.shape == exp.shape, what
    iv = _INT_VIEW[out.element_size()]
    ob, eb = out.contiguous().view(iv), exp.contiguous().view(iv)
    if out.is_floating_point():
        on, en = torch.isnan(out.float()), torch.isnan(exp.float())
        assert torch.equal(on, en), f"{what}: NaN positions differ"
        ob, eb = ob.masked_fill(en, 0), eb.masked_fill(en, 0)
    if not torch.equal(ob, eb):
        bad = (ob != eb).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} elements differ, first at "
                             f"{bad[0].tolist()}")


@pytest.fixture(scope="module")
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cuda:0")
    assert s.mode == "hip", "GPU test must exercise the native HIP path"
    yield s
    s.free()


_shards = {}


def shard_for(store, dtype, dim):
    """One variable per (dtype, dim), added once; returns (name, device copy)."""
    key = (dtype, dim)
    if key not in _shards:
        name = f"t_{str(dtype).split('.')[-1]}_{dim}"
        arr = make_shard(dtype, NROWS, dim, seed=dim)
        store.add(name, arr)
        _shards[key] = (name, arr.to("cuda:0"))
    return _shards[key]


def batch_idx(nidx, seed=0):
    g = torch.Generator().manual_seed(1000 + nidx + seed)
    return torch.randint(0, NROWS, (nidx,), generator=g).to("cuda:0")


@pytest.mark.parametrize("tin,tout,dim", TRIPLES,
                         ids=lambda v: str(v).split(".")[-1])
def test_tile_edges(store, tin, tout, dim):
    name, dev = shard_for(store, tin, dim)
    for nidx in NIDX:
        idx = batch_idx(nidx)
        out = store.get_batch(name, idx, dtype=tout)
        torch.cuda.synchronize()
        assert_bits_equal(out, dev[idx].to(tout), f"nidx={nidx}")
    assert store.query(name)["oob_skipped"] == 0


@pytest.mark.parametrize("tin,tout,dim", [(torch.uint8, torch.bfloat16, 64),
                                          (torch.float32, torch.float32, 128),
                                          # three chunks per row: vector one-shot
                                          (torch.uint8, torch.bfloat16, 24),
                                          # 5 % 4 != 0: scalar one-shot
                                          (torch.float16, torch.float32, 5)],
                         ids=lambda v: str(v).split(".")[-1])
def test_affine(store, tin, tout, dim):
    # scale and shift have 2 significant bits each, so x * scale + shift in
    # float64 is the exactly rounded f32 fmaf once rounded to f32
    scale, shift = 0.0234375, -1.5
    name, dev = shard_for(store, tin, dim)
    for nidx in NIDX:
        idx = batch_idx(nidx, seed=7)
        out = store.get_batch(name, idx, dtype=tout, affine=(scale, shift))
        torch.cuda.synchronize()
        x = dev[idx].to(torch.float32).to(torch.float64)
        exp = (x * scale + shift).to(torch.float32).to(tout)
        assert_bits_equal(out, exp, f"nidx={nidx}")


@pytest.mark.parametrize("dim", [32776, 32780])
def test_rows_above_tiled_limit(store, dim):
    """Rows of more than 4096 output chunks take the one-shot kernels even by
    default. dim 32776 (131,104-B rows, a multiple of 32): f32->f32 is 8194
    16-B chunks and moves 32-B chunks, f32->bf16 is 4097 chunks of the vector
    cast. dim 32780 (131,120 B, a multiple of 16 only): f32->f32 moves 16-B
    chunks, f32->bf16 (32780 % 8 != 0) runs the scalar cast."""
    nrows = 8
    name = f"wide_{dim}"
    arr = make_shard(torch.float32, nrows, dim, seed=dim)
    store.add(name, arr)
    dev = arr.to("cuda:0")
    idx = torch.tensor([3, 0, 7, 3, nrows, 5], dtype=torch.int64, device="cuda:0")
    good = idx < nrows
    sentinel = -123.0
    for tout in (torch.float32, torch.bfloat16):
        out = torch.full((idx.numel(), dim), sentinel, dtype=tout, device="cuda:0")
        before = store.query(name)["oob_skipped"]
        store.get_batch(name, idx, out=out)
        torch.cuda.synchronize()
        assert (out[~good] == sentinel).all(), f"{tout}: a skipped row was written"
        assert_bits_equal(out[good], dev[idx[good]].to(tout), f"{tout} valid rows")
        assert store.query(name)["oob_skipped"] - before == 1


def test_special_values_f32_bf16(store):
    bits = [
        0x00000000, 0x80000000,              # +-0
        0x7F800000, 0xFF800000,              # +-Inf
        0x7FC00000, 0xFFC00001, 0x7F800001,  # NaNs (quiet, signed, signalling)
        0x00000001, 0x807FFFFF, 0x00400000,  # denormals
        0x3F808000,                          # tie, rounds to even (down)
        0x3F818000,                          # tie, rounds to even (up)
        0x7F7FFFFF,                          # rounds to Inf
        0x3F800000, 0xC2F70000,              # ordinary values
    ]
    dim = 128
    t = torch.tensor(bits, dtype=torch.int64)
    t = torch.where(t >= 2**31, t - 2**32, t).to(torch.int32)
    rows = t.view(torch.float32).repeat(dim // len(bits) + 1)[:dim]
    # row k is the pattern rotated by k, so every value meets every lane slot
    arr = torch.stack([rows.roll(k) for k in range(64)])
    store.add("special", arr)
    dev = arr.to("cuda:0")
    idx = torch.arange(63, -1, -1, device="cuda:0")
    out = store.get_batch("special", idx, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    exp = dev[idx].to(torch.bfloat16)
    assert torch.isnan(exp.float()).any() and torch.isinf(exp.float()).any()
    assert_bits_equal(out, exp, "special values")


@pytest.mark.parametrize("tout", [torch.bfloat16, torch.float32],
                         ids=["f32_bf16", "f32_f32"])
def test_bad_indices(store, tout):
    # at this batch size both shapes run 16-row tiles (one group of passes
    # per tile), so rows 0/15, 16/31 are first/last rows of full tiles and
    # rows 80..86 form the last, partial tile
    name, dev = shard_for(store, torch.float32, 128)
    nidx = 87
    i64 = torch.iinfo(torch.int64)
    bad = {0: -1, 15: NROWS, 16: i64.min, 31: i64.max, 80: -1, 86: NROWS,
           83: i64.max}
    idx = batch_idx(nidx, seed=3).cpu()
    for pos, v in bad.items():
        idx[pos] = v
    idx = idx.to("cuda:0")
    sentinel = -123.0
    out = torch.full((nidx, 128), sentinel, dtype=tout, device="cuda:0")
    before = store.query(name)["oob_skipped"]
    store.get_batch(name, idx, out=out)
    torch.cuda.synchronize()
    good = torch.ones(nidx, dtype=torch.bool)
    good[list(bad)] = False
    good = good.to("cuda:0")
    assert (out[~good] == sentinel).all(), "a skipped row was written"
    assert_bits_equal(out[good], dev[idx[good]].to(tout), "valid rows")
    assert store.query(name)["oob_skipped"] - before == len(bad)


def test_duplicates(store):
    name, dev = shard_for(store, torch.float32, 128)
    one = torch.full((1000,), 1234, dtype=torch.int64, device="cuda:0")
    out = store.get_batch(name, one, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert_bits_equal(out, dev[one].to(torch.bfloat16), "one repeated index")
    twice = batch_idx(500, seed=11).repeat_interleave(2)
    out = store.get_batch(name, twice, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert_bits_equal(out, dev[twice].to(torch.bfloat16), "every index twice")


_VARIANT_CODE = """
import hashlib, sys
import torch
sys.path.insert(0, {root!r})
from ddstore_amd import DDStore
from tests.test_gpu_gather_tiled import make_shard, assert_bits_equal
s = DDStore(device="cuda:0")
for tin, tout, dim in [(torch.float32, torch.bfloat16, 128),
                       (torch.float32, torch.float32, 128),
                       (torch.float32, torch.bfloat16, 8),
                       (torch.float32, torch.bfloat16, 24),
                       (torch.float32, torch.float32, 4),
                       (torch.float32, torch.float32, 36)]:
    arr = make_shard(tin, 3000, dim, seed=dim)
    name = "v%d_%s" % (dim, str(tout).split(".")[-1])
    s.add(name, arr)
    g = torch.Generator().manual_seed(99)
    idx = torch.randint(0, 3000, (4099,), generator=g).to("cuda:0")
    out = s.get_batch(name, idx, dtype=tout)
    torch.cuda.synchronize()
    assert_bits_equal(out, arr.to("cuda:0")[idx].to(tout), name)
    assert s.query(name)["oob_skipped"] == 0
    raw = out.cpu().contiguous().view(torch.uint8).numpy().tobytes()
    print("HASH", name, hashlib.sha256(raw).hexdigest())
s._backend.free_all()
print("VARIANT-OK")
"""


def test_many_tiles_per_wave_and_variants():
    """Three workgroups for 4099 rows: every wave runs several tiles and one
    is partial. The kernel-argument directory, the LDS directory, the legacy
    kernels and the tiled kernel forced onto the short rows must agree."""
    variants = {
        "blocks3": {"DDSTORE_GATHER_BLOCKS": "3"},
        "blocks3_lds": {"DDSTORE_GATHER_BLOCKS": "3", "DDSTORE_GATHER_DIR": "lds"},
        "legacy": {"DDSTORE_GATHER_BLOCKS": "3", "DDSTORE_GATHER_KERNEL": "legacy"},
        "blocks3_tiled": {"DDSTORE_GATHER_BLOCKS": "3",
                          "DDSTORE_GATHER_KERNEL": "tiled"},
        "blocks3_tiled_lds": {"DDSTORE_GATHER_BLOCKS": "3",
                              "DDSTORE_GATHER_KERNEL": "tiled",
                              "DDSTORE_GATHER_DIR": "lds"},
    }
    code = _VARIANT_CODE.format(root=ROOT)
    procs = {}
    for k, extra in variants.items():
        env = {e: v for e, v in os.environ.items()
               if not e.startswith("DDSTORE_GATHER_")}
        env.update(extra)
        procs[k] = subprocess.Popen([sys.executable, "-c", code], env=env, cwd=ROOT,
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                    text=True)
    hashes = {}
    for k, p in procs.items():
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, f"{k}: {se}"
        assert "VARIANT-OK" in so, f"{k}: {so}"
        hashes[k] = sorted(l for l in so.splitlines() if l.startswith("HASH"))
        assert len(hashes[k]) == 6
    for k in variants:
        assert hashes[k] == hashes["blocks3"], f"{k} differs from blocks3"


def _w_two_parts(rank, world):
    from ddstore_amd import DDStore

    dev = f"cuda:{rank % max(torch.cuda.device_count(), 1)}"
    s = DDStore(device=dev)
    shards = [make_shard(torch.float32, n, 128, seed=50 + r)
              for r, n in enumerate((100, 37))]
    s.add("x", shards[rank])
    full = torch.cat(shards).to(dev)
    idx = torch.tensor([99, 100, 136, 137, 0, 36, 37, 98, 101, 135, 100, 99],
                       dtype=torch.int64, device=dev)
    good = idx < 137
    for tout in (torch.float32, torch.bfloat16):
        out = torch.full((idx.numel(), 128), -7.0, dtype=tout, device=dev)
        before = s.query("x")["oob_skipped"]
        s.get_batch("x", idx, out=out)
        torch.cuda.synchronize()
        exp = full[idx[good]].to(tout)
        got = out[good]
        for r in range(exp.shape[0]):
            assert_bits_equal(got[r], exp[r], f"{tout} row {r}")
        assert (out[~good] == -7.0).all()
        assert s.query("x")["oob_skipped"] - before == 1
    s.free()


def test_two_parts_uneven():
    run_dist(_w_two_parts, 2)


def test_misaligned_output_falls_back(store):
    name, dev = shard_for(store, torch.float32, 128)
    idx = batch_idx(65, seed=5)
    for tout in (torch.float32, torch.bfloat16):
        back = torch.empty(65 * 128 + 1, dtype=tout, device="cuda:0")
        out = back[1: 1 + 65 * 128].view(65, 128)  # element-aligned only
        assert out.data_ptr() % 16 != 0
        store.gather_into(name, idx, out)
        torch.cuda.synchronize()
        assert_bits_equal(out.contiguous(), dev[idx].to(tout), str(tout))
