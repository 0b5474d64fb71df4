"""The one-call CSR fetch on the GPU, ``get_csr(name, idx, out=buf)``: the
plan kernels (k_csr_plan1/2/3) and the work-item gather
(k_gather_csr_items) against the CPU model of tests/csr_fast_ref.py.

Every call writes into a capacity buffer cut out of a sentinel-filled
backing buffer, and every byte is accounted for: offsets equal, kept
samples bit-identical, everything else (inside ``out`` and around it) still
the sentinel, counters grown by exactly the model's amounts. Run with
``pytest -m gpu``."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import csr_fast_ref as ref
from tests.dist_utils import run_dist
from tests.test_gpu_csr_padded import store  # noqa: F401  (the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.id)
def test_case_table(store, case):  # noqa: F811
    """Every element kind at exact capacity: lengths 0..12 (all four
    destination phases, every head and tail), samples of one, two and three
    work items with short last pieces, the dword and the byte kernel, an
    element wider than an item, two plan tiles."""
    name, vals, lens, idx = ref.register(store, case)
    f = ref.check(store, name, vals, lens, idx, ref.exact_cap(lens, idx),
                  case.byte_offset)
    # the kernel choice the case is in the table for
    dword = ref.elem_bytes(case) % 4 == 0 and f.out.data_ptr() % 4 == 0
    assert dword == (case.id not in ("bf16x1", "u8x3", "u8x4_off1"))


@pytest.mark.parametrize("nidx", [1, 255, 256, 257, 513, 66000])
def test_plan_tiles_full_payload(store, nidx):  # noqa: F811
    """Plan tile edges with the WHOLE payload checked; 66000 requests are
    258 tiles, so k_csr_plan2 runs a second chunk of tile aggregates."""
    lens = [i % 9 for i in range(64)]
    vals = ref.random_values(sum(lens), torch.float32, 1, 77)
    store.add_csr("tiles", vals, lens)
    idx = torch.from_numpy(np.random.default_rng(nidx).integers(0, 64, nidx))
    ref.check(store, "tiles", vals, lens, idx, ref.exact_cap(lens, idx))


def test_bad_indices(store):  # noqa: F811
    case = ref.CASE_BY_ID["f32x1"]
    name, vals, lens, idx = ref.register(store, case)
    ns = len(lens)
    idx = idx.clone()
    bad_at = [0, 3, 17, 100, 255, 256, 257, 299]
    idx[bad_at] = torch.tensor([-1, ns, 2 ** 40, -2 ** 63, ns, -1, 2 ** 40, ns + 1])
    good = (idx >= 0) & (idx < ns)
    assert int((~good).sum()) == len(bad_at)
    cap = int(torch.tensor(lens)[idx[good]].sum())
    f = ref.check(store, name, vals, lens, idx, cap)
    off = f.off.cpu()
    assert bool((off[1:] - off[:-1])[~good].eq(0).all())
    assert store.query(name)["oob_skipped"] == len(bad_at)


@pytest.mark.parametrize("case_id", ["f32x1", "u8x3"])
def test_clamp_models(store, case_id):  # noqa: F811
    """Capacity cuts on the dword and the byte path: after the first
    sample, after and inside a sample of several work items, exactly on a
    sample boundary, and with nothing kept. The request ends in empty
    samples, which lie behind every cut and are never counted."""
    case = ref.CASE_BY_ID[case_id]
    name, vals, lens, idx = ref.register(store, case)
    caps = ref.clamp_caps(case, lens, idx)
    for label, cap in caps.items():
        before = store.query(name)["cap_skipped"]
        f = ref.check(store, name, vals, lens, idx, cap, case.byte_offset)
        _, keep, _ = ref.expected(vals, lens, idx, cap)
        assert store.query(name)["cap_skipped"] > before, label
        if label in ("none_fit", "zero"):
            assert not bool(keep.any()), label
        else:
            assert bool(keep.any()), label
        if label == "on_boundary":
            assert int(f.off.cpu()[keep.nonzero().max() + 1]) == cap


def _four_of_60(store):  # noqa: F811
    lens = [60, 60, 60, 60]
    vals = ref.random_values(240, torch.float32, 1, 5)
    store.add_csr("c60", vals, lens)
    return vals, lens, torch.arange(4)


def test_clamp_after_larger_call(store):  # noqa: F811
    """A clamped call right after a larger one of the same scratch sizes: the
    work-item slots of its skipped samples hold whatever the allocator hands
    back, typically the larger call's valid descriptors, whose destinations
    lie behind this call's 8-element buffer."""
    vals, lens, idx = _four_of_60(store)
    a = ref.Fetch(store, "c60", vals, lens, idx, 255)
    b = ref.Fetch(store, "c60", vals, lens, idx, 8)  # same desc_cap: 0 + 4
    a.run()
    a.off = a.off.cpu()  # hand call A's offsets block back as well
    b.run()
    a.verify(counters=False)  # its counts are in b's "before"
    b.verify()
    q = store.query("c60")
    assert q["cap_skipped"] == 4 and q["bytes_gathered"] == 240 * 4, q


def test_clamp_after_primed_scratch(store):  # noqa: F811
    """The same clamped call after blocks of the descriptor list's size were
    filled with one-unit descriptors aimed 3 elements behind ``out`` and
    freed: a slot consumed without having been written this call lands in
    the sentinel behind ``out``."""
    vals, lens, idx = _four_of_60(store)
    cap, desc_cap = 8, 8 // 256 + 4
    b = ref.Fetch(store, "c60", vals, lens, idx, cap)
    stale = torch.tensor([0, (1 << 44) | (cap + 3)], dtype=torch.int64).repeat(desc_cap)
    primed = [stale.to(store.device) for _ in range(32)]
    assert primed[0].numel() == 2 * desc_cap
    torch.cuda.synchronize()
    del primed
    b.run().verify()
    assert store.query("c60")["cap_skipped"] == 4


@pytest.mark.parametrize("short_first", [False, True])
def test_clamp_more_items_than_slots(store, short_first):  # noqa: F811
    """Four samples of 10 000 f32 into 8 elements: 160 work items counted
    against 4 (5) descriptor slots."""
    lens = ([5] if short_first else []) + [10000] * 4
    vals = ref.random_values(sum(lens), torch.float32, 1, 6)
    store.add_csr("big4", vals, lens)
    ref.check(store, "big4", vals, lens, torch.arange(len(lens)), 8)
    q = store.query("big4")
    assert q["cap_skipped"] == 4
    assert q["bytes_gathered"] == (20 if short_first else 0)


def test_per_sample_kernel_same_empty_rule(store):  # noqa: F811
    """k_gather_csr_wave, given the same offsets, keeps the model's rule for
    empty samples behind the capacity: not written, not counted."""
    lens = [4, 4, 0, 4, 0]
    vals = ref.random_values(12, torch.float32, 1, 8)
    store.add_csr("ps", vals, lens)
    f = ref.Fetch(store, "ps", vals, lens, torch.arange(5), 8)
    f.off, _, _ = ref.expected(vals, lens, f.idx, 8)
    store._backend.gather_csr("ps", f.idx_dev, f.off.to(store.device), f.out, 8)
    f.verify(counters=False)  # this entry point accounts bytes on the host
    q = store.query("ps")
    assert q["cap_skipped"] == 1 and q["oob_skipped"] == 0, q


_SHARD_LENS = [
    [3, 300, 0, 513] + [(7 * i) % 13 for i in range(31)] + [767, 2],   # 37
    [600],                                                             # 1
    [257, 0, 1024] + [(5 * i) % 11 for i in range(45)] + [1, 9],       # 50
]


def _w_three_ranks(rank, world):
    from ddstore_amd import DDStore

    s = DDStore(device=f"cuda:{rank % max(torch.cuda.device_count(), 1)}")
    assert s.mode == "hip"
    shards = [ref.random_values(sum(l), torch.float32, 1, 300 + r)
              for r, l in enumerate(_SHARD_LENS)]
    s.add_csr("c", shards[rank], _SHARD_LENS[rank])
    lens = sum(_SHARD_LENS, [])
    vals = torch.cat(shards)
    edges = [0, 36, 37, 38, 87]  # each shard's first and last sample
    idx = torch.cat([torch.tensor(edges), torch.from_numpy(
        np.random.default_rng(9 + rank).integers(0, 88, 120))])
    ref.check(s, "c", vals, lens, idx, ref.exact_cap(lens, idx))
    q = s.query("c")
    assert q["oob_skipped"] == 0 and q["cap_skipped"] == 0, q
    s.comm.barrier()  # no rank frees its shard while another still reads it
    s.free()


def test_three_ranks_one_gpu():
    """Peer indices 1 and 2 in the descriptors: shards of 37, 1 and 50
    samples, multi-item samples in each, every rank fetching across all."""
    assert [len(l) for l in _SHARD_LENS] == [37, 1, 50]
    run_dist(_w_three_ranks, 3)


_KNOB_CODE = """
import hashlib, sys
import torch
sys.path.insert(0, {root!r})
from ddstore_amd import DDStore
from tests import csr_fast_ref as ref
s = DDStore(device="cuda:0")
assert s.mode == "hip"
for cid in ("f32x1", "u8x3", "f32x3"):
    case = ref.CASE_BY_ID[cid]
    name, vals, lens, idx = ref.register(s, case)
    f = ref.check(s, name, vals, lens, idx, ref.exact_cap(lens, idx))
    raw = f.out.cpu().contiguous().view(torch.uint8).numpy().tobytes()
    print("HASH", cid, hashlib.sha256(raw).hexdigest())
s.free()
print("KNOB-OK")
"""


def test_item_knobs_agree():
    """DDSTORE_CSR_ITEM and DDSTORE_CSR_ITEM_GROUP change how samples are cut
    into work items and how many lanes copy one, never the result."""
    variants = {
        "default": {},
        "item64": {"DDSTORE_CSR_ITEM": "64"},
        "item64_g8": {"DDSTORE_CSR_ITEM": "64", "DDSTORE_CSR_ITEM_GROUP": "8"},
        "item4096_g32": {"DDSTORE_CSR_ITEM": "4096", "DDSTORE_CSR_ITEM_GROUP": "32"},
    }
    code = _KNOB_CODE.format(root=ROOT)
    procs = {}
    for k, extra in variants.items():
        env = {e: v for e, v in os.environ.items() if not e.startswith("DDSTORE_CSR_")}
        env.update(extra)
        procs[k] = subprocess.Popen([sys.executable, "-c", code], env=env, cwd=ROOT,
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                    text=True)
    hashes = {}
    for k, p in procs.items():
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, f"{k}: {se}"
        assert "KNOB-OK" in so, f"{k}: {so}"
        hashes[k] = sorted(l for l in so.splitlines() if l.startswith("HASH"))
        assert len(hashes[k]) == 3
    for k in variants:
        assert hashes[k] == hashes["default"], f"{k} differs from default"
    # and the default is the model's payload, not merely self-consistent
    vals, lens, idx = ref.case_data("f32x1")
    _, _, packed = ref.expected(vals, lens, idx, ref.exact_cap(lens, idx))
    want = hashlib.sha256(packed.contiguous().view(torch.uint8).numpy().tobytes())
    assert f"HASH f32x1 {want.hexdigest()}" in hashes["default"]
