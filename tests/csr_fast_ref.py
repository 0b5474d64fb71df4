"""Reference model, checker and case table for the one-call CSR fetch,
``get_csr(name, idx, out=buf)``.

Everything here is plain torch on the CPU. ``tests/test_csr_fast_cpu.py``
runs the table against the host backend (which proves the model and the
inputs without a GPU) and ``tests/test_gpu_csr_fast.py`` runs it against the
plan + work-item kernels.

The model, for a request ``idx`` into a capacity buffer of ``cap`` elements:

* a bad index (outside ``[0, nsamples)``) is a sample of length 0 and counts
  once in ``oob_skipped``;
* ``off`` is the exclusive cumsum of the requested lengths, never clamped;
* sample ``i`` is kept iff ``L_i > 0 and off[i+1] <= cap``. A kept sample's
  bytes land at ``off[i]``; a sample with ``L_i > 0`` that is not kept counts
  once in ``cap_skipped`` and writes nothing. An empty sample writes nothing
  and is never counted, wherever its offset lies;
* ``bytes_gathered`` grows by the kept elements times the element size;
* no byte outside the kept samples' slices is written, inside ``out`` or
  around it.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

SENTINEL = 0xA5
HEAD_BYTES = 4096   # sentinel in front of `out` (keeps `out` 16-B aligned)
TAIL_BYTES = 8192   # sentinel behind `out`
ITEM_BYTES = 1024   # default work-item size of the GPU path

# (id, dtype, disp, byte offset of `out` in its backing buffer)
Case = namedtuple("Case", "id dtype disp byte_offset")

CASES = [
    Case("f32x1", torch.float32, 1, 0),          # 4 B, dword path, ie 256
    Case("f32x3", torch.float32, 3, 0),          # 12 B, dword, ie 85 (item < 1024 B)
    Case("f32x4", torch.float32, 4, 0),          # 16 B, dword, ie 64
    Case("i64x1", torch.int64, 1, 0),            # 8 B, dword, ie 128
    Case("bf16x2", torch.bfloat16, 2, 0),        # 4 B, dword, ie 256
    Case("bf16x1", torch.bfloat16, 1, 0),        # 2 B, byte path, ie 512
    Case("u8x3", torch.uint8, 3, 0),             # 3 B, byte, ie 341
    Case("u8x4", torch.uint8, 4, 0),             # 4 B into an aligned out: dword
    Case("u8x4_off1", torch.uint8, 4, 1),        # same, out offset by 1 B: byte
    Case("f32x300", torch.float32, 300, 0),      # 1200 B > one item: ie clamps to 1
]
CASE_BY_ID = {c.id: c for c in CASES}
NIDX = 300  # more than one 256-sample plan tile, the second one partial


def elem_bytes(case):
    return case.disp * torch.empty(0, dtype=case.dtype).element_size()


def case_lengths(case):
    """Stored sample lengths, built not drawn: 0..12 in a row walks the
    destination through all four dword phases with every head and tail size,
    then the lengths around one, two and three work items, then zeros."""
    eb = elem_bytes(case)
    if eb > ITEM_BYTES:
        return list(range(6)) + [0, 0, 3]
    ie = ITEM_BYTES // eb
    return (list(range(13))
            + [ie - 1, ie, ie + 1, 2 * ie, 2 * ie + 1, 3 * ie - 1]
            + [0, 0, 0]
            + [7, 2 * ie + 3, 1, 0, ie + 2, 5, 3 * ie, 9, 2, 0, 11, ie, 4, 6,
               0, 1, 3])


def case_idx(case, n=NIDX):
    """Every stored sample at least once, in a shuffled order, then
    duplicates; position 0 holds sample 5 (length 5 in every case)."""
    ns = len(case_lengths(case))
    rng = np.random.default_rng(4242 + ns)
    idx = np.concatenate([rng.permutation(ns), rng.integers(0, ns, n - ns)])
    five = int(np.nonzero(idx == 5)[0][0])
    idx[[0, five]] = idx[[five, 0]]
    return torch.from_numpy(idx.astype(np.int64))


def random_values(n, dtype, disp, seed):
    """(n, disp) values of random BITS (every byte pattern, NaNs included:
    the fetch is a byte move and is compared as bytes)."""
    isz = torch.empty(0, dtype=dtype).element_size()
    g = torch.Generator().manual_seed(seed)
    raw = torch.randint(0, 256, (n, disp * isz), dtype=torch.uint8, generator=g)
    return raw.view(dtype)


@functools.lru_cache(maxsize=None)
def case_data(case_id):
    """(vals, lens, idx) of a table case; computed once and shared."""
    case = CASE_BY_ID[case_id]
    lens = case_lengths(case)
    vals = random_values(sum(lens), case.dtype, case.disp, 1000 + len(case_id))
    return vals, lens, case_idx(case)


def expected(vals, lens, idx, cap):
    """``(off, keep, packed)`` of the model in the module docstring:
    ``packed`` is the whole unclamped packed payload, (off[-1], disp)."""
    lens = torch.as_tensor(lens, dtype=torch.int64)
    idx = torch.as_tensor(idx, dtype=torch.int64)
    ns = lens.numel()
    good = (idx >= 0) & (idx < ns)
    safe = torch.where(good, idx, torch.zeros_like(idx))
    L = torch.where(good, lens[safe], torch.zeros_like(idx))
    off = torch.zeros(idx.numel() + 1, dtype=torch.int64)
    torch.cumsum(L, 0, out=off[1:])
    keep = (L > 0) & (off[1:] <= cap)
    goff = torch.zeros(ns + 1, dtype=torch.int64)
    torch.cumsum(lens, 0, out=goff[1:])
    total = int(off[-1])
    # source element of every packed element, all samples at once
    src = torch.repeat_interleave(goff[safe] - off[:-1], L) + torch.arange(total)
    return off, keep, vals[src]


def model_counts(off, keep, idx, nsamples, eb):
    """(oob_skipped, cap_skipped, bytes_gathered) the call must add."""
    idx = torch.as_tensor(idx, dtype=torch.int64)
    L = off[1:] - off[:-1]
    return (int(((idx < 0) | (idx >= nsamples)).sum()),
            int(((L > 0) & ~keep).sum()), int(L[keep].sum()) * eb)


class Fetch:
    """One checked ``get_csr(out=)`` call, in three steps so that a test can
    allocate everything first and then issue calls back to back:
    ``Fetch(...)`` builds the sentinel backing buffer and the device index,
    ``run()`` calls the store, ``verify()`` asserts the model."""

    def __init__(self, store, name, vals, lens, idx, cap, byte_offset=0):
        self.store, self.name, self.vals, self.lens = store, name, vals, lens
        self.idx = torch.as_tensor(idx, dtype=torch.int64)
        self.cap = int(cap)
        self.eb = vals.shape[1] * vals.element_size()
        self.head = HEAD_BYTES + byte_offset
        dev = store.device
        self.backing = torch.full((self.head + self.cap * self.eb + TAIL_BYTES,),
                                  SENTINEL, dtype=torch.uint8, device=dev)
        self.out = self.backing[self.head: self.head + self.cap * self.eb] \
            .view(vals.dtype).view(self.cap, vals.shape[1])
        self.idx_dev = self.idx.to(dev)
        self.before = None
        self.off = None

    def run(self):
        q = self.store.query(self.name)
        self.before = {k: q[k] for k in ("oob_skipped", "cap_skipped",
                                         "bytes_gathered")}
        got, self.off = self.store.get_csr(self.name, self.idx_dev, out=self.out)
        assert got is self.out
        return self

    def verify(self, counters=True):
        """``counters=False`` when another call ran between run() and here."""
        if self.backing.is_cuda:
            torch.cuda.synchronize()
        tag = f"{self.name} cap={self.cap}"
        off, keep, packed = expected(self.vals, self.lens, self.idx, self.cap)
        assert torch.equal(self.off.cpu(), off), f"{tag}: offsets differ"

        L = off[1:] - off[:-1]
        kept_elem = torch.repeat_interleave(keep, L)     # per packed element
        pos = torch.nonzero(kept_elem).flatten()         # all < cap
        assert pos.numel() == 0 or int(pos[-1]) < self.cap
        got = self.backing.cpu()
        region = got[self.head: self.head + self.cap * self.eb].view(self.cap, self.eb)
        want = packed.contiguous().view(torch.uint8).view(-1, self.eb)
        same = (region[pos] == want[pos]).all(dim=1)
        if not bool(same.all()):
            e = int(pos[int(torch.nonzero(~same)[0])])
            s = int(torch.searchsorted(off, torch.tensor(e), right=True)) - 1
            raise AssertionError(
                f"{tag}: payload differs at element {e} (request {s}, "
                f"sample {int(self.idx[s])}, length {int(L[s])}, "
                f"offset {int(off[s])})")

        untouched = torch.ones(got.numel(), dtype=torch.bool)
        inside = untouched[self.head: self.head + self.cap * self.eb].view(self.cap, self.eb)
        inside[pos] = False
        dirty = torch.nonzero(untouched & (got != SENTINEL)).flatten()
        assert dirty.numel() == 0, (
            f"{tag}: {dirty.numel()} bytes outside the kept samples were "
            f"written, first at byte {int(dirty[0]) - self.head} relative to out "
            f"(out is {self.cap * self.eb} bytes)")

        if not counters:
            return self
        q = self.store.query(self.name)
        delta = tuple(q[k] - self.before[k] for k in ("oob_skipped", "cap_skipped",
                                                      "bytes_gathered"))
        assert delta == model_counts(off, keep, self.idx, len(self.lens), self.eb), (
            f"{tag}: (oob, cap, bytes) grew by {delta}")
        return self


def check(store, name, vals, lens, idx, cap, byte_offset=0):
    """Run one fetch and assert the whole model; returns the Fetch."""
    return Fetch(store, name, vals, lens, idx, cap, byte_offset).run().verify()


def register(store, case):
    """add_csr a table case; returns (name, vals, lens, idx)."""
    vals, lens, idx = case_data(case.id)
    name = f"t_{case.id}"
    store.add_csr(name, vals, lens)
    return name, vals, lens, idx


def exact_cap(lens, idx):
    return int(torch.as_tensor(lens, dtype=torch.int64)[idx].sum())


def clamp_caps(case, lens, idx):
    """{label: cap} for an in-range ``idx``: the cuts the clamp has to get
    right. Each is derived from the request's own offsets."""
    L = torch.as_tensor(lens, dtype=torch.int64)[idx]
    off = torch.zeros(idx.numel() + 1, dtype=torch.int64)
    torch.cumsum(L, 0, out=off[1:])
    ie = max(ITEM_BYTES // elem_bytes(case), 1)
    multi = [i for i in range(100, idx.numel()) if int(L[i]) > 2 * ie][0]
    mid = [i for i in range(200, idx.numel()) if int(L[i]) > 0][0]
    assert int(L[0]) == 5
    return {
        "after_first": int(off[1]) + 1,
        "after_multi_item": int(off[multi + 1]) + 1,
        "inside_multi_item": int(off[multi]) + ie + 1,
        "on_boundary": int(off[mid + 1]),
        "none_fit": int(L[0]) - 1,
        "zero": 0,
    }
