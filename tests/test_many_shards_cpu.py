"""Worlds of 4 to 128 shards on the host backend, through the thread-per-rank
harness of ``tests/virtual_world.py``: every layout of its table, the same
helper functions and expected values as ``tests/test_gpu_many_shards.py``.
This proves the harness, the layouts and the models before a GPU sees them,
and it is the host backend's own test of ``owner_of_host`` beyond 3 ranks.

The expected value is always built from the concatenated shards on the CPU.
The host backend refuses a bad index instead of skipping it, so the index
sets here hold none; the refusals are asserted on their own.

A host store maps every peer's segment, W * W mappings per variable, so a
128-shard world holds two or three variables at a time here."""
import os
import struct

import numpy as np
import pytest
import torch

from tests import virtual_world as vw
from tests.test_column_stats_cpu import check as check_stats
from tests.test_column_stats_cpu import col_params

pytestmark = pytest.mark.timeout(600)

PAD = -3


def readers(w, lid):
    return [w.stores[r] for r in vw.LAYOUTS[lid].readers()]


# ------------------------------------------------------------------ harness
def test_layout_table():
    """The properties the table is there for, so a later edit cannot lose
    them quietly."""
    for lid, lay in vw.LAYOUTS.items():
        lens = vw.csr_lens(lid)
        _, nl, _, el = vw.graphs(lid)
        lo, hi = lay.span(lay.last)
        assert lens[hi - 1] == 600 and nl[hi - 1] == 70 and el[hi - 1] == 130
        assert 0 in lens or lay.total < 4
        if lay.zero is not None:
            zlo, zhi = lay.span(lay.zero)
            assert zhi > zlo and not any(lens[zlo:zhi])
            assert nl[zlo:zhi].sum() > 0 and el[zlo:zhi].sum() == 0
            assert {256, 300, 600} <= set(lens)
        per_shard = [(int(nl[a:b].sum()), int(el[a:b].sum()))
                     for a, b in (lay.span(r) for r in lay.nonempty)]
        # the two variables' element prefixes part ways (a kernel that took
        # one for the other would read elsewhere)
        assert per_shard[-1][0] != per_shard[-1][1]
        assert 2 * sum(n != e for n, e in per_shard) > len(per_shard)
        rd = lay.readers()
        assert rd[0] == 0 and rd[-1] == lay.W - 1 and len(rd) == 3
        assert lay.rows[rd[1]] == 0
        n = vw.index_set(lid).numel()
        assert 300 <= n <= 800, (lid, n)   # clean, skipped-row and partial tiles
        assert vw.index_set(lid, bad=True).numel() == n + 3
    w128 = vw.LAYOUTS["w128"]
    assert w128.W == 128 and w128.rows[64] == 70 and w128.rows[127] == 3
    assert w128.rows[1] == 0 and w128.rows[2] == 2 and w128.rows[3] == 3
    assert [vw.LAYOUTS[k].W for k in vw.LAYOUT_IDS] == [4, 8, 8, 9, 128, 128, 128]


def test_reaches_128_shards():
    lid = "w128"
    with vw.world(lid, "cpu", ["enc128"]) as w:
        assert all(s.size == 128 and s.mode == "shm" for s in w.stores)
        assert [s.rank for s in w.stores] == list(range(128))
        lay = vw.LAYOUTS[lid]
        lo, hi = lay.span(127)
        assert hi - lo == 3 and hi == lay.total
        full = vw.var_data(lid, "enc128")[1]
        for s in readers(w, lid):
            got = s.get_batch("enc128", list(range(lo, hi)))
            assert torch.equal(got.view(torch.int32), full[lo:hi].view(torch.int32))
            # the bits name their owner
            assert int(got.view(torch.int32)[0, 0]) >> 24 == 127


def test_a_rank_failure_is_raised_and_nobody_waits():
    def reg(store, rank):
        store.add("a", torch.zeros(2, 3))
        if rank == 2:
            raise ValueError("rank 2 gives up")
        store.add("b", torch.zeros(2, 3))   # the others wait here for rank 2

    with pytest.raises(ValueError, match="rank 2 gives up"):
        vw.VirtualWorld(4, "cpu", reg)


def test_teardown_after_a_failed_test_body():
    with pytest.raises(ZeroDivisionError):
        with vw.world("w4", "cpu", ["u8x7"]) as w:
            stores = list(w.stores)
            1 / 0
    assert all(s._freed for s in stores)


def test_world_of_129_is_refused():
    with pytest.raises(RuntimeError, match=r"world size must be in \[1, 128\]"):
        vw.VirtualWorld(129, "cpu")


@pytest.mark.gpu
def test_device_world_of_129_is_refused():
    from ddstore_amd import _C

    with pytest.raises(RuntimeError, match=r"world size must be in \[1, 128\]"):
        _C.DeviceStore(0, 0, 129)


# ------------------------------------------------------- same-process peers
def test_same_process_entry_with_a_foreign_pid_is_refused():
    from ddstore_amd import _C

    mine = struct.pack("=qQ", os.getpid(), 0x7F0000001000)
    assert _C.DeviceStore.decode_local_peer(mine) == 0x7F0000001000
    with pytest.raises(RuntimeError, match="written by pid"):
        _C.DeviceStore.decode_local_peer(struct.pack("=qQ", os.getpid() + 1, 0x1000))
    with pytest.raises(RuntimeError, match="without a pointer"):
        _C.DeviceStore.decode_local_peer(struct.pack("=qQ", os.getpid(), 0))
    with pytest.raises(RuntimeError):
        _C.DeviceStore.decode_local_peer(b"\0" * 64)


class _StubBackend:
    def __init__(self):
        self.calls = []

    def ipc_handle(self, name):
        self.calls.append("ipc_handle")
        return b"H" * 64

    def base_ptr(self, name):
        self.calls.append("base_ptr")
        return 0xABC000

    def open_peers(self, name, handles):
        self.opened = list(handles)


class _StubComm:
    def __init__(self, size):
        self.size, self.sent = size, []

    def allgather(self, obj):
        self.sent.append(obj)
        return [obj] * self.size

    def barrier(self):
        pass


def _exchange(comm, size):
    from ddstore_amd import DDStore

    s = DDStore.__new__(DDStore)
    s._freed = True                      # nothing to free
    s.mode, s.size, s.comm, s._backend = "hip", size, comm, _StubBackend()
    s._exchange_and_open("v")
    return s._backend, comm.sent


def test_exchange_bytes_unchanged_without_the_opt_in():
    from ddstore_amd.comm import Comm, _MpiWrap

    # no attribute, a false one, and a truthy value that is not True
    plain, false, truthy = _StubComm(2), _StubComm(2), _StubComm(2)
    false.same_process = False
    truthy.same_process = 1
    for comm in (plain, false, truthy):
        be, sent = _exchange(comm, 2)
        assert sent == [b"H" * 64] and be.calls == ["ipc_handle"]
        assert be.opened == [b"H" * 64] * 2
    be, sent = _exchange(_StubComm(1), 1)
    assert sent == [b""] and be.calls == []
    # the opt-in: (pid, pointer), 16 bytes, and only then
    opted = _StubComm(2)
    opted.same_process = True
    be, sent = _exchange(opted, 2)
    assert sent == [struct.pack("=qQ", os.getpid(), 0xABC000)] and be.calls == ["base_ptr"]
    assert len(sent[0]) == 16
    # _MpiWrap carries the attribute over from the wrapped object, Comm has none
    assert Comm.same_process is False

    class Mpi:
        def Get_rank(self):  # noqa: N802
            return 0

        def Get_size(self):  # noqa: N802
            return 1

    assert _MpiWrap(Mpi()).same_process is False
    m = Mpi()
    m.same_process = True
    assert _MpiWrap(m).same_process is True
    m.same_process = "yes"
    assert _MpiWrap(m).same_process is False


# ------------------------------------------------------------ fixed stride
@pytest.mark.parametrize("lid", vw.LAYOUT_IDS)
def test_get_batch(lid):
    idx = vw.index_set(lid)
    with vw.world(lid, "cpu", ["enc128", "u8x7", "val5"]) as w:
        for s in readers(w, lid):
            vw.check_batch(s, lid, "enc128", idx)
            vw.check_batch(s, lid, "u8x7", idx)
            vw.check_batch(s, lid, "val5", idx, torch.bfloat16)
            vw.check_batch(s, lid, "val5", idx, torch.bfloat16, byte_offset=2)
            vw.check_ranges(s, lid, "enc128")
    with vw.world(lid, "cpu", ["enc_i64", "val128", "val8"]) as w:
        for s in readers(w, lid):
            vw.check_batch(s, lid, "enc_i64", idx)
            vw.check_batch(s, lid, "val128", idx, torch.bfloat16)
            vw.check_batch(s, lid, "val8", idx, torch.bfloat16)


@pytest.mark.parametrize("lid,per_column", [("w8", False), ("w9", True)])
def test_get_batch_affine(lid, per_column):
    idx = vw.index_set(lid)
    scale, shift = col_params(128) if per_column else (0.0234375, -1.5)
    full = vw.var_data(lid, "val128")[1]
    exp = vw.affine_model(full, "bf16", scale, shift, fused=False)
    with vw.world(lid, "cpu", ["val128"]) as w:
        for s in readers(w, lid):
            vw.check_batch(s, lid, "val128", idx, torch.bfloat16,
                           affine=(scale, shift), expect_full=exp)


def test_bad_index_is_refused():
    lid = "w9"
    total = vw.LAYOUTS[lid].total
    with vw.world(lid, "cpu", ["val8", "c_f32x1"]) as w:
        s = w.stores[0]
        for bad in (-1, total, 2 ** 40):
            with pytest.raises(RuntimeError, match="index out of range"):
                s.get_batch("val8", [0, bad])
            with pytest.raises(IndexError, match="index out of range"):
                s.get_csr("c_f32x1", [0, bad])
        # the message names the call, not an accident inside it
        with pytest.raises(IndexError, match="ddstore get_csr: index out of range"):
            s.get_csr("c_f32x1", [total])
        vals, off = s.get_csr("c_f32x1", [])
        assert vals.shape[0] == 0 and off.tolist() == [0]


# --------------------------------------------------------------------- CSR
@pytest.mark.parametrize("lid", vw.LAYOUT_IDS)
def test_get_csr(lid):
    idx = vw.index_set(lid)
    with vw.world(lid, "cpu", ["c_f32x4", "c_f32x1", "c_u8x3"]) as w:
        q = w.stores[0].query("c_f32x1")
        lay = vw.LAYOUTS[lid]
        if lay.zero is not None:   # samples advance, elements do not
            assert q["prefix"][lay.zero + 1] > q["prefix"][lay.zero]
            assert q["elem_prefix"][lay.zero + 1] == q["elem_prefix"][lay.zero]
        for s in readers(w, lid):
            for name in ("c_f32x4", "c_f32x1", "c_u8x3"):
                vw.check_csr_alloc(s, lid, name, idx)
            for name in ("c_f32x1", "c_u8x3"):
                vw.check_csr_out(s, lid, name, idx)
                f = vw.check_csr_out(s, lid, name, idx, cut=True)
                assert s.query(name)["cap_skipped"] > 0 and f.cap < int(f.off[-1])
                s.reset_counters(name)


@pytest.mark.parametrize("lid", vw.LAYOUT_IDS)
def test_get_csr_padded(lid):
    idx = vw.index_set(lid)
    scale, shift = col_params(4)
    vals = vw.var_data(lid, "c_val4")[1]
    exp = vw.affine_model(vals, "bf16", scale, shift, fused=False)
    with vw.world(lid, "cpu", ["c_val4"]) as w:
        for s in readers(w, lid):
            vw.check_padded(s, lid, "c_val4", idx, 6, torch.float32, PAD)
            vw.check_padded(s, lid, "c_val4", idx, 6, torch.bfloat16, PAD)
            vw.check_padded(s, lid, "c_val4", idx, 6, torch.bfloat16, PAD,
                            affine=(scale, shift), expect_vals=exp)


@pytest.mark.parametrize("lid", vw.LAYOUT_IDS)
def test_get_graph_batch(lid):
    idx = vw.index_set(lid).numpy()
    for stored, out in ((torch.int64, torch.int64), (torch.int32, torch.int32)):
        name = "g_ei64" if stored == torch.int64 else "g_ei32"
        with vw.world(lid, "cpu", ["g_x", name]) as w:
            for s in readers(w, lid):
                vw.check_graph(s, lid, stored, out, idx, coo=True)
                vw.check_graph(s, lid, stored, out, idx, coo=False)


# ------------------------------------------------------------ column_stats
@pytest.mark.parametrize("lid", ["w9", "w128"])
def test_column_stats_merged(lid):
    full = vw.stats_array(lid)
    vals = vw.var_data(lid, "c_val4")[1].numpy()
    with vw.world(lid, "cpu", ["st", "c_val4"]) as w:
        for name, a, disp in (("st", full, 3), ("c_val4", vals, 4)):
            got = w.run(lambda s, r: s.column_stats(name))   # noqa: B023
            check_stats(got[0], a, disp)
            assert got[0].std[0] == 0.0 or name != "st"
            for cs in got[1:]:
                assert cs.count == got[0].count
                for x, y in zip(cs[1:], got[0][1:]):
                    assert torch.equal(x, y)     # identical on every rank
            for t in got[0][1:]:
                assert not torch.isnan(t).any()  # the empty parts injected nothing
        # a rank that holds nothing reports nothing, on its own
        lay = vw.LAYOUTS[lid]
        empty = w.stores[lay.readers()[1]].column_stats("st", local=True)
        assert empty.count == 0 and torch.isnan(empty.mean).all()
