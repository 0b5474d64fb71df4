"""Every gather kernel's owner lookup on directories of 4 to 128 shards.

Each fetch kernel carries its own copy of the step "index -> owning shard ->
pointer into that shard". The worlds here come from the thread-per-rank
harness of ``tests/virtual_world.py`` (W stores in this process, peers as
plain device pointers), its layout table puts empty shards in front, between
and behind the owners, a shard with samples and no elements, slot 7 of the
kernel-argument directory and shard 127, and every check is the one
``tests/test_many_shards_cpu.py`` has already run on the host backend. What
each test reaches:

* ``test_tiled``: k_gather_tiled, the kernel-argument compare chain for
  W <= 8 and LdsDir + binary search for W >= 9;
* ``test_oneshot``: k_gather_oneshot (LdsDir) in its 16-B, element-wise and
  byte-move forms;
* ``test_csr_alloc``: csr_lens + k_gather_csr_wave (two prefixes);
* ``test_csr_out``: k_csr_plan3 packing the owner into a descriptor and
  k_gather_csr_items unpacking it, owner 127 included;
* ``test_padded``: k_gather_csr_padded and count_padded (LdsDir<..., 2>);
* ``test_graph``: k_gather_csr_relabel, once per variable;
* ``test_ranges_and_stats``: owner_of_host behind get_range, and the merge
  of column_stats over parts with count 0.

Data is self-verifying: byte-moved rows encode (owner, local row, column) in
every element, converted rows hold small integers that every float format
holds exactly (the roundings are test_gpu_cast_numerics.py's business).
Every output lies in a sentinel-filled buffer; rows of bad indices and the
guard bytes must keep the sentinel and the counters must grow by exactly the
number of bad indices. One 9-process world over real hipIpc holds the two
kinds of world to the same model. Run with ``pytest -m gpu``."""
import os
import struct
import subprocess
import sys

import pytest
import torch

from tests import graph_ref
from tests import virtual_world as vw
from tests.dist_utils import run_dist
from tests.test_column_stats_cpu import check as check_stats
from tests.test_column_stats_cpu import col_params

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
PAD = -3
ALL = list(vw.FIXED) + list(vw.CSR) + list(vw.GRAPH)


@pytest.fixture(scope="module", params=vw.LAYOUT_IDS)
def world(request):
    """(layout id, world) with every variable registered; one world per
    layout for the whole module."""
    lid = request.param
    with vw.world(lid, DEV, ALL) as w:
        assert all(s.mode == "hip" and s.size == vw.LAYOUTS[lid].W for s in w.stores), \
            "GPU test must exercise the native HIP path"
        yield lid, w


def readers(w, lid):
    return [w.stores[r] for r in vw.LAYOUTS[lid].readers()]


# ------------------------------------------------------------ fixed stride
def test_tiled(world):
    """Rows of 128 f32: 16 (cast to bf16) and 32 (byte move) 16-B chunks per
    row, both at or above the tiled kernel's 8."""
    lid, w = world
    assert os.environ.get("DDSTORE_GATHER_DIR") != "lds", \
        "the kernel-argument directory must not be switched off here"
    assert os.environ.get("DDSTORE_GATHER_KERNEL") in (None, "tiled")
    idx = vw.index_set(lid, bad=True)
    for s in readers(w, lid):
        vw.check_batch(s, lid, "val128", idx, torch.bfloat16)
        vw.check_batch(s, lid, "enc128", idx)


def test_oneshot(world):
    lid, w = world
    idx = vw.index_set(lid, bad=True)
    for s in readers(w, lid):
        vw.check_batch(s, lid, "val8", idx, torch.bfloat16)     # one 16-B chunk per row
        vw.check_batch(s, lid, "val5", idx, torch.bfloat16)     # element-wise
        # an output view offset by one element: element-wise again
        vw.check_batch(s, lid, "val8", idx, torch.bfloat16, byte_offset=2)
        vw.check_batch(s, lid, "val5", idx, torch.float32, byte_offset=4)
        vw.check_batch(s, lid, "u8x7", idx)                     # odd row bytes
        vw.check_batch(s, lid, "enc_i64", idx)                  # 16-B byte move


@pytest.mark.parametrize("lid,per_column", [("w8", False), ("w9", True)])
def test_affine(lid, per_column):
    """Only the transform differs from test_tiled, not the directory: the
    scalar affine on the kernel-argument chain, the per-column one on the LDS
    search."""
    idx = vw.index_set(lid, bad=True)
    scale, shift = col_params(128) if per_column else (0.0234375, -1.5)
    exp = vw.affine_model(vw.var_data(lid, "val128")[1], "bf16", scale, shift, fused=True)
    with vw.world(lid, DEV, ["val128"]) as w:
        for s in readers(w, lid):
            vw.check_batch(s, lid, "val128", idx, torch.bfloat16, affine=(scale, shift),
                           expect_full=exp)


_LDS_CODE = """
import sys
sys.path.insert(0, {root!r})
from tests import virtual_world as vw
with vw.world("w8", "cuda:0", ["val128", "enc128"]) as w:
    assert all(s.mode == "hip" for s in w.stores)
    print("DIGEST", vw.tiled_digest(w, "w8", True))
print("CHILD-OK")
"""


def test_w8_kernel_argument_and_lds_directory_agree():
    """All 8 slots of the kernel-argument directory in use, slot 7 an empty
    shard behind the last owner: the compare chain and the LDS binary search
    (a child process with DDSTORE_GATHER_DIR=lds) must write the same bytes,
    each checked against the model on the way."""
    assert os.environ.get("DDSTORE_GATHER_DIR") != "lds"
    env = {e: v for e, v in os.environ.items() if not e.startswith("DDSTORE_GATHER_")}
    env["DDSTORE_GATHER_DIR"] = "lds"
    child = subprocess.Popen([sys.executable, "-c", _LDS_CODE.format(root=ROOT)],
                             env=env, cwd=ROOT, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
    try:
        with vw.world("w8", DEV, ["val128", "enc128"]) as w:
            mine = vw.tiled_digest(w, "w8", True)
    finally:
        so, se = child.communicate(timeout=300)
    assert child.returncode == 0, se
    assert "CHILD-OK" in so, so
    theirs = [ln.split()[1] for ln in so.splitlines() if ln.startswith("DIGEST")]
    assert theirs == [mine]


# --------------------------------------------------------------------- CSR
def test_csr_alloc(world):
    """get_csr without out, in the wave kernel's three copy units: 16-B
    elements, dwords, bytes."""
    lid, w = world
    idx = vw.index_set(lid, bad=True)
    for s in readers(w, lid):
        for name in ("c_f32x4", "c_f32x1", "c_u8x3"):
            vw.check_csr_alloc(s, lid, name, idx)


def test_csr_out(world):
    """get_csr(out=): the last non-empty shard's three-item sample puts its
    owner (7 in w8_last, 127 in w128 and w128_last) into descriptors; at the
    exact capacity and with the capacity cut inside that sample, dword and
    byte kernel."""
    lid, w = world
    idx = vw.index_set(lid, bad=True)
    for s in readers(w, lid):
        for name in ("c_f32x1", "c_u8x3"):
            f = vw.check_csr_out(s, lid, name, idx)
            assert s.query(name)["cap_skipped"] == 0
            dword = f.eb % 4 == 0 and f.out.data_ptr() % 4 == 0
            assert dword == (name == "c_f32x1")
            f = vw.check_csr_out(s, lid, name, idx, cut=True)
            assert s.query(name)["cap_skipped"] > 0 and f.cap < int(f.off[-1])
            s.reset_counters(name)


def test_padded(world):
    lid, w = world
    idx = vw.index_set(lid, bad=True)
    scale, shift = col_params(4)
    exp = vw.affine_model(vw.var_data(lid, "c_val4")[1], "bf16", scale, shift, fused=True)
    for s in readers(w, lid):
        vw.check_padded(s, lid, "c_val4", idx, 6, torch.float32, PAD)
        vw.check_padded(s, lid, "c_val4", idx, 6, torch.bfloat16, PAD)
        vw.check_padded(s, lid, "c_val4", idx, 6, torch.bfloat16, PAD,
                        affine=(scale, shift), expect_vals=exp)


def test_graph(world):
    lid, w = world
    idx = vw.index_set(lid, bad=True).numpy()
    for s in readers(w, lid):
        for stored, out in graph_ref.DTYPE_PAIRS:
            for coo in (True, False):
                vw.check_graph(s, lid, stored, out, idx, coo)


# ------------------------------------------------- get_range, column_stats
def test_ranges_and_stats(world):
    lid, w = world
    for s in readers(w, lid):
        vw.check_ranges(s, lid, "enc128")       # device to device
    for name, a, disp in (("st", vw.stats_array(lid), 3),
                          ("c_val4", vw.var_data(lid, "c_val4")[1].numpy(), 4)):
        got = w.run(lambda s, r: s.column_stats(name))   # noqa: B023
        check_stats(got[0], a, disp)
        for cs in got[1:]:
            assert cs.count == got[0].count
            for x, y in zip(cs[1:], got[0][1:]):
                assert torch.equal(x, y)         # identical on every rank
        for t in got[0][1:]:
            assert not torch.isnan(t).any()      # parts with count 0 injected nothing


# ------------------------------------------------------ same-process peers
def test_open_peers_refuses_a_foreign_pid():
    from ddstore_amd import _C

    be = _C.DeviceStore(0, 0, 2)
    t = torch.arange(8, dtype=torch.float32).reshape(4, 2)
    be.add("v", t, 4, 2, [4, 4])
    ptr = be.base_ptr("v")
    assert ptr == be.local_shard("v").data_ptr()
    try:
        with pytest.raises(RuntimeError, match="written by pid"):
            be.open_peers("v", [b"", struct.pack("=qQ", os.getpid() + 1, ptr)])
        with pytest.raises(RuntimeError, match="bad handle bytes"):
            be.open_peers("v", [b"", struct.pack("=qQQ", os.getpid(), ptr, 0)])
        # this process's own entry is taken as it is: rank 1's rows are ours
        be.open_peers("v", [b"", struct.pack("=qQ", os.getpid(), ptr)])
        out = torch.zeros(2, 2, device=DEV)
        be.gather("v", torch.tensor([5, 2], device=DEV), out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), t[[1, 2]])
    finally:
        be.free_all()


# ------------------------------------------------- real hipIpc, nine shards
def _w_nine(rank, world):
    from ddstore_amd import DDStore

    lid = "w9"
    s = DDStore(device=DEV)
    try:
        assert s.mode == "hip" and s.size == 9 and s.comm.same_process is False
        vw.register(lid, ["enc128", "val128", "c_f32x1", "c_u8x3"])(s, rank)
        if rank in (0, 4, 8):
            idx = vw.index_set(lid, bad=True)
            vw.check_batch(s, lid, "val128", idx, torch.bfloat16)
            vw.check_batch(s, lid, "enc128", idx)
            for name in ("c_f32x1", "c_u8x3"):
                vw.check_csr_out(s, lid, name, idx)
                vw.check_csr_out(s, lid, name, idx, cut=True)
    finally:
        s.comm.barrier()  # no rank frees its shard while another still reads it
        s.free()


def test_nine_processes_one_gpu():
    """The w9 layout once more with one process per rank and IPC handles:
    the same checks and the same model as the same-process world."""
    run_dist(_w_nine, 9)
