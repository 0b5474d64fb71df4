"""MX block-scaled storage on the GPU: quantize_rows_mx and gather_rows_mx
against the float64 model (tests/mx_ref.py) and cast_ref, bit for bit (a NaN
only has to be a NaN)."""
import numpy as np
import pytest
import torch

from ddstore_amd import DDStore, PrefetchLoader, mx
from tests import cast_ref, mx_ref
from tests.virtual_world import VirtualWorld

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 257
DISPS = (1, 32, 33, 96, 128, 1000)
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
BITS = {"f32": torch.int32, "f16": torch.int16, "bf16": torch.int16}
SENT = 0x5A
# repeats, reversed order, two out-of-range values (positions 3 and 40)
IDX = np.concatenate([[5, 5, 256, -1], np.arange(N)[::-1][:36], [N], np.arange(0, N, 7)])
OOB = np.array([3, 40])


def _bits(t, kind):
    return t.cpu().view(BITS[kind]).numpy().view(cast_ref.BITS[kind])


def _expected(dec_f32, kind, affine=None):
    """Model bits of a fetch of decoded f32 rows; affine = (scale, shift)
    numbers or per-column float32 vectors."""
    if affine is None:
        return cast_ref.model_cast(dec_f32.view(np.uint32), "f32", kind)[0]
    sc = np.broadcast_to(np.asarray(affine[0], np.float32), dec_f32.shape)
    sh = np.broadcast_to(np.asarray(affine[1], np.float32), dec_f32.shape)
    y = cast_ref.fma_f32(dec_f32.astype(np.float64), sc.astype(np.float64),
                         sh.astype(np.float64))
    return cast_ref.model_cast(y.view(np.uint32), "f32", kind)[0]


def _check_fetch(store, name, dec, kind, affine=None, idx=IDX, oob=OOB):
    """get_batch into a sentinel-filled buffer: in-range rows equal the model,
    out-of-range rows are untouched."""
    out = torch.full((len(idx), dec.shape[1]), 0, dtype=TORCH[kind], device=DEV)
    out.view(torch.uint8).fill_(SENT)
    store.get_batch(name, idx, out=out, affine=affine)
    got = _bits(out, kind)
    ok = np.ones(len(idx), bool)
    ok[oob] = False
    exp = _expected(dec[idx[ok]], kind, affine)
    bad = cast_ref.mismatches(got[ok], exp, np.ones(exp.shape, bool), kind)
    assert bad.size == 0, (bad[:5], got[ok].reshape(-1)[bad[:5]], exp.reshape(-1)[bad[:5]])
    assert (out[torch.from_numpy(oob)].view(torch.uint8) == SENT).all()


@pytest.fixture()
def store():
    s = DDStore(device=DEV)
    yield s
    s.free()


@pytest.mark.parametrize("disp", DISPS)
@pytest.mark.parametrize("elem", mx_ref.ELEMS)
def test_ingest_and_fetch(store, elem, disp):
    x = mx_ref.inputs(N, disp)
    for src in ("f32", "f16", "bf16"):      # 1. packed shard == model
        with np.errstate(over="ignore"):
            t = torch.from_numpy(x.copy()).to(TORCH[src])
        store.add_mx(src, t.to(DEV) if src == "f16" else t, elem)
        packed = mx_ref.quantize(t.to(torch.float32).numpy(), elem)
        shard = store.local_shard(src).cpu().numpy()
        assert shard.shape == packed.shape and np.array_equal(shard, packed), \
            (src, np.argwhere(shard != packed)[:5])
    dec = mx_ref.decode(mx_ref.quantize(x, elem), disp, elem)
    for kind in ("f32", "bf16", "f16"):     # 2. fetch == cast of the model's decode
        _check_fetch(store, "f32", dec, kind)
    q = store.query("f32")
    assert q["oob_skipped"] == 6 and q["mx_elem"] == elem and q["mx_disp"] == disp
    assert q["bytes_gathered"] == 3 * len(IDX) * mx_ref.row_bytes(disp, elem)


@pytest.mark.parametrize("kind", ("f32", "bf16", "f16"))
@pytest.mark.parametrize("disp", (33, 128))
@pytest.mark.parametrize("elem", mx_ref.ELEMS)
def test_affine(store, elem, disp, kind):
    x = mx_ref.inputs(N, disp)
    store.add_mx("v", x, elem)
    dec = mx_ref.decode(mx_ref.quantize(x, elem), disp, elem)
    rng = np.random.default_rng(5)
    _check_fetch(store, "v", dec, kind, affine=(1.7, -0.3))
    cols = (rng.uniform(0.5, 2, disp).astype(np.float32),
            rng.uniform(-1, 1, disp).astype(np.float32))
    _check_fetch(store, "v", dec, kind, affine=cols)
    _check_fetch(store, "v", dec, kind, affine=(cols[0], 0.25))


@pytest.mark.parametrize("world,cuts", [(2, (0, 0, N)), (9, (0, 3, 3, 40, 41, 100, 101, 200, 250, N))])
@pytest.mark.parametrize("disp", (33, 96))      # element-wise kernel, tiled kernel
@pytest.mark.parametrize("elem", mx_ref.ELEMS)
def test_sharded(elem, disp, world, cuts):
    """2 shards, one empty; 9 shards: past DDS_DIR_KPARTS, the LDS directory."""
    x = mx_ref.inputs(N, disp)
    dec = mx_ref.decode(mx_ref.quantize(x, elem), disp, elem)
    with VirtualWorld(world, DEV, lambda s, r: s.add_mx(
            "v", torch.from_numpy(x[cuts[r]:cuts[r + 1]].copy()), elem)) as w:
        for r in (0, world - 1):
            for kind in ("f32", "bf16", "f16"):
                _check_fetch(w.stores[r], "v", dec, kind)
            assert w.stores[r].query("v")["oob_skipped"] == 6


def test_plumbing(store, tmp_path, monkeypatch):
    disp, elem = 128, "e4m3"
    x = mx_ref.inputs(N, disp)
    dec = mx_ref.decode(mx_ref.quantize(x, elem), disp, elem)
    idx = np.arange(N)
    none = np.array([], np.int64)
    # update_mx at an offset, host array larger than one staging piece
    monkeypatch.setattr(mx, "STAGE_BYTES", 7 * disp * 4)
    store.init_mx("v", N, disp, elem)
    store.update_mx("v", x[:10])
    store.update_mx("v", np.asfortranarray(x[10:]), offset=10)   # not C-contiguous
    _check_fetch(store, "v", dec, "f32", idx=idx, oob=none)
    # gather_into
    out = torch.empty((N, disp), dtype=torch.bfloat16, device=DEV)
    store.gather_into("v", torch.arange(N, device=DEV), out)
    exp = _expected(dec, "bf16")
    assert cast_ref.mismatches(_bits(out, "bf16"), exp, np.ones(exp.shape, bool), "bf16").size == 0
    # PrefetchLoader
    got = torch.cat([b.clone() for b in PrefetchLoader(
        store, "v", idx, batch_size=100, out_dtype=torch.bfloat16)])
    assert cast_ref.mismatches(_bits(got, "bf16"), exp, np.ones(exp.shape, bool), "bf16").size == 0
    # the refused calls
    for call in (lambda: store.update("v", np.zeros((1, 144), np.uint8)),
                 lambda: store.column_stats("v"),
                 lambda: store.get_csr("v", [0]),
                 lambda: store.get_csr_padded("v", [0], 4),
                 lambda: store.get_graph_batch("v", "v", [0]),
                 lambda: store.get_batch("v", [0], dtype=torch.int32),
                 lambda: store.gather_into("v", torch.arange(1, device=DEV),
                                           torch.empty((1, disp), dtype=torch.int64, device=DEV))):
        with pytest.raises(TypeError):
            call()
    # reshuffle, then dump / load: the decoded rows survive as a set and as bits
    store.reshuffle("v", seed=3)
    perm = torch.randperm(N, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV).cpu().numpy()
    _check_fetch(store, "v", dec[perm], "f32", idx=idx, oob=none)
    store.dump("v", str(tmp_path / "v.pt"))
    fresh = DDStore(device=DEV)
    try:
        fresh.load("v", str(tmp_path / "v.pt"))
        assert fresh.query("v")["mx_elem"] == elem
        _check_fetch(fresh, "v", dec[perm], "bf16", idx=idx, oob=none)
    finally:
        fresh.free()
