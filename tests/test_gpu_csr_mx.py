"""MX block-scaled CSR variables on the GPU: update_csr_mx and the fused dequantizing
fetches (k_gather_csr_mx, both placements, and its element-wise fallback), bit for bit
against the models, dataset and request of tests/test_csr_mx_cpu.py."""
import numpy as np
import pytest
import torch

from ddstore_amd import DDStore, GraphPrefetchLoader, PrefetchLoader, mx
from tests import mx_ref
from tests.test_csr_mx_cpu import (GOFF, IDX, LENS, NS, TORCH, bits, model, padded_model,
                                   request, same)
from tests.virtual_world import VirtualWorld

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0x5A
KINDS = ("f32", "bf16", "f16")
T = int(GOFF[-1])


@pytest.fixture()
def store():
    s = DDStore(device=DEV)
    yield s
    s.free()


def _data(disp, elem):
    x = mx_ref.inputs(T, disp)
    return x, mx_ref.decode(mx_ref.quantize(x, elem), disp, elem)


def _sentinel(shape, kind):
    out = torch.empty(shape, dtype=TORCH[kind], device=DEV)
    out.view(torch.uint8).fill_(SENT)
    return out


def _check_packed(store, name, dec, kind, cap=None, affine=None, idx=IDX, like=None):
    """get_csr(out=) into `cap` sentinel-filled rows (+2 of slack): kept samples equal the
    model, the rest is untouched. `like`: the request in the stored samples the model knows."""
    rlen, off, ids = request(idx if like is None else like)
    cap = int(off[-1]) if cap is None else cap
    buf = _sentinel((cap + 2, dec.shape[1]), kind)
    _, got_off = store.get_csr(name, idx, out=buf[:cap], dtype=TORCH[kind], affine=affine)
    assert np.array_equal(got_off.cpu().numpy(), off)      # unclamped
    k = int((off[1:] <= cap).sum())                        # the kept prefix
    rows = np.concatenate(ids[:k] + [np.empty(0, np.int64)]).astype(np.int64)
    same(bits(buf[:off[k]], kind), model(dec[rows], kind, affine), kind)
    assert (buf[off[k]:].view(torch.uint8) == SENT).all()
    return int((rlen[k:] > 0).sum()), int(off[k])           # dropped samples, kept elements


def _check_padded(store, name, dec, kind, max_len, affine=None):
    dense = _sentinel((len(IDX), max_len, dec.shape[1]), kind)
    _, lengths = store.get_csr_padded(name, IDX, max_len, out=dense, affine=affine,
                                      pad_value=-1.5)
    exp, rlen = padded_model(model(dec, kind, affine), kind, IDX, max_len, -1.5)
    assert np.array_equal(lengths.cpu().numpy(), rlen)
    same(bits(dense, kind), exp, kind)                      # so no sentinel byte is left
    return int(np.minimum(rlen, max_len).sum())


@pytest.mark.parametrize("disp", (1, 33, 96, 128))
@pytest.mark.parametrize("elem", mx_ref.ELEMS)
def test_ingest(store, elem, disp, monkeypatch):
    x = mx_ref.inputs(T, disp)
    for src in KINDS:
        with np.errstate(over="ignore"):
            t = torch.from_numpy(x.copy()).to(TORCH[src])
        store.add_csr_mx(src, t.to(DEV) if src == "f16" else t, LENS, elem)
        packed = mx_ref.quantize(t.to(torch.float32).numpy(), elem)
        shard = store.local_shard(src).cpu().numpy()
        assert shard.shape == packed.shape and np.array_equal(shard, packed), \
            (src, np.argwhere(shard != packed)[:5])
    # at a sample offset, a host array larger than one staging piece
    monkeypatch.setattr(mx, "STAGE_BYTES", 7 * disp * 4)
    store.init_csr_mx("u", LENS, disp, elem)
    store.update_csr_mx("u", x[:GOFF[5]])
    store.update_csr_mx("u", np.asfortranarray(x[GOFF[5]:]), offset=5)
    assert np.array_equal(store.local_shard("u").cpu().numpy(), mx_ref.quantize(x, elem))
    assert store.query("u")["row_bytes"] == mx_ref.row_bytes(disp, elem)


@pytest.mark.parametrize("disp", (1, 33, 96, 128, 256))    # 256: the 64-lane group
@pytest.mark.parametrize("elem", mx_ref.ELEMS)
def test_packed_and_capacity(store, elem, disp):
    x, dec = _data(disp, elem)
    store.add_csr_mx("v", x, LENS, elem)
    rb = mx_ref.row_bytes(disp, elem)
    for kind in KINDS:
        assert _check_packed(store, "v", dec, kind) == (0, request(IDX)[1][-1])
    q = store.query("v")
    assert q["oob_skipped"] == 6 and q["cap_skipped"] == 0
    assert q["bytes_gathered"] == 3 * request(IDX)[1][-1] * rb
    # a capacity that cuts the request in the middle; values without out=
    store.reset_counters("v")
    cap = int(request(IDX)[1][len(IDX) // 2]) + 1
    dropped, kept = _check_packed(store, "v", dec, "bf16", cap=cap)
    q = store.query("v")
    assert dropped > 0 and q["cap_skipped"] == dropped and q["bytes_gathered"] == kept * rb
    vals, _ = store.get_csr("v", IDX)
    same(bits(vals, "f32"), model(dec[np.concatenate(request(IDX)[2])], "f32"), "f32")


@pytest.mark.parametrize("max_len", (8, 80))
@pytest.mark.parametrize("disp", (33, 96, 128, 256))
@pytest.mark.parametrize("elem", mx_ref.ELEMS)
def test_padded(store, elem, disp, max_len):
    x, dec = _data(disp, elem)
    store.add_csr_mx("v", x, LENS, elem)
    rng = np.random.default_rng(5)
    cols = (rng.uniform(0.5, 2, disp).astype(np.float32),
            rng.uniform(-1, 1, disp).astype(np.float32))
    taken = 0
    for kind in KINDS:
        for affine in (None, (1.7, -0.3), cols):
            taken += _check_padded(store, "v", dec, kind, max_len, affine)
            if affine is not None:
                _check_packed(store, "v", dec, kind, affine=affine)
    q = store.query("v")
    assert q["bytes_gathered"] == (taken + 6 * request(IDX)[1][-1]) * mx_ref.row_bytes(disp, elem)
    assert q["oob_skipped"] == 2 * 15


# 2 shards, one empty; 9 shards
@pytest.mark.parametrize("world,cuts", [(2, (0, 0, NS)), (9, (0, 3, 3, 10, 11, 20, 21, 30, 40, NS))])
@pytest.mark.parametrize("disp", (33, 96))      # element-wise kernel, vector kernel
@pytest.mark.parametrize("elem", mx_ref.ELEMS)
def test_sharded(elem, disp, world, cuts):
    x, dec = _data(disp, elem)
    with VirtualWorld(world, DEV, lambda s, r: s.add_csr_mx(
            "v", torch.from_numpy(x[GOFF[cuts[r]]:GOFF[cuts[r + 1]]].copy()),
            LENS[cuts[r]:cuts[r + 1]], elem)) as w:
        for r in (0, world - 1):
            for kind in KINDS:
                _check_packed(w.stores[r], "v", dec, kind)
                _check_padded(w.stores[r], "v", dec, kind, 8)
            assert w.stores[r].query("v")["oob_skipped"] == 12


def _eq(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_graph_batch_and_loaders(store):
    disp, bf16 = 128, torch.bfloat16
    x, _ = _data(disp, "e4m3")
    rng = np.random.default_rng(7)
    edges = np.concatenate([rng.integers(0, n, (2 * n, 2)) for n in LENS if n] ).astype(np.int64)
    store.add_csr_mx("x", x, LENS, "e4m3")
    store.add_csr("xf", x, LENS)
    store.add_csr("e", edges, 2 * LENS)
    gb = store.get_graph_batch("x", "e", IDX, x_dtype=bf16)
    tw = store.get_graph_batch("xf", "e", IDX)
    assert _eq(gb.x, store.get_csr("x", IDX, dtype=bf16)[0])
    assert all(_eq(getattr(gb, f), getattr(tw, f)) for f in ("ptr", "batch", "edge_index", "edge_ptr"))
    order = np.arange(NS)[::-1].copy()
    batches = [order[i:i + 16] for i in range(0, NS, 16)]
    for b, (vals, off) in zip(batches, PrefetchLoader(store, "x", order, 16, out_dtype=bf16)):
        ref, roff = store.get_csr("x", b, dtype=bf16)
        assert _eq(off, roff) and _eq(vals[:ref.shape[0]], ref)
    for b, (dense, lengths) in zip(batches, PrefetchLoader(store, "x", order, 16,
                                                           out_dtype=bf16, pad_to=8)):
        ref, rlen = store.get_csr_padded("x", b, 8, dtype=bf16)
        assert _eq(dense, ref) and _eq(lengths, rlen)
    for b, g in zip(batches, GraphPrefetchLoader(store, "x", "e", order, 16, x_dtype=bf16)):
        ref = store.get_graph_batch("x", "e", b, x_dtype=bf16)
        n = ref.x.shape[0]
        assert _eq(g.x[:n], ref.x) and _eq(g.ptr, ref.ptr) and _eq(g.batch[:n], ref.batch)


def test_refusals_dump_load_reshuffle(store, tmp_path):
    disp, elem = 96, "e2m1"
    x, dec = _data(disp, elem)
    store.add_csr_mx("v", x, LENS, elem)
    store.add_mx("fixed", x[:4], elem)
    store.add_csr("plain", x, LENS)
    store.add_csr("e", np.zeros((T, 2), np.int64), LENS)
    for call in (lambda: store.update_csr("v", x), lambda: store.column_stats("v"),
                 lambda: store.get_csr_padded("v", IDX, 4, dtype=torch.int32),
                 lambda: store.get_graph_batch("e", "v", IDX),
                 lambda: store.get_graph_batch("plain", "e", IDX, x_dtype=torch.bfloat16),
                 lambda: store.get_graph_batch("fixed", "e", [0])):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: store.get_batch("v", [0]),
                 lambda: store.update("v", x),
                 lambda: store.gather_into("v", torch.arange(1, device=DEV),
                                           torch.empty((1, disp), device=DEV))):
        with pytest.raises((TypeError, RuntimeError)):
            call()
    # reshuffle, then dump / load: sample j is the old sample perm[j], bit for bit
    store.reshuffle("v", seed=3)
    perm = torch.randperm(NS, generator=torch.Generator(device=DEV).manual_seed(3),
                          device=DEV).cpu().numpy()
    every = np.arange(NS)
    assert store.query("v")["mx_elem"] == elem
    _check_packed(store, "v", dec, "f32", idx=every, like=perm)
    store.dump("v", str(tmp_path / "v.pt"))
    fresh = DDStore(device=DEV)
    fresh.load("v", str(tmp_path / "v.pt"))
    assert fresh.query("v")["mx_disp"] == disp
    _check_packed(fresh, "v", dec, "bf16", idx=every, like=perm)
    fresh.free()
