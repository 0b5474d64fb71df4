"""MX block-scaled CSR variables on the host backend: ingest, get_csr and
get_csr_padded against the float64 model (tests/mx_ref.py) and cast_ref, bit
for bit (a NaN only has to be a NaN). The dataset and the request of
tests/test_gpu_csr_mx.py live here too."""
import numpy as np
import pytest
import torch

from ddstore_amd import DDStore
from tests import cast_ref, mx_ref

TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
# 44 samples: 0, 1, 2, one of 70 (whole passes of the gather plus a tail), the rest 3 to 33
LENS = np.array([0, 1, 2, 70, 3, 33, 5, 8, 13, 21, 4, 6, 7, 9, 10, 11, 12, 14, 15, 16, 17, 18,
                 19, 20, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 3, 0, 5, 1, 33, 2, 7, 9, 4])
NS = len(LENS)
GOFF = np.concatenate([[0], np.cumsum(LENS)])
# repeats, reversed order, two out-of-range values (positions 3 and 24)
IDX = np.concatenate([[3, 3, NS - 1, -1], np.arange(NS)[::-1][:20], [NS], np.arange(0, NS, 3)])


def request(idx, goff=GOFF):
    """Per requested sample: length (0 for a bad index), output offsets, and
    the stored element ids of each sample."""
    ok = (idx >= 0) & (idx < len(goff) - 1)
    g = np.where(ok, idx, 0)
    rlen = np.where(ok, goff[g + 1] - goff[g], 0)
    ids = [np.arange(goff[a], goff[a] + n) for a, n in zip(g, rlen)]
    return rlen, np.concatenate([[0], np.cumsum(rlen)]), ids


def model(dec_f32, kind, affine=None, fused=True):
    """Bits of decoded f32 elements through the optional affine (numbers or
    per-column float32 vectors; `fused`: the kernels' fma) and the cast."""
    if affine is None:
        return cast_ref.model_cast(dec_f32.view(np.uint32), "f32", kind)[0]
    if not fused:
        return cast_ref.model_affine_unfused(dec_f32.view(np.uint32), "f32", kind, *affine)[0]
    sc, sh = (np.broadcast_to(np.asarray(a, np.float32), dec_f32.shape).astype(np.float64)
              for a in affine)
    y = cast_ref.fma_f32(dec_f32.astype(np.float64), sc, sh)
    return cast_ref.model_cast(y.view(np.uint32), "f32", kind)[0]


bits = cast_ref.from_torch


def padded_model(enc, kind, idx, max_len, pad_value):
    """(n, max_len, disp) bits of a padded fetch; `enc` holds the model bits
    of every stored element."""
    rlen, _, ids = request(idx)
    pad = bits(torch.tensor([pad_value], dtype=TORCH[kind]), kind)[0]
    exp = np.full((len(idx), max_len, enc.shape[1]), pad, dtype=enc.dtype)
    for i, e in enumerate(ids):
        exp[i, :min(len(e), max_len)] = enc[e[:max_len]]
    return exp, rlen


def same(got, exp, kind):
    bad = cast_ref.mismatches(got, exp, np.ones(exp.shape, bool), kind)
    assert got.shape == exp.shape and bad.size == 0, (
        got.shape, exp.shape, bad[:5], got.reshape(-1)[bad[:5]], exp.reshape(-1)[bad[:5]])


@pytest.fixture()
def store():
    s = DDStore(device="cpu")
    yield s
    s.free()


@pytest.mark.parametrize("disp", (33, 128))
@pytest.mark.parametrize("elem", mx_ref.ELEMS)
def test_host_backend(store, elem, disp):
    x = mx_ref.inputs(int(GOFF[-1]), disp)
    packed = mx_ref.quantize(x, elem)
    dec = mx_ref.decode(packed, disp, elem)
    # ingest: add, and init + update at a sample offset
    store.add_csr_mx("v", torch.from_numpy(x.copy()).to(torch.bfloat16), LENS, elem)
    assert np.array_equal(store.local_shard("v").numpy(), mx_ref.quantize(
        torch.from_numpy(x.copy()).to(torch.bfloat16).float().numpy(), elem))
    store.init_csr_mx("u", LENS, disp, elem)
    store.update_csr_mx("u", x[:GOFF[5]])
    store.update_csr_mx("u", x[GOFF[5]:], offset=5)
    assert np.array_equal(store.local_shard("u").numpy(), packed)
    assert [store.query("u")[k] for k in ("mx_elem", "mx_disp", "row_bytes")] == [
        elem, disp, mx_ref.row_bytes(disp, elem)]
    # packed fetch (the host backend refuses a bad index)
    idx = IDX[(IDX >= 0) & (IDX < NS)]
    _, off, ids = request(idx)
    for kind in ("f32", "bf16", "f16"):
        vals, got_off = store.get_csr("u", idx, dtype=TORCH[kind])
        assert np.array_equal(got_off.numpy(), off)
        same(bits(vals, kind), model(dec[np.concatenate(ids)], kind), kind)
    cap = int(off[len(idx) // 2]) + 1      # cuts the request in the middle
    out = torch.full((cap + 2, disp), 7.0)
    store.get_csr("u", idx, out=out[:cap], affine=(0.5, 1.0))
    kept = int(off[(off[1:] <= cap).sum()])
    same(bits(out[:kept], "f32"),
         model(dec[np.concatenate(ids)[:kept]], "f32", (0.5, 1.0), fused=False), "f32")
    assert (out[kept:] == 7.0).all()
    # padded fetch, bad indices included
    for max_len in (8, 80):
        for kind, aff in (("f32", None), ("bf16", (1.7, -0.3)), ("f16", None)):
            dense, lengths = store.get_csr_padded("u", IDX, max_len, dtype=TORCH[kind],
                                                  affine=aff, pad_value=-1.5)
            exp, rlen = padded_model(model(dec, kind, aff, fused=False), kind, IDX, max_len, -1.5)
            assert np.array_equal(lengths.numpy(), rlen)
            same(bits(dense, kind), exp, kind)
    # the refused calls
    store.add_mx("fixed", x[:4], elem)
    store.add_csr("plain", x, LENS)
    for call in (lambda: store.update_csr("u", packed), lambda: store.update_mx("u", x),
                 lambda: store.update_csr_mx("plain", x), lambda: store.column_stats("u"),
                 lambda: store.get_csr("u", idx, dtype=torch.int32),
                 lambda: store.get_csr("plain", idx, dtype=torch.bfloat16),
                 lambda: store.get_csr("plain", idx, affine=(1.0, 0.0)),
                 lambda: store.get_csr("fixed", [0]),
                 lambda: store.get_csr_padded("fixed", [0], 4)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: store.get_batch("u", [0]), lambda: store.update("u", packed)):
        with pytest.raises((TypeError, RuntimeError)):
            call()
