"""Per-column normalization on the GPU: ``column_stats`` against NumPy
float64 and the per-column ``affine=`` of ``get_batch``, ``get_csr_padded``
and ``PrefetchLoader`` bit for bit against ``cast_ref.model_affine`` applied
column by column. Run with ``pytest -m gpu``.

Tolerances of the statistics (u = 2^-53, n = count): summation in any order
errs by at most (n - 1) u sum|x_i|, so |mean - ref| <= 4 n u max|x|; the
shifted sum of squares cancels by 1 + (mean - pivot)^2 / var, small for a
pivot taken from the data, so |std - ref| <= 64 n u ref; min and max are
exact. ``test_column_stats_cpu.py::test_bounds_hold_for_the_worst_pivot``
checks on the CPU that a shifted sum with the worst in-data pivot meets both
on the data used here, and that the raw-moment form does not."""
import numpy as np
import pytest
import torch

from tests import cast_ref
from tests.test_column_stats_cpu import (TORCH_KINDS, cancellation_data, check, col_params,
                                         make_t)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = "cuda:0"


@pytest.fixture
def store():
    from ddstore_amd import DDStore

    s = DDStore(device=DEV)
    assert s.mode == "hip", "GPU test must exercise the native HIP path"
    yield s
    s.free()


# ------------------------------------------------------------- column_stats
# R = 5000 with D = 1000 runs many blocks; D = 1000 is beyond the 512 columns
# one block covers for 8-byte types (blocks own column ranges) and inside the
# 1024 / 2048 it covers for the others (a partial second replica); D = 1, 3, 8
# fold up to 2048 slots of a block into one column.
@pytest.mark.parametrize("kind", list(TORCH_KINDS))
def test_column_stats_shapes(store, kind):
    for rows in (0, 1, 257, 5000):
        for disp in (1, 3, 8, 128, 1000):
            name = f"v{rows}_{disp}"
            t, x = make_t(kind, rows, disp)
            if rows:
                store.add(name, t)
            else:
                store.init(name, 0, disp, dtype=TORCH_KINDS[kind])
            cs = store.column_stats(name)
            check(cs, x.reshape(rows, disp), disp)
            if rows:
                assert cs.std[0] == 0.0 and cs.mean[0] == x[0, 0], (rows, disp)


def test_column_split_image_rows(store):
    # a whole image per row: columns are split across blocks
    disp = 150528
    a = np.random.default_rng(8).integers(0, 256, (3, disp)).astype(np.uint8)
    store.add("img", a)
    check(store.column_stats("img"), a, disp)


@pytest.mark.parametrize("disp", [1, 3])
def test_column_stats_csr(store, disp):
    lens = np.random.default_rng(3).integers(0, 10, 64)
    lens[0] = 0
    t, x = make_t("f32", int(lens.sum()), disp)
    store.add_csr("c", t, lens)
    cs = store.column_stats("c")
    assert cs.count == int(lens.sum())
    check(cs, x, disp)


def test_cancellation(store):
    a = cancellation_data()
    store.add("v", a)
    cs = store.column_stats("v")
    check(cs, a, 3)
    # the bound is far below what the raw-moment form loses
    ref = np.sqrt(((a[:, 1].astype(np.longdouble) - a[:, 1].astype(np.longdouble).mean())
                   ** 2).mean())
    assert abs(float(cs.std[1]) - float(ref)) <= 64 * 4096 * 2.0 ** -53 * float(ref)


def test_determinism_nan_constant_counters(store):
    t, x = make_t("f32", 5000, 128)
    x = x.copy()
    t[4321, 5] = float("nan")
    x[4321, 5] = np.nan
    store.add("v", t)
    idx = torch.arange(64, device=DEV)
    store.get_batch("v", idx)
    before = store.query("v")
    a = store.column_stats("v")
    b = store.column_stats("v")
    c = store.column_stats("v", local=True)
    for p, q, r in zip(a[1:], b[1:], c[1:]):   # bit-identical
        assert torch.equal(p.view(torch.int64), q.view(torch.int64))
        assert torch.equal(p.view(torch.int64), r.view(torch.int64))
    assert a.count == b.count == 5000
    for s in (a.mean, a.std, a.min, a.max):
        assert torch.isnan(s[5]) and int(torch.isnan(s).sum()) == 1
    assert a.std[0] == 0.0
    check(a, x, 128)
    after = store.query("v")
    for key in ("n_gather", "rows_gathered", "bytes_gathered", "oob_skipped",
                "cap_skipped"):
        assert before[key] == after[key], key


def test_inf_keeps_min_max(store):
    a = np.random.default_rng(2).standard_normal((300, 3)).astype(np.float32)
    a[7, 1], a[9, 1] = np.inf, -np.inf
    store.add("v", a)
    cs = store.column_stats("v")
    assert cs.min[1] == -np.inf and cs.max[1] == np.inf
    assert not torch.isfinite(cs.mean[1]) and not torch.isfinite(cs.std[1])
    assert torch.isfinite(cs.mean[0]) and torch.isfinite(cs.std[2])


# ------------------------------------------------- per-column affine, fixed
def model_cols(bits, in_kind, out_kind, scale, shift):
    """cast_ref.model_affine, one call per column."""
    out = np.empty(bits.shape, dtype=cast_ref.BITS[out_kind])
    for c in range(bits.shape[-1]):
        out[..., c], _ = cast_ref.model_affine(
            bits[..., c], in_kind, out_kind, float(scale[c]), float(shift[c]))
    return out


def assert_model(got, exp, out_kind, msg=""):
    bad = cast_ref.mismatches(cast_ref.from_torch(got, out_kind).reshape(-1), exp,
                              np.ones(exp.size, bool), out_kind)
    assert bad.size == 0, (msg, bad[:8])


def table_rows(in_kind, disp, max_rows=512):
    """The affine table as rows of `disp`: consecutive table entries sit in
    different columns, so each meets a different (scale, shift)."""
    rows = cast_ref.as_rows(cast_ref.affine_table(in_kind), disp)
    return rows[:: max(1, rows.shape[0] // max_rows)][:max_rows]


@pytest.mark.parametrize("out_kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("in_kind", ["u8", "f16", "bf16", "f32", "e4m3"])
def test_get_batch_vector_affine(store, in_kind, out_kind):
    odt = cast_ref.torch_dtype(out_kind)
    # tiled (96 rows: whole groups of passes, the tile of the skipped row goes
    # pass by pass; 101 rows: a partial last tile); one-shot with VEC > 1, VEC = 1
    for disp, n in ((128, 96), (128, 101), (8, 40), (3, 40)):
        rows = table_rows(in_kind, disp)
        name = f"t{disp}_{n}"
        store.add(name, cast_ref.to_torch(rows, in_kind))
        idx = np.random.default_rng(disp).integers(0, rows.shape[0], n)
        idx[11] = rows.shape[0]          # out of range: the row is skipped
        scale, shift = col_params(disp)
        sentinel = torch.full((n, disp), 7.0, dtype=odt, device=DEV)
        got = store.get_batch(name, idx, out=sentinel, affine=(scale, shift))
        torch.cuda.synchronize()
        assert got.data_ptr() == sentinel.data_ptr()
        keep = np.arange(n) != 11
        exp = model_cols(rows[idx[keep]], in_kind, out_kind, scale, shift)
        assert_model(got[torch.from_numpy(keep)], exp.reshape(-1), out_kind,
                     (in_kind, out_kind, disp))
        assert (got[11] == 7.0).all()
        assert store.query(name)["oob_skipped"] == 1
        store.reset_counters(name)


def test_f16_output_rounds_twice(store):
    """fma to f32, then f32 to f16: on columns where rounding the exact sum
    straight to f16 gives other bits, the fetch gives the model's."""
    disp = 128
    rows = table_rows("f32", disp)
    # The table holds the f16 midpoints. A power-of-two scale keeps them
    # midpoints and a shift far below half an f32 ulp nudges the exact sum off
    # the tie: rounding once to f16 follows the nudge, rounding to f32 first
    # lands on the tie again and goes to even. Different in every column.
    k = np.arange(disp)
    scale = (2.0 ** (k % 3 - 1)).astype(np.float32)
    shift = ((-1.0) ** k * 2.0 ** -(30 + k % 5) * (1 + k / 1024)).astype(np.float32)
    x = cast_ref._f32_values(rows, "f32")
    with np.errstate(all="ignore"):
        exact = x * scale.astype(np.float64) + shift.astype(np.float64)
    once = cast_ref.round_to_format(
        *cast_ref.decode(exact.view(np.uint64), "f64"), "f16").astype(np.uint16)
    twice = model_cols(rows, "f32", "f16", scale, shift)
    differ = (once != twice) & ~cast_ref.is_nan_bits(twice, "f16")
    assert differ.any(), "the table does not separate the two roundings"
    store.add("v", cast_ref.to_torch(rows, "f32"))
    got = store.get_batch("v", np.arange(rows.shape[0]), dtype=torch.float16,
                          affine=(scale, shift))
    gb = cast_ref.from_torch(got, "f16").reshape(twice.shape)
    assert (gb[differ] == twice[differ]).all()
    assert_model(got, twice.reshape(-1), "f16")


def test_device_vectors_are_used_without_sync(store):
    disp = 128
    rows = table_rows("u8", disp)
    store.add("v", cast_ref.to_torch(rows, "u8"))
    scale, shift = col_params(disp)
    ds = torch.from_numpy(scale).to(DEV)
    dh = torch.from_numpy(shift).to(DEV)
    assert store.prepare_affine("v", (ds, dh))[0].data_ptr() == ds.data_ptr()
    idx = torch.arange(rows.shape[0], device=DEV)
    out = torch.empty((rows.shape[0], disp), dtype=torch.bfloat16, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        store.get_batch("v", idx, out=out, affine=(ds, dh))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert_model(out, model_cols(rows, "u8", "bf16", scale, shift).reshape(-1), "bf16")
    with pytest.raises(ValueError):
        store.get_batch("v", idx, dtype=torch.bfloat16, affine=(ds[:-1], dh))
    with pytest.raises(TypeError):
        store.get_batch("v", idx, dtype=torch.int32, affine=(ds, dh))


def test_scalar_affine_unchanged(store):
    disp = 128
    rows = table_rows("f16", disp)
    store.add("v", cast_ref.to_torch(rows, "f16"))
    idx = np.arange(rows.shape[0])
    for odt in (torch.float32, torch.float16, torch.bfloat16):
        a = store.get_batch("v", idx, dtype=odt, affine=(2.0, -1.0))
        b = store.get_batch("v", idx, dtype=odt,
                            affine=(np.full(disp, 2.0, np.float32), torch.full((disp,), -1.0)))
        c = store.get_batch("v", idx, dtype=odt, affine=(2.0, np.full(disp, -1.0)))
        torch.cuda.synchronize()
        ai = a.view(torch.int16 if a.element_size() == 2 else torch.int32)
        for other in (b, c):
            assert torch.equal(ai, other.view(ai.dtype))


# ------------------------------------------------ per-column affine, padded
NS, NI, L, PAD = 64, 40, 6, -3


def _lens():
    lens = np.random.default_rng(0).integers(0, 10, NS)
    lens[0], lens[1] = 0, 9
    return lens


LENS = _lens()
IDX = np.random.default_rng(1).integers(0, NS, NI)
IDX[5], IDX[6], IDX[7] = 0, 1, NS      # empty, truncated, out of range
GOFF = np.concatenate([[0], np.cumsum(LENS)])


def padded_values(in_kind, disp):
    n = int(LENS.sum())
    tbl = cast_ref.affine_table(in_kind)
    pick = np.random.default_rng(disp).integers(0, tbl.size, n * disp)
    return tbl[pick].reshape(n, disp)


def padded_model(bits, in_kind, out_kind, idx, scale, shift, L=L):
    disp = bits.shape[1]
    pad = cast_ref.from_torch(torch.tensor([PAD], dtype=cast_ref.torch_dtype(out_kind)),
                              out_kind)[0]
    exp = np.full((len(idx), L, disp), pad, dtype=cast_ref.BITS[out_kind])
    lens = np.zeros(len(idx), np.int64)
    for i, g in enumerate(idx):
        if not 0 <= g < NS:
            continue
        lens[i] = LENS[g]
        k = min(int(LENS[g]), L)
        if k:
            exp[i, :k] = model_cols(bits[GOFF[g]: GOFF[g] + k], in_kind, out_kind,
                                    scale, shift)
    return exp, lens


@pytest.mark.parametrize("in_kind,out_kind", [("f32", "bf16"), ("u8", "f32")])
@pytest.mark.parametrize("disp", [1, 3, 4, 8])
def test_get_csr_padded_vector_affine(store, disp, in_kind, out_kind):
    bits = padded_values(in_kind, disp)
    store.add_csr("c", cast_ref.to_torch(bits, in_kind), LENS)
    scale, shift = col_params(disp)
    exp, lens = padded_model(bits, in_kind, out_kind, IDX, scale, shift)
    dense, lengths = store.get_csr_padded(
        "c", IDX, L, dtype=cast_ref.torch_dtype(out_kind), affine=(scale, shift),
        pad_value=PAD)
    torch.cuda.synchronize()
    assert dense.shape == (NI, L, disp)
    assert_model(dense, exp.reshape(-1), out_kind, (disp, in_kind, out_kind))
    assert lengths.cpu().tolist() == lens.tolist()
    assert LENS[IDX[6]] > L and lengths[6] == 9 and lengths[5] == 0 and lengths[7] == 0
    # pad positions hold the raw pad
    assert float(dense[5, 0, 0]) == PAD and float(dense[7, L - 1, disp - 1]) == PAD
    assert store.query("c")["oob_skipped"] == 1
    store.reset_counters("c")
    with pytest.raises(ValueError):
        store.get_csr_padded("c", IDX, L, dtype=cast_ref.torch_dtype(out_kind),
                             affine=(np.ones(disp + 1, np.float32), shift))


@pytest.mark.parametrize("disp", [1, 3])
def test_get_csr_padded_column_wraps_inside_a_chunk(store, disp):
    """max_len = 8 makes the row a whole number of 16-B bf16 chunks while
    disp < 8: a chunk spans several elements and its column wraps at disp."""
    bits = padded_values("f32", disp)
    store.add_csr("c", cast_ref.to_torch(bits, "f32"), LENS)
    scale, shift = col_params(disp)
    exp, lens = padded_model(bits, "f32", "bf16", IDX, scale, shift, L=8)
    dense, lengths = store.get_csr_padded("c", IDX, 8, dtype=torch.bfloat16,
                                          affine=(scale, shift), pad_value=PAD)
    torch.cuda.synchronize()
    assert_model(dense, exp.reshape(-1), "bf16", disp)
    assert lengths.cpu().tolist() == lens.tolist()
    store.reset_counters("c")


# ------------------------------------------------------------------ loaders
def test_prefetch_loaders_vector_affine(store):
    from ddstore_amd import PrefetchLoader

    disp = 4
    bits = padded_values("u8", disp)
    store.add_csr("c", cast_ref.to_torch(bits, "u8"), LENS)
    scale, shift = col_params(disp)
    order = torch.from_numpy(np.random.default_rng(3).permutation(NS))
    loader = PrefetchLoader(store, "c", order, 16, pad_to=L, pad_value=PAD,
                            out_dtype=torch.bfloat16, affine=(scale, shift))
    assert loader.affine[0].is_cuda and loader.affine[0].dtype == torch.float32
    nb = 0
    for k, (dense, lengths) in enumerate(loader):
        d, n = store.get_csr_padded("c", order[16 * k: 16 * (k + 1)], L,
                                    dtype=torch.bfloat16, affine=(scale, shift),
                                    pad_value=PAD)
        assert torch.equal(dense.view(torch.int16), d.view(torch.int16))
        assert torch.equal(lengths, n)
        nb += 1
    assert nb == NS // 16

    rows = table_rows("f16", 128)[:80]
    assert rows.shape[0] == 80
    store.add("v", cast_ref.to_torch(rows, "f16"))
    scale, shift = col_params(128)
    order = torch.from_numpy(np.random.default_rng(4).permutation(80))
    loader = PrefetchLoader(store, "v", order, 32, out_dtype=torch.bfloat16,
                            affine=(scale, shift))
    nb = 0
    for k, batch in enumerate(loader):
        ids = order[32 * k: 32 * (k + 1)]
        d = store.get_batch("v", ids, dtype=torch.bfloat16, affine=(scale, shift))
        assert torch.equal(batch.view(torch.int16), d.view(torch.int16))
        assert_model(d, model_cols(rows[ids.numpy()], "f16", "bf16", scale, shift).reshape(-1),
                     "bf16")
        nb += 1
    assert nb == 3


def test_stats_to_fetch_pipeline(store):
    # the whole per-feature pipeline: statistics, then the normalized fetch
    t, x = make_t("f32", 5000, 128)
    store.add("v", t)
    cs = store.column_stats("v")
    out = store.get_batch("v", np.arange(5000), dtype=torch.float32, affine=cs.affine())
    torch.cuda.synchronize()
    z = out.double().cpu()
    assert (z[:, 0] == 0).all()                  # the constant column maps to 0
    assert z[:, 1:].mean(0).abs().max() < 1e-4
    assert (z[:, 1:].std(0, unbiased=False) - 1).abs().max() < 1e-4
