"""Column statistics and the per-column affine on the host backend
(``device="cpu"``): ``column_stats`` against NumPy float64 on the arrays
handed to ``add`` / ``add_csr``, the cross-rank merge on two gloo ranks,
``ColumnStats.affine``, and vector ``affine=`` in ``get_batch`` and
``get_csr_padded`` bit for bit against ``cast_ref.model_affine_unfused``
applied column by column."""
import numpy as np
import pytest
import torch

from tests import cast_ref
from tests.dist_utils import run_dist

U = 2.0 ** -53
NP_DTYPES = {"f32": np.float32, "f64": np.float64, "u8": np.uint8, "i64": np.int64}


def make(kind, rows, disp, seed=0):
    """(rows, disp) test data: column 0 constant, the rest random; integers
    beyond 2^53 for i64 so the rounding to float64 shows."""
    rng = np.random.default_rng(seed + 17 * disp + rows)
    if kind == "u8":
        a = rng.integers(0, 256, (rows, disp)).astype(np.uint8)
    elif kind == "i64":
        a = rng.integers(-2 ** 62, 2 ** 62, (rows, disp)).astype(np.int64)
    else:
        a = (rng.standard_normal((rows, disp)) * 3 + 100).astype(NP_DTYPES[kind])
    if rows:
        a[:, 0] = a[0, 0]
    return a


TORCH_KINDS = {"f32": torch.float32, "f64": torch.float64, "u8": torch.uint8,
               "i64": torch.int64, "i32": torch.int32, "f16": torch.float16,
               "bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn}


def make_t(kind, rows, disp, seed=0):
    """The same for every stored kind: (tensor handed to the store, its exact
    values as a float64 array)."""
    if kind in NP_DTYPES:
        a = make(kind, rows, disp, seed)
        return torch.from_numpy(a), a.astype(np.float64)
    g = torch.Generator().manual_seed(seed + 17 * disp + rows)
    if kind == "i32":
        x = torch.randint(-2 ** 30, 2 ** 30, (rows, disp), generator=g, dtype=torch.int32)
    else:   # f16 and bf16 around 100, e4m3 (largest finite 448) around 16
        x = torch.randn(rows, disp, generator=g)
        x = x * 4 + 16 if kind == "e4m3" else x * 3 + 100
    if rows:
        x[:, 0] = x[0, 0]
    t = x.to(TORCH_KINDS[kind])
    wide = t if kind == "i32" else t.to(torch.float32)
    return t, wide.to(torch.float64).numpy()


def np_stats(a):
    """Two-pass statistics of the columns of a (n, disp) array: values as
    float64, the arithmetic in long double so that the reference's own error
    stays well below the bounds; a column of equal values has its exact
    answer (the rounded mean of n equal values need not be that value)."""
    x = a.astype(np.float64)
    n = x.shape[0]
    if n == 0:
        nan = np.full(x.shape[1], np.nan)
        return 0, nan, nan, nan, nan
    with np.errstate(invalid="ignore"):
        xl = x.astype(np.longdouble)
        mean = xl.mean(0)
        std = np.sqrt(((xl - mean) ** 2).mean(0)).astype(np.float64)
        mean = mean.astype(np.float64)
        mn, mx = x.min(0), x.max(0)   # NumPy's min/max propagate NaN
    flat = mn == mx
    return n, np.where(flat, mn, mean), np.where(flat, 0.0, std), mn, mx


def check(cs, a, disp):
    n, mean, std, mn, mx = np_stats(a.reshape(-1, disp))
    assert isinstance(cs.count, int) and cs.count == n
    for t in (cs.mean, cs.std, cs.min, cs.max):
        assert t.dtype == torch.float64 and t.shape == (disp,) and t.device.type == "cpu"
    np.testing.assert_array_equal(cs.min.numpy(), mn)
    np.testing.assert_array_equal(cs.max.numpy(), mx)
    if n == 0:
        assert torch.isnan(cs.mean).all() and torch.isnan(cs.std).all()
        return
    amax = np.abs(a.astype(np.float64)).max(0)
    with np.errstate(invalid="ignore"):
        ok = np.isnan(mean) | (np.abs(cs.mean.numpy() - mean) <= 4 * n * U * amax)
        assert ok.all(), (cs.mean, mean)
        ok = np.isnan(std) | (np.abs(cs.std.numpy() - std) <= 64 * n * U * std)
        assert ok.all(), (cs.std, std)
    assert np.array_equal(np.isnan(cs.mean.numpy()), np.isnan(mean))
    assert np.array_equal(np.isnan(cs.std.numpy()), np.isnan(std))


@pytest.fixture
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    yield s
    s.free()


@pytest.mark.parametrize("disp", [1, 3, 128])
@pytest.mark.parametrize("kind", ["f32", "f64", "u8", "i64"])
def test_fixed_stride(store, kind, disp):
    a = make(kind, 257, disp)
    store.add("v", a)
    cs = store.column_stats("v")
    check(cs, a, disp)
    assert cs.std[0] == 0.0 and cs.mean[0] == float(a[0, 0])   # the constant column
    again = store.column_stats("v", local=True)
    for x, y in zip(cs[1:], again[1:]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("disp", [1, 3, 128])
@pytest.mark.parametrize("kind", ["f32", "f64", "u8", "i64"])
def test_csr(store, kind, disp):
    lens = np.random.default_rng(3).integers(0, 10, 64)
    lens[0] = 0
    a = make(kind, int(lens.sum()), disp)
    store.add_csr("c", a, lens)
    cs = store.column_stats("c")
    assert cs.count == int(lens.sum())     # elements, not samples
    check(cs, a, disp)
    assert cs.std[0] == 0.0


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_nan_column(store, kind):
    a = make(kind, 100, 3)
    a[57, 1] = np.nan
    store.add("v", a)
    cs = store.column_stats("v")
    for t in (cs.mean, cs.std, cs.min, cs.max):
        assert torch.isnan(t[1]) and not torch.isnan(t[0]) and not torch.isnan(t[2])
    check(cs, a, 3)


def test_empty_variable(store):
    store.init("v", 0, 3, dtype=torch.float32)    # no rows, three columns
    cs = store.column_stats("v")
    assert cs.count == 0
    for t in (cs.mean, cs.std, cs.min, cs.max):
        assert t.dtype == torch.float64 and t.shape == (3,) and torch.isnan(t).all()
    store.init_csr("c", np.zeros(4, dtype=np.int64), disp=2)   # four empty samples
    cs = store.column_stats("c")
    assert cs.count == 0
    for t in (cs.mean, cs.std, cs.min, cs.max):
        assert t.shape == (2,) and torch.isnan(t).all()
    # an added empty array has no width to report either
    store.add("w", np.zeros((0, 3), dtype=np.float32))
    assert store.column_stats("w").count == 0


def test_large_mean_small_spread(store):
    # what the raw-moment formula loses: 1e9 + N(0, 1) in float64
    a = cancellation_data()
    store.add("v", a)
    check(store.column_stats("v"), a, 3)


def cancellation_data():
    """(4096, 3) float64: column 1 is 1e9 + N(0, 1), beside two ordinary ones."""
    a = np.random.default_rng(5).standard_normal((4096, 3))
    a[:, 1] += 1e9
    return a


def _shifted(x, pivot, seed):
    """mean and std of a float64 column by shifted sums around `pivot`,
    accumulated one after the other within shuffled chunks of 64 and then
    over the chunks: some order, as the bounds hold for any."""
    d = x[np.random.default_rng(seed).permutation(x.size)] - pivot
    n = x.size
    s1 = s2 = 0.0
    for k in range(0, n, 64):
        s1 += float(np.cumsum(d[k: k + 64])[-1])
        s2 += float(np.cumsum(d[k: k + 64] ** 2)[-1])
    return pivot + s1 / n, np.sqrt(max(s2 - s1 * (s1 / n), 0.0) / n)


@pytest.mark.parametrize("kind", list(TORCH_KINDS) + ["cancel"])
def test_bounds_hold_for_the_worst_pivot(kind):
    """The tolerances of both test files (4 n u max|x| on the mean, 64 n u std
    on the std) are met by a shifted sum whose pivot is the worst the data
    holds, its minimum or maximum, on the data the tests use; the raw-moment
    form misses the std bound on the cancellation column."""
    x = cancellation_data() if kind == "cancel" else make_t(kind, 5000, 3)[1]
    n, mean, std, _, _ = np_stats(x)
    for c in (1, 2):
        col = x[:, c]
        for pivot in (col.min(), col.max()):
            m, s = _shifted(col, pivot, c)
            assert abs(m - mean[c]) <= 4 * n * U * np.abs(col).max()
            assert abs(s - std[c]) <= 64 * n * U * std[c]
    if kind == "cancel":
        col = x[:, 1]
        raw = np.sqrt(abs(np.sum(col * col) - np.sum(col) ** 2 / n) / n)
        assert abs(raw - std[1]) > 64 * n * U * std[1]


def _w_two_ranks(rank, world):
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    rows = [0, 37]                    # rank 0 holds nothing
    full = make("f32", sum(rows), 3, seed=9)
    lo = sum(rows[:rank])
    mine = full[lo: lo + rows[rank]]
    s.add("v", mine)
    check(s.column_stats("v"), full, 3)
    check(s.column_stats("v", local=True), mine, 3)
    # both ranks non-empty and unequal, CSR: the merge itself
    lens = [np.array([2, 0, 5]), np.array([1, 4, 4, 3])][rank]
    allv = make("f64", 19, 2, seed=11)
    allv[:, 1] += 1e6
    off = [0, 7][rank]
    mine = allv[off: off + int(lens.sum())]
    s.add_csr("c", mine, lens)
    cs = s.column_stats("c")
    check(cs, allv, 2)
    assert cs.std[0] == 0.0
    check(s.column_stats("c", local=True), mine, 2)
    s.free()


def test_two_ranks():
    run_dist(_w_two_ranks, 2)


def test_affine_from_stats():
    from ddstore_amd import ColumnStats

    f = lambda *v: torch.tensor(v, dtype=torch.float64)
    cs = ColumnStats(10, f(3.0, 7.0, 0.1), f(2.0, 0.0, 0.3), f(1.0, 7.0, -1.0),
                     f(5.0, 7.0, 2.0))
    scale, shift = cs.affine()
    assert scale.dtype == torch.float32 and shift.dtype == torch.float32
    assert scale.device.type == "cpu" and scale.shape == (3,)
    exp_scale = np.array([0.5, 1.0, 1 / 0.3]).astype(np.float32)
    exp_shift = np.array([-1.5, -7.0, -(0.1 / 0.3)]).astype(np.float32)
    np.testing.assert_array_equal(scale.numpy(), exp_scale)
    np.testing.assert_array_equal(shift.numpy(), exp_shift)
    scale, shift = cs.affine("minmax")
    np.testing.assert_array_equal(scale.numpy(),
                                  np.array([0.25, 1.0, 1 / 3.0]).astype(np.float32))
    np.testing.assert_array_equal(shift.numpy(),
                                  np.array([-0.25, -7.0, 1 / 3.0]).astype(np.float32))
    with pytest.raises(ValueError):
        cs.affine("robust")


# ---- per-column affine on the host path -----------------------------------
def col_params(disp):
    """A different (scale, shift) in every column, full 24-bit significands
    among them."""
    k = np.arange(disp)
    scale = (np.float32(1 / 255) * (1 + k % 7)).astype(np.float32)
    shift = (np.float32(-0.4914) + k.astype(np.float32) / 3).astype(np.float32)
    return scale, shift


def model_cols(bits, in_kind, out_kind, scale, shift):
    """cast_ref.model_affine_unfused, one call per column."""
    out = np.empty(bits.shape, dtype=cast_ref.BITS[out_kind])
    for c in range(bits.shape[-1]):
        out[..., c], _ = cast_ref.model_affine_unfused(
            bits[..., c], in_kind, out_kind, float(scale[c]), float(shift[c]))
    return out


@pytest.mark.parametrize("out_kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("in_kind,disp", [("u8", 3), ("f32", 8), ("f16", 128)])
def test_get_batch_vector_affine(store, in_kind, out_kind, disp):
    rows = cast_ref.as_rows(cast_ref.affine_table(in_kind)[:4096], disp)
    store.add("v", cast_ref.to_torch(rows, in_kind))
    idx = np.random.default_rng(2).integers(0, rows.shape[0], 40)
    scale, shift = col_params(disp)
    odt = cast_ref.torch_dtype(out_kind)
    exp = model_cols(rows[idx], in_kind, out_kind, scale, shift)
    for aff in ((scale, shift), (torch.from_numpy(scale), list(map(float, shift)))):
        got = store.get_batch("v", idx, dtype=odt, affine=aff)
        bad = cast_ref.mismatches(cast_ref.from_torch(got, out_kind), exp,
                                  np.ones(exp.shape, bool), out_kind)
        assert bad.size == 0, bad[:8]
    # a scalar beside a vector is broadcast
    got = store.get_batch("v", idx, dtype=odt, affine=(float(scale[1]), shift))
    exp = model_cols(rows[idx], in_kind, out_kind, np.full(disp, scale[1]), shift)
    assert cast_ref.mismatches(cast_ref.from_torch(got, out_kind), exp,
                               np.ones(exp.shape, bool), out_kind).size == 0
    got = store.get_batch("v", idx, dtype=odt, affine=(scale, 0.25))
    exp = model_cols(rows[idx], in_kind, out_kind, scale, np.full(disp, 0.25))
    assert cast_ref.mismatches(cast_ref.from_torch(got, out_kind), exp,
                               np.ones(exp.shape, bool), out_kind).size == 0
    for bad_len in (disp + 1, 2 * disp):
        with pytest.raises(ValueError):
            store.get_batch("v", idx, dtype=odt,
                            affine=(np.ones(bad_len, np.float32), shift))
    with pytest.raises(ValueError):
        store.get_batch("v", idx, dtype=odt, affine=(2.0, np.ones((disp, 1))))


@pytest.mark.parametrize("disp", [1, 3, 8])
def test_get_csr_padded_vector_affine(store, disp):
    lens = np.random.default_rng(0).integers(0, 10, 64)
    lens[0], lens[1] = 0, 9
    goff = np.concatenate([[0], np.cumsum(lens)])
    n = int(lens.sum())
    vals = np.random.default_rng(1).standard_normal((n, disp)).astype(np.float32)
    store.add_csr("c", vals, lens)
    idx = np.random.default_rng(4).integers(0, 64, 40)
    idx[5] = 64                       # out of range: an all-pad row
    scale, shift = col_params(disp)
    L, pad = 6, -3.0
    dense, lengths = store.get_csr_padded("c", idx, L, dtype=torch.bfloat16,
                                          affine=(scale, shift), pad_value=pad)
    padbits = cast_ref.from_torch(torch.tensor([pad], dtype=torch.bfloat16), "bf16")[0]
    exp = np.full((40, L, disp), padbits, dtype=np.uint16)
    for i, g in enumerate(idx):
        if g >= 64:
            continue
        k = min(int(lens[g]), L)
        exp[i, :k] = model_cols(vals[goff[g]: goff[g] + k].view(np.uint32), "f32", "bf16",
                                scale, shift)
    np.testing.assert_array_equal(cast_ref.from_torch(dense, "bf16").reshape(exp.shape), exp)
    assert lengths.tolist() == [0 if g >= 64 else int(lens[g]) for g in idx]
    store.reset_counters("c")
    with pytest.raises(ValueError):
        store.get_csr_padded("c", idx, L, dtype=torch.bfloat16,
                             affine=(np.ones(disp + 2, np.float32), shift))


def test_prefetch_loader_vector_affine(store):
    from ddstore_amd import PrefetchLoader

    a = np.random.default_rng(6).integers(0, 256, (64, 5)).astype(np.uint8)
    store.add("v", a)
    scale, shift = col_params(5)
    loader = PrefetchLoader(store, "v", np.arange(64), 16, out_dtype=torch.float32,
                            affine=(scale, shift))
    assert isinstance(loader.affine[0], torch.Tensor)    # converted once
    for k, batch in enumerate(loader):
        exp = store.get_batch("v", np.arange(16 * k, 16 * k + 16), dtype=torch.float32,
                              affine=(scale, shift))
        assert torch.equal(batch, exp)
