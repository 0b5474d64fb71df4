"""The cast model of tests/cast_ref.py, proved without a GPU: equal to torch's
CPU ``Tensor.to`` on every defined table entry of every (in, out) pair, its
``defined`` masks exactly the float -> int rule, its fused multiply-add exact,
the two affine forms separated by the second (scale, shift) pair, and the host
backend following it through get_batch, get_batch(affine=) and
get_csr_padded(dtype=)."""
import numpy as np
import pytest
import torch

from tests import cast_ref as cr


def _first(bad, tbl, in_kind):
    i = int(bad[0])
    width = 2 * np.dtype(cr.BITS[in_kind]).itemsize
    v = int(tbl[i]) & ((1 << (4 * width)) - 1)
    return f"{bad.size} differ, first input 0x{v:0{width}X} (entry {i})"


@pytest.mark.parametrize("in_kind", cr.KINDS)
def test_model_equals_torch_cpu(in_kind):
    failures = []
    for out_kind in cr.KINDS:
        tbl = cr.table(in_kind, out_kind)
        exp, defined = cr.model_cast(tbl, in_kind, out_kind)
        t = cr.to_torch(tbl, in_kind)
        got = cr.from_torch(t if in_kind == out_kind
                            else t.to(cr.torch_dtype(out_kind)), out_kind)
        bad = cr.mismatches(got, exp, defined, out_kind)
        if bad.size:
            failures.append(f"{in_kind} -> {out_kind}: {_first(bad, tbl, in_kind)}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("in_kind", cr.KINDS)
def test_defined_masks_are_the_float_to_int_rule(in_kind):
    for out_kind in cr.KINDS:
        tbl = cr.table(in_kind, out_kind)
        _, defined = cr.model_cast(tbl, in_kind, out_kind)
        if in_kind in cr.INT_KINDS or out_kind in cr.FLOAT_KINDS:
            assert defined.all(), f"{in_kind} -> {out_kind}"
            continue
        lo, hi = cr.IRANGE[out_kind]
        x = cr.to_f64(tbl, in_kind)
        with np.errstate(invalid="ignore"):
            rule = np.isfinite(x) & (np.trunc(x) >= float(lo)) & (np.trunc(x) < float(hi + 1))
        assert np.array_equal(defined, rule), f"{in_kind} -> {out_kind}"


def test_mask_worked_examples():
    f16 = cr.table("f16", "u8")
    assert f16.size == 65536
    assert (~cr.model_cast(f16, "f16", "u8")[1]).sum() == 26624
    assert (~cr.model_cast(f16, "f16", "i32")[1]).sum() == 2048
    # -0.5 truncates to 0, which u8 holds; -1.0 does not fit
    b, d = cr.model_cast(np.array([0xB800, 0xBC00, 0x5BF8], np.uint16), "f16", "u8")
    assert d.tolist() == [True, False, True] and b[0] == 0 and b[2] == 255


def test_tables_hold_what_they_claim():
    for k, n in (("f16", 65536), ("bf16", 65536), ("e4m3", 256), ("e5m2", 256),
                 ("u8", 256)):
        assert np.unique(cr.table(k, "f32")).size == n
    # the issue's boundary entries: 464 / 500 / inf for e4m3fn, 61439 / 61440
    # for e5m2, and where they go
    f = np.array([464.0, 500.0, np.inf, 61439.0, 61440.0, 1e9], np.float32).view(np.uint32)
    assert cr.model_cast(f[:3], "f32", "e4m3")[0].tolist() == [0x7E, 0x7F, 0x7F]
    assert cr.model_cast(f[3:], "f32", "e5m2")[0].tolist() == [0x7B, 0x7C, 0x7C]
    t32 = set(cr.table("f32", "e4m3").tolist())
    assert {int(f[0]), int(f[0]) + 1, int(f[2]), int(f[4]), int(f[4]) - 1} <= t32
    # f64 -> f16 is rounded twice: 1 + 2^-11 + 2^-40 goes to 0x3C00 through
    # f32 and would go to 0x3C01 in one rounding; the table holds such probes
    probe = np.array([1 + 2.0**-11 + 2.0**-40]).view(np.uint64)
    assert cr.model_cast(probe, "f64", "f16")[0][0] == 0x3C00
    once = cr.round_to_format(*cr.decode(probe, "f64"), "f16")
    assert once[0] == 0x3C01
    tbl = cr.table("f64", "f16")
    two = cr.model_cast(tbl, "f64", "f16")[0]
    one = cr.round_to_format(*cr.decode(tbl, "f64"), "f16").astype(np.uint16)
    assert (two != one).sum() > 1000
    # i32 -> bf16 goes through f32 as well, and the table separates that
    ti = cr.table("i32", "bf16")
    one = cr.round_to_format(*cr.decode(ti, "i32"), "bf16").astype(np.uint16)
    assert (cr.model_cast(ti, "i32", "bf16")[0] != one).any()


def test_rounding_routine_against_hardware_f32():
    """The generic routine, asked for f32, equals NumPy's float64 -> float32
    (IEEE hardware rounding) on the whole f64 table, and int64 -> float64."""
    tbl = cr.table("f64", "f16")
    mine = cr.round_to_format(*cr.decode(tbl, "f64"), "f32").astype(np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        hw = tbl.view(np.float64).astype(np.float32).view(np.uint32)
    assert cr.mismatches(mine, hw, np.ones(tbl.shape, bool), "f32").size == 0
    ti = cr.table("i64", "f64")
    mine = cr.round_to_format(*cr.decode(ti, "i64"), "f64")
    assert np.array_equal(mine, ti.astype(np.float64).view(np.uint64))


@pytest.mark.parametrize("scale,shift", [cr.AFFINE_EXACT, cr.AFFINE_FULL])
def test_fma_model_is_exact(scale, shift):
    sc, sh = np.float32(scale), np.float32(shift)
    for in_kind in cr.AFFINE_IN:
        x = cr._f32_values(cr.affine_table(in_kind), in_kind)
        y = cr.fma_f32(x, sc, sh)
        step = max(1, x.size // 1500)
        for i in range(0, x.size, step):
            e = cr.fma_f32_exact(x[i], sc, sh)
            assert (np.isnan(e) and np.isnan(y[i])) or e.view(np.uint32) == y[i].view(np.uint32), \
                f"{in_kind} entry {i}"


def test_affine_forms_differ_on_the_full_pair():
    """The exact pair cannot tell the forms apart where the product is exact
    (inputs of at most 22 significant bits); the full pair does, for every
    input kind."""
    for in_kind in cr.AFFINE_IN:
        tbl = cr.affine_table(in_kind)
        for out_kind in cr.AFFINE_OUT if in_kind not in ("f32", "i64") else ():
            a, _ = cr.model_affine(tbl, in_kind, out_kind, *cr.AFFINE_EXACT)
            b, _ = cr.model_affine_unfused(tbl, in_kind, out_kind, *cr.AFFINE_EXACT)
            assert cr.mismatches(a, b, np.ones(tbl.shape, bool), out_kind).size == 0
        a, _ = cr.model_affine(tbl, in_kind, "f32", *cr.AFFINE_FULL)
        b, _ = cr.model_affine_unfused(tbl, in_kind, "f32", *cr.AFFINE_FULL)
        assert cr.mismatches(a, b, np.ones(tbl.shape, bool), "f32").size > 0, \
            f"{in_kind}: the table does not separate fused from unfused"


# ----------------------------------------------------------- host backend
WIDTH = 128


@pytest.fixture(scope="module")
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    yield s
    s.free()


_added = {}


def _var(store, in_kind, out_kind, csr=False):
    """The pair's table as a variable of WIDTH-element rows (or as CSR samples
    of WIDTH elements), added once per distinct table."""
    tbl = cr.table(in_kind, out_kind)
    key = (in_kind, id(tbl), csr)
    if key not in _added:
        rows = cr.as_rows(tbl, WIDTH)
        name = f"h{len(_added)}"
        t = cr.to_torch(rows, in_kind)
        if csr:
            store.add_csr(name, t.reshape(-1),
                          torch.full((rows.shape[0],), WIDTH, dtype=torch.int64))
        else:
            store.add(name, t)
        _added[key] = (name, rows)
    return _added[key]


@pytest.mark.parametrize("in_kind", cr.KINDS)
def test_host_get_batch_follows_the_model(store, in_kind):
    failures = []
    for out_kind in cr.KINDS:
        name, rows = _var(store, in_kind, out_kind)
        idx = torch.arange(rows.shape[0] - 1, -1, -1)
        out = store.get_batch(name, idx, dtype=cr.torch_dtype(out_kind))
        exp, defined = cr.model_cast(rows[::-1], in_kind, out_kind)
        bad = cr.mismatches(cr.from_torch(out, out_kind), exp, defined, out_kind)
        if bad.size:
            failures.append(f"{in_kind} -> {out_kind}: "
                            f"{_first(bad, rows[::-1].reshape(-1), in_kind)}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("in_kind", cr.KINDS)
def test_host_csr_padded_follows_the_model(store, in_kind):
    failures = []
    for out_kind in cr.KINDS:
        name, rows = _var(store, in_kind, out_kind, csr=True)
        n = rows.shape[0]
        idx = torch.arange(n - 1, -1, -1)
        dense, lengths = store.get_csr_padded(name, idx, WIDTH + 3,
                                              dtype=cr.torch_dtype(out_kind),
                                              pad_value=1)
        assert (lengths == WIDTH).all()
        got = cr.from_torch(dense, out_kind).reshape(n, WIDTH + 3)
        exp, defined = cr.model_cast(rows[::-1], in_kind, out_kind)
        bad = cr.mismatches(got[:, :WIDTH], exp, defined, out_kind)
        if bad.size:
            failures.append(f"{in_kind} -> {out_kind}: "
                            f"{_first(bad, rows[::-1].reshape(-1), in_kind)}")
        pad = cr.from_torch(torch.tensor([1], dtype=cr.torch_dtype(out_kind)), out_kind)
        assert (got[:, WIDTH:] == pad[0]).all(), f"{in_kind} -> {out_kind}: pad"
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("scale,shift", [cr.AFFINE_EXACT, cr.AFFINE_FULL])
def test_host_affine_is_the_unfused_form(store, scale, shift):
    failures = []
    for in_kind in cr.AFFINE_IN:
        tbl_kind = "f16" if in_kind == "f32" else "f32"   # affine_table's key
        for csr in (False, True):
            name, rows = _var(store, in_kind, tbl_kind, csr=csr)
            idx = torch.arange(rows.shape[0])
            for out_kind in cr.AFFINE_OUT:
                dt = cr.torch_dtype(out_kind)
                if csr:
                    out, _ = store.get_csr_padded(name, idx, WIDTH, dtype=dt,
                                                  affine=(scale, shift))
                else:
                    out = store.get_batch(name, idx, dtype=dt, affine=(scale, shift))
                exp, defined = cr.model_affine_unfused(rows, in_kind, out_kind,
                                                       scale, shift)
                bad = cr.mismatches(cr.from_torch(out, out_kind), exp, defined, out_kind)
                if bad.size:
                    failures.append(f"{in_kind} -> {out_kind} csr={csr}: "
                                    f"{_first(bad, rows.reshape(-1), in_kind)}")
    assert not failures, "; ".join(failures)


# ------------------------------------------------------------------- bool
def test_bool_output_is_refused_unless_stored_as_bool(store):
    store.add("b_u8", torch.arange(24, dtype=torch.uint8).view(6, 4))
    store.add("b_f32", torch.arange(24, dtype=torch.float32).view(6, 4) / 2)
    store.add_csr("b_csr", torch.arange(6, dtype=torch.uint8),
                  torch.tensor([1, 2, 3]))
    idx = torch.tensor([5, 0, 3])
    for name in ("b_u8", "b_f32"):
        with pytest.raises(TypeError, match="bool"):
            store.get_batch(name, idx, dtype=torch.bool)
        with pytest.raises(TypeError, match="bool"):
            store.get_batch(name, idx, out=torch.empty(3, 4, dtype=torch.bool))
        with pytest.raises(TypeError, match="bool"):
            store.gather_into(name, idx, torch.empty(3, 4, dtype=torch.bool))
    with pytest.raises(TypeError, match="bool"):
        store.get_csr_padded("b_csr", torch.tensor([2, 0]), 3, dtype=torch.bool)
    with pytest.raises(TypeError, match="bool"):
        store.get_csr_padded("b_csr", torch.tensor([2, 0]), 3,
                             out=torch.empty(2, 3, 1, dtype=torch.bool))


def test_bool_variable_round_trips_as_bytes(store):
    arr = (torch.arange(40).view(10, 4) % 3 == 0)
    store.add("b_bool", arr)
    store.add_csr("b_bool_csr", arr.reshape(-1), torch.full((10,), 4))
    idx = torch.tensor([9, 0, 4, 4])
    as_bool = store.get_batch("b_bool", idx, dtype=torch.bool)
    assert as_bool.dtype == torch.bool and torch.equal(as_bool, arr[idx])
    as_u8 = store.get_batch("b_bool", idx, dtype=torch.uint8)
    assert as_u8.dtype == torch.uint8
    assert torch.equal(as_u8, arr[idx].view(torch.uint8))
    assert set(as_u8.unique().tolist()) == {0, 1}
    out = torch.empty(4, 4, dtype=torch.bool)
    store.gather_into("b_bool", idx, out)
    assert torch.equal(out, arr[idx])
    dense, _ = store.get_csr_padded("b_bool_csr", idx, 5, dtype=torch.bool,
                                    pad_value=True)
    assert torch.equal(dense[:, :4, 0], arr[idx]) and dense[:, 4].all()
    dense, _ = store.get_csr_padded("b_bool_csr", idx, 5, dtype=torch.uint8)
    assert torch.equal(dense[:, :4, 0], arr[idx].view(torch.uint8))
