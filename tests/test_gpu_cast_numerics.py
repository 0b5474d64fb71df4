"""The cast numerics of every gather kernel that converts, against the exact
model of tests/cast_ref.py (which tests/test_cast_ref_cpu.py proves equal to
torch's CPU cast): every accepted (in, out) pair over its table -- every bit
pattern of the 8- and 16-bit kinds, every rounding tie of the narrower float
targets with its neighbours, overflow thresholds, subnormals, NaNs, integer
limits -- through each kernel path that carries ``cvt``:

  k_gather_tiled        branch-free groups and the predicated tail
  k_gather_oneshot      16-B vector chunks, element-wise, misaligned output
  k_gather_csr_padded   aligned vector, element-fed chunk, boundary chunk, VEC=1

Bit for bit where the contract defines the result (everything but float ->
int of a non-finite or unrepresentable value); a NaN only has to be a NaN.
Rows are requested in a shuffled order; tables are padded with zeros.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cast_ref as cr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TILED_W = 128        # >= 8 output chunks of 16 B for every output type


def vec(out_kind):
    """Elements per 16-B output chunk."""
    return 16 // np.dtype(cr.BITS[out_kind]).itemsize


@pytest.fixture(scope="module")
def store():
    from ddstore_amd import DDStore

    s = DDStore(device=DEV)
    assert s.mode == "hip", "GPU test must exercise the native HIP path"
    yield s
    s.free()


_model = {}


def model(in_kind, out_kind):
    """(table, expected bits, defined) of a pair, computed once."""
    key = (in_kind, out_kind)
    if key not in _model:
        tbl = cr.table(in_kind, out_kind)
        _model[key] = (tbl,) + cr.model_cast(tbl, in_kind, out_kind)
    return _model[key]


def request(nrows, seed):
    """Shuffled row indices covering every row, at least 128 of them and 37
    past a multiple of 64: whatever the tile size (8..64 rows), full tiles run
    their branch-free groups and the last tile is partial."""
    rng = np.random.default_rng(seed)
    n = max(nrows, 128)
    n += (37 - n) % 64
    reps = -(-n // nrows)
    return np.concatenate([rng.permutation(nrows) for _ in range(reps)])[:n]


def first_bad(bad, in_bits, in_kind):
    i = int(bad[0])
    width = 2 * np.dtype(cr.BITS[in_kind]).itemsize
    v = int(in_bits.reshape(-1)[i]) & ((1 << (4 * width)) - 1)
    return f"{bad.size} differ, first input 0x{v:0{width}X}"


def expect(in_kind, out_kind, affine):
    """(table, expected bits, defined, expected bits of a padding zero)."""
    if affine is None:
        tbl, exp, defined = model(in_kind, out_kind)
        zero = cr.model_cast(np.zeros(1, tbl.dtype), in_kind, out_kind)[0][0]
    else:   # the zero padding of the table is scaled and shifted too
        tbl = cr.affine_table(in_kind)
        exp, defined = cr.model_affine(tbl, in_kind, out_kind, *affine)
        zero = cr.model_affine(np.zeros(1, tbl.dtype), in_kind, out_kind, *affine)[0][0]
    return tbl, exp, defined, zero


def padded_to(total, exp, defined, zero):
    e = np.full(total, zero, dtype=exp.dtype)
    e[:exp.size] = exp
    d = np.ones(total, dtype=bool)
    d[:defined.size] = defined
    return e, d


_fixed = {}


def fixed_var(store, in_kind, tbl, width):
    key = (in_kind, id(tbl), width)
    if key not in _fixed:
        name = f"f{len(_fixed)}"
        rows = cr.as_rows(tbl, width)
        store.add(name, cr.to_torch(rows, in_kind))
        _fixed[key] = (name, rows)
    return _fixed[key]


def run_fixed(store, width_of, offset_view=False, pairs=None, affine=None,
              seed=0):
    """Every pair through get_batch (or gather_into an output view offset by
    one element) at row width width_of(out_kind); returns the failures."""
    failures = []
    for in_kind, out_kind in pairs or cr.pairs():
        tbl, exp, defined, zero = expect(in_kind, out_kind, affine)
        width = width_of(out_kind)
        name, rows = fixed_var(store, in_kind, tbl, width)
        idx = request(rows.shape[0], seed)
        idx_dev = torch.from_numpy(idx).to(DEV)
        dt = cr.torch_dtype(out_kind)
        if offset_view:
            back = torch.empty(idx.size * width + 1, dtype=dt, device=DEV)
            out = back[1:].view(idx.size, width)
            assert out.data_ptr() % 16 != 0
            store.gather_into(name, idx_dev, out)
        elif affine is not None:
            out = store.get_batch(name, idx_dev, dtype=dt, affine=affine)
        else:
            out = store.get_batch(name, idx_dev, dtype=dt)
        torch.cuda.synchronize()
        got = cr.from_torch(out, out_kind)
        e, d = padded_to(rows.size, exp, defined, zero)
        bad = cr.mismatches(got, e.reshape(rows.shape)[idx],
                            d.reshape(rows.shape)[idx], out_kind)
        if bad.size:
            failures.append(f"{in_kind} -> {out_kind}: "
                            f"{first_bad(bad, rows[idx], in_kind)}")
        assert store.query(name)["oob_skipped"] == 0
    return failures


def test_tiled(store):
    failures = run_fixed(store, lambda o: TILED_W)
    assert not failures, "; ".join(failures)


def test_oneshot_vector(store):
    # 4 chunks of 16 B per row: below the tiled kernel's minimum
    failures = run_fixed(store, lambda o: 4 * vec(o), seed=1)
    assert not failures, "; ".join(failures)


def test_oneshot_elementwise(store):
    failures = run_fixed(store, lambda o: 5, seed=2)
    assert not failures, "; ".join(failures)


def test_oneshot_misaligned_output(store):
    failures = run_fixed(store, lambda o: 4 * vec(o), offset_view=True, seed=3)
    assert not failures, "; ".join(failures)


# ----------------------------------------------------------------- padded CSR
# sub-path -> (disp and max_len as functions of the output kind, sample lengths
# cycled over the samples). No sample is longer than max_len, so every table
# entry is fetched.
PADDED = {
    # disp a multiple of VEC: one vector load per chunk
    "aligned": (vec, lambda o: 8, (8, 3, 7, 8, 5)),
    # disp = 1, rows and samples whole chunks: 16-B chunks fed by element loads
    "element_fed": (lambda o: 1, lambda o: 32, (32, 16)),
    # one chunk per row, one valid element in it: every entry sits in a
    # boundary chunk
    "boundary": (lambda o: 1, vec, (1,)),
    # an odd row: VEC = 1
    "vec1": (lambda o: 1, lambda o: 7, (7, 5, 6, 7)),
    # affine: whole chunks and boundary chunks in one shape
    "mixed": (lambda o: 1, lambda o: 32, (32, 16, 31, 7)),
}

_csr = {}


def csr_var(store, in_kind, tbl, disp, lens_cycle):
    key = (in_kind, id(tbl), disp, lens_cycle)
    if key not in _csr:
        nelem = -(-tbl.size // disp)
        per = sum(lens_cycle)
        ncyc = -(-nelem // per)
        lens = np.tile(np.array(lens_cycle, dtype=np.int64), ncyc)
        vals = np.zeros(lens.sum() * disp, dtype=tbl.dtype)
        vals[:tbl.size] = tbl
        name = f"c{len(_csr)}"
        store.add_csr(name, cr.to_torch(vals, in_kind).view(-1, disp),
                      torch.from_numpy(lens))
        off = np.zeros(lens.size + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        _csr[key] = (name, vals, lens, off)
    return _csr[key]


def run_padded(store, sub, pairs=None, affine=None, seed=0):
    disp_of, max_len_of, lens_cycle = PADDED[sub]
    failures = []
    for in_kind, out_kind in pairs or cr.pairs():
        tbl, exp, defined, zero = expect(in_kind, out_kind, affine)
        disp, max_len = disp_of(out_kind), max_len_of(out_kind)
        name, vals, lens, off = csr_var(store, in_kind, tbl, disp, lens_cycle)
        idx = np.random.default_rng(seed).permutation(lens.size)
        dt = cr.torch_dtype(out_kind)
        dense, lengths = store.get_csr_padded(
            name, torch.from_numpy(idx).to(DEV), max_len, dtype=dt,
            affine=affine, pad_value=1)
        torch.cuda.synchronize()
        assert np.array_equal(lengths.cpu().numpy(), lens[idx]), f"{sub}: lengths"
        got = cr.from_torch(dense, out_kind).reshape(idx.size, max_len * disp)
        # where each output slot comes from: flat position in vals, or pad
        pos = np.arange(max_len * disp)[None, :]
        valid = pos < (lens[idx] * disp)[:, None]
        src = np.where(valid, off[idx][:, None] * disp + pos, 0)
        pad = cr.from_torch(torch.tensor([1], dtype=dt), out_kind)[0]
        e, d = padded_to(vals.size, exp, defined, zero)
        want = np.where(valid, e[src], pad)
        bad = cr.mismatches(got, want, d[src] | ~valid, out_kind)
        if bad.size:
            where = "pad slot" if not valid.reshape(-1)[bad[0]] else \
                first_bad(bad, vals[src], in_kind)
            failures.append(f"{in_kind} -> {out_kind}: {where}")
        assert store.query(name)["oob_skipped"] == 0
    return failures


@pytest.mark.parametrize("sub", ["aligned", "element_fed", "boundary", "vec1"])
def test_csr_padded(store, sub):
    failures = run_padded(store, sub, seed=4)
    assert not failures, "; ".join(failures)


# -------------------------------------------------------------------- affine
AFFINE_PAIRS = [(i, o) for i in cr.AFFINE_IN for o in cr.AFFINE_OUT]


@pytest.mark.parametrize("scale,shift", [cr.AFFINE_EXACT, cr.AFFINE_FULL],
                         ids=["exact", "full"])
@pytest.mark.parametrize("shape", ["tiled", "oneshot", "padded"])
def test_affine_is_fused(store, shape, scale, shift):
    """fma(x_f32, scale, shift) rounded once, then cast. With the full pair
    the unfused form gives other bits on these tables
    (test_cast_ref_cpu.py::test_affine_forms_differ_on_the_full_pair)."""
    aff = (scale, shift)
    if shape == "tiled":
        failures = run_fixed(store, lambda o: TILED_W, pairs=AFFINE_PAIRS,
                             affine=aff, seed=5)
    elif shape == "oneshot":
        failures = run_fixed(store, lambda o: 4 * vec(o), pairs=AFFINE_PAIRS,
                             affine=aff, seed=6)
    else:
        failures = run_padded(store, "mixed", pairs=AFFINE_PAIRS, affine=aff,
                              seed=7)
    assert not failures, "; ".join(failures)


# ------------------------------------------------------ cross-kernel agreement
def _canonical_bytes(bits, defined, out_kind):
    """Undefined positions zeroed and every NaN made the same pattern."""
    b = np.where(defined, bits, bits.dtype.type(0))
    nan = cr.is_nan_bits(b, out_kind)
    b = np.where(nan, bits.dtype.type(np.iinfo(bits.dtype).max), b)
    return np.ascontiguousarray(b).tobytes()


def _child_main():
    """Fetch every pair's table at the tiled width, in table order, and print
    one SHA-256 per pair (run in a child process per kernel variant)."""
    from ddstore_amd import DDStore

    s = DDStore(device=DEV)
    for in_kind, out_kind in cr.pairs():
        tbl, _, defined = model(in_kind, out_kind)
        name, rows = fixed_var(s, in_kind, tbl, TILED_W)
        idx = torch.arange(rows.shape[0], device=DEV)
        out = s.get_batch(name, idx, dtype=cr.torch_dtype(out_kind))
        torch.cuda.synchronize()
        got = cr.from_torch(out, out_kind).reshape(-1)[:tbl.size]
        h = hashlib.sha256(_canonical_bytes(got, defined, out_kind)).hexdigest()
        print("HASH", in_kind, out_kind, h)
    s._backend.free_all()
    print("CHILD-OK")


def test_cross_kernel_agreement():
    """The legacy one-shot kernels, the tiled kernel with the LDS directory
    and the default dispatch give the same bytes as each other and as the
    model: no instantiation's packed convert rounds differently."""
    variants = {
        "legacy": {"DDSTORE_GATHER_KERNEL": "legacy"},
        "tiled_lds": {"DDSTORE_GATHER_KERNEL": "tiled", "DDSTORE_GATHER_DIR": "lds"},
        "default": {},
    }
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); "
            "from tests.test_gpu_cast_numerics import _child_main; _child_main()")
    procs = {}
    for k, extra in variants.items():
        env = {e: v for e, v in os.environ.items()
               if not e.startswith("DDSTORE_GATHER_")}
        env.update(extra)
        procs[k] = subprocess.Popen([sys.executable, "-c", code], env=env, cwd=ROOT,
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                    text=True)
    want = []
    for in_kind, out_kind in cr.pairs():
        _, exp, defined = model(in_kind, out_kind)
        h = hashlib.sha256(_canonical_bytes(exp, defined, out_kind)).hexdigest()
        want.append(f"HASH {in_kind} {out_kind} {h}")
    hashes = {}
    for k, p in procs.items():
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, f"{k}: {se[-2000:]}"
        assert "CHILD-OK" in so, f"{k}: {so[-2000:]}"
        hashes[k] = [l for l in so.splitlines() if l.startswith("HASH")]
    for k in variants:
        diff = [a.split()[1:3] for a, b in zip(hashes[k], want) if a != b]
        assert len(hashes[k]) == len(want) and not diff, \
            f"{k} differs from the model on {diff}"
        assert hashes[k] == hashes["default"]


# ---------------------------------------------------------------------- bool
def test_bool_output_is_refused_unless_stored_as_bool(store):
    store.add("b_u8", torch.arange(24, dtype=torch.uint8).view(6, 4))
    store.add("b_f32", torch.arange(24, dtype=torch.float32).view(6, 4) / 2)
    store.add_csr("b_csr", torch.arange(6, dtype=torch.uint8),
                  torch.tensor([1, 2, 3]))
    idx = torch.tensor([5, 0, 3], device=DEV)
    for name in ("b_u8", "b_f32"):
        with pytest.raises(TypeError, match="bool"):
            store.get_batch(name, idx, dtype=torch.bool)
        out = torch.empty(3, 4, dtype=torch.bool, device=DEV)
        with pytest.raises(TypeError, match="bool"):
            store.get_batch(name, idx, out=out)
        with pytest.raises(TypeError, match="bool"):
            store.gather_into(name, idx, out)
    with pytest.raises(TypeError, match="bool"):
        store.get_csr_padded("b_csr", torch.tensor([2, 0]), 3, dtype=torch.bool)
    with pytest.raises(TypeError, match="bool"):
        store.get_csr_padded("b_csr", torch.tensor([2, 0]), 3,
                             out=torch.empty(2, 3, 1, dtype=torch.bool, device=DEV))


def test_bool_variable_round_trips_as_bytes(store):
    arr = (torch.arange(40).view(10, 4) % 3 == 0)
    store.add("b_bool", arr)
    store.add_csr("b_bool_csr", arr.reshape(-1), torch.full((10,), 4))
    idx = torch.tensor([9, 0, 4, 4], device=DEV)
    hidx = idx.cpu()
    as_bool = store.get_batch("b_bool", idx, dtype=torch.bool)
    as_u8 = store.get_batch("b_bool", idx, dtype=torch.uint8)
    out = torch.empty(4, 4, dtype=torch.bool, device=DEV)
    store.gather_into("b_bool", idx, out)
    dense_b, _ = store.get_csr_padded("b_bool_csr", idx, 5, dtype=torch.bool,
                                      pad_value=True)
    dense_u, _ = store.get_csr_padded("b_bool_csr", idx, 5, dtype=torch.uint8)
    torch.cuda.synchronize()
    assert as_bool.dtype == torch.bool and as_u8.dtype == torch.uint8
    # the bytes themselves are 0 / 1
    want = arr[hidx].view(torch.uint8)
    assert torch.equal(as_bool.cpu().view(torch.uint8), want)
    assert torch.equal(as_u8.cpu(), want)
    assert torch.equal(out.cpu().view(torch.uint8), want)
    assert torch.equal(dense_b.cpu().view(torch.uint8)[:, :4, 0], want)
    assert (dense_b.cpu().view(torch.uint8)[:, 4] == 1).all()
    assert torch.equal(dense_u.cpu()[:, :4, 0], want)
