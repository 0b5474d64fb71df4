"""Padded CSR gather on the GPU: ``get_csr_padded`` and
``PrefetchLoader(pad_to=...)`` against a pure-torch reference built on the
CPU from the arrays handed to ``add_csr``:
``ref[i, :min(len, L)] = transform(sample[:L])``, the rest of each row is the
pad, lengths come from the input. Run with ``pytest -m gpu``."""
import functools

import numpy as np
import pytest
import torch

from tests.dist_utils import run_dist

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

NS, NI, L, PAD = 64, 40, 6, -3


def _lens():
    lens = np.random.default_rng(0).integers(0, 10, NS)
    lens[0], lens[1] = 0, 9
    return lens


LENS = _lens()
IDX = np.random.default_rng(1).integers(0, NS, NI)
GOFF = np.concatenate([[0], np.cumsum(LENS)])


@functools.lru_cache(maxsize=None)
def values(dtype, disp):
    """The (total_elems, disp) payload handed to add_csr, on the CPU."""
    g = torch.Generator().manual_seed(1234 + disp)
    n = int(LENS.sum())
    if dtype == torch.bool:
        return torch.randint(0, 2, (n, disp), generator=g).to(torch.bool)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (n, disp), generator=g).to(torch.uint8)
    if dtype == torch.int64:
        return torch.randint(-(2 ** 50), 2 ** 50, (n, disp), generator=g)
    return torch.randn(n, disp, generator=g).to(dtype)


def reference(vals, idx, max_len, out_dtype, pad_value, transform=None):
    """(dense, lengths) on the CPU; an index outside [0, NS) is an all-pad
    row of length 0."""
    disp = vals.shape[1]
    dense = torch.tensor([pad_value], dtype=out_dtype).repeat(len(idx), max_len, disp)
    lens = torch.zeros(len(idx), dtype=torch.int64)
    for i, g in enumerate(idx):
        g = int(g)
        if not 0 <= g < NS:
            continue
        lens[i] = int(LENS[g])
        k = min(int(LENS[g]), max_len)
        x = vals[GOFF[g]: GOFF[g] + k]
        dense[i, :k] = transform(x) if transform is not None else x.to(out_dtype)
    return dense, lens


def assert_bits_equal(got, exp, msg=""):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (msg, got.shape, got.dtype)
    a = got.cpu().contiguous().view(torch.uint8)
    b = exp.contiguous().view(torch.uint8)
    assert torch.equal(a, b), msg


@pytest.fixture
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cuda:0")
    assert s.mode == "hip", "GPU test must exercise the native HIP path"
    yield s
    s.free()


def add(store, dtype, disp):
    name = f"c_{str(dtype).split('.')[-1]}_{disp}"
    store.add_csr(name, values(dtype, disp), LENS)
    return name


def check(store, name, vals, idx, max_len, out_dtype, pad_value=PAD, **kw):
    dense, lengths = store.get_csr_padded(name, idx, max_len, pad_value=pad_value, **kw)
    torch.cuda.synchronize()
    assert dense.is_cuda and lengths.is_cuda and lengths.dtype == torch.int64
    ref, rl = reference(vals, idx, max_len, out_dtype, pad_value)
    assert_bits_equal(dense, ref, f"{name} L={max_len}")
    assert torch.equal(lengths.cpu(), rl)
    return dense, lengths


def test_vector_byte_move(store):
    name = add(store, torch.float32, 4)
    check(store, name, values(torch.float32, 4), IDX, L, torch.float32)
    assert store.query(name)["oob_skipped"] == 0


def test_elementwise_fallbacks(store):
    # 12-B elements: no 16-B unit
    name = add(store, torch.float32, 3)
    check(store, name, values(torch.float32, 3), IDX, L, torch.float32)
    # 5 % 8 != 0: element-wise cast
    name = add(store, torch.uint8, 5)
    check(store, name, values(torch.uint8, 5), IDX, L, torch.bfloat16,
          dtype=torch.bfloat16)
    # a 4-byte-offset view as the output: vector-eligible rows, unaligned out
    name = add(store, torch.float32, 4)
    vals = values(torch.float32, 4)
    for dt in (torch.float32, torch.bfloat16):
        nel = NI * L * 4
        big = torch.full((nel + 8,), 99.0, dtype=dt, device="cuda:0")
        off = 4 // big.element_size()
        view = big[off: off + nel]
        assert view.data_ptr() % 16 == 4
        dense, _ = store.get_csr_padded(name, IDX, L, out=view, pad_value=PAD)
        torch.cuda.synchronize()
        ref, _ = reference(vals, IDX, L, dt, PAD)
        assert dense.data_ptr() == view.data_ptr()
        assert_bits_equal(dense, ref)
        # nothing outside the view was touched
        assert (big[:off] == 99.0).all() and (big[off + nel:] == 99.0).all()


@pytest.mark.parametrize("tin,disp,tout,max_len", [
    (torch.float32, 1, torch.float32, 8),    # same dtype, dword-granular
    (torch.float32, 3, torch.float32, 4),    # 12 elements = 3 chunks per row
    (torch.float32, 3, torch.bfloat16, 8),
    (torch.uint8, 5, torch.bfloat16, 8),     # byte loads, 40 elements = 5 chunks
    (torch.int64, 1, torch.int64, 6),        # two elements per chunk
], ids=lambda v: str(v).split(".")[-1])
def test_vector_stores_element_loads(store, tin, disp, tout, max_len):
    """disp % VEC != 0 but the row is a whole number of 16-B chunks: 16-B
    stores fed by element loads, chunks straddling the valid/pad boundary
    (lengths 0..9 put the boundary at every position in a chunk)."""
    name = add(store, tin, disp)
    vals = values(tin, disp)
    check(store, name, vals, IDX, max_len, tout, dtype=tout)
    # and with a sentinel underneath: every element written
    sentinel = 99
    out = torch.full((NI, max_len, disp), sentinel, dtype=tout, device="cuda:0")
    store.get_csr_padded(name, IDX, max_len, out=out, pad_value=PAD)
    torch.cuda.synchronize()
    ref, _ = reference(vals, IDX, max_len, tout, PAD)
    assert_bits_equal(out, ref)
    scale, shift = 0.0234375, -1.5
    if tout.is_floating_point and tin != torch.float32:
        dense, _ = store.get_csr_padded(name, IDX, max_len, dtype=tout,
                                        affine=(scale, shift), pad_value=PAD)
        ref, _ = reference(
            vals, IDX, max_len, tout, PAD,
            transform=lambda x: (x.to(torch.float64) * scale + shift).to(
                torch.float32).to(tout))
        assert_bits_equal(dense, ref)


@pytest.mark.parametrize("max_len", [8, 9, 16, 17, 32, 33, 64, 65, 300])
def test_lane_group_sizes(store, max_len):
    """f32 disp=4 is one 16-B chunk per element, so max_len is the chunks per
    row: both sides of every lane-group threshold (8, 16, 32, 64 lanes), the
    whole-block group for few long rows, and rows of more chunks than lanes."""
    name = add(store, torch.float32, 4)
    check(store, name, values(torch.float32, 4), IDX, max_len, torch.float32)
    name = add(store, torch.uint8, 16)
    check(store, name, values(torch.uint8, 16), IDX, max_len, torch.float32,
          dtype=torch.float32)


def test_long_rows_many_samples(store):
    # >= 4096 rows of 70 chunks: 64 lanes per row, two passes over the row
    idx = np.random.default_rng(4).integers(0, NS, 4096)
    name = add(store, torch.float32, 4)
    check(store, name, values(torch.float32, 4), idx, 70, torch.float32)


@pytest.mark.parametrize("tin,disp,tout", [
    (torch.uint8, 16, torch.bfloat16),
    (torch.uint8, 16, torch.float32),
    (torch.float16, 8, torch.float32),
    (torch.float8_e4m3fn, 16, torch.bfloat16),
], ids=lambda v: str(v).split(".")[-1])
def test_cast_vector_path(store, tin, disp, tout):
    name = add(store, tin, disp)
    vals = values(tin, disp)
    dense, lengths = store.get_csr_padded(name, IDX, L, dtype=tout, pad_value=PAD)
    torch.cuda.synchronize()
    ref, rl = reference(vals, IDX, L, tout, PAD)  # the torch cast of the samples
    assert dense.dtype == tout and torch.equal(dense.cpu(), ref)
    assert torch.equal(lengths.cpu(), rl)


@pytest.mark.parametrize("tout", [torch.float32, torch.bfloat16],
                         ids=lambda v: str(v).split(".")[-1])
@pytest.mark.parametrize("tin,disp", [(torch.uint8, 16), (torch.float16, 8),
                                      (torch.uint8, 5)],
                         ids=lambda v: str(v).split(".")[-1])
def test_affine(store, tin, disp, tout):
    # scale and shift have 2 significant bits each, so x * scale + shift in
    # float64 is the exactly rounded f32 fmaf once rounded to f32
    scale, shift = 0.0234375, -1.5
    name = add(store, tin, disp)
    vals = values(tin, disp)
    dense, lengths = store.get_csr_padded(name, IDX, L, dtype=tout,
                                          affine=(scale, shift), pad_value=PAD)
    torch.cuda.synchronize()

    def xf(x):
        return (x.to(torch.float32).to(torch.float64) * scale + shift).to(
            torch.float32).to(tout)

    ref, rl = reference(vals, IDX, L, tout, PAD, transform=xf)
    assert_bits_equal(dense, ref)
    assert torch.equal(lengths.cpu(), rl)
    # the pad is -3 exactly, not -3 * scale + shift
    short = int(np.argmin(LENS[IDX]))
    assert LENS[IDX[short]] < L and float(dense[short, L - 1, 0]) == float(PAD)
    with pytest.raises(TypeError):
        store.get_csr_padded(name, IDX, L, dtype=torch.int32, affine=(scale, shift))


@pytest.mark.parametrize("disp", [1, 2])
def test_pad_bits_int64(store, disp):
    # exact 64-bit pad, not routed through a float
    pad = -(2 ** 40)
    name = add(store, torch.int64, disp)
    dense, _ = check(store, name, values(torch.int64, disp), IDX, L, torch.int64,
                     pad_value=pad)
    short = int(np.argmin(LENS[IDX]))
    assert int(dense[short, L - 1, 0]) == pad


@pytest.mark.parametrize("disp", [3, 16])
def test_pad_bits_bool(store, disp):
    name = add(store, torch.bool, disp)
    dense, _ = check(store, name, values(torch.bool, disp), IDX, L, torch.bool,
                     pad_value=True)
    assert dense.dtype == torch.bool
    short = int(np.argmin(LENS[IDX]))
    assert bool(dense[short, L - 1, 0]) is True


@pytest.mark.parametrize("tin,disp,tout,sentinel", [
    (torch.float32, 4, torch.float32, 1e30),     # vector byte move
    (torch.uint8, 16, torch.bfloat16, 1e30),     # vector cast
    (torch.float32, 3, torch.float32, 1e30),     # element-wise
], ids=lambda v: str(v).split(".")[-1])
def test_every_element_written(store, tin, disp, tout, sentinel):
    name = add(store, tin, disp)
    vals = values(tin, disp)
    for max_len in (L, 1, 9):
        out = torch.full((NI, max_len, disp), sentinel, dtype=tout, device="cuda:0")
        dense, lengths = store.get_csr_padded(name, IDX, max_len, out=out,
                                              pad_value=PAD)
        torch.cuda.synchronize()
        assert dense.data_ptr() == out.data_ptr()
        ref, rl = reference(vals, IDX, max_len, tout, PAD)
        assert not (ref == torch.tensor(sentinel, dtype=tout)).any()
        assert not (out == sentinel).any(), f"sentinel survived, L={max_len}"
        assert_bits_equal(out, ref, f"L={max_len}")
        assert torch.equal(lengths.cpu(), rl)


def test_out_of_range(store):
    name = add(store, torch.float32, 4)
    idx = IDX.copy()
    idx[3], idx[17] = -1, NS
    dense, lengths = check(store, name, values(torch.float32, 4), idx, L, torch.float32)
    assert (dense[3] == PAD).all() and (dense[17] == PAD).all()
    assert lengths[3] == 0 and lengths[17] == 0
    assert store.query(name)["oob_skipped"] == 2
    store.reset_counters(name)  # keep a DDSTORE_STRICT=1 run clean


def test_stats(store):
    disp = 4
    name = add(store, torch.float32, disp)
    store.get_csr_padded(name, IDX, L)  # counters start from a used state
    store.reset_counters(name)
    store.get_csr_padded(name, IDX, L, pad_value=PAD)
    q = store.query(name)
    assert q["bytes_gathered"] == int(np.minimum(LENS[IDX], L).sum()) * disp * 4
    assert q["rows_gathered"] == NI
    assert q["n_gather"] == 1


def test_argument_errors(store):
    name = add(store, torch.float32, 4)
    store.add("fixed", torch.zeros(4, 2))
    with pytest.raises(ValueError):
        store.get_csr_padded("fixed", [0], L)
    with pytest.raises(ValueError):
        store.get_csr_padded(name, [0], 0)
    with pytest.raises(ValueError):
        store.get_csr_padded(name, [0, 1], L,
                             out=torch.empty(3, L, 4, device="cuda:0"))
    with pytest.raises(ValueError):  # not on the store device
        store.get_csr_padded(name, [0, 1], L, out=torch.empty(2, L, 4))
    dense, lengths = store.get_csr_padded(name, [], L)
    assert dense.shape == (0, L, 4) and lengths.shape == (0,)
    assert dense.is_cuda and lengths.is_cuda


@pytest.mark.parametrize("tin,disp,tout", [(torch.float32, 4, torch.float32),
                                           (torch.uint8, 5, torch.bfloat16)],
                         ids=lambda v: str(v).split(".")[-1])
def test_kernel_tail(store, tin, disp, tout):
    # 257 indices: more than one block, not a multiple of the block
    idx = np.random.default_rng(2).integers(0, NS, 257)
    name = add(store, tin, disp)
    check(store, name, values(tin, disp), idx, L, tout, dtype=tout)


def _dev(rank):
    return f"cuda:{rank % max(torch.cuda.device_count(), 1)}"


def _w_two_ranks(rank, world):
    from ddstore_amd import DDStore

    s = DDStore(device=_dev(rank))
    all_lens = [np.random.default_rng(100 + r).integers(1, 20, size=50)
                for r in range(world)]
    gid0 = rank * 50
    vals = torch.cat([torch.full((int(n), 2), float(gid0 + i))
                      for i, n in enumerate(all_lens[rank])])
    s.add_csr("c", vals, all_lens[rank])
    glens = np.concatenate(all_lens)
    idx = np.random.default_rng(5).integers(0, 50 * world, size=40)
    max_len, pad = 8, -3.0
    dense, lengths = s.get_csr_padded("c", idx, max_len, pad_value=pad)
    torch.cuda.synchronize()
    d = dense.cpu()
    assert d.shape == (40, max_len, 2)
    assert lengths.cpu().tolist() == [int(glens[g]) for g in idx]
    for k, g in enumerate(idx):
        n = min(int(glens[g]), max_len)
        assert (d[k, :n] == float(g)).all(), (g, d[k])
        assert (d[k, n:] == pad).all(), (g, d[k])
    assert s.query("c")["oob_skipped"] == 0
    s.free()


def test_two_ranks_one_gpu():
    run_dist(_w_two_ranks, 2)


def test_prefetch_side_stream(store):
    from ddstore_amd import PrefetchLoader

    name = add(store, torch.uint8, 16)
    affine = (0.0234375, -1.5)
    order = torch.from_numpy(np.random.default_rng(3).permutation(NS))
    loader = PrefetchLoader(store, name, order, 16, pad_to=L, pad_value=PAD,
                            out_dtype=torch.bfloat16, affine=affine)
    nb = 0
    for k, (dense, lengths) in enumerate(loader):
        ids = order[16 * k: 16 * (k + 1)]
        d, n = store.get_csr_padded(name, ids, L, dtype=torch.bfloat16,
                                    affine=affine, pad_value=PAD)
        assert dense.shape == (16, L, 16) and dense.dtype == torch.bfloat16
        assert_bits_equal(dense, d.cpu())
        assert torch.equal(lengths, n)
        nb += 1
    assert nb == NS // 16
    ref, rl = reference(
        values(torch.uint8, 16), order[-16:].tolist(), L, torch.bfloat16, PAD,
        transform=lambda x: (x.to(torch.float64) * affine[0] + affine[1]).to(
            torch.float32).to(torch.bfloat16))
    assert_bits_equal(d, ref)  # the direct call itself is right
    assert torch.equal(n.cpu(), rl)
