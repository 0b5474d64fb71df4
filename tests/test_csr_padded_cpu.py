"""Padded CSR gather, host (shm) path: ``get_csr_padded`` and
``PrefetchLoader(pad_to=...)`` against a pure-torch reference built from the
arrays handed to ``add_csr``: ``ref[i, :min(len, L)] = transform(sample[:L])``,
the rest of each row is the pad, lengths come from the input."""
import numpy as np
import pytest
import torch

from tests.dist_utils import run_dist

pytestmark = pytest.mark.timeout(300)

LENS = [3, 0, 4, 2, 5, 2, 1, 6]
DISP = 2


def _samples(lens, disp, dtype=torch.float32, base=0):
    """Per-sample (len, disp) tensors with distinct values."""
    out, v = [], base
    for n in lens:
        out.append(torch.arange(v, v + n * disp).reshape(n, disp).to(dtype))
        v += n * disp
    return out


def _ref(samples, idx, L, disp, out_dtype, pad_value, transform=None):
    """Reference batch; an index outside the sample list is an all-pad row."""
    pad = torch.tensor([pad_value], dtype=out_dtype)
    dense = pad.repeat(len(idx), L, disp)
    lens = torch.zeros(len(idx), dtype=torch.int64)
    for i, g in enumerate(idx):
        if not 0 <= g < len(samples):
            continue
        s = samples[g]
        lens[i] = s.shape[0]
        k = min(s.shape[0], L)
        x = s[:k]
        dense[i, :k] = transform(x) if transform is not None else x.to(out_dtype)
    return dense, lens


@pytest.fixture
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    yield s
    s.free()


def _add(store, name, samples, lens):
    store.add_csr(name, torch.cat(samples), np.asarray(lens))


def test_semantics(store):
    samples = _samples(LENS, DISP)
    _add(store, "c", samples, LENS)
    idx = [7, 1, 1, 4, 0]
    dense, lengths = store.get_csr_padded("c", idx, 4, pad_value=-1)
    ref, _ = _ref(samples, idx, 4, DISP, torch.float32, -1)
    assert dense.shape == (5, 4, DISP) and dense.dtype == torch.float32
    assert torch.equal(dense, ref)
    assert lengths.dtype == torch.int64
    assert lengths.tolist() == [6, 0, 0, 5, 3]


def test_cast_and_affine(store):
    samples = _samples(LENS, DISP, torch.uint8)
    _add(store, "u", samples, LENS)
    idx = [7, 1, 1, 4, 0]
    dense, lengths = store.get_csr_padded("u", idx, 4, dtype=torch.float32,
                                          pad_value=-1)
    ref, rl = _ref(samples, idx, 4, DISP, torch.float32, -1)
    assert dense.dtype == torch.float32
    assert torch.equal(dense, ref) and torch.equal(lengths, rl)

    dense, _ = store.get_csr_padded("u", idx, 4, dtype=torch.float32,
                                    affine=(2.0, -1.0), pad_value=-1)
    ref, _ = _ref(samples, idx, 4, DISP, torch.float32, -1,
                  transform=lambda x: x.to(torch.float32) * 2.0 - 1.0)
    assert torch.equal(dense, ref)  # the pad stays -1, not -1*2-1

    with pytest.raises(TypeError):
        store.get_csr_padded("u", idx, 4, dtype=torch.int32, affine=(2.0, -1.0))


def test_out_of_range(store):
    samples = _samples(LENS, DISP)
    _add(store, "c", samples, LENS)
    idx = [2, 8, 5]
    dense, lengths = store.get_csr_padded("c", idx, 4, pad_value=-1)
    ref, rl = _ref(samples, idx, 4, DISP, torch.float32, -1)
    assert torch.equal(dense, ref)
    assert (dense[1] == -1).all()
    assert lengths.tolist() == [4, 0, 2] and torch.equal(lengths, rl)
    assert store.query("c")["oob_skipped"] == 1


def test_argument_errors(store):
    samples = _samples(LENS, DISP)
    _add(store, "c", samples, LENS)
    store.add("fixed", torch.zeros(4, 2))
    with pytest.raises(ValueError):
        store.get_csr_padded("fixed", [0], 4)
    with pytest.raises(ValueError):
        store.get_csr_padded("c", [0], 0)
    with pytest.raises(ValueError):  # one row too many
        store.get_csr_padded("c", [0, 1], 4, out=torch.empty(3, 4, DISP))
    with pytest.raises(ValueError):  # right size, wrong dtype
        store.get_csr_padded("c", [0, 1], 4,
                             out=torch.empty(2, 4, DISP, dtype=torch.float64),
                             dtype=torch.float32)
    # n == 0: empty results
    dense, lengths = store.get_csr_padded("c", [], 4)
    assert dense.shape == (0, 4, DISP) and lengths.shape == (0,)
    # a matching out is filled and returned
    buf = torch.full((2, 4, DISP), 7.0)
    dense, _ = store.get_csr_padded("c", [0, 1], 4, out=buf, pad_value=-1)
    ref, _ = _ref(samples, [0, 1], 4, DISP, torch.float32, -1)
    assert dense.data_ptr() == buf.data_ptr() and torch.equal(buf, ref)


def _w_two_ranks(rank, world):
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    all_lens = [LENS, LENS[::-1]]
    per_rank = [_samples(all_lens[0], DISP, base=0),
                _samples(all_lens[1], DISP, base=1000)]
    s.add_csr("c", torch.cat(per_rank[rank]), np.asarray(all_lens[rank]))
    samples = per_rank[0] + per_rank[1]
    idx = [15, 0, 8, 7, 9, 4, 12, 1]  # both shards, from every rank
    dense, lengths = s.get_csr_padded("c", idx, 4, pad_value=-1)
    ref, rl = _ref(samples, idx, 4, DISP, torch.float32, -1)
    assert torch.equal(dense, ref)
    assert torch.equal(lengths, rl)
    s.free()


def test_two_ranks():
    run_dist(_w_two_ranks, 2)


def test_gnn_example_padded():
    """The GNN example's opt-in --padded path trains end to end."""
    import os
    import re
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(
        [sys.executable, "examples/gnn_csr_train.py", "--epochs", "1",
         "--graphs-per-rank", "1500", "--device", "cpu", "--padded"],
        cwd=root, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"loss ([0-9.]+) acc ([0-9.]+)", r.stdout)
    assert m, r.stdout
    assert np.isfinite(float(m.group(1)))


def test_prefetch_pad_to(store):
    from ddstore_amd import PrefetchLoader

    samples = _samples(LENS, DISP)
    _add(store, "c", samples, LENS)
    store.add("y", torch.arange(8, dtype=torch.int64).unsqueeze(1))
    order = torch.tensor([5, 2, 7, 0, 1, 6, 3, 4])
    loader = PrefetchLoader(store, "c", order, 3, pad_to=4, pad_value=-1)
    batches = list(loader)
    assert [b[0].shape for b in batches] == [(3, 4, DISP), (3, 4, DISP), (2, 4, DISP)]
    for k, (dense, lengths) in enumerate(batches):
        ids = order[3 * k: 3 * k + 3]
        d, l = store.get_csr_padded("c", ids, 4, pad_value=-1)
        assert lengths.shape == (ids.numel(),)
        assert torch.equal(dense, d) and torch.equal(lengths, l)
    # with a label variable, a cast and an affine
    loader = PrefetchLoader(store, "c", order, 3, pad_to=4, pad_value=-1,
                            out_dtype=torch.bfloat16, affine=(0.5, 1.0),
                            label_name="y")
    for k, ((dense, lengths), y) in enumerate(loader):
        ids = order[3 * k: 3 * k + 3]
        d, l = store.get_csr_padded("c", ids, 4, dtype=torch.bfloat16,
                                    affine=(0.5, 1.0), pad_value=-1)
        assert dense.dtype == torch.bfloat16
        assert torch.equal(dense, d) and torch.equal(lengths, l)
        assert torch.equal(y.view(-1), ids)
    # unchanged without pad_to: affine on ragged CSR is still refused, and
    # pad_to on a fixed-stride variable is an error
    with pytest.raises(ValueError, match="affine is not supported for CSR"):
        PrefetchLoader(store, "c", order, 3, affine=(0.5, 1.0))
    with pytest.raises(ValueError):
        PrefetchLoader(store, "y", order, 3, pad_to=4)
