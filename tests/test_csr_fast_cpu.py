"""The one-call CSR fetch model (tests/csr_fast_ref.py) proven without a
GPU: the vectorised ``expected`` against a per-sample loop, and the whole
case table -- exact capacity and every clamp cut -- through the same
``check`` the GPU tests use, against the host backend."""
import pytest
import torch

from tests import csr_fast_ref as ref


@pytest.fixture
def store():
    from ddstore_amd import DDStore

    s = DDStore(device="cpu")
    yield s
    s.free()


def loop_expected(vals, lens, idx, cap):
    """The model of csr_fast_ref's docstring, one sample at a time."""
    goff = [0]
    for n in lens:
        goff.append(goff[-1] + int(n))
    off, keep, chunks = [0], [], []
    for g in idx.tolist():
        n = int(lens[g]) if 0 <= g < len(lens) else 0
        if n:
            chunks.append(vals[goff[g]: goff[g] + n])
        off.append(off[-1] + n)
        keep.append(n > 0 and off[-1] <= cap)
    packed = torch.cat(chunks) if chunks else vals[:0]
    return torch.tensor(off), torch.tensor(keep, dtype=torch.bool), packed


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.id)
def test_table_is_what_it_claims(case):
    eb = ref.elem_bytes(case)
    vals, lens, idx = ref.case_data(case.id)
    assert idx.numel() == ref.NIDX and idx.unique().numel() == len(lens)
    assert vals.shape == (sum(lens), case.disp) and vals.dtype == case.dtype
    if eb <= ref.ITEM_BYTES:
        ie = ref.ITEM_BYTES // eb
        assert lens[:13] == list(range(13))
        assert lens[13:19] == [ie - 1, ie, ie + 1, 2 * ie, 2 * ie + 1, 3 * ie - 1]
    else:
        assert lens[:6] == list(range(6))
    assert ref.exact_cap(lens, idx) * eb < 4 << 20  # a few MB at most


@pytest.mark.parametrize("case", [ref.CASE_BY_ID[k] for k in ("f32x1", "u8x3", "f32x300")],
                         ids=lambda c: c.id)
def test_expected_matches_loop(case):
    vals, lens, idx = ref.case_data(case.id)
    ns = len(lens)
    bad = idx.clone()
    bad[[3, 17, 256, 299]] = torch.tensor([-1, ns, 2 ** 40, -2 ** 63])
    total = ref.exact_cap(lens, idx)
    for ix in (idx, bad):
        for cap in (total, total // 2, 4, 0):
            off, keep, packed = ref.expected(vals, lens, ix, cap)
            off2, keep2, packed2 = loop_expected(vals, lens, ix, cap)
            assert torch.equal(off, off2) and torch.equal(keep, keep2)
            assert torch.equal(packed.view(torch.uint8), packed2.view(torch.uint8))


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.id)
def test_case_table_host_backend(store, case):
    name, vals, lens, idx = ref.register(store, case)
    f = ref.check(store, name, vals, lens, idx, ref.exact_cap(lens, idx),
                  case.byte_offset)
    assert f.out.data_ptr() % 4 == (case.byte_offset % 4)


def test_checker_sees_single_bytes(store):
    """verify() itself: one wrong payload byte, one byte written inside out
    behind the kept samples, one in front of out, one far behind it, and one
    wrong offset are each reported."""
    case = ref.CASE_BY_ID["u8x3"]
    name, vals, lens, idx = ref.register(store, case)
    cap = ref.clamp_caps(case, lens, idx)["after_multi_item"]
    f = ref.check(store, name, vals, lens, idx, cap)
    kept_bytes = int(f.off[:-1][ref.expected(vals, lens, idx, cap)[1]].max()) * f.eb
    assert 0 < kept_bytes < cap * f.eb
    for pos, what in [(f.head + kept_bytes // 2, "payload differs"),
                      (f.head + cap * f.eb - 1, "outside the kept samples"),
                      (f.head - 1, "outside the kept samples"),
                      (f.backing.numel() - 1, "outside the kept samples")]:
        old = int(f.backing[pos])
        f.backing[pos] = old ^ 0x10
        with pytest.raises(AssertionError, match=what):
            f.verify(counters=False)
        f.backing[pos] = old
    f.verify(counters=False)
    f.off = f.off.clone()
    f.off[7] += 1
    with pytest.raises(AssertionError, match="offsets differ"):
        f.verify(counters=False)


@pytest.mark.parametrize("case", [ref.CASE_BY_ID[k] for k in ("f32x1", "u8x3")],
                         ids=lambda c: c.id)
def test_clamp_models_host_backend(store, case):
    # the table ends in zero-length samples, so every cut also has empty
    # samples behind the capacity: they are neither written nor counted
    name, vals, lens, idx = ref.register(store, case)
    for label, cap in ref.clamp_caps(case, lens, idx).items():
        f = ref.check(store, name, vals, lens, idx, cap, case.byte_offset)
        assert f.store.query(name)["cap_skipped"] > 0, label
