"""Contract of the native store classes (``_C.HostStore`` here, ``_C.DeviceStore``
in ``tests/test_gpu_native_contract.py``) below the Python layer: what the
registration, update and gather entry points refuse and with which words, that
a refused registration leaves the name free, and what one call of every gather
form adds to ``query()``'s counters.

The shapes are the smallest that tell the paths apart: one rank, a
fixed-stride variable of 8 rows of 4 f32 (16-byte rows), a CSR variable with
lengths ``[0, 3, 1, 2]`` and 2 f32 per element, the request ``[1, 3, 1]``,
``max_len = 2``. The expected counters follow from them:

* fixed-stride forms: 3 rows of 16 bytes = 48 bytes;
* ragged CSR forms: lengths 3 + 2 + 3 = 8 elements of 8 bytes = 64 bytes;
* padded forms: min(len, 2) summed = 6 elements = 48 bytes.

The ``check_*`` functions take a backend description and are shared with the
GPU file; kernel results are the other suites' business, a gathered value is
compared here only to show that the call went through."""
import itertools
import os
import struct

import pytest
import torch

pytestmark = pytest.mark.timeout(60)

F = torch.arange(32, dtype=torch.float32).reshape(8, 4)
LENS = [0, 3, 1, 2]
DISP = 2
V = torch.arange(12, dtype=torch.float32).reshape(6, DISP)
GOFF = torch.tensor([0, 0, 3, 4, 6], dtype=torch.int64)
IDX = [1, 3, 1]
OUT_OFF = [0, 3, 5, 8]                      # exclusive scan of the requested lengths
CSR_REF = torch.cat([V[0:3], V[4:6], V[0:3]])
MAX_LEN = 2
PAD_BITS = struct.unpack("<I", struct.pack("<f", -1.0))[0]

FIXED_BYTES = 3 * 16
CSR_BYTES = 8 * 8
PADDED_BYTES = 6 * 8

_serial = itertools.count()


class Host:
    """``_C.HostStore`` and the words that differ from the device store's."""
    dev = "cpu"
    add_contig = "ddstore add: array must be C-contiguous on CPU"
    add_csr_contig = "ddstore add_csr: values must be contiguous on CPU"
    update_contig = "ddstore update: array must be C-contiguous on CPU"
    # query() key order behind the static keys
    counter_keys = ["n_gather", "rows_gathered", "bytes_gathered", "oob_skipped",
                    "cap_skipped"]

    @staticmethod
    def new():
        from ddstore_amd import _C

        # a shm name of its own per store: nothing here meets another test's
        return _C.HostStore(f"contract{os.getpid()}n{next(_serial)}", 0, 1)


def refused(msg, fn, *args):
    """`fn(*args)` raises, and the first line of its text is exactly `msg`."""
    with pytest.raises(RuntimeError) as e:
        fn(*args)
    assert str(e.value).splitlines()[0] == msg


def counters(be, name):
    q = be.query(name)
    return q["n_gather"], q["rows_gathered"], q["bytes_gathered"]


def dev_tensor(b, data, dtype=torch.int64):
    return torch.tensor(data, dtype=dtype, device=b.dev)


def register(be):
    """The two variables every check below reads, finalized."""
    be.add("f", F, 8, 4, [8])
    be.open_peers("f", [b""])
    be.add_csr("c", V, 4, 6, DISP, [4], [6], GOFF)
    be.open_peers("c", [b""])


# ------------------------------------------------------------- registration
def registration_forms(b):
    """form -> (clean call, expected shard, [(refused call, its words)])."""
    f32 = torch.float32
    return {
        "add": (
            lambda be, n: be.add(n, F, 8, 4, [8]), F,
            [(lambda be, n: be.add(n, F, 7, 4, [7]), "ddstore add: shape mismatch"),
             (lambda be, n: be.add(n, F.t(), 8, 4, [8]), b.add_contig),
             (lambda be, n: be.add(n, F.to(torch.int16), 8, 4, [8]),
              "ddstore: unsupported dtype Short")]),
        "init": (
            lambda be, n: be.init(n, 8, 4, f32, [8]), torch.zeros_like(F),
            [(lambda be, n: be.init(n, 8, 4, torch.int16, [8]),
              "ddstore: unsupported dtype Short")]),
        "add_csr": (
            lambda be, n: be.add_csr(n, V, 4, 6, DISP, [4], [6], GOFF), V,
            [(lambda be, n: be.add_csr(n, V, 4, 5, DISP, [4], [5], GOFF),
              "ddstore add_csr: shape mismatch"),
             (lambda be, n: be.add_csr(n, V.t(), 4, 6, DISP, [4], [6], GOFF),
              b.add_csr_contig),
             (lambda be, n: be.add_csr(n, V, 4, 6, DISP, [4], [6], GOFF[:-1].clone()),
              "ddstore add_csr: bad global offsets"),
             (lambda be, n: be.add_csr(n, V, 4, 6, DISP, [4], [6], GOFF.to(torch.int32)),
              "ddstore add_csr: bad global offsets")]),
        "init_csr": (
            lambda be, n: be.init_csr(n, 4, 6, DISP, f32, [4], [6], GOFF),
            torch.zeros_like(V),
            [(lambda be, n: be.init_csr(n, 4, 6, DISP, f32, [4], [6],
                                        torch.cat([GOFF, GOFF[-1:]])),
              "ddstore init_csr: bad global offsets"),
             (lambda be, n: be.init_csr(n, 4, 6, DISP, f32, [4], [6],
                                        GOFF.to(torch.float64)),
              "ddstore init_csr: bad global offsets")]),
    }


def check_registration(b, form):
    clean, shard, bad = registration_forms(b)[form]
    be = b.new()
    try:
        for call, msg in bad:
            refused(msg, call, be, "v")
            assert not be.has("v")              # a refused name stays free
        clean(be, "v")
        assert be.has("v")
        assert torch.equal(be.local_shard("v").cpu(), shard)
        q = be.query("v")
        assert (q["nrows_total"], q["is_csr"], q["itemsize"]) == \
            (8 if shard.shape[1] == 4 else 4, shard.shape[1] == DISP, 4)
        refused("ddstore: variable 'v' already exists", clean, be, "v")
        for call, _ in bad:                     # the name is checked first
            refused("ddstore: variable 'v' already exists", call, be, "v")
        assert torch.equal(be.local_shard("v").cpu(), shard)
        be.free_var("v")
        assert not be.has("v")
        clean(be, "v")                          # and registers again
    finally:
        be.free_all()


@pytest.mark.parametrize("form", ["add", "init", "add_csr", "init_csr"])
def test_registration(form):
    check_registration(Host, form)


# ------------------------------------------------------------------ updates
def check_updates(b):
    be = b.new()
    try:
        be.init("f", 8, 4, torch.float32, [8])
        be.init_csr("c", 4, 6, DISP, torch.float32, [4], [6], GOFF)
        one = torch.ones(2, 4)
        refused("ddstore update: itemsize mismatch", be.update, "f", one.double(), 0)
        refused("ddstore update: shape mismatch", be.update, "f", torch.ones(6), 0)
        refused("ddstore update: out of range", be.update, "f", one, 7)
        refused("ddstore update: out of range", be.update, "f", one, -1)
        refused(b.update_contig, be.update, "f", torch.ones(4, 2).t(), 0)
        refused("ddstore update_elems: CSR variables only", be.update_elems, "f", one, 0)
        be.update("f", one, 6)                  # up to the end
        want = torch.zeros(8, 4)
        want[6:] = 1
        assert torch.equal(be.local_shard("f").cpu(), want)

        el = torch.ones(2, DISP)
        refused("ddstore update: itemsize mismatch", be.update_elems, "c", el.double(), 0)
        refused("ddstore update: shape mismatch", be.update_elems, "c", torch.ones(3), 0)
        refused("ddstore update: out of range", be.update_elems, "c", el, 5)
        refused("ddstore update: out of range", be.update_elems, "c", el, -1)
        refused(b.update_contig, be.update_elems, "c", torch.ones(DISP, 2).t(), 0)
        refused("ddstore update: not supported for CSR variables", be.update, "c", el, 0)
        be.update_elems("c", el, 4)
        want = torch.zeros(6, DISP)
        want[4:] = 1
        assert torch.equal(be.local_shard("c").cpu(), want)
        assert counters(be, "f") == (0, 0, 0) and counters(be, "c") == (0, 0, 0)
    finally:
        be.free_all()


def test_updates():
    check_updates(Host)


# ----------------------------------------------------------------- counters
def gather_forms(b):
    """form -> (variable, call(be) -> (result, reference), counters after it).
    The host store has the first and the fourth only."""
    idx = dev_tensor(b, IDX)

    def fixed(call, ref):
        def run(be):
            out = torch.empty(3, 4, device=b.dev)
            call(be, out)
            return out, ref
        return run

    def ragged(call):
        def run(be):
            out = torch.empty(8, DISP, device=b.dev)
            call(be, out)
            return out, CSR_REF
        return run

    def padded(call, xf):
        def run(be):
            out = torch.empty(3 * MAX_LEN * DISP, device=b.dev)
            lengths = torch.empty(3, dtype=torch.int64, device=b.dev)
            call(be, out, lengths)
            assert lengths.tolist() == [3, 2, 3]
            ref = torch.stack([V[0:2], V[4:6], V[0:2]])
            return out.view(3, MAX_LEN, DISP), xf(ref)
        return run

    def ones(n, v):
        return torch.full((n,), v, dtype=torch.float32, device=b.dev)

    rows = F[IDX]
    forms = {
        "gather": ("f", fixed(lambda be, o: be.gather("f", idx, o), rows),
                   (1, 3, FIXED_BYTES)),
        "gather_csr": ("c", ragged(lambda be, o: be.gather_csr(
            "c", idx, dev_tensor(b, OUT_OFF), o, 8)), (1, 3, CSR_BYTES)),
    }
    if b.dev == "cpu":
        return forms
    forms.update({
        "gather_affine": ("f", fixed(
            lambda be, o: be.gather_affine("f", idx, o, 2.0, 1.0), rows * 2 + 1),
            (1, 3, FIXED_BYTES)),
        "gather_affine_cols": ("f", fixed(
            lambda be, o: be.gather_affine_cols("f", idx, o, ones(4, 2.0), ones(4, 1.0)),
            rows * 2 + 1), (1, 3, FIXED_BYTES)),
        "gather_csr_fast": ("c", ragged(
            lambda be, o: be.gather_csr_fast("c", idx, o)), (1, 3, CSR_BYTES)),
        "gather_csr_padded": ("c", padded(
            lambda be, o, ln: be.gather_csr_padded("c", idx, o, ln, MAX_LEN, PAD_BITS),
            lambda r: r), (1, 3, PADDED_BYTES)),
        "gather_csr_padded_affine": ("c", padded(
            lambda be, o, ln: be.gather_csr_padded("c", idx, o, ln, MAX_LEN, PAD_BITS,
                                                   True, 2.0, 1.0),
            lambda r: r * 2 + 1), (1, 3, PADDED_BYTES)),
        "gather_csr_padded_cols": ("c", padded(
            lambda be, o, ln: be.gather_csr_padded_cols(
                "c", idx, o, ln, MAX_LEN, PAD_BITS, ones(DISP, 2.0), ones(DISP, 1.0)),
            lambda r: r * 2 + 1), (1, 3, PADDED_BYTES)),
    })
    return forms


def check_counters(b, form):
    name, run, want = gather_forms(b)[form]
    be = b.new()
    try:
        register(be)
        keys = ["nrows_local", "nrows_total", "disp", "itemsize", "is_csr", "prefix"]
        assert list(be.query("f")) == keys + b.counter_keys
        assert list(be.query("c")) == keys + ["nelems_local", "elem_prefix"] + \
            b.counter_keys
        assert counters(be, name) == (0, 0, 0)
        got, ref = run(be)
        assert counters(be, name) == want
        assert torch.equal(got.cpu(), ref)
        other = "c" if name == "f" else "f"
        assert counters(be, other) == (0, 0, 0)
        q = be.query(name)
        assert (q["oob_skipped"], q["cap_skipped"]) == (0, 0)
        run(be)
        assert counters(be, name) == tuple(2 * x for x in want)
        be.reset_counters(name)
        assert counters(be, name) == (0, 0, 0)
    finally:
        be.free_all()


@pytest.mark.parametrize("form", ["gather", "gather_csr"])
def test_counters(form):
    check_counters(Host, form)


# ------------------------------------------------------------ output checks
def test_output_checks():
    be = Host.new()
    try:
        register(be)
        idx = torch.tensor(IDX)
        words = "ddstore gather: output must be a contiguous CPU tensor of the store dtype"
        refused(words, be.gather, "f", idx, torch.empty(4, 3).t())
        refused(words, be.gather, "f", idx, torch.empty(3, 4, dtype=torch.float64))
        refused("ddstore gather: shape mismatch", be.gather, "f", idx, torch.empty(2, 4))
        off = torch.tensor(OUT_OFF)
        words = "ddstore gather_csr: bad output tensor"
        refused(words, be.gather_csr, "c", idx, off, torch.empty(DISP, 8).t(), 8)
        refused(words, be.gather_csr, "c", idx, off, torch.empty(7, DISP), 8)
        refused(words, be.gather_csr, "c", idx, off,
                torch.empty(8, DISP, dtype=torch.float64), 8)
        refused("ddstore gather: use gather_csr for CSR variables", be.gather, "c", idx,
                torch.empty(3, 4))
        refused("ddstore gather_csr: not a CSR variable", be.gather_csr, "f", idx, off,
                torch.empty(8, DISP), 8)
        # a refused call counts nothing
        assert counters(be, "f") == (0, 0, 0) and counters(be, "c") == (0, 0, 0)
    finally:
        be.free_all()
