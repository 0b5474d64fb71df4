"""The contract of ``tests/test_native_contract_cpu.py`` on ``_C.DeviceStore``:
the same checks through the same functions, every gather form the device
store has (fixed-stride plain, scalar and per-column affine; ragged CSR into a
sized and into a capacity buffer; padded CSR plain, scalar and per-column
affine), and the output check of each form. Run with ``pytest -m gpu``."""
import pytest
import torch

from tests import test_native_contract_cpu as nc
from tests.test_native_contract_cpu import DISP, IDX, MAX_LEN, OUT_OFF, PAD_BITS, refused

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

DEV = "cuda:0"


class Device:
    """``_C.DeviceStore`` and the words that differ from the host store's."""
    dev = DEV
    add_contig = "ddstore add: array must be C-contiguous"
    add_csr_contig = "ddstore add_csr: values must be contiguous"
    update_contig = "ddstore update: array must be C-contiguous"
    counter_keys = ["n_gather", "rows_gathered", "oob_skipped", "cap_skipped",
                    "bytes_gathered"]

    @staticmethod
    def new():
        from ddstore_amd import _C

        return _C.DeviceStore(0, 0, 1)


@pytest.mark.parametrize("form", ["add", "init", "add_csr", "init_csr"])
def test_registration(form):
    nc.check_registration(Device, form)


def test_goff_must_be_on_the_cpu():
    be = Device.new()
    try:
        goff = nc.GOFF.to(DEV)
        refused("ddstore add_csr: bad global offsets", be.add_csr, "v", nc.V, 4, 6, DISP,
                [4], [6], goff)
        refused("ddstore init_csr: bad global offsets", be.init_csr, "v", 4, 6, DISP,
                torch.float32, [4], [6], goff)
        assert not be.has("v")
    finally:
        be.free_all()


def test_updates():
    nc.check_updates(Device)


FORMS = ["gather", "gather_affine", "gather_affine_cols", "gather_csr", "gather_csr_fast",
         "gather_csr_padded", "gather_csr_padded_affine", "gather_csr_padded_cols"]


@pytest.mark.parametrize("form", FORMS)
def test_counters(form):
    nc.check_counters(Device, form)


def test_csr_lens_counts_nothing():
    be = Device.new()
    try:
        nc.register(be)
        lens = torch.empty(3, dtype=torch.int64, device=DEV)
        be.csr_lens("c", nc.dev_tensor(Device, IDX), lens)
        assert lens.tolist() == [3, 2, 3]
        assert nc.counters(be, "c") == (0, 0, 0)
    finally:
        be.free_all()


def test_output_checks():
    be = Device.new()
    try:
        nc.register(be)
        idx = nc.dev_tensor(Device, IDX)
        off = nc.dev_tensor(Device, OUT_OFF)

        def ones(n):
            return torch.ones(n, device=DEV)

        # fixed-stride forms: (3, 4) f32 wanted
        place = "ddstore gather: output must be a contiguous tensor on the store device"
        count = "ddstore gather: shape mismatch"
        for call in (lambda o: be.gather("f", idx, o),
                     lambda o: be.gather_affine("f", idx, o, 2.0, 1.0),
                     lambda o: be.gather_affine_cols("f", idx, o, ones(4), ones(4))):
            refused(place, call, torch.empty(4, 3, device=DEV).t())
            refused(place, call, torch.empty(3, 4))
            refused(count, call, torch.empty(2, 4, device=DEV))
        words = "ddstore gather: affine output must be f32/f16/bf16"
        i32 = torch.empty(3, 4, dtype=torch.int32, device=DEV)
        refused(words, be.gather_affine, "f", idx, i32, 2.0, 1.0)
        refused(words, be.gather_affine_cols, "f", idx, i32, ones(4), ones(4))

        # ragged forms: 8 elements of 2 f32 wanted (the capacity form takes any size)
        place = "ddstore gather_csr: bad output tensor"
        for call in (lambda o: be.gather_csr("c", idx, off, o, 8),
                     lambda o: be.gather_csr_fast("c", idx, o)):
            refused(place, call, torch.empty(DISP, 8, device=DEV).t())
            refused(place, call, torch.empty(8, DISP))
            refused(place, call, torch.empty(8, DISP, dtype=torch.float64, device=DEV))
        refused("ddstore gather_csr: output too small", be.gather_csr, "c", idx, off,
                torch.empty(7, DISP, device=DEV), 8)

        # padded forms: 3 * 2 * 2 f32 wanted
        lengths = torch.empty(3, dtype=torch.int64, device=DEV)
        place = ("ddstore gather_csr_padded: output must be a contiguous tensor on the "
                 "store device")
        count = "ddstore gather_csr_padded: shape mismatch"
        for call in (
                lambda o: be.gather_csr_padded("c", idx, o, lengths, MAX_LEN, PAD_BITS),
                lambda o: be.gather_csr_padded("c", idx, o, lengths, MAX_LEN, PAD_BITS,
                                               True, 2.0, 1.0),
                lambda o: be.gather_csr_padded_cols("c", idx, o, lengths, MAX_LEN,
                                                    PAD_BITS, ones(DISP), ones(DISP))):
            refused(place, call, torch.empty(4, 3, device=DEV).t())
            refused(place, call, torch.empty(12))
            refused(count, call, torch.empty(11, device=DEV))
        words = "ddstore gather_csr_padded: bad lengths tensor"
        good = torch.empty(12, device=DEV)
        refused(words, be.gather_csr_padded, "c", idx, good, lengths[:2], MAX_LEN, PAD_BITS)
        refused(words, be.gather_csr_padded_cols, "c", idx, good, lengths[:2], MAX_LEN,
                PAD_BITS, ones(DISP), ones(DISP))
        words = "ddstore gather_csr_padded: affine output must be f32/f16/bf16"
        i32 = torch.empty(12, dtype=torch.int32, device=DEV)
        refused(words, be.gather_csr_padded, "c", idx, i32, lengths, MAX_LEN, PAD_BITS,
                True, 2.0, 1.0)
        refused(words, be.gather_csr_padded_cols, "c", idx, i32, lengths, MAX_LEN,
                PAD_BITS, ones(DISP), ones(DISP))

        # a per-column vector of the wrong length, and the wrong variable kind
        refused("ddstore: a per-column affine vector must be a contiguous float32 "
                "tensor of disp = 4 values on the store device",
                be.gather_affine_cols, "f", idx, torch.empty(3, 4, device=DEV), ones(3),
                ones(4))
        refused("ddstore gather: use gather_csr for CSR variables", be.gather_affine_cols,
                "c", idx, torch.empty(3, 4, device=DEV), ones(4), ones(4))
        refused("ddstore gather_csr_padded: not a CSR variable", be.gather_csr_padded_cols,
                "f", idx, torch.empty(12, device=DEV), lengths, MAX_LEN, PAD_BITS,
                ones(DISP), ones(DISP))
        # a refused call counts nothing
        assert nc.counters(be, "f") == (0, 0, 0) and nc.counters(be, "c") == (0, 0, 0)
    finally:
        be.free_all()
