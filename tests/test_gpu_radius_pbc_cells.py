"""The cell-list path of the periodic radius-graph fetch on the GPU:
k_pbc_cells_box / count / fill with the k_cells_* binning kernels, on the cases
of tests/test_radius_pbc_cells_cpu.py against the float64 models. The shared
request's T+1 graph spans more than one block of dsts; the binning request
holds cells whose images are mostly skipped, atoms outside their cell, a
two-layer slab, a coarsened grid, a dst whose every image overflows its LDS
column, non-finite coordinates and a zero-volume cell; the large translation
needs the bin width per graph. Run with ``pytest -m gpu``."""
import pytest

from tests import test_radius_pbc_cells_cpu as cases
from tests.test_gpu_csr_padded import store  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(cases.brute.CASES))
def test_case(store, monkeypatch, case):  # noqa: F811
    cases.run_case(store, monkeypatch, case)


def test_capacity_cuts(store, monkeypatch):  # noqa: F811
    cases.run_capacity_cuts(store, monkeypatch)


@pytest.mark.parametrize("pbc", [(True, True, True), (True, True, False)])
def test_binning(store, pbc):  # noqa: F811
    cases.run_binning(store, pbc)


def test_large_translation(store):  # noqa: F811
    cases.run_binning(store, (True, True, True), scale=2.0 ** 14)


def test_refusals_and_dispatch(store):  # noqa: F811
    cases.run_refusals_and_dispatch(store)
