"""The cell-list path of the radius-graph fetch on the GPU: k_cells_* between
the unchanged CSR gather and k_radius_scan / k_graph_fill, on the cases of
tests/test_radius_cells_cpu.py, against the model of tests/radius_ref.py. The
shape request's 2T+3 graph spans three blocks of the count and fill kernels;
the boundary request holds a coarsened box, nodes without a bin and a dst with
more edges than it orders in LDS. Run with ``pytest -m gpu``."""
import pytest

from tests import test_radius_cells_cpu as cases
from tests.test_gpu_csr_padded import store  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", cases.GRID_CASES)
def test_grid(store, monkeypatch, case):  # noqa: F811
    cases.run_grid_case(store, monkeypatch, case)


def test_capacity_cuts(store, monkeypatch):  # noqa: F811
    cases.run_capacity_cuts(store, monkeypatch)


@pytest.mark.parametrize("K", [None, 3])
def test_boundary(store, monkeypatch, K):  # noqa: F811
    cases.run_boundary(store, monkeypatch, K)


def test_random_f32(store, monkeypatch):  # noqa: F811
    cases.run_random_f32(store, monkeypatch)


def test_refusals_and_dispatch(store):  # noqa: F811
    cases.run_refusals_and_dispatch(store)
