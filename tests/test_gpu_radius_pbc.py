"""The periodic radius-graph fetch on the GPU: k_radius_pbc_count and
k_radius_pbc_fill (behind the unchanged CSR and fixed-stride gathers, with
k_radius_scan and k_graph_fill) on the cases of tests/test_radius_pbc_cpu.py,
against its float64 model. The request holds cells of 1, 2, 3, 17, 63, 65 and
T+1 nodes (T the LDS slice: streamed tiles) with 27 to 125 images, so item
blocks of one to four items per lane and several rounds per graph; "small_group"
runs it at 16 lanes per graph, everything else at 64. Run with
``pytest -m gpu``."""
import pytest

from tests import test_radius_pbc_cpu as cases
from tests.test_gpu_csr_padded import store  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(cases.CASES))
def test_case(store, case):  # noqa: F811
    cases.run_case(store, **cases.CASES[case])


def test_capacity_cuts(store):  # noqa: F811
    cases.run_capacity_cuts(store)


def test_sized_by_the_call(store):  # noqa: F811
    cases.run_sized_by_the_call(store)


def test_refusals(store):  # noqa: F811
    cases.run_refusals(store)
