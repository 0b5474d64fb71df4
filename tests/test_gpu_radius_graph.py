"""The radius-graph fetch on the GPU: k_radius_count, k_radius_scan and
k_radius_fill (behind the unchanged CSR gather and k_graph_fill) on the cases
of tests/test_radius_graph_cpu.py, against the model of tests/radius_ref.py.
The shape request holds graphs of 0, 1, 2, 63..65 nodes and of T-1, T, T+1 and
2T+3, T the LDS slice of the kernels (one slice, streamed tiles, several centre
passes); "small_mean" runs it at 16 lanes per graph, everything else at 64,
and the random case at 16. Run with ``pytest -m gpu``."""
import pytest

from tests import test_radius_graph_cpu as cases
from tests.test_gpu_csr_padded import store  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(cases.CASES))
def test_grid(store, case):  # noqa: F811
    cases.run_grid_case(store, **cases.CASES[case])


def test_capacity_cuts(store):  # noqa: F811
    cases.run_capacity_cuts(store)


def test_random_f32(store):  # noqa: F811
    cases.run_random_f32(store)


def test_sized_by_the_call(store):  # noqa: F811
    cases.run_sized_by_the_call(store)
