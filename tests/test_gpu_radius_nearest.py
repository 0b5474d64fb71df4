"""The nearest-K cap on the GPU: k_radius_nearest_select and the nearest
variants of k_radius_fill / k_radius_pbc_fill on the cases of
tests/test_radius_nearest_cpu.py, against its thinned float64 model. The dense
graph of T+1 nodes has degrees near T (several queue flushes per dst, sources
read past the LDS slice) at the K the best list splits on; the periodic request
has cells of 1 to T+1 atoms with 27 to 125 images. Run with ``pytest -m gpu``."""
import pytest

from tests import test_radius_nearest_cpu as cases
from tests.test_gpu_csr_padded import store  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(cases.OPEN))
def test_open(store, case):  # noqa: F811
    cases.run_open(store, **cases.OPEN[case])


@pytest.mark.parametrize("K", [1, 6])
@pytest.mark.parametrize("rule", list(cases.PBC_RULES))
def test_pbc(store, rule, K):  # noqa: F811
    cases.run_pbc(store, rule, K)


@pytest.mark.parametrize("run", [cases.run_noop, cases.run_capacity_cuts,
                                 cases.run_refusals])
def test_properties(store, run):  # noqa: F811
    run(store)
