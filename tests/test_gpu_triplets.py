"""The triplet builder on the GPU: k_triplet_runs, k_triplet_count,
k_triplet_rebase and k_triplet_fill on the cases of tests/test_triplets_cpu.py,
against its brute-force reference. In ``test_cases`` every block of the fill
has one tile and finds its first edge by the search over the whole array:
``tiles`` has some 320 such tiles with 15 edges each, ``zero_span`` a tile whose
edges outnumber the LDS slice (the global-memory search). ``test_many_tiles``
gives the same two batches 3072 tiles, two per block on 256 CUs: the step from
a tile's first edge to the next one's, within one round (``tiles``) and past it
(``zero_span``), and the slice reused between tiles. ``test_capacity`` takes the
16-B stores with the cut inside a lane's four slots, and the element stores for
an odd ``Tcap`` and for a buffer 8 bytes off a 16-B boundary. Run with ``pytest
-m gpu``."""
import pytest

from tests import test_triplets_cpu as cases
from tests.test_gpu_csr_padded import store  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=["int32", "int64"])
@pytest.mark.parametrize("case", list(cases.CASES))
def test_cases(store, case, dtype, mode):  # noqa: F811
    cases.run_case(store, case, dtype, mode)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=["int32", "int64"])
@pytest.mark.parametrize("run", [cases.run_capacity, cases.run_cut_batches])
def test_capacity(store, run, dtype):  # noqa: F811
    run(store, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=["int32", "int64"])
@pytest.mark.parametrize("case", ["tiles", "zero_span"])
def test_many_tiles(store, case, dtype):  # noqa: F811
    cases.run_many_tiles(store, case, dtype)


def test_refusals(store):  # noqa: F811
    cases.run_refusals(store)
