"""`-m gpu` twin of tests/test_emu_vector_values.py: the bf16 bracket k-NN on hostile value distributions (bodies and the list of families:
tests/vector_values_common.py) through libtsgpu.so on a real MI355X, bit for bit against the oracle's exact flat scan. Every family runs both routes
and n_q = 4 / 70 / 130 (vec_hscan_kernel<1>, <2>, <4>) at both dimensions."""
import pytest

from typesense_amd import _lib as B
from tests import helpers as H
from tests import vector_values_common as V

pytestmark = pytest.mark.gpu

FAILING = sorted(V.FAMILY_A) + sorted(V.FAMILY_B)


@pytest.fixture(autouse=True)
def _real_library(monkeypatch):
    """a guard: the bodies take the library path as an argument; should a helper they import ever ask for the emulator build, it gets the real library"""
    monkeypatch.setattr(H, "emu_lib_path", lambda *a, **k: H.gpu_lib_path())


@pytest.mark.parametrize("dim", V.DIMS)
@pytest.mark.parametrize("name", sorted(V.CASES))
def test_every_family_both_routes_every_query_tile(name, dim):
    V.body_case(H.gpu_lib_path(), name, dim)


@pytest.mark.parametrize("dim", V.DIMS)
@pytest.mark.parametrize("name", ["b-1e-4x1e-4", "b-3e-4x3e-4", "d-giant", "e-heavy", "e-spike"])
def test_finite_threshold_from_a_partial_sample(name, dim):
    for n_q in V.N_QS:
        V.body_partial_sample(H.gpu_lib_path(), name, dim, n_q=n_q)


@pytest.mark.parametrize("dim", V.DIMS)
def test_bracket_that_cannot_prune_with_tiny_segments(dim):
    V.body_offset_with_tiny_segments(H.gpu_lib_path(), dim)


@pytest.mark.parametrize("dim", V.DIMS)
def test_giant_rows_upserted_and_overwritten_move_the_tile_maxima_both_ways(dim):
    for n_q in V.N_QS:
        V.body_giant_rows_come_and_go(H.gpu_lib_path(), dim, n_q=n_q)


@pytest.mark.parametrize("dim", V.DIMS)
def test_non_finite_rows_leave_every_other_rank_alone(dim):
    V.body_nonfinite(H.gpu_lib_path(), dim)


@pytest.mark.parametrize("name", FAILING)
def test_cosine(name):
    V.body_case(H.gpu_lib_path(), name, 64, metric=B.METRIC_COSINE)


@pytest.mark.parametrize("name", FAILING + ["c-offset", "d-giant", "e-heavy", "e-spike"])
def test_fp32_scan(name):
    V.body_fp32_scan(H.gpu_lib_path(), name, 64)


def test_vector_search_with_a_filter_at_1e_4():
    V.body_vector_search_with_filter(H.gpu_lib_path())
