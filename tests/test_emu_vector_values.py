"""The bf16 bracket k-NN on hostile value distributions (bodies and the list of families: tests/vector_values_common.py), executed on the CPU under the
SIMT emulator and compared bit for bit with the oracle's exact flat scan. The `-m gpu` twin is tests/test_gpu_vector_values.py.

Families a and b (the ones the bracket got wrong before its radius was made underflow-proof and its survivor test moved to distance space) run both routes
at n_q = 4 at both dimensions; the wider query tiles (n_q = 70 -> vec_hscan_kernel<2>, 130 -> <4>) run on two cases of each family (one of them all-unbounded / all-tied at n_q = 70), one route each: where
a whole collection is unbounded every row of every query is re-scored, which the emulator does at ~100 s per case for the full cross product. The GPU
twin runs the full cross product of every family. The other families run one route at n_q = 4 here."""
import pytest

from typesense_amd import _lib as B
from tests import helpers as H
from tests import vector_values_common as V

FAILING = sorted(V.FAMILY_A) + sorted(V.FAMILY_B)


@pytest.mark.parametrize("name", FAILING)
def test_tiny_products_and_unseen_distance_ties_both_routes(name):
    V.body_case(H.emu_lib_path(), name, 64, n_qs=(4,))


@pytest.mark.parametrize("name,route,n_q", [("a-mixed", 2, 70), ("a-mixed", 512, 130), ("b-1e-4x1e-4", 512, 70), ("b-1e-4x1e-4", 2, 130),
                                            ("a-1e-25x1e18", 2, 70), ("b-1e-20x1", 512, 70)])      # (the last two: every row unbounded / every distance tied)
def test_tiny_products_and_unseen_distance_ties_wider_query_tiles(name, route, n_q):
    V.body_case(H.emu_lib_path(), name, 64, routes=(route,), n_qs=(n_q,))


@pytest.mark.parametrize("name", FAILING)
def test_tiny_products_and_unseen_distance_ties_residual_dimension(name):
    V.body_case(H.emu_lib_path(), name, 70, n_qs=(4,))


@pytest.mark.parametrize("name,dim,route", [("c-offset", 64, 2), ("c-offset", 70, 512), ("d-giant", 64, 512), ("d-giant", 70, 512), ("e-heavy", 64, 2), ("e-heavy", 70, 512),
                                            ("e-spike", 64, 512), ("e-spike", 70, 2), ("f-zeros", 64, 2), ("f-zeros", 70, 512)])
def test_other_value_families(name, dim, route):
    V.body_case(H.emu_lib_path(), name, dim, routes=(route,), n_qs=(4,))


@pytest.mark.parametrize("name,dim", [("b-1e-4x1e-4", 64), ("b-3e-4x3e-4", 70), ("d-giant", 64), ("e-heavy", 70)])
def test_finite_threshold_from_a_partial_sample(name, dim):
    V.body_partial_sample(H.emu_lib_path(), name, dim)


@pytest.mark.parametrize("dim", V.DIMS)
def test_bracket_that_cannot_prune_with_tiny_segments(dim):
    V.body_offset_with_tiny_segments(H.emu_lib_path(), dim)


@pytest.mark.parametrize("dim", V.DIMS)
def test_giant_rows_upserted_and_overwritten_move_the_tile_maxima_both_ways(dim):
    V.body_giant_rows_come_and_go(H.emu_lib_path(), dim)


@pytest.mark.parametrize("dim,route", [(64, 2), (70, 512)])
def test_non_finite_rows_leave_every_other_rank_alone(dim, route):
    V.body_nonfinite(H.emu_lib_path(), dim, routes=(route,), n_qs=(4,))


@pytest.mark.parametrize("name", FAILING)
def test_cosine(name):
    V.body_case(H.emu_lib_path(), name, 64, routes=(2,), n_qs=(4,), metric=B.METRIC_COSINE)


@pytest.mark.parametrize("name", FAILING + ["c-offset", "d-giant", "e-heavy", "e-spike"])
def test_fp32_scan(name):
    V.body_fp32_scan(H.emu_lib_path(), name, 64)


def test_vector_search_with_a_filter_at_1e_4():
    V.body_vector_search_with_filter(H.emu_lib_path())
