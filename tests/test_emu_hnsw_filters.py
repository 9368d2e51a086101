"""Per-query filters in one HNSW search batch and the coalescer of small HNSW calls (bodies and what they compare: tests/hnsw_filters_common.py),
executed on the CPU under the SIMT emulator. The `-m gpu` twin is tests/test_gpu_hnsw_filters.py.

Smaller here than there: the mixed batch runs 16 queries (two rounds of the eight filter kinds) instead of 24 — the emulator needs about a second
for a query that walks the whole graph, and every query also runs alone. Everything else is the GPU tier's shape."""
import pytest

from typesense_amd import _lib as B
from tests import helpers as H
from tests import hnsw_filters_common as V

N_Q = 16


@pytest.mark.parametrize("k,ef", V.MIXED_K_EF)
@pytest.mark.parametrize("metric", [B.METRIC_IP, B.METRIC_COSINE])
def test_mixed_filters_in_one_batch_match_the_oracle_and_the_single_filter_call(metric, k, ef):
    V.body_mixed_batch(H.emu_lib_path(), metric, k, ef, n_q=N_Q)


@pytest.mark.parametrize("k,ef", V.MIXED_K_EF)
def test_the_batch_is_one_launch_and_the_same_traversal(k, ef):
    V.body_one_launch_same_traversal(H.emu_lib_path(), B.METRIC_IP, k, ef, n_q=N_Q)


def test_a_batch_whose_maps_do_not_fit_is_split_into_groups():
    V.body_group_split(H.emu_lib_path(), B.METRIC_IP, 10, 64, n_q=N_Q)


@pytest.mark.parametrize("n,label_base", [(129, 0), (33, 0), (200, 1000)])
def test_small_and_ragged_shapes(n, label_base):
    V.body_small_shape(H.emu_lib_path(), n, label_base)


def test_masks_follow_a_query_through_the_rerun_ladder():
    V.body_masks_through_the_rerun_ladder(H.emu_lib_path())


def test_a_block_serves_queries_with_different_maps_in_turn():
    V.body_several_queries_per_block(H.emu_lib_path())


def test_one_query_calls_from_8_threads_coalesce_across_both_entry_points():
    V.body_calls_coalesce(H.emu_lib_path())


def test_arguments():
    V.body_arguments(H.emu_lib_path())
