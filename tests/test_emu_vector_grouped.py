"""group_by for the pure vector search, on the CPU under the SIMT emulator (cases and what they compare: tests/vector_grouped_common.py)."""
import pytest

from typesense_amd import _lib as B
from tests import helpers as H
from tests import vector_grouped_common as VG


@pytest.mark.parametrize("dim,metric", [(24, B.METRIC_COSINE), (48, B.METRIC_IP)])
def test_mixed_batch_equals_the_oracle_and_the_calls_issued_alone(dim, metric):
    VG.case_mixed_batch(H.emu_lib_path(), dim, metric)


def test_flat_compaction_at_the_tile_edges_by_every_cause_of_dropping():
    VG.case_compaction_edges(H.emu_lib_path())


def test_group_edges_on_both_branches():
    VG.case_group_edges(H.emu_lib_path())


def test_k_cut_prefixes_filters_query_documents_and_thresholds():
    VG.case_kcut(H.emu_lib_path())


def test_vector_distance_is_delivered_by_both_passes_and_both_delivery_routes():
    VG.case_delivery(H.emu_lib_path())


def test_refusals_are_per_query_and_the_neighbours_are_answered():
    VG.case_refusals(H.emu_lib_path())


def test_ten_flat_and_ten_k_cut_queries_cost_one_launch_one_batch_and_one_sync():
    VG.case_cost(H.emu_lib_path())


def test_eight_threads_issue_the_mixed_batch_at_once():
    VG.case_concurrency(H.emu_lib_path())


def test_ungrouped_per_query_results_are_unchanged_around_grouped_calls():
    VG.case_ungrouped_unchanged(H.emu_lib_path())
