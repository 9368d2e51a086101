"""One parameter block per query in a pure vector search batch, on the CPU under the SIMT emulator (cases and what they compare:
tests/vector_search_pq_common.py)."""
import pytest

from typesense_amd import _lib as B
from tests import helpers as H
from tests import vector_search_pq_common as V


@pytest.mark.parametrize("dim,metric", [(24, B.METRIC_COSINE), (48, B.METRIC_IP), (70, B.METRIC_IP)])     # 16 lanes per row / the quad path / unaligned rows
def test_mixed_batch_equals_the_single_calls_and_the_oracle(dim, metric):
    V.case_mixed_batch(H.emu_lib_path(), dim, metric)


def test_queries_sharing_one_list_upload_it_once_and_keep_their_own_query_document():
    V.case_shared_lists(H.emu_lib_path())


def test_different_k_in_one_k_cut_group_are_prefixes_of_the_largest():
    V.case_different_k(H.emu_lib_path())


def test_ten_flat_and_ten_k_cut_queries_cost_one_launch_and_one_filtered_batch():
    V.case_one_pass(H.emu_lib_path())


def test_forced_split_of_the_ragged_launch_changes_nothing():
    V.case_forced_split(H.emu_lib_path())


def test_refusals_are_per_query():
    V.case_refusals(H.emu_lib_path())


def test_eight_threads_issue_the_mixed_batch_at_once():
    V.case_concurrency(H.emu_lib_path())
