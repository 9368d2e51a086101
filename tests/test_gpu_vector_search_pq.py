"""One parameter block per query in a pure vector search batch, on the MI355X (cases and what they compare: tests/vector_search_pq_common.py)."""
import pytest

from typesense_amd import _lib as B
from tests import helpers as H
from tests import vector_search_pq_common as V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dim,metric", [(24, B.METRIC_COSINE), (48, B.METRIC_IP), (70, B.METRIC_IP)])     # 16 lanes per row / the quad path / unaligned rows
def test_mixed_batch_equals_the_single_calls_and_the_oracle(dim, metric):
    V.case_mixed_batch(H.gpu_lib_path(), dim, metric)


def test_queries_sharing_one_list_upload_it_once_and_keep_their_own_query_document():
    V.case_shared_lists(H.gpu_lib_path())


def test_different_k_in_one_k_cut_group_are_prefixes_of_the_largest():
    V.case_different_k(H.gpu_lib_path())


def test_ten_flat_and_ten_k_cut_queries_cost_one_launch_and_one_filtered_batch():
    V.case_one_pass(H.gpu_lib_path())


def test_forced_split_of_the_ragged_launch_changes_nothing():
    V.case_forced_split(H.gpu_lib_path())


def test_refusals_are_per_query():
    V.case_refusals(H.gpu_lib_path())


def test_eight_threads_issue_the_mixed_batch_at_once():
    V.case_concurrency(H.gpu_lib_path())


def test_300_queries_over_20000_rows_each_with_its_own_list_half_on_each_branch():
    V.case_medium(H.gpu_lib_path())
