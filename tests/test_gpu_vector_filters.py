"""Per-query filters in one exact k-NN batch, on the MI355X (cases and what they compare: tests/vector_filters_common.py)."""
import numpy as np
import pytest

from typesense_amd import _lib as B
from tests import helpers as H
from tests import vector_filters_common as V

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,dim,metric,n_q,prefilter,sample_tiles,k,short", [
    (1000, 48, B.METRIC_IP, 3, 1, 2, 200, 150),
    (1000, 70, B.METRIC_COSINE, 70, 1, 0, 200, 150),
    (1000, 48, B.METRIC_COSINE, 130, 1, 2, 200, 150),
    (129, 70, B.METRIC_IP, 3, 1, 0, 50, 30),
    (1000, 70, B.METRIC_IP, 70, 0, 2, 200, 150),
    (1000, 48, B.METRIC_IP, 3, 0, 0, 200, 150),
    (129, 48, B.METRIC_COSINE, 130, 0, 2, 50, 30),
])
def test_mixed_filters_in_one_batch_match_the_oracle_and_the_single_filter_call(n, dim, metric, n_q, prefilter, sample_tiles, k, short):
    V.case_mixed_batch(H.gpu_lib_path(), n, dim, metric, n_q, prefilter, sample_tiles, k, short)


def test_non_identity_labels_are_translated_and_an_all_direct_group_launches_no_scan():
    V.case_non_identity_labels(H.gpu_lib_path())


def test_hybrid_batch_with_40_different_filters_runs_one_vector_pass():
    V.case_hybrid_one_pass(H.gpu_lib_path())


def test_filtered_one_query_calls_from_8_threads_coalesce():
    V.case_filtered_calls_coalesce(H.gpu_lib_path())


def test_one_query_hybrid_calls_from_8_threads_share_their_vector_pass():
    V.case_hybrid_calls_coalesce(H.gpu_lib_path())


@pytest.mark.parametrize("direct_max", [65536, 0])
def test_300_queries_over_20000_rows_with_filters_from_50_ids_to_60_percent(direct_max):
    """20 000 x 96, 300 queries, k = 100, allow lists from 50 ids to 60 % of the rows (every fourth query also excludes ids), once per route setting:
    the oracle's neighbours bit for bit. 157 tiles: the default sample covers them all (dense single pass of the bracket path)"""
    n, dim, n_q, k = 20000, 96, 300, 100
    g, orc, rng, labels, live = V.build(H.gpu_lib_path(), n, dim, B.METRIC_IP, 41, deleted=(7, 12345))
    g.set_option("vec_filter_direct_max", direct_max)
    Q = rng.standard_normal((n_q, dim)).astype(np.float32)
    sizes = np.linspace(50, 0.6 * n, n_q).astype(np.int64)
    filters = []
    for i in range(n_q):
        a = np.sort(rng.choice(n, size=int(sizes[i]), replace=False)).astype(np.uint32)
        filters.append((a, a[::5].copy() if i % 4 == 0 else None))
    res = g.vec_knn_batch_filtered(1, Q, k, filters)
    V.check_against_oracle(orc, Q, k, filters, live, True, res, bits=True, what=("20000x96", direct_max))
    assert g.counter("vec_prefilter_fallbacks") == 0
    if direct_max:
        assert g.counter("vec_filter_direct_queries") == n_q and g.counter("vec_filter_scan_queries") == 0
    else:
        assert g.counter("vec_filter_direct_queries") == 0 and g.counter("vec_filter_scan_queries") == n_q
    orc.close()
    g.close()
