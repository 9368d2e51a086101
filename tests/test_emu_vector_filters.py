"""Per-query filters in one exact k-NN batch, on the CPU under the SIMT emulator (cases and what they compare: tests/vector_filters_common.py)."""
import pytest

from typesense_amd import _lib as B
from tests import helpers as H
from tests import vector_filters_common as V


@pytest.mark.parametrize("n,dim,metric,n_q,prefilter,sample_tiles,k,short", [
    (1000, 48, B.METRIC_IP, 3, 1, 2, 200, 150),          # vec_hscan_kernel<1>, sample of 2 of the 8 tiles -> L1 -> masked scan
    (1000, 70, B.METRIC_COSINE, 70, 1, 0, 200, 150),     # <2>, dense single pass, unaligned dim
    (1000, 48, B.METRIC_COSINE, 130, 1, 2, 200, 150),    # <4>
    (129, 70, B.METRIC_IP, 3, 1, 0, 50, 30),             # a tile with one row
    (1000, 70, B.METRIC_IP, 70, 0, 2, 200, 150),         # fp32 scan, 128-query tile, unaligned loads, sample -> tau -> filtered pass
    (1000, 48, B.METRIC_IP, 3, 0, 0, 200, 150),          # fp32 scan, 64-query tile, aligned loads, dense single pass
    (129, 48, B.METRIC_COSINE, 130, 0, 2, 50, 30),       # fp32 scan, two query tiles, a tile with one row
])
def test_mixed_filters_in_one_batch_match_the_oracle_and_the_single_filter_call(n, dim, metric, n_q, prefilter, sample_tiles, k, short):
    V.case_mixed_batch(H.emu_lib_path(), n, dim, metric, n_q, prefilter, sample_tiles, k, short, single_calls=16)


def test_non_identity_labels_are_translated_and_an_all_direct_group_launches_no_scan():
    V.case_non_identity_labels(H.emu_lib_path())


def test_hybrid_batch_with_40_different_filters_runs_one_vector_pass():
    V.case_hybrid_one_pass(H.emu_lib_path())


def test_filtered_one_query_calls_from_8_threads_coalesce():
    V.case_filtered_calls_coalesce(H.emu_lib_path())


def test_one_query_hybrid_calls_from_8_threads_share_their_vector_pass():
    V.case_hybrid_calls_coalesce(H.emu_lib_path())
