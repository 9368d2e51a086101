"""Infix search on the device (tsgpu_infix_search_batch; kw_infix.hip.h) through libtsgpu.so on a real MI355X, checked against a Python restatement
of the reference's front plus the oracle's wildcard ranking (bodies: tests/infix_common.py). The emulator twin is tests/test_emu_infix.py."""
import pytest

from tests import helpers as H
from tests import infix_common as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    w = X.make_world(H.gpu_lib_path())
    yield w
    w.close()


def test_prefix_and_suffix_limits_golden():
    X.run_golden(H.gpu_lib_path())


def test_scan_semantics(world):
    X.run_scan_semantics(world)


def test_no_match_across_neighbouring_tokens():
    X.run_across_tokens(H.gpu_lib_path())


def test_search_on_a_held_snapshot_keeps_its_vocabulary():
    X.run_held_snapshot(H.gpu_lib_path())


def test_scan_shapes():
    X.run_scan_shapes(H.gpu_lib_path())


def test_one_scan_per_field_for_68_queries(world):
    X.run_batch_of_68(world)


def test_union_edges_and_incremental_postings():
    X.run_union_edges(H.gpu_lib_path())


def test_exclusion_filter_and_rounds(world):
    X.run_exclusion_and_filter(world)


def test_sort_keys_and_statuses(world):
    X.run_sorts_and_statuses(world)


def test_incremental_vocabulary_and_compaction():
    X.run_incremental_vocabulary(H.gpu_lib_path())


def test_threads_get_their_own_results(world):
    X.run_threads(world, n_threads=8, per=5)
