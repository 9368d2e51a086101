"""The HNSW traversal on distance ties, hand-made graphs, tier edges and re-used query slots (bodies and the list of cases:
tests/hnsw_traversal_common.py), executed on the CPU under the SIMT emulator and compared bit for bit with the oracle's traversal of the same graph.
The `-m gpu` twin is tests/test_gpu_hnsw_traversal.py.

Smaller here than there: (1024, 1024) and the walk of a 5 000-node ring run fewer queries (the emulator needs seconds per query for them); the
boosted visited sets (a 40 000-node ring) and a batch larger than the 4 096 natural query slots run on the GPU only."""
import pytest

from tests import helpers as H
from tests import hnsw_traversal_common as V


@pytest.mark.parametrize("k,ef", V.TIE_K_EF)
@pytest.mark.parametrize("family,M", [("tri", 8), ("tri", 4), ("dup", 8), ("dup", 4)])
def test_ties_in_both_heaps(family, M, k, ef):
    V.body_ties(H.emu_lib_path(), family, M, k, ef)


@pytest.mark.parametrize("k,ef", [(10, 64), (100, 128)])
def test_ties_cosine(k, ef):
    V.body_ties_cosine(H.emu_lib_path(), k, ef)


@pytest.mark.parametrize("k,ef", [(10, 64), (100, 128)])
def test_ties_non_strict_stop_rule(k, ef):
    V.body_ties_non_strict_stop(H.emu_lib_path(), k, ef)


@pytest.mark.parametrize("k,ef", [(10, 64), (100, 128)])
def test_ties_allow_list(k, ef):
    V.body_ties_allow_list(H.emu_lib_path(), k, ef)


@pytest.mark.parametrize("need", V.TIER_EDGES)
def test_every_tier_on_its_edges(need):
    V.body_tier_edge(H.emu_lib_path(), need, n_q=8 if need <= 513 else 3)


def test_the_largest_tier_with_k_and_ef_at_its_edge():
    V.body_tier_edge(H.emu_lib_path(), 1024, n_q=3, both_at_need=True)


def test_beyond_the_largest_tier_is_unsupported():
    V.body_beyond_the_largest_tier_is_unsupported(H.emu_lib_path())


def test_full_width_lists():
    V.body_full_width_lists(H.emu_lib_path())


def test_query_not_staged_in_lds():
    V.body_query_not_staged_in_lds(H.emu_lib_path())


def test_dead_ends_and_an_unreachable_component():
    V.body_dead_ends_and_an_unreachable_component(H.emu_lib_path())


def test_entry_point_rejected():
    V.body_entry_point_rejected(H.emu_lib_path())


def test_visited_set_past_half_full_runs_again_on_the_largest_tier():
    V.body_visited_set_past_half_full(H.emu_lib_path(), n_q=1)


def test_candidate_heap_beyond_the_largest_tier_is_reported():
    V.body_candidate_heap_beyond_the_largest_tier(H.emu_lib_path())


def test_more_queries_than_query_slots():
    V.body_more_queries_than_slots(H.emu_lib_path())


def test_tag_epoch_wrap_clears_the_tags():
    V.body_tag_epoch_wrap(H.emu_lib_path())
