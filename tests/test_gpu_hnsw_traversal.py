"""`-m gpu` twin of tests/test_emu_hnsw_traversal.py: the HNSW traversal on distance ties, hand-made graphs, tier edges and re-used query slots
(bodies and the list of cases: tests/hnsw_traversal_common.py) through libtsgpu.so on a real MI355X, bit for bit against the oracle's traversal of the
same graph. The hash-mode visited set (concurrent atomicCAS from 64 lanes behind a workgroup release fence) is where the hardware and the emulator
can differ. Only here: the boosted visited sets (a 40 000-node ring) and a batch of 2 x 4 096 + 37 queries on the natural 4 096 query slots."""
import pytest

from tests import helpers as H
from tests import hnsw_traversal_common as V

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _real_library(monkeypatch):
    """a guard: the bodies take the library path as an argument; should a helper they import ever ask for the emulator build, it gets the real library"""
    monkeypatch.setattr(H, "emu_lib_path", lambda *a, **k: H.gpu_lib_path())


@pytest.mark.parametrize("k,ef", V.TIE_K_EF)
@pytest.mark.parametrize("family,M", [("tri", 8), ("tri", 4), ("dup", 8), ("dup", 4)])
def test_ties_in_both_heaps(family, M, k, ef):
    V.body_ties(H.gpu_lib_path(), family, M, k, ef)


@pytest.mark.parametrize("k,ef", [(10, 64), (100, 128)])
def test_ties_cosine(k, ef):
    V.body_ties_cosine(H.gpu_lib_path(), k, ef)


@pytest.mark.parametrize("k,ef", [(10, 64), (100, 128)])
def test_ties_non_strict_stop_rule(k, ef):
    V.body_ties_non_strict_stop(H.gpu_lib_path(), k, ef)


@pytest.mark.parametrize("k,ef", [(10, 64), (100, 128)])
def test_ties_allow_list(k, ef):
    V.body_ties_allow_list(H.gpu_lib_path(), k, ef)


@pytest.mark.parametrize("need", V.TIER_EDGES)
def test_every_tier_on_its_edges(need):
    V.body_tier_edge(H.gpu_lib_path(), need)


def test_the_largest_tier_with_k_and_ef_at_its_edge():
    V.body_tier_edge(H.gpu_lib_path(), 1024, both_at_need=True)


def test_beyond_the_largest_tier_is_unsupported():
    V.body_beyond_the_largest_tier_is_unsupported(H.gpu_lib_path())


def test_full_width_lists():
    V.body_full_width_lists(H.gpu_lib_path())


def test_query_not_staged_in_lds():
    V.body_query_not_staged_in_lds(H.gpu_lib_path())


def test_dead_ends_and_an_unreachable_component():
    V.body_dead_ends_and_an_unreachable_component(H.gpu_lib_path())


def test_entry_point_rejected():
    V.body_entry_point_rejected(H.gpu_lib_path())


def test_visited_set_past_half_full_runs_again_on_the_largest_tier():
    V.body_visited_set_past_half_full(H.gpu_lib_path())


def test_visited_set_past_half_of_the_largest_tiers_runs_again_with_boosted_sets():
    V.body_visited_set_past_half_full(H.gpu_lib_path(), n=40000, reruns_per_query=2)


def test_candidate_heap_beyond_the_largest_tier_is_reported():
    V.body_candidate_heap_beyond_the_largest_tier(H.gpu_lib_path())


def test_more_queries_than_query_slots():
    V.body_more_queries_than_slots(H.gpu_lib_path())


def test_tag_epoch_wrap_clears_the_tags():
    V.body_tag_epoch_wrap(H.gpu_lib_path())


def test_more_queries_than_the_natural_query_slots():
    V.body_more_queries_than_the_natural_slots(H.gpu_lib_path())
