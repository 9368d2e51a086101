"""The list table of kw_find2_kernel and kw_score_kernel (tests/list_table_common.py): third-list probes through a table row, run loads through a table
row with two-load BlockMeta records and one-window offset_index pairs. Executed on the CPU under the SIMT emulator of tests/hipemu: same sources as
libtsgpu.so; the score world's companion list is shorter here and the mutated world is built once for the module. The `-m gpu` twin is
tests/test_gpu_list_table.py."""
import pytest

from tests import helpers as H
from tests import list_table_common as LT
from tests import mutated_index_common as M


@pytest.fixture(scope="module")
def probes():
    w = LT.ProbeWorld(H.emu_lib_path())
    yield w
    w.close()


@pytest.fixture(scope="module")
def scores():
    w = LT.ScoreWorld(H.emu_lib_path(), thin=True)
    yield w
    w.close()


def test_third_list_with_a_directory_is_probed_through_its_row(probes):
    LT.body_third_list_with_directory(probes)


def test_third_list_without_a_directory_takes_the_two_level_search(probes):
    LT.body_third_list_without_directory(probes)


def test_full_batches_and_a_tail_batch_of_one_work_item(probes):
    LT.body_batch_fill(probes)


def test_query_shapes_one_to_ten_tokens(probes):
    LT.body_query_shapes(probes)


def test_three_queries_over_disjoint_lists(probes):
    LT.body_three_queries_over_disjoint_lists(probes)


def test_pair_wider_than_the_tile_probes_the_second_list_through_its_row():
    LT.body_wide_run(H.emu_lib_path())


def test_ids_beyond_the_directories_range():
    LT.body_beyond_the_directories_range(H.emu_lib_path())


def test_marked_directory_entry_of_a_mutated_list():
    w = M.World(H.emu_lib_path())
    try:
        LT.body_split_entry(w)
    finally:
        w.close()


def test_score_layout_has_every_width_and_slot(scores):
    LT.body_score_layout(scores)


@pytest.mark.parametrize("n_tokens", [1, 2, 3])
def test_score_cases_one_hit_each(scores, n_tokens):
    LT.body_score_cases(scores, token_counts=(n_tokens,))
