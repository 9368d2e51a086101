"""`-m gpu`: the id directory as the pair-find kernel reads it (tests/find_dir_tile_common.py) on a real MI355X through libtsgpu.so: entries without
the split mark behind full blocks, the directory tile of stage 1 against the window path, pairs wider than the tile. The CPU twin is
tests/test_emu_find_dir_tile.py."""
import pytest

from tests import helpers as H
from tests import find_dir_tile_common as F
from tests import mutated_index_common as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zipf():
    w = F.ZipfWorld(H.gpu_lib_path())
    yield w
    w.close()


@pytest.fixture(scope="module")
def mutated():
    w = M.World(H.gpu_lib_path())
    yield w
    w.close()


def test_directory_entries_behind_full_blocks_carry_no_split_mark():
    F.body_split_free_entries(H.gpu_lib_path())


def test_directory_tile_equals_the_window_path(zipf):
    F.body_dir_tile_equals_window_path(zipf)


def test_directory_tile_from_the_device_planner_equals_the_host_planner(zipf):
    F.body_device_planner_equals_host_planner(zipf)


def test_directory_tile_over_mutated_second_lists(mutated):
    F.body_mutated_lists(mutated)


def test_pair_wider_than_the_tile_inside_a_directory_mode_item():
    F.body_pair_wider_than_the_tile(H.gpu_lib_path())


def test_item_beyond_the_directories_range_keeps_the_window_path():
    F.body_item_beyond_the_directories_range(H.gpu_lib_path())
