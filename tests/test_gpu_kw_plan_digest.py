"""`-m gpu`: the keyword planner's plan, pinned by digests (tests/kw_plan_digest_common.py), on a real MI355X through libtsgpu.so. The device planner's
LAYOUT digest is left to the emulator tier: its heaviest-first order follows a float cost that the GPU compiler may contract into FMAs (its hits are
compared with the host plan's and the oracle's here). The CPU twin is tests/test_emu_kw_plan_digest.py."""
import pytest

from tests import helpers as H
from tests import kw_plan_digest_common as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    w = C.World(H.gpu_lib_path())
    yield w
    w.close()


def test_mixed_batch_planned_in_slices_has_the_serial_plan_and_the_pinned_one(world):
    C.body_mixed_batch(world)


@pytest.mark.parametrize("n", C.BATCH_SIZES)
def test_chunk_merge_and_order_options_give_the_pinned_plans(world, n):
    C.body_option_grid(world, n)


def test_work_items_are_capped_at_256_blocks():
    C.body_block_cap(H.gpu_lib_path())


def test_wildcard_plans_on_the_collection_and_on_a_doc_range(world):
    C.body_wildcard(world)


def test_host_and_device_planner_give_the_pinned_plans(world):
    C.body_both_planners(world, False)
