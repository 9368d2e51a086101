"""Every search path over posting lists that incremental commits have mutated (tests/mutated_index_common.py), executed on the CPU under the SIMT
emulator of tests/hipemu: same sources as libtsgpu.so. The world is the GPU tier's; the option grid is thinner here (the full query sets run under the
default options, the other options get THIN_SETS). The tests share one world and run in file order: the last one compacts it. The `-m gpu` twin is
tests/test_gpu_mutated_index.py."""
import pytest

from tests import helpers as H
from tests import mutated_index_common as M


@pytest.fixture(scope="module")
def world():
    w = M.World(H.emu_lib_path())
    yield w
    w.close()


BODIES = [("default", lambda w: M.body_single_field(w, "default"))]
BODIES += [(name, lambda w, name=name: M.body_single_field(w, name, token_sets=M.THIN_SETS)) for name in ("chunk1", "chunk3", "fused", "one_block_find", "device_plan")]
BODIES += [("field 1", lambda w: M.body_single_field(w, "default", f=1, token_sets=M.THIN_SETS)),
           ("two fields, pipelined", lambda w: M.body_two_fields(w, 1, token_sets=M.THIN_SETS[1:8])),
           ("two fields, a block at a time", lambda w: M.body_two_fields(w, 0, chunk=3, token_sets=M.THIN_SETS[1:8])),
           ("grouped, first pass", lambda w: M.body_grouped(w, 1)),
           ("grouped, second pass", lambda w: M.body_grouped(w, 0)),
           ("candidates", M.body_candidates),
           ("aux scores", M.body_aux_scores)]


def test_commits_stayed_incremental_and_left_every_block_state(world):
    M.body_coverage(world)


@pytest.mark.parametrize("body", [b for _, b in BODIES], ids=[n for n, _ in BODIES])
def test_mutated_lists(world, body):
    body(world)


def test_directories_off_on_broken_lists(world):
    M.body_directories_off(world, token_sets=M.THIN_SETS)


def test_compaction_changes_no_result(world):
    """commit_full: no garbage, no list with breaks, and every body returns what it returned on the mutated snapshot (and what the oracle says)"""
    M.compact(world)
    for _, body in BODIES:
        body(world)
