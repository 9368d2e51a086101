"""`-m gpu`: every search path over posting lists that incremental commits have mutated (tests/mutated_index_common.py) on a real MI355X through
libtsgpu.so, the full option grid, every hit bit-exact against an oracle loaded from the Python model. The tests share one world and run in file order:
the last one compacts it. The CPU twin is tests/test_emu_mutated_index.py."""
import pytest

from tests import helpers as H
from tests import mutated_index_common as M

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _real_library(monkeypatch):
    """a guard: the shared bodies take their library from the `world` fixture below and never ask for the emulator build; should a helper they import
    ever do, it gets the real library here too"""
    monkeypatch.setattr(H, "emu_lib_path", lambda *a, **k: H.gpu_lib_path())


@pytest.fixture(scope="module")
def world():
    w = M.World(H.gpu_lib_path())            # (a module-scoped fixture is set up before the function-scoped monkeypatch: resolve the real library here)
    assert "emu" not in w.g.lib_path, w.g.lib_path
    yield w
    w.close()


BODIES = [(name, lambda w, name=name: M.body_single_field(w, name)) for name in M.OPTION_SETS]
BODIES += [("field 1", lambda w: M.body_single_field(w, "default", f=1)), ("field 1, chunk1", lambda w: M.body_single_field(w, "chunk1", f=1))]
BODIES += [("two fields, pipelined=%d chunk=%d" % (p, c), lambda w, p=p, c=c: M.body_two_fields(w, p, chunk=c)) for p in (1, 0) for c in (0, 1, 3)]
BODIES += [("grouped, first pass", lambda w: M.body_grouped(w, 1)),
           ("grouped, second pass", lambda w: M.body_grouped(w, 0)),
           ("candidates", M.body_candidates),
           ("aux scores", M.body_aux_scores)]


def test_commits_stayed_incremental_and_left_every_block_state(world):
    assert "emu" not in world.g.lib_path
    M.body_coverage(world)


@pytest.mark.parametrize("body", [b for _, b in BODIES], ids=[n for n, _ in BODIES])
def test_mutated_lists(world, body):
    body(world)


def test_directories_off_on_broken_lists(world):
    M.body_directories_off(world)


def test_compaction_changes_no_result(world):
    """commit_full: no garbage, no list with breaks, and every body returns what it returned on the mutated snapshot (and what the oracle says)"""
    M.compact(world)
    for _, body in BODIES:
        body(world)
