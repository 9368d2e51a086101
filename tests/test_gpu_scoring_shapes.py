"""`-m gpu`: the offsets -> text_match core of the keyword kernels on crafted document shapes (tests/scoring_shapes_common.py) on a real MI355X
through libtsgpu.so, every hit bit-exact against the oracle. The CPU twin is tests/test_emu_scoring_shapes.py."""
import pytest

from tests import helpers as H
from tests import scoring_shapes_common as S

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _real_library(monkeypatch):
    """a guard: the shared bodies take their library from the `world` fixture below and never ask for the emulator build; should a helper
    they import ever do, it gets the real library here too"""
    monkeypatch.setattr(H, "emu_lib_path", lambda *a, **k: H.gpu_lib_path())


@pytest.fixture(scope="module")
def world():
    w = S.World(H.gpu_lib_path())            # (a module-scoped fixture is set up before the function-scoped monkeypatch: resolve the real library here)
    assert "emu" not in w.g.lib_path, w.g.lib_path
    yield w
    w.close()


def test_corpus_reaches_every_decoder_path(world):
    assert "emu" not in world.g.lib_path
    S.body_lists_reach_every_decoder_path(world)


def test_plain_field_two_kernels(world):
    S.body_plain_field(world, {}, "two kernels")


def test_plain_field_fused_kernel(world):
    S.body_plain_field(world, {"kw_two_kernels": (0, 1)}, "fused")


def test_plain_field_one_block_per_work_item(world):
    S.body_plain_field(world, {"kw_chunk_blocks": (1, 0)}, "chunk 1")


def test_two_plain_fields(world):
    S.body_two_plain_fields(world)


def test_array_field_alone_and_mixed(world):
    S.body_array_field(world)


def test_aux_scores_of_every_document(world):
    S.body_aux_scores(world)


def test_grouped_first_pass(world):
    S.body_grouped_first_pass(world)
