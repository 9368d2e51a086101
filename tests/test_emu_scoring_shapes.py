"""The offsets -> text_match core of the keyword kernels on crafted document shapes (tests/scoring_shapes_common.py), executed on the CPU under the
SIMT emulator of tests/hipemu: same sources as libtsgpu.so. The `-m gpu` twin is tests/test_gpu_scoring_shapes.py."""
import pytest

from tests import helpers as H
from tests import scoring_shapes_common as S


@pytest.fixture(scope="module")
def world():
    w = S.World(H.emu_lib_path())
    yield w
    w.close()


def test_corpus_reaches_every_decoder_path(world):
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
