"""Phrase search on the device (tsgpu_phrase_search_batch; kw_phrase.hip.h) through libtsgpu.so on a real MI355X, checked against a Python restatement of the
reference's do_phrase_search / handle_exclusion / get_phrase_matches (bodies: tests/phrase_common.py). 12 011 documents: the natural weight cut of 10 000 ids
per field is crossed. The emulator twin is tests/test_emu_phrase.py."""
import pytest

from tests import helpers as H
from tests import phrase_common as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    w = X.make_world(H.gpu_lib_path(), n_docs=12011, cut=10000)
    yield w
    w.close()


def test_adjacency_near_misses_repeats_wrap_and_list_lengths(world):
    X.run_adjacency(world)


def test_fold_of_a_fields_phrases(world):
    X.run_fold(world)


def test_fields_weights_and_the_weight_cut(world):
    X.run_fields_and_cut(world)


def test_exclusion_filter_ids_and_exclude_modes(world):
    X.run_exclusion_and_filter(world)


def test_batch_of_40_equals_40_calls_and_rounds(world):
    X.run_batching(world)


def test_argument_contract(world):
    X.run_statuses(world)


def test_mutated_index():
    X.run_mutated(H.gpu_lib_path())


def test_reference_phrase_cases_golden():
    X.run_golden(H.gpu_lib_path())
