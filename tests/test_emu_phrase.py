"""Phrase search on the device (tsgpu_phrase_search_batch; kw_phrase.hip.h) executed on the CPU under the SIMT emulator and checked against a Python restatement
of the reference's do_phrase_search / handle_exclusion / get_phrase_matches (bodies: tests/phrase_common.py). The weight cut is 50 here (option
phrase_weight_cut), so that a few hundred documents cross it. The `-m gpu` twin is tests/test_gpu_phrase.py."""
import pytest

from tests import helpers as H
from tests import phrase_common as X


@pytest.fixture(scope="module")
def world():
    w = X.make_world(H.emu_lib_path(), n_docs=331, cut=50)
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
    X.run_mutated(H.emu_lib_path())


def test_reference_phrase_cases_golden():
    X.run_golden(H.emu_lib_path())
