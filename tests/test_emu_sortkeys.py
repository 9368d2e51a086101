"""sort_by on the device — `_eval`, missing_values: first and string-rank keys (TSGPU_SORT_EVAL .. TSGPU_SORT_STRING_RANK_FLIP) — executed on the CPU under
the SIMT emulator and checked bit-exactly against the oracle (bodies: tests/sortkeys_common.py). The `-m gpu` twin is tests/test_gpu_sortkeys.py."""
import json
import os

import pytest

from tests import helpers as H
from tests import sortkeys_common as S


@pytest.fixture(scope="module")
def world():
    w = S.World(3000, H.emu_lib_path())
    yield w
    w.close()


@pytest.mark.parametrize("dense_div", [0, 1])
def test_every_path_both_forms(world, dense_div):
    S.run_matrix(world, dense_div)


def test_default_threshold_picks_the_form_and_results_agree(world):
    """sortkey_dense_div = 64 (default): 3000 / 64 -> a key of 3 ids is sparse, a key of a third of the documents dense"""
    S.run_matrix(world, 64, topster_sizes=(250,))


def test_refusals_and_lifetime(world):
    S.run_refusals_and_lifetime(world)


def test_group_members_refuse_the_new_kinds(world):
    S.run_group_members_refuse(world, H.emu_lib_path())


def test_handle_exhaustion(world):
    S.run_exhaustion(world)


def test_key_churn_on_another_thread_while_searching(world):
    S.run_churn_while_searching(world, rounds=12)


def test_reference_expectations():
    with open(os.path.join(H.ROOT, "tests", "golden", "sort_eval_cases.json")) as f:
        S.run_golden(H.emu_lib_path(), json.load(f)["cases"])
