"""sort_by=_vector_query(field:([...])) on the device (TSGPU_SORT_VECTOR_QUERY; kw_vq_sort.hip.h) executed on the CPU under the SIMT emulator and checked
bit-exactly against the oracle (bodies: tests/vq_sort_common.py). The `-m gpu` twin is tests/test_gpu_vq_sort.py.
Dimensions: 5 (> 4 with residual), 16 (the quad form), 20 (% 4 == 0), 48 (the quad form, three blocks); 3 (<= 4) and 19 (> 16 with residual) in the
semantics fields."""
import pytest

from typesense_amd import _lib as B
from tests import helpers as H
from tests import vq_sort_common as V


@pytest.fixture(scope="module")
def world():
    w = V.VqWorld(3000, H.emu_lib_path())
    yield w
    w.close()


@pytest.fixture(scope="module")
def semantics_world():
    w = V.VqWorld(3000, H.emu_lib_path())
    V.add_semantics_fields(w, 16, 19, 3)
    yield w
    w.close()


def test_reference_pin():
    V.run_reference_pin(H.emu_lib_path())


@pytest.mark.parametrize("metric", [B.METRIC_IP, B.METRIC_COSINE])
@pytest.mark.parametrize("dim", [5, 16, 20, 48])
def test_distance_bits(world, dim, metric):
    V.run_distance_bits(world, 100 + 2 * dim + metric, dim, metric)


def test_semantics_and_every_entry_point(semantics_world):
    V.run_semantics_and_entry_points(semantics_world)


def test_refusals_and_key_lifetime(semantics_world):
    V.run_refusals(semantics_world)


def test_field_mutations_under_a_live_key(semantics_world):
    V.run_field_mutations_under_a_live_key(semantics_world, dim=20)


def test_threads_with_keys_of_their_own_coalesce(semantics_world):
    V.run_threads_with_keys_of_their_own(semantics_world, per=3)
