"""Every delivery route of a keyword batch returns the same bits (tests/delivery_routes_common.py), executed on the CPU under the SIMT emulator of
tests/hipemu: same sources as libtsgpu.so. The `-m gpu` twin is tests/test_gpu_delivery_routes.py."""
import pytest

from tests import helpers as H
from tests import delivery_routes_common as D


@pytest.fixture(scope="module")
def world():
    w = D.World(H.emu_lib_path())
    yield w
    w.close()


def test_small_batch_device_zero_copy_staged_and_sliced_routes_return_the_same_bits(world):
    D.body_small_batch_every_route(world)


def test_image_over_8_mib_direct_copies_return_the_device_outputs_bits(world):
    D.body_large_image_direct_copies(world)
