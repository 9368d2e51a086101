"""`-m gpu`: every delivery route of a keyword batch returns the same bits (tests/delivery_routes_common.py) on a real MI355X through libtsgpu.so;
the device-output runs write torch device tensors. The CPU twin is tests/test_emu_delivery_routes.py."""
import pytest

from tests import helpers as H
from tests import delivery_routes_common as D

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _real_library(monkeypatch):
    """bodies shared with the emulator tier ask for the emulator build: give them the real library here"""
    monkeypatch.setattr(H, "emu_lib_path", lambda *a, **k: H.gpu_lib_path())


@pytest.fixture(scope="module")
def world():
    w = D.World(H.gpu_lib_path())            # (a module-scoped fixture is set up before the function-scoped monkeypatch: resolve the real library here)
    assert w.on_gpu, w.g.lib_path
    yield w
    w.close()


def test_small_batch_device_zero_copy_staged_and_sliced_routes_return_the_same_bits(world):
    D.body_small_batch_every_route(world)


def test_image_over_8_mib_direct_copies_return_the_device_outputs_bits(world):
    D.body_large_image_direct_copies(world)
