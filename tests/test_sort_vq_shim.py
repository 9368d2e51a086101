"""typesense_amd/csrc/host/tsgpu_sort_shim.h's `_vector_query(...)` slot class compiled with g++ against a mock of the reference's sort_by that has the
vector_query member (tests/host_shims/sort_vq_shim_driver.cpp), linked to the C-ABI library and run: the key lands on the mirrored vector field, a search
sorted by the mapped slot returns the reference's scores, errors create nothing, the RAII guard destroys the keys. Both tiers, like tests/test_sort_shim.py."""
import os
import subprocess

import pytest

from tests import helpers as H


def _run(lib, tmp_path):
    exe = str(tmp_path / "sort_vq_shim_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-o", exe, os.path.join(H.ROOT, "tests", "host_shims", "sort_vq_shim_driver.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-lpthread", "-ldl"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_sort_vq_shim_compiles_and_maps_emulator(tmp_path):
    _run(H.emu_lib_path(), tmp_path)


@pytest.mark.gpu
def test_sort_vq_shim_compiles_and_maps_gpu(tmp_path):
    _run(H.gpu_lib_path(), tmp_path)
