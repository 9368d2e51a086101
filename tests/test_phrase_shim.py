"""typesense_amd/csrc/host/tsgpu_phrase_shim.h compiled with g++ against mocks of the reference's KV, Topster and searched_queries (tests/host_shims/phrase_shim_driver.cpp), linked to the
C-ABI library and run: do_phrase_search's ranking and bookkeeping for a query of phrases only, the filter hand-over of a mixed query, handle_exclusion's merge, 400 / 408 / 501."""
import os
import subprocess

import pytest

from tests import helpers as H


def _run(lib, tmp_path):
    exe = str(tmp_path / "phrase_shim_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-o", exe, os.path.join(H.ROOT, "tests", "host_shims", "phrase_shim_driver.cpp"),
                           lib, "-Wl,-rpath," + os.path.dirname(lib), "-lpthread", "-ldl"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


def test_phrase_shim_emulator(tmp_path):
    _run(H.emu_lib_path(), tmp_path)


@pytest.mark.gpu
def test_phrase_shim_gpu(tmp_path):
    _run(H.gpu_lib_path(), tmp_path)
