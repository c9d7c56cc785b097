"""Builds and runs the C++ checks of LeannIndex::set_refine_rows / refine_storage / search_refined_batch / rescore
(tests/cpp/test_refine.cpp) against libislands_amd.so: what is answered without a device here, a 300-row index on
the device under -m gpu."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "islands_amd", "lib")
EXE = os.path.join(LIBDIR, "test_refine")


def _run(mode):
    src = os.path.join(ROOT, "tests", "cpp", "test_refine.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src,
                           "-L", LIBDIR, "-lislands_amd", f"-Wl,-rpath,{LIBDIR}", "-o", EXE])
    return subprocess.run([EXE, mode], capture_output=True, text=True, timeout=300)


def test_cpp_refine_cpu():
    r = _run("cpu")
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_refine_gpu():
    r = _run("gpu")
    assert r.returncode == 0, r.stdout + r.stderr
