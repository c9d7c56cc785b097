"""Builds and runs the C++ checks of LeannIndex::convert_rows / read_rows (tests/cpp/test_convert_rows.cpp)
against libislands_amd.so: the host-only half here, the conversions of a built index on the device under -m gpu."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "islands_amd", "lib")
EXE = os.path.join(LIBDIR, "test_convert_rows")


def _run(mode):
    src = os.path.join(ROOT, "tests", "cpp", "test_convert_rows.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src,
                           "-L", LIBDIR, "-lislands_amd", f"-Wl,-rpath,{LIBDIR}", "-o", EXE])
    return subprocess.run([EXE, mode], capture_output=True, text=True, timeout=300)


def test_cpp_convert_rows_cpu():
    r = _run("cpu")
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_convert_rows_gpu():
    r = _run("gpu")
    assert r.returncode == 0, r.stdout + r.stderr
