"""Builds and runs the C++ checks of LeannIndex::reachability / cover_entry_seeds and HnswGraph::reachability
(tests/cpp/test_graph_reach.cpp) against libislands_amd.so: what is answered without a device here, hand graphs on
the device under -m gpu."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "islands_amd", "lib")
EXE = os.path.join(LIBDIR, "test_graph_reach")


def _run(mode):
    src = os.path.join(ROOT, "tests", "cpp", "test_graph_reach.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src,
                           "-L", LIBDIR, "-lislands_amd", f"-Wl,-rpath,{LIBDIR}", "-o", EXE])
    return subprocess.run([EXE, mode], capture_output=True, text=True, timeout=300)


def test_cpp_graph_reach_cpu():
    r = _run("cpu")
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_graph_reach_gpu():
    r = _run("gpu")
    assert r.returncode == 0, r.stdout + r.stderr
