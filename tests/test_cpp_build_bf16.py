"""Builds and runs the C++ checks of LeannIndex::build_bf16 (tests/cpp/test_build_bf16.cpp) against
libislands_amd.so: the host-only half here; under -m gpu one build on the device, whose bytes the program
compares with the bytes made here from the oracle's graph of the widened rows."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "islands_amd", "lib")
EXE = os.path.join(LIBDIR, "test_build_bf16")


def _run(*args):
    src = os.path.join(ROOT, "tests", "cpp", "test_build_bf16.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src,
                           "-L", LIBDIR, "-lislands_amd", f"-Wl,-rpath,{LIBDIR}", "-o", EXE])
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)


def test_cpp_build_bf16_cpu():
    r = _run("cpu")
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_build_bf16_gpu(orc, tmp_path):
    import islands_amd as ia
    from _data import clustered_vectors
    from test_build_bf16_cpu import to_bf16_bits, widen

    n, d = 300, 100
    bits = to_bf16_bits(clustered_vectors(n, d, 41))
    cfg = ia.LeannConfig.paper_default()
    cfg.m, cfg.m0, cfg.ef_construction = 8, 16, 40
    csr = orc.leann_build(widen(bits), m=cfg.m, m0=cfg.m0, ef_construction=cfg.ef_construction,
                          metric=int(cfg.metric), high_degree_pruning=cfg.high_degree_pruning,
                          hub_percentile=cfg.hub_percentile, levels=None)
    g = ia.CsrGraph(node_offsets=csr.node_offsets, neighbors=csr.neighbors, levels=csr.levels,
                    entry_point=csr.entry_point, max_level=csr.max_level, num_nodes=csr.num_nodes,
                    degree_counts=csr.degree_counts)
    rows_path, want_path = str(tmp_path / "rows.bin"), str(tmp_path / "want.bin")
    bits.tofile(rows_path)
    with open(want_path, "wb") as f:
        f.write(ia.LeannIndex.from_csr(g, cfg, dimension=d).to_bytes())
    r = _run("gpu", rows_path, str(n), str(d), want_path)
    assert r.returncode == 0, r.stdout + r.stderr
