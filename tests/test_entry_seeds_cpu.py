"""Entry seeds without a GPU: the four ABI symbols and their device-free argument errors, the host-only
arithmetic of entry_seeds_plan.hpp under AddressSanitizer (a stand-alone program), and -- with the oracle
alone -- the property of the shared fixture that tests/test_gpu_entry_seeds.py relies on: an exact 8-NN
graph of 40 tight clusters entered at node 0 finds almost nothing, the same graph entered at the
reference pick among 64 reference seeds finds almost everything."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import islands_amd as ia
from islands_amd import _ffi

import _entry_seeds_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = {
    "isl_index_select_entry_seeds": "isl_index* idx, uint64_t count, uint64_t* out_ids, uint64_t* out_count",
    "isl_index_set_entry_seeds": "isl_index* idx, const uint64_t* ids, uint64_t count",
    "isl_index_entry_seeds": "const isl_index* idx, uint64_t* out, uint64_t cap, uint64_t* count",
    "isl_index_pick_entries": "const isl_index* idx, const float* queries, uint64_t nq, uint64_t d, "
                              "uint64_t* out_ids, int32_t mem, void* stream",
}
CAP = 65536


def test_symbols_and_signatures():
    lib = _ffi.lib()
    hdr = open(os.path.join(ROOT, "include", "islands_amd.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for name, args in DECLARED.items():
        assert hasattr(lib, name), name
        assert f"isl_status {name}({args});" in flat, name
        res, argtypes = _ffi.SIGNATURES[name]
        assert res is _ffi.i32 and len(argtypes) == args.count(",") + 1, name
    assert re.search(r"#define ISL_MAX_ENTRY_SEEDS 65536ull\b", hdr)
    assert lib.isl_abi_version() == 3
    for m in ("select_entry_seeds", "set_entry_seeds", "entry_seeds", "pick_entries"):
        assert callable(getattr(ia.LeannIndex, m))
    for text in (open(os.path.join(ROOT, "include", "islands_amd.hpp")).read(),
                 open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        for name in DECLARED:
            assert name in text, name


def test_argument_errors_without_a_device():
    lib = _ffi.lib()
    n = C.c_uint64(7)
    ids = np.zeros(4, np.uint64)
    q = np.zeros((1, 4), np.float32)
    INVALID, UNSUPPORTED = 101, 102
    assert lib.isl_index_select_entry_seeds(None, 4, None, C.byref(n)) == INVALID and n.value == 0
    assert lib.isl_index_set_entry_seeds(None, ids.ctypes.data, 4) == INVALID
    assert lib.isl_index_entry_seeds(None, None, 0, C.byref(n)) == INVALID
    assert lib.isl_index_pick_entries(None, q.ctypes.data, 1, 4, ids.ctypes.data, 0, None) == INVALID
    idx = ia.LeannIndex.with_defaults()
    with pytest.raises(ia.CoreError) as e:
        idx.select_entry_seeds(CAP + 1)
    assert e.value.kind == "Unsupported"
    big = np.zeros(CAP + 1, np.uint64)
    assert lib.isl_index_set_entry_seeds(idx._h, big.ctypes.data, CAP + 1) == UNSUPPORTED
    # no table is the default, clearing an empty index is fine, and an empty index takes no seeds
    assert idx.entry_seeds().size == 0
    idx.set_entry_seeds([])
    for call in (lambda: idx.select_entry_seeds(4), lambda: idx.set_entry_seeds([0])):
        with pytest.raises(ia.CoreError) as e:
            call()
        assert e.value.kind == "EmptyCollection"
    # a graph without rows on a device: what isl_select_neighbors answers there
    g = ia.CsrGraph()
    g.add_node([], 0)
    g.add_node([0], 0)
    host = ia.LeannIndex.from_csr(g, dimension=4)
    for call in (lambda: host.select_entry_seeds(2), lambda: host.set_entry_seeds([1]),
                 lambda: host.pick_entries(q)):
        with pytest.raises(ia.CoreError) as e:
            call()
        assert e.value.kind == "Unsupported"


@pytest.mark.timeout(600)
def test_host_arithmetic_under_address_sanitizer():
    """tests/cpp/entry_seeds_host.cpp: ISL_ENTRY_SEEDS parsing, the seed-list check and the pick's grid
    (islands_amd/csrc/entry_seeds_plan.hpp) as a stand-alone program built with -fsanitize=address."""
    csrc = os.path.join(ROOT, "islands_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "../lib/asan/entry_seeds_host", "-s"])
    exe = os.path.join(ROOT, "islands_amd", "lib", "asan", "entry_seeds_host")
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:halt_on_error=1")
    pr = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = pr.stdout.decode(errors="replace")
    assert pr.returncode == 0 and "entry seeds host: ok" in out and "AddressSanitizer" not in out, out[-3000:]


def _recall(orc, metric, x, q, csr, entries, k=5, ef=32):
    ids, cnt = [], []
    for i, qi in enumerate(q):
        r = orc.leann_search(ref.with_entry(orc, csr, entries[i]), x, qi, k, ef, metric=metric)
        assert r.status == 0
        ids.append(r.ids)
        cnt.append(r.ids.size)
    return ref.recall_at(orc, metric, q, x, ids, cnt, k)


@pytest.mark.parametrize("case", ["Cosine", "Euclidean", "DotProduct", "Manhattan", "bf16"])
def test_fixture_property(orc, case):
    """Conditions on the fixture, not on the code under test (measured: 0.031 from node 0 and 0.975-0.994
    from the reference pick)."""
    x, q = ref.fixture()
    metric = 0 if case == "bf16" else ["Cosine", "Euclidean", "DotProduct", "Manhattan"].index(case)
    if case == "bf16":
        x = ref.bf16_image(ref.bf16_bits(x))
    csr = ref.knn_csr(orc, metric, x, tag=case)
    seeds = ref.select(orc, metric, x, 0, 64)
    assert len(set(seeds)) == 64 and seeds[0] == 0
    cold = _recall(orc, metric, x, q, csr, [0] * len(q))
    warm = _recall(orc, metric, x, q, csr, ref.pick(orc, metric, q, x, seeds))
    print(f"{case}: recall@5 from node 0 = {cold:.3f}, from the reference pick = {warm:.3f}")
    assert cold <= 0.1, cold
    assert warm >= 0.9, warm
