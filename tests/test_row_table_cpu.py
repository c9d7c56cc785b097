"""The row table without a device.  The layout rule of islands_amd/csrc/row_table_plan.hpp, printed by
tests/cpp/row_table_dump.cpp over a grid of shapes, against a Python restatement of the rule; and the owning
type of islands_amd/csrc/row_table.hpp over fake allocators, a stand-alone program under AddressSanitizer
and UndefinedBehaviorSanitizer (tests/cpp/row_table_host.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
DS = list(range(1, 71)) + [768, 4096, 65536]
NS = [1, 1000, 10 ** 7]


def ceil_to(d, m):
    return (d + m - 1) // m * m


def elem_size(dtype):
    return 2 if dtype == BF16 else 4


def stride(dtype, d):
    return ceil_to(d, 8) if dtype == BF16 else ceil_to(d, 4)


def slack(dtype):
    return 512 if dtype == BF16 else 256


def expected_lines():
    out = []
    for dtype in (F32, BF16):
        for d in DS:
            assert stride(dtype, d) * elem_size(dtype) % 16 == 0 and slack(dtype) * elem_size(dtype) == 1024
            out.append(f"layout {dtype} {d} -> {elem_size(dtype)} {stride(dtype, d)} {slack(dtype)}")
            for n in NS:
                out.append(f"alloc {dtype} {d} {n} -> {n * stride(dtype, d) + slack(dtype)}")
    for d in DS:
        s32 = ceil_to(d, 4)
        for n in NS:
            chunk = max(1, min(n, (256 << 20) // (s32 * 4)))
            out.append(f"norms {d} {n} -> {chunk} {chunk * s32 + 256}")
            for slab in (0, min(n, 256), n):
                out.append(f"cache {d} {slab} {n} -> {(slab * s32 + 256) * 4 + slab * 12 + (n + 1) * 4}")
    return out


def test_layout_rule_against_its_restatement():
    src = os.path.join(ROOT, "tests", "cpp", "row_table_dump.cpp")
    exe = os.path.join(ROOT, "islands_amd", "lib", "row_table_dump")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", src, "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    want = expected_lines()
    assert len(got) == len(want) == 2 * len(DS) * (1 + len(NS)) + len(DS) * len(NS) * 4
    for g, w in zip(got, want):
        assert g == w


@pytest.mark.timeout(600)
def test_owning_type_under_sanitizers():
    """tests/cpp/row_table_host.cpp: moves, reset, a dtype without a block, the free-before-allocate order and
    the entry-seed group, as a stand-alone program built with -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "islands_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "../lib/asan/row_table_host", "-s"])
    exe = os.path.join(ROOT, "islands_amd", "lib", "asan", "row_table_host")
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:halt_on_error=1")
    pr = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = pr.stdout.decode(errors="replace")
    assert pr.returncode == 0 and "row table host: ok" in out, out[-3000:]
    assert "Sanitizer" not in out and "runtime error" not in out, out[-3000:]
