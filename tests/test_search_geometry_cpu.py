"""The launch geometry of the search path (islands_amd/csrc/search_geometry.hpp: LDS per wave,
resident waves, visited-table sizes, state-block words, the lane's slots) over a grid of calls,
against tests/golden/search_geometry.txt.  The fixture was recorded from the arithmetic as it stood
when it was still spread over search.hip, by the same driver (tests/cpp/geometry_dump.cpp, which
then included search.hip; the columns the record gained with the move, the fast kernel's bf16-query
variant among them, were computed from that file's expressions).  A change of any figure is a
change of behaviour on the card and has to be meant: re-record the fixture with it.  No device is
needed: the driver is host-only and built by `make -C islands_amd/csrc geometry`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_search_geometry_matches_recorded():
    csrc = os.path.join(ROOT, "islands_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "geometry", "-s"])
    exe = os.path.join(ROOT, "islands_amd", "lib", "geometry_dump")
    # the experiment switches (ISL_HBITS, ISL_HCAP, ...) change the geometry on purpose
    env = {k: v for k, v in os.environ.items() if not k.startswith("ISL_")}
    pr = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-2000:]
    got = pr.stdout.decode().splitlines()
    with open(os.path.join(ROOT, "tests", "golden", "search_geometry.txt")) as f:
        want = f.read().splitlines()
    assert len(want) > 1000
    diff = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, f"{len(diff)} lines differ, first: line {diff[0][0]}\n  recorded {diff[0][1]}\n  now      {diff[0][2]}"
    assert len(got) == len(want)
