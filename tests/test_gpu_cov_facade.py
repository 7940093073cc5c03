"""GPU: isam::Covariances of the C++ facade (include/pps_isam.hpp: Slam::covariances(), marginal(list), marginal(lists), access(pairs))
against the C-ABI calls it forwards to, bit for bit (tests/cpp/cov_facade.cpp prints both as hex doubles)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_covariances_equal_the_cabi_values(built, tmp_path):
    exe = tmp_path / "cov_facade"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cov_facade.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "pop_up_slam_amd"), "-lpps",
                           "-Wl,-rpath," + os.path.join(ROOT, "pop_up_slam_amd")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {"F": [], "C": []}
    note = None
    for line in out.stdout.splitlines():
        tag, rest = line.split(" ", 1)
        if tag == "X":
            note = rest
        else:
            rows[tag].append(rest)
    assert len(rows["F"]) == len(rows["C"]) == 2 * (13 + 26 + 2)       # per round: 13 nodes, 26 pairs, 2 lists
    for f, c in zip(rows["F"], rows["C"]):
        assert f == c                                       # same block, same bits
    kinds = {r.split(" ", 1)[0] for r in rows["F"]}
    assert kinds == {"marginal", "access", "joint", "marginal2", "access2", "joint2"}
    # (round 2: after update() the facade recovered again by itself, and the C-ABI reads saw that recovery)
    first = [r.split(" ", 3)[3] for r in rows["F"] if r.startswith("marginal ")]
    second = [r.split(" ", 3)[3] for r in rows["F"] if r.startswith("marginal2 ")]
    assert len(first) == len(second) == 13
    for r in rows["F"]:
        vals = [float.fromhex(v) for v in r.split(" ")[3:]]
        assert all(v == v for v in vals)
    assert note and "share no front" in note
