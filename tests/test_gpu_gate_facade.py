"""GPU: Covariances::gate of the C++ facade (include/pps_isam.hpp) against pps_assoc_gate -- the call the Python binding
Graph.assoc_gate makes -- on the same handle, bit for bit (tests/cpp/gate_facade.cpp prints both as hex doubles), for all planes and for
a permuted subset, with a valid recovery and after an update() that ended it (gate() recovers by itself, like the other members)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_gate_equals_the_cabi_values(built, tmp_path):
    exe = tmp_path / "gate_facade"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gate_facade.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "pop_up_slam_amd"), "-lpps",
                           "-Wl,-rpath," + os.path.join(ROOT, "pop_up_slam_amd")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {"F": [], "C": []}
    empty = None
    for line in out.stdout.splitlines():
        tag, rest = line.split(" ", 1)
        if tag == "E":
            empty = rest
        else:
            rows[tag].append(rest)
    assert len(rows["F"]) == len(rows["C"]) == 2 * 2 * 3               # per round and plane list: the matrix by both overloads, best
    for f, c in zip(rows["F"], rows["C"]):
        assert f == c                                                   # same candidates, same bits, same best
    mats = [r.split(" ") for r in rows["F"] if r.startswith("d2 ")]
    assert {(m[1], m[2]) for m in mats} == {("4", "4"), ("4", "2")}
    for m in mats:
        vals = [float.fromhex(v) for v in m[3:]]
        assert len(vals) == int(m[1]) * int(m[2]) and all(v == v and v >= 0.0 for v in vals)
    # the subset {plane 2, plane 0} returns the bits those candidates have among all planes
    full, sub = mats[0][3:], mats[2][3:]
    assert [full[i * 4 + j] for i in range(4) for j in (2, 0)] == sub
    # each measurement was taken from its own plane: that plane is the best candidate
    assert rows["F"][2] == "best 0 1 2 3"
    sub_best = rows["F"][5].split(" ")[1:]
    assert sub_best[0] == "1" and sub_best[2] == "0"                    # planes 0 and 2 sit at places 1 and 0 of the subset
    assert empty == "4 0"
