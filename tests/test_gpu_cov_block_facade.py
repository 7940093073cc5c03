"""GPU: Covariances::block and Covariances::marginal_any of the C++ facade (include/pps_isam.hpp) against pps_cov_block, which they
forward to, bit for bit (tests/cpp/cov_block_facade.cpp prints both as hex doubles); marginal_any answers for the list of nodes for
which marginal keeps throwing "share no front"."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_blocks_equal_the_cabi_values(built, tmp_path):
    exe = tmp_path / "cov_block_facade"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cov_block_facade.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "pop_up_slam_amd"), "-lpps",
                           "-Wl,-rpath," + os.path.join(ROOT, "pop_up_slam_amd")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {"F": [], "C": []}
    notes = {}
    for line in out.stdout.splitlines():
        tag, rest = line.split(" ", 1)
        if tag in ("X", "Y"):
            notes[tag] = rest
        else:
            rows[tag].append(rest)
    assert len(rows["F"]) == len(rows["C"]) == 2 * (2 + 3)             # per round: 2 joint marginals, 3 rectangular blocks
    for f, c in zip(rows["F"], rows["C"]):
        assert f == c                                       # same block, same bits
    assert {r.split(" ", 1)[0] for r in rows["F"]} == {"any", "block", "any2", "block2"}
    for r in rows["F"]:
        vals = [float.fromhex(v) for v in r.split(" ")[3:]]
        assert vals and all(v == v for v in vals)
    # (first pose) x (last pose) is 6 x 6, and the joint of the two is 12 x 12 with that block in its corner
    blk = next(r for r in rows["F"] if r.startswith("block 6 6 ")).split(" ")[3:]
    joint = next(r for r in rows["F"] if r.startswith("any 12 12 ")).split(" ")[3:]
    assert [joint[a * 12 + 6 + c] for a in range(6) for c in range(6)] == blk
    assert "share no front" in notes["X"]                   # marginal() keeps its strict contract ...
    assert notes["Y"] == "12 12"                            # ... where marginal_any() answers
