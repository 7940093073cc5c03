"""GPU: Covariances::marginal_any, block and gate of the C++ facade (include/pps_isam.hpp) on a dense-front graph, where pps_cov_recover
refuses and the facade goes on with pps_cov_factor, against the C-ABI results bit for bit (tests/cpp/cov_factor_facade.cpp prints both as
hex doubles); on a band graph against pps_cov_recover + the C-ABI, which is what they returned before."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_answers_on_a_dense_front_graph_with_the_cabi_bits(built, tmp_path):
    exe = tmp_path / "cov_factor_facade"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cov_factor_facade.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "pop_up_slam_amd"), "-lpps",
                           "-Wl,-rpath," + os.path.join(ROOT, "pop_up_slam_amd")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {"F": [], "C": []}
    notes = {}
    for line in out.stdout.splitlines():
        tag, rest = line.split(" ", 1)
        if tag in rows:
            rows[tag].append(rest)
        else:
            name, text = rest.split(" ", 1)
            notes[tag + name] = text
    assert int(notes["Sdense"]) > 127 and int(notes["Sband"]) <= 127
    assert notes["Rdense"].startswith("5 ") and "dense-front" in notes["Rdense"]       # PPS_ESTATE: the full recovery refuses the graph ...
    assert notes["Rband"].strip() == "0"
    assert len(rows["F"]) == len(rows["C"]) == 2 * 4                     # ... and the facade answers: joint, block, d2, best per graph
    for f, c in zip(rows["F"], rows["C"]):
        assert f == c                                                    # same query, same bits
    for r in rows["F"]:
        if not r.startswith("best"):
            vals = [float.fromhex(v) for v in r.split(" ")[3:]]
            assert vals and all(v == v for v in vals)
    assert "pps_cov_factor" in notes["Xdense"] and "pps_cov_recover" in notes["Xdense"] or "dense-front" in notes["Xdense"]      # marginal() keeps ensure()
    assert notes["Xband"] == "ok"
