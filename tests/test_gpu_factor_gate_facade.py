"""GPU: Covariances::factor_gate of the C++ facade (include/pps_isam.hpp) on the physically weighted corridor (60 poses, 14 planes).

tests/cpp/factor_gate_facade.cpp builds the graph this test writes out (hex doubles) through the facade, optimises it and prints the gate of
all factors (an empty list) and of a sub-list with a repeated factor, once through Slam::covariances() and once through the C-ABI on the
same handle -- the call the Python binding Graph.factor_gate makes.  The two are compared bit for bit; the facade computes the selected
inverse by itself both times (no recovery at first, none after an update()).  The Python binding on its own handle is compared too: the
same flagged entries, d2 to 1e-6 relative (the facade hands a pose measurement on as Pose3d::vector(), which moves the odometry
measurements by an ulp, so the two LM runs do not end on the same bits: tests/test_gpu_merge_gate_facade.py)."""
import os
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from pop_up_slam_amd import synth
from test_gpu_merge_gate_facade import _write

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = [40, 3, 17, 3, 0, 200]


def _parse(lines):
    out = []
    for k in range(0, len(lines), 4):
        d2 = lines[k].split(" "); n = int(d2[1])
        assert d2[0] == "d2" and lines[k + 1].startswith("lev") and lines[k + 2].startswith("flagged") and lines[k + 3].startswith("untestable")
        fl = [int(v) for v in lines[k + 2].split(" ")[1:]]
        out.append(dict(n=n, d2=np.array([float.fromhex(v) for v in d2[2:]]), lev=np.array([float.fromhex(v) for v in lines[k + 1].split(" ")[1:]]),
                        flagged=fl[1:], count=fl[0], untestable=int(lines[k + 3].split(" ")[1])))
    return out


def test_facade_factor_gate_equals_the_cabi_values(built, tmp_path):
    exe = tmp_path / "factor_gate_facade"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "factor_gate_facade.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "pop_up_slam_amd"), "-lpps",
                           "-Wl,-rpath," + os.path.join(ROOT, "pop_up_slam_amd")])
    spec = synth.corridor(60, 14, seed=7, physical_weights=True)
    _write(spec, tmp_path / "graph.txt")
    out = subprocess.run([str(exe), str(tmp_path / "graph.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {"F": [], "C": []}
    for line in out.stdout.splitlines():
        tag, rest = line.split(" ", 1)
        rows[tag].append(rest)
    assert len(rows["F"]) == len(rows["C"]) == 2 * 2 * 4
    assert rows["F"] == rows["C"]                                       # the same bits, the same flagged entries, the same count
    res = _parse(rows["F"])
    n_all = len(spec.f_type)
    assert [r["n"] for r in res] == [n_all, len(SUB), n_all, len(SUB)]
    m = np.where(np.isin(spec.f_type, (synth.F_POSE_PRIOR, synth.F_ODOMETRY)), 6, 3)
    for r, idx in zip(res, (np.arange(n_all), np.array(SUB)) * 2):
        thr = np.where(m[idx] == 3, 7.815, 12.592)
        assert len(r["d2"]) == len(r["lev"]) == r["n"] and np.all(np.isfinite(r["lev"]))
        assert r["untestable"] == int(np.sum(np.isnan(r["d2"]))) == int(np.sum(idx == 0))      # the pose prior, wherever it is listed
        assert r["count"] == len(r["flagged"]) and r["flagged"] == [i for i in range(r["n"]) if np.isfinite(r["d2"][i]) and r["d2"][i] > thr[i]]
    assert 0.01 <= len(res[0]["flagged"]) / (n_all - 1) <= 0.10
    assert abs(float(res[0]["lev"].sum()) - 402) <= 1e-8
    for a, b in ((res[0], res[1]), (res[2], res[3])):                   # an entry has the bits it has among all factors
        assert np.array_equal(b["d2"], a["d2"][SUB], equal_nan=True) and np.array_equal(b["lev"], a["lev"][SUB])
    # the Python binding on a handle of its own
    g = P.Graph(); spec.replay(g)
    g.batch_optimize(); g.cov_recover()
    d2, lev, flagged = g.factor_gate()
    ok = np.isfinite(d2)
    assert np.array_equal(ok, np.isfinite(res[0]["d2"])) and np.max(np.abs(d2 - res[0]["d2"])[ok] / d2[ok]) <= 1e-6
    assert list(flagged) == res[0]["flagged"]
    g.close()
