"""GPU: Covariances::merge_gate of the C++ facade (include/pps_isam.hpp) on corridor_60_14.

tests/cpp/merge_gate_facade.cpp builds the graph this test writes out (hex doubles) through the facade, optimises it and prints the merge
gate of all 14 planes and of a permuted sub-list, once through Slam::covariances() and once through the C-ABI on the same handle -- the
call the Python binding Graph.merge_gate makes.  The two are compared bit for bit.  The Python binding on its own handle is compared too:
best and pairs equal, d2 to 1e-6 relative -- the facade hands a pose measurement on as Pose3d::vector() (Euler angles back from a quaternion),
which moves the odometry measurements by an ulp, so the two LM runs do not end on the same bits."""
import os
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from pop_up_slam_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(spec, path):
    hx = lambda v: " ".join(float(x).hex() for x in v)
    with open(path, "w") as f:
        for t, v in zip(spec.node_type, spec.node_init):
            f.write(("P " + hx(v[:7]) if t == synth.NODE_POSE else "L " + hx(v[:4])) + "\n")
        for t, (a, b), m, w in zip(spec.f_type, spec.f_nodes, spec.f_meas, spec.f_sqrtinf):
            if t == synth.F_POSE_PRIOR: f.write(f"p {a} {hx(m[:6])} {hx(w[:21])}\n")
            elif t == synth.F_ODOMETRY: f.write(f"o {a} {b} {hx(m[:6])} {hx(w[:21])}\n")
            elif t == synth.F_PLANE_OBS: f.write(f"l {a} {b} {hx(m[:4])} {hx(w[:6])}\n")
            else: f.write(f"q {a} {hx(m[:4])} {hx(w[:6])}\n")


def _parse(lines):
    out = []
    for k in range(0, len(lines), 4):
        d2 = lines[k].split(" "); n = int(d2[1])
        assert d2[0] == "d2" and lines[k + 1].startswith("best") and lines[k + 2].startswith("pairs") and lines[k + 3].startswith("notpd")
        pr = [int(v) for v in lines[k + 2].split(" ")[1:]]
        out.append(dict(n=n, d2=np.array([float.fromhex(v) for v in d2[2:]]).reshape(n, n), best=[int(v) for v in lines[k + 1].split(" ")[1:]],
                        pairs=list(zip(pr[1::2], pr[2::2])), count=pr[0], notpd=int(lines[k + 3].split(" ")[1])))
    return out


def test_facade_merge_gate_equals_the_cabi_values(built, tmp_path):
    exe = tmp_path / "merge_gate_facade"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "merge_gate_facade.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "pop_up_slam_amd"), "-lpps",
                           "-Wl,-rpath," + os.path.join(ROOT, "pop_up_slam_amd")])
    spec = synth.corridor(60, 14, seed=7)
    _write(spec, tmp_path / "graph.txt")
    out = subprocess.run([str(exe), str(tmp_path / "graph.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = {"F": [], "C": []}
    single = None
    for line in out.stdout.splitlines():
        tag, rest = line.split(" ", 1)
        if tag == "E":
            single = rest
        else:
            rows[tag].append(rest)
    assert len(rows["F"]) == len(rows["C"]) == 2 * 2 * 4
    assert rows["F"] == rows["C"]                                       # the same bits, the same best, the same pairs
    res = _parse(rows["F"])
    assert [r["n"] for r in res] == [14, 5, 14, 5]
    for r in res:
        n = r["n"]; off = ~np.eye(n, dtype=bool)
        assert np.array_equal(r["d2"], r["d2"].T) and not np.diag(r["d2"]).any() and np.all(np.isfinite(r["d2"])) and np.all(r["d2"][off] > 0)
        assert r["count"] == len(r["pairs"]) and r["notpd"] == 0
        assert r["pairs"] == [(i, j) for i in range(n) for j in range(i + 1, n) if r["d2"][i, j] < 7.815]
        assert r["best"] == [int(np.argmin(np.where(off, r["d2"], np.inf)[i])) for i in range(n)]
    sub = [9, 2, 5, 0, 11]                                              # a pair that keeps its order has the bits it has among all planes
    for x in range(5):
        for y in range(x + 1, 5):
            if sub[x] < sub[y]:
                assert res[1]["d2"][x, y] == res[0]["d2"][sub[x], sub[y]]
    assert single == "1 1 -1 0"
    # the Python binding on a handle of its own
    g = P.Graph(); nid, _ = spec.replay(g)
    g.batch_optimize(); g.cov_recover()
    planes = [int(n) for n, t in zip(nid, spec.node_type) if t == synth.NODE_PLANE]
    d2, best, pairs = g.merge_gate(planes)
    off = ~np.eye(14, dtype=bool)
    assert np.max(np.abs(d2 - res[0]["d2"])[off] / d2[off]) <= 1e-6
    assert list(best) == res[0]["best"] and [tuple(p) for p in pairs] == res[0]["pairs"]
    g.close()
