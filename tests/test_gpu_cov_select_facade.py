"""GPU: Covariances::select of the C++ facade (include/pps_isam.hpp) on a dense-front graph (tests/cpp/cov_select_facade.cpp).  marginal() throws
before select(); after it marginal({pose}), marginal({pose, plane}) of a factor-joined pair and access() in both orders agree with
marginal_any() / block() of the same handle -- column solves on the same factor, an independent route -- to the rule of
tests/test_gpu_cov_select.py: e = |M - M0|_F / sqrt(|S(r, r)|_F |S(c, c)|_F) per node pair, e <= max(16 d, 1e-12).  No dense inverse is built
here, so d is zero and the bound is its floor, 1e-12 (the two routes differed by 1e-15 .. 1e-14 on this graph's relatives in
tests/test_gpu_cov_select.py).  After add_factor the strict forms throw again."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_select_serves_the_strict_forms_on_a_dense_front_graph(built, tmp_path):
    exe = tmp_path / "cov_select_facade"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cov_select_facade.cpp"), "-o", str(exe),
                           "-L", os.path.join(ROOT, "pop_up_slam_amd"), "-lpps",
                           "-Wl,-rpath," + os.path.join(ROOT, "pop_up_slam_amd")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    mats = {"F": {}, "C": {}}
    notes = {}
    for line in out.stdout.splitlines():
        tag, rest = line.split(" ", 1)
        if tag in mats:
            what, r, c, *vals = rest.split(" ")
            mats[tag][what] = np.array([float.fromhex(v) for v in vals]).reshape(int(r), int(c))      # (row-major)
        else:
            name, text = rest.split(" ", 1)
            notes[tag + name] = text
    assert int(notes["Sfront"]) > 127
    assert notes["Xbefore"] != "ok" and ("dense-front" in notes["Xbefore"] or "pps_cov_recover" in notes["Xbefore"])
    assert notes["Xafter"] != "ok"
    assert sorted(mats["F"]) == sorted(mats["C"]) == ["one", "plane_pose", "pose_plane", "two"]
    Spp, Sll = mats["C"]["two"][:6, :6], mats["C"]["two"][6:, 6:]
    nrm = np.linalg.norm
    e = 0.0
    assert mats["F"]["one"].shape == (6, 6) and mats["F"]["two"].shape == (9, 9) and mats["F"]["pose_plane"].shape == (6, 3) and mats["F"]["plane_pose"].shape == (3, 6)
    assert np.array_equal(mats["F"]["one"], mats["F"]["one"].T) and np.array_equal(mats["F"]["two"], mats["F"]["two"].T)
    assert np.array_equal(mats["F"]["pose_plane"], mats["F"]["plane_pose"].T)
    e = max(e, nrm(mats["F"]["one"] - mats["C"]["one"]) / nrm(Spp))
    for (r0, r1, Sr) in ((0, 6, Spp), (6, 9, Sll)):
        for (c0, c1, Sc) in ((0, 6, Spp), (6, 9, Sll)):
            e = max(e, nrm(mats["F"]["two"][r0:r1, c0:c1] - mats["C"]["two"][r0:r1, c0:c1]) / np.sqrt(nrm(Sr) * nrm(Sc)))
    for what in ("pose_plane", "plane_pose"):
        e = max(e, nrm(mats["F"][what] - mats["C"][what]) / np.sqrt(nrm(Spp) * nrm(Sll)))
    print(f"COVSEL facade: e {e:.3e} (select against the column solves) bound 1.000e-12")
    assert e <= 1e-12, e
