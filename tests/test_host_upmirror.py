"""CPU: the bookkeeping of the difference upload as a thing of its own (csrc/pps_upmirror.h: UploadMirror -- slots, owners, what differs from the
pinned mirror, what a flush sends), driven without a device by tests/cpp/upmirror_host.cpp.  The program is stand-alone: it is built twice with
g++ alone -- once plain, once with the address and undefined-behaviour sanitizers -- and both builds run as child processes.  It asserts, after
every flush of its seeded layout sequences, that the simulated device holds every array, that refreshed entries of exact rows survive, that the
mirror equals the device over every slot's capacity, and that every piece is aligned and stays inside its slot and below the high-water mark;
under verification, that a lying hint -- and nothing else -- raises the violation flag.  Here: both builds pass, agree line for line, and the
program's own log shows that every branch was taken often enough and that no run skipped more than a quarter of the steps it drew."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "upmirror_host.cpp")
CSRC = os.path.join(ROOT, "pop_up_slam_amd", "csrc")
# (the sanitizer runtimes are linked into the program: it stands alone, whatever the environment of the test preloads)
BUILDS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]}
# every one at least three times over the seed set (spill: the arena had no room, the caller allocates)
BRANCHES = ("fresh", "kept", "moved", "shift", "identical", "exact", "whole", "hint4k", "spill")
# ... and, in the runs with verification on: a false claim that was examined, a claim (true or false) about a slot that had changed owner
VERIFY_BRANCHES = ("lie_caught", "lie_dropped", "hint_dropped")


@pytest.fixture(scope="module")
def logs(tmp_path_factory):
    out = {}
    d = tmp_path_factory.mktemp("upmirror")
    for name, flags in BUILDS.items():
        exe = str(d / ("upmirror_host_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        runs = []
        for line in r.stdout.splitlines():
            w = line.split()
            assert w[0] == "run" and len(w) % 2 == 1, line
            runs.append({w[i]: int(w[i + 1]) for i in range(1, len(w), 2)})
        out[name] = runs
    return out


def test_the_header_is_host_only():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include", os.path.join(CSRC, "pps_upmirror.h"), os.devnull])
    text = open(os.path.join(CSRC, "pps_upmirror.h")).read()
    assert "#include <hip" not in text and '#include "' not in text


def test_both_builds_pass_and_agree(logs):
    assert logs["plain"] == logs["sanitized"] and len(logs["plain"]) >= 8
    assert {r["verify"] for r in logs["plain"]} == {0, 1}


def test_every_branch_is_taken_and_few_steps_are_skipped(logs):
    runs = logs["plain"]
    for r in runs:
        assert r["drawn"] >= 40 and 4 * r["skipped"] <= r["drawn"], r
        assert r["sent"] < r["compared"] and r["patches"] > 0, r            # (a difference upload: most of what is compared stays)
        if not r["verify"]:
            assert r["lie_caught"] == r["lie_dropped"] == 0, r
    total = {b: sum(r[b] for r in runs) for b in BRANCHES}
    assert all(total[b] >= 3 for b in BRANCHES), total
    vtotal = {b: sum(r[b] for r in runs if r["verify"]) for b in VERIFY_BRANCHES}
    assert all(vtotal[b] >= 3 for b in VERIFY_BRANCHES), vtotal
