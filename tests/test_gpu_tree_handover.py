"""GPU: the hand-over between the workgroups of the whole-tree K3 launches (k_band_factor_all / k_band_solve_all, XGroup in csrc/pps_k3.hip).
A group's top front hands its update matrix, and a front with children in another group its local solution, to another workgroup of the SAME
launch through write-through stores, a flag and cache-bypassing loads.  Nothing of the arithmetic differs from the launch-per-stage schedule,
so every solved step must have the bits that schedule gives; a value left over from the launch before belongs to another damping value and
cannot pass for the current one."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import pop_up_slam_amd as P
from pop_up_slam_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every graph takes the whole-tree form (checked on the CPU: groups / stages / fronts whose parent sits in another group)
GRAPHS = {
    "corridor_24_6": lambda: synth.corridor(24, 6, seed=1),            # 3 / 2 / 2: the smallest tree with a crossing
    "corridor_120_26": lambda: synth.corridor(120, 26, seed=42),       # 9 / 2 / 8
    "corridor_300_60": lambda: synth.corridor(300, 60, seed=4),        # 26 / 3 / 25
    "small_world_50_10": lambda: synth.small_world(50, 10, seed=3),    # 5 / 2 / 4; p up to 36, b up to 42: the LDS-panel branch of the walk back
}
LAMBDAS = (0.0, 1e-3, 10.0)
DUALS = ((1e-3, 1e-2), (10.0, 100.0))
CYCLE = ((1e-3, 1e-2), (10.0, 100.0), (0.0, 1.0), (0.3, 3e-5))       # test 2: four pairs, ten rounds

# the same calls, written to an .npz: run in a process of its own with PPS_PLAIN_SCHEDULE=4 (a handle reads the switch when it is created)
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_tree_handover as T
np.savez(sys.argv[1], **T.solve_all_cases())
""" % (ROOT, os.path.join(ROOT, "tests"))


def solve_all_cases():
    """name -> array: every delta of every graph, and the form each call reported"""
    out = {}
    for name, make in GRAPHS.items():
        g = P.Graph()
        make().replay(g)
        forms = []
        for lam in LAMBDAS:
            d, _, form, bad = g.debug_solve(lam)
            assert bad == 0.0
            out[f"{name}|{lam!r}"] = d.copy(); forms.append(form)
        for la, lb in DUALS:
            d, d2, form, bad = g.debug_solve(la, lb)
            assert bad == 0.0
            out[f"{name}|{la!r},{lb!r}|0"] = d.copy(); out[f"{name}|{la!r},{lb!r}|1"] = d2.copy(); forms.append(form)
        out[f"{name}|forms"] = np.asarray(forms)
        g.close()
    return out


@pytest.fixture(scope="module")
def whole_tree(built):
    return solve_all_cases()


@pytest.fixture(scope="module")
def per_stage(built, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("handover") / "per_stage.npz")
    e = dict(os.environ)
    e["PPS_PLAIN_SCHEDULE"] = "4"
    r = subprocess.run([sys.executable, "-c", CHILD, path], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_whole_tree_steps_have_the_bits_of_the_per_stage_launches(whole_tree, per_stage, name):
    """debug_solve for three damping values and two dual pairs: form 1 here, form 0 in the child, every delta equal bit for bit"""
    assert (whole_tree[f"{name}|forms"] == 1).all(), whole_tree[f"{name}|forms"]
    assert (per_stage[f"{name}|forms"] == 0).all(), per_stage[f"{name}|forms"]
    keys = [k for k in whole_tree if k.startswith(name + "|") and not k.endswith("|forms")]
    assert len(keys) == len(LAMBDAS) + 2 * len(DUALS)
    for k in keys:
        assert np.isfinite(whole_tree[k]).all() and np.abs(whole_tree[k]).max() > 0, k
        assert_array_equal(whole_tree[k], per_stage[k], err_msg=k)


def _cycle(g, rounds=10):
    """40 consecutive dual solves on one handle, four damping pairs in turn: the results, call by call"""
    res = []
    for k in range(rounds * len(CYCLE)):
        la, lb = CYCLE[k % len(CYCLE)]
        d, d2, form, bad = g.debug_solve(la, lb)
        assert form == 1 and bad == 0.0
        res.append((d.copy(), d2.copy()))
    return res


def _assert_cycle_repeats(res):
    for k in range(len(CYCLE), len(res)):
        assert_array_equal(res[k][0], res[k % len(CYCLE)][0], err_msg=f"call {k}, first damping value")
        assert_array_equal(res[k][1], res[k % len(CYCLE)][1], err_msg=f"call {k}, second damping value")
    for k in range(1, len(CYCLE)):       # (the pairs really differ: a step of the launch before cannot pass for this one)
        assert not np.array_equal(res[k][0], res[0][0]) and not np.array_equal(res[k][1], res[0][1])


@pytest.mark.parametrize("name", list(GRAPHS))
def test_epochs_do_not_leak(built, name):
    """the flags carry the number of the launch pair and are never reset, the buffers are written again by every launch: every call must
    give what the first call with its damping pair gave (the reader's caches hold the lines of the launch before)"""
    g = P.Graph()
    GRAPHS[name]().replay(g)
    _assert_cycle_repeats(_cycle(g))
    g.close()


def test_uneven_load(built, whole_tree):
    """the same cycle on corridor(300, 60) while two host threads keep solving graphs of other sizes on handles of their own: the same bits
    as alone"""
    g = P.Graph()
    GRAPHS["corridor_300_60"]().replay(g)
    alone = _cycle(g, rounds=1)
    others = []
    for spec in (synth.corridor(120, 26, seed=42), synth.corridor()):        # (the second one: the C2 graph)
        h = P.Graph(); spec.replay(h); h.save_state(); h.batch_optimize()
        others.append(h)
    stop = threading.Event()
    errors = []

    def load(h):
        try:
            while not stop.is_set():
                h.restore_state(); h.batch_optimize()
        except Exception as e:      # noqa: BLE001 -- reported by the test below
            errors.append(e)

    threads = [threading.Thread(target=load, args=(h,)) for h in others]
    for t in threads:
        t.start()
    try:
        busy = _cycle(g)
    finally:
        stop.set()
        for t in threads:
            t.join()
    assert not errors, errors
    _assert_cycle_repeats(busy)
    for k in range(len(CYCLE)):
        assert_array_equal(busy[k][0], alone[k][0]); assert_array_equal(busy[k][1], alone[k][1])
    key = "corridor_300_60|0.001,0.01|"
    assert_array_equal(busy[0][0], whole_tree[key + "0"]); assert_array_equal(busy[0][1], whole_tree[key + "1"])
    for h in others:
        h.close()
    g.close()
