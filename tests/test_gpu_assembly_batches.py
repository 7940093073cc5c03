"""GPU: the assembly of a front in the whole-tree factor launch (k_band_factor_all, csrc/pps_k3.hip) -- the gather of the original entries
in batches whose items exist by the lane's item count (el_issue / el_apply), one batch of 3, 8 or 11 items per lane by the front's size and a
tail loop behind the largest class, and the paired extend-add of a front with two children whose wave waits for them (targets requested in
front of the wait, both children's values in one round trip, a child beyond one batch of 640 entries continued by the sequential loop).

Every graph is asserted -- from pps_analysis_dump alone -- to hold the shapes it is there for, and to take the whole-tree form
(pps_debug_solve form 1).  Every solved step is checked two ways: against the dense reference of tests/linsolve_helpers.py with that helper's own
bound (max(16 d, 1e-12), whole step and per node block) -- the yardstick that does not depend on the code under test --, and bit for bit against
a fresh process with PPS_PLAIN_SCHEDULE=4 (one launch per band stage, plain walk: the sequential extend-add), which holds the two schedules
together.

A leaf above 704 original entries (the tail loop behind the batch of eleven) inside a front of at most 64 rows was looked for among the synth
generators -- corridor and small_world over 20 .. 100 poses, 4 .. 20 planes, 5 .. 12 observations per pose, seeds 1 .. 5 -- and found:
small_world(20, 6, 8) has two leaves of 720 entries (p = 24, b = 30) at every seed tried; seed 1 is the fifth graph here."""
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import pop_up_slam_amd as P
import linsolve_helpers as LH
from pop_up_slam_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRAPHS = {
    "corridor_60_14": lambda: synth.corridor(60, 14, seed=7),          # the smallest tree found with leaves in the 513 .. 704 class
    "small_world_20_6": lambda: synth.small_world(20, 6, seed=2),      # 9 fronts, three of them in that class
    "small_world_50_10": lambda: synth.small_world(50, 10, seed=3),    # children whose update matrix exceeds one batch of 640 entries
    "corridor_24_6": lambda: synth.corridor(24, 6, seed=1),            # every child within one batch; the smallest tree with a group crossing
    "small_world_20_6_8": lambda: synth.small_world(20, 6, 8, seed=1), # two leaves of 720 entries: the tail loop behind the batch of eleven
}
LAMBDAS = (0.0, 1e-3, 10.0)
DUALS = ((1e-3, 1e-2), (10.0, 100.0))
LM_GRAPH = "corridor_60_14"
EA_BATCH = 640                                                         # kEaDepth x 64


def tree_shapes(A):
    """(original entries per front, entries of every front's own update matrix, children per front, parent, fronts whose parent sits in
    another band group) from the analysis alone"""
    nf = A["n_fronts"]
    n_el = np.diff(A["f_el_off"])[:nf]
    upd = (A["f_b"] + 1) * (A["f_b"] + 2) // 2                         # packed lower triangle of the boundary rows + the rhs row
    par = A["f_parent"]
    nch = np.bincount(par[par >= 0], minlength=nf)
    grp = np.zeros(nf, dtype=np.int64)
    for gi in range(A["n_groups"]):
        a, e = A["glvl_front_off"][A["grp_lvl_off"][gi]], A["glvl_front_off"][A["grp_lvl_off"][gi + 1]]
        grp[A["glvl_fronts"][a:e]] = gi
    cross = np.array([s for s in range(nf) if par[s] >= 0 and grp[par[s]] != grp[s]], dtype=np.int64)
    return n_el, upd, nch, par, cross


def el_classes(n_el):
    return [int((n_el <= 192).sum()), int(((n_el > 192) & (n_el <= 512)).sum()), int(((n_el > 512) & (n_el <= 704)).sum()), int((n_el > 704).sum())]


def assert_shapes(name, A):
    n_el, upd, nch, par, cross = tree_shapes(A)
    child_upd = upd[par >= 0]
    assert A["max_front"] <= 64 and A["n_stages"] >= 2 and len(cross) >= 2, "whole-tree form: register-resident fronts, a group crossing"
    assert set(np.unique(nch)) <= {0, 2}, "every front above the leaves has exactly two children: the paired extend-add"
    if name == "corridor_60_14":
        assert A["n_fronts"] == 31 and el_classes(n_el) == [15, 14, 2, 0], (A["n_fronts"], el_classes(n_el))
        assert (nch[n_el > 512] == 0).all(), "the largest fronts are leaves"
    elif name == "small_world_20_6":
        assert A["n_fronts"] == 9 and el_classes(n_el)[2:] == [3, 0], (A["n_fronts"], el_classes(n_el))
    elif name == "small_world_50_10":
        assert int((child_upd > EA_BATCH).sum()) == 13 and int(child_upd.max()) == 946, (int((child_upd > EA_BATCH).sum()), int(child_upd.max()))
        assert (upd[cross] > EA_BATCH).any() and (np.delete(upd, cross)[np.delete(par, cross) >= 0] > EA_BATCH).any(), "beyond one batch inside a group AND across groups"
    elif name == "corridor_24_6":
        assert A["n_fronts"] == 15 and int(child_upd.max()) <= EA_BATCH and A["n_groups"] == 3 and len(cross) == 2
    elif name == "small_world_20_6_8":
        assert A["n_fronts"] == 9 and el_classes(n_el) == [4, 2, 1, 2] and int(n_el.max()) == 720 and (nch[n_el > 704] == 0).all(), el_classes(n_el)
    else:
        raise AssertionError(name)


# the same calls, written to an .npz: run in a process of its own with PPS_PLAIN_SCHEDULE=4 (a handle reads the switch when it is created)
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_assembly_batches as T
np.savez(sys.argv[1], **T.solve_all_cases())
""" % (ROOT, os.path.join(ROOT, "tests"))


def solve_all_cases():
    """name -> array: every delta of every graph, the form each call reported; LM_GRAPH: the iteration count and trace of batch_optimize"""
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
        if name == LM_GRAPH:
            out["lm|iters"] = np.asarray([g.batch_optimize()])
            out["lm|trace"] = np.asarray([(lam, chi, float(acc)) for lam, chi, acc in g.trace()])
        g.close()
    return out


@pytest.fixture(scope="module")
def whole_tree(built):
    return solve_all_cases()


@pytest.fixture(scope="module")
def plain(built, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("assembly") / "plain.npz")
    e = dict(os.environ)
    e["PPS_PLAIN_SCHEDULE"] = "4"
    r = subprocess.run([sys.executable, "-c", CHILD, path], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def references(built):
    """per graph: the analysis, the normal equations at the initial estimate and the dense solves of every damping value -- computed once,
    never modified"""
    out = {}
    for name, make in GRAPHS.items():
        spec = make()
        g = P.Graph(); spec.replay(g); g.analyze()
        A = g.analysis_dump()
        mode = int(g.props.jacobian_mode)
        H, b, lay = LH.assemble_normal_equations(g, spec, A, mode)
        g.close()
        refs = {}
        for lam in sorted(set(LAMBDAS) | {x for p in DUALS for x in p}):
            Hl = LH.damped(H, lam)
            x1, x2, d = LH.reference_solves(Hl, b)
            for v in (x1, x2, Hl):
                v.setflags(write=False)
            refs[lam] = (Hl, (x1, x2, d), LH.cond_spd(Hl))
        b.setflags(write=False)
        out[name] = (A, b, lay, refs)
    return out


@pytest.mark.parametrize("name", list(GRAPHS))
def test_graph_has_its_shapes_and_takes_the_whole_tree_form(references, whole_tree, plain, name):
    assert_shapes(name, references[name][0])
    assert (whole_tree[f"{name}|forms"] == 1).all(), whole_tree[f"{name}|forms"]
    assert (plain[f"{name}|forms"] == 0).all(), plain[f"{name}|forms"]


@pytest.mark.parametrize("name", list(GRAPHS))
def test_steps_against_the_dense_solve(references, whole_tree, name):
    A, b, lay, refs = references[name]

    def check(key, lam):
        Hl, r, cond = refs[lam]
        LH.check_step(f"{name} {key}", whole_tree[f"{name}|{key}"], Hl, b, lay, 1, r, cond)

    for lam in LAMBDAS:
        check(repr(lam), lam)
    for la, lb in DUALS:
        check(f"{la!r},{lb!r}|0", la)
        check(f"{la!r},{lb!r}|1", lb)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_steps_have_the_bits_of_the_plain_schedule(whole_tree, plain, name):
    keys = [k for k in whole_tree if k.startswith(name + "|") and not k.endswith("|forms")]
    assert len(keys) == len(LAMBDAS) + 2 * len(DUALS)
    for k in keys:
        assert np.isfinite(whole_tree[k]).all() and np.abs(whole_tree[k]).max() > 0, k
        assert_array_equal(whole_tree[k], plain[k], err_msg=k)


def test_lm_run_is_the_same_in_both_schedules(whole_tree, plain):
    assert whole_tree["lm|iters"][0] == plain["lm|iters"][0] > 0
    assert_array_equal(whole_tree["lm|trace"], plain["lm|trace"])
