"""CPU: the graphs, the reference and the bounds of tests/test_gpu_sweep_counts.py, without a device (tests/sweep_count_helpers.py).

  generator     every case builds, has its counts (asserted in counted_graph from spec.counts(), and here per type slot), is the case it is
                named for, and meets the visibility condition from the oracle alone: at the start, and -- where the oracle's first LM trial
                is accepted -- at the state after it, the smallest r*'r* of any factor is at least 8 x the bound in force
  yardstick     d = |chi2*_oracle - chi2*_numpy| / chi2* <= 1e-13 on every case
  mutations     one mistake at a time in a copy of the reference sum -- the last factor of a type left out, the first one after a multiple of
                256, factor 0 of the next type counted twice, the whole tail [256 floor(n / 256), n), the last Factor2 edge -- breaks the
                bound on the case named for that count
  rejected      the kicked graph's first LM trial at lambda0 = 1e-6 and its second at 1e-5 are rejected by the oracle
"""
import numpy as np
import pytest

import sweep_count_helpers as SC
from oracle import oracle_py as O
from pop_up_slam_amd import synth

NAMES = list(SC.CASES)
_REF = {}


def _ref(name):
    if name not in _REF:
        _REF[name] = SC.Reference(SC.make(name))
    return _REF[name]


def _after_first_trial(name):
    """(accepted, state after the oracle's first LM trial) -- the state the device's first accepted trial is compared at"""
    spec = SC.make(name)
    o = O.OracleGraph(max_iterations=1)
    nid, _ = spec.replay(o)
    o.batch_optimize()
    tr = o.trace()
    ref = _ref(name)
    poses = np.array([o.get_pose(int(nid[i])) for i in ref.pose_nodes]).reshape(-1, 7)
    planes = np.array([o.get_plane(int(nid[i])) for i in ref.plane_nodes]).reshape(-1, 4)
    return (tr[0][2] if tr else False), (poses, planes)


def test_block_constants_and_count_lists():
    assert (SC.CHI, SC.LIN, SC.PER_BLOCK, SC.OBS_PER_BLOCK) == (256, 128, 8, 12)
    for axis in ("pp", "lp", "odo", "obs", "repop"):
        for n in SC.COUNTS[axis]:
            assert f"{axis}-{n}" in SC.CASES
            if axis == "repop":
                assert f"repop_short-{n}" in SC.CASES
    for name in ("nodes-255", "nodes-256", "nodes-257", "nodes-512", "nodes-513", "nodes-pose256", "nodes-pose250", "zero-pp", "zero-lp", "zero-obs", "zero-obs_fixed"):
        assert name in SC.CASES


@pytest.mark.parametrize("name", NAMES)
def test_case_builds_is_what_it_is_named_for_and_is_visible(name):
    spec = SC.make(name)
    c = SC.CASES[name]
    assert c["is_case"](spec)
    slots = SC.type_slots(spec)
    counts = spec.counts()
    assert len(slots["obs"]) + len(slots["repop"]) == counts[synth.F_PLANE_OBS] and len(slots["odo"]) == counts[synth.F_ODOMETRY]
    assert len(slots["pp"]) == counts[synth.F_POSE_PRIOR] and len(slots["lp"]) == counts[synth.F_PLANE_PRIOR]
    assert len(spec.f_type) <= 1400 and len(spec.node_type) <= 520, (len(spec.f_type), len(spec.node_type))
    if SC.varied_type(name):
        n = c["count"]
        assert len(slots[SC.varied_type(name)]) == n
    # visibility: no factor starts at r = 0 -- pose 0 and the ground have left the values their priors measure
    ref = _ref(name)
    res = ref.residuals()
    chi2, d, dr = ref.yardstick(res)
    ratio = SC.assert_visible((name, "start"), res, SC.bound_exact(chi2, d))
    accepted, state = _after_first_trial(name)
    ratio1 = None
    if accepted:
        ref.set_state(*state)
        res1 = ref.residuals()
        chi1, d1, _ = ref.yardstick(res1)
        assert d1 <= 1e-13, (name, d1)
        ratio1 = SC.assert_visible((name, "after the first accepted trial"), res1, SC.bound_exact(chi1, d1))
        ref.set_state(*ref.start)
    print(f"SWEEPCOUNTS {name}: {len(spec.f_type)} factors {len(spec.node_type)} nodes chi2* {chi2:.6g} d {d:.2e} worst |dr| {dr:.2e} "
          f"min r'r / bound {ratio:.3g} at the start, {'-' if ratio1 is None else format(ratio1, '.3g')} after the first accepted trial")


@pytest.mark.parametrize("name", NAMES)
def test_two_cpu_statements_agree(name):
    chi2, d, dr = _ref(name).yardstick()
    assert d <= 1e-13, (name, d)
    assert dr <= 1e-12, (name, dr)


@pytest.mark.parametrize("name", [n for n in NAMES if SC.varied_type(n)])
def test_the_bound_catches_a_mistake_at_the_edge_it_is_named_for(name):
    spec, ref = SC.make(name), _ref(name)
    res = ref.residuals()
    chi2, d, _ = ref.yardstick(res)
    bound = SC.bound_exact(chi2, d)
    which = SC.varied_type(name)
    muts = SC.mutated_sums(spec, res, which)
    n = SC.CASES[name]["count"]
    first = len(SC.type_slots(spec)["obs"]) if which == "repop" else 0
    # which mutations the count must offer
    want = {"drop_last"} if n > 0 else set()
    if first + n > SC.CHI:
        want.add("drop_after_256")
    if (first + n) % SC.CHI and n > 0:
        want.add("drop_tail")
    if which != "lp":
        want.add("next_twice")
    if which == "repop":
        want.add("drop_last_repop")
    assert want <= set(muts), (name, want, sorted(muts))
    for m, v in muts.items():
        assert abs(v - chi2) > bound, (name, m, v, chi2, bound)
        assert abs(v - chi2) >= 8.0 * bound, (name, m, abs(v - chi2) / bound)
    assert abs(SC.Reference.chi2_of(res) - chi2) == 0.0


def test_rejected_first_and_second_trial():
    spec = SC.make("rejected")
    assert (spec.n_poses, spec.n_planes, spec.counts()[synth.F_PLANE_OBS]) == (256, 30, 768)
    o = O.OracleGraph(max_iterations=2)
    spec.replay(o)
    c0 = o.chi2()
    it = o.batch_optimize()
    tr = o.trace()
    print("SWEEPCOUNTS rejected: chi2", c0, "trace", tr)
    assert it == 2 and len(tr) == 2
    assert tr[0][0] == SC.LAMBDA0 and tr[1][0] == SC.LAMBDA0 * SC.LAMBDA_FACTOR
    assert not tr[0][2] and not tr[1][2] and tr[0][1] > c0 and tr[1][1] > c0
    # the start is visible under the exact bound, and the two CPU statements agree on it
    ref = SC.Reference(spec)
    res = ref.residuals()
    chi2, d, _ = ref.yardstick(res)
    assert d <= 1e-13 and abs(chi2 - c0) <= 1e-12 * chi2
    SC.assert_visible("rejected start", res, SC.bound_exact(chi2, d))
