"""Shared by tests/test_host_sweep_counts.py and tests/test_gpu_sweep_counts.py: the CPU side of the per-type count tests of K1 (the
linearisation sweep, csrc/pps_k1*.hip) and K4 (the chi2 / retraction launches, csrc/pps_k4.hip, and their robust copies).  Nothing in here
is code under test: block constants read from the headers, graphs with an exact count of every factor type, the reference and the bounds.

  BLOCKS / COUNTS      kChiBlock, kLinBlock, kLanesPerBlock, kLaneGroup, kObsLanes read out of csrc/pps_k4_body.h and csrc/pps_k1_body.h
                       (today's values asserted) and the count lists derived from them: 8 priors / 12 observations per block of the lane
                       form, 64 Factor2 edges per wave, 128 factors per block of the thread form, 256 per chi2 and retraction block
  counted_graph        a synth.corridor brought to exactly n_pp pose priors, n_odo odometry edges, n_obs plane observations (n_repop of
                       them Pose3d_Plane3d_Factor2 edges) and n_lp plane priors; every measurement truth (+) noise under its own seed;
                       EVERY node's initial value moved by exmap of seeded noise, pose 0 and the ground too, so that no factor starts
                       with r = 0 (a factor left out of a sum would not show)
  CASES / make         one axis varied at a time around 64 poses / 14 planes / 4 observations per pose, the zero-count graphs, and the
                       kicked graph whose first LM trial is rejected; every case asserts from its inputs that it is the case it is named for
  Reference            the C oracle at a state set with set_pose / set_plane: r* per factor (factor_error; phi of tests/robust_helpers.py
                       with a cost function), chi2* = math.fsum of the squares, J* (factor_jacobian; central differences through phi
                       with a cost function), the retraction of a state by a step delta, S = sum 2 |r*|' |J*| 1; and the second CPU
                       statement (oracle/numpy_ref.py through robust_helpers.RobustGraph) summed the same way:
                       d = |chi2*_oracle - chi2*_numpy| / chi2*
  bound_exact / bound_retracted / eta / assert_visible
                       the bounds (all figures are the suite's own: test_chi2_matches_oracle's 1e-12, linsolve_helpers.check_step's
                       16 d, test_the_hook_measures_the_shipped_path's 1e-13 |delta|_inf + 64 eps max(1, |x|_inf)) and the visibility
                       condition: the smallest r*'r* of any factor is at least 8 x the bound in force, so that one factor left out or
                       counted twice misses the bound by a factor of 8
"""
import math
import os
import re

import numpy as np

import k2_shape_helpers as KS
import robust_helpers as RH
from oracle import oracle_py as O
from pop_up_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pop_up_slam_amd", "csrc")
EPS = float(np.finfo(float).eps)
LAMBDA0, LAMBDA_FACTOR = 1e-6, 10.0           # Properties.h / pps_default_props: lm_lambda0, lm_lambda_factor
NUM_DIFF_EPS = 1e-4                           # numericalDiff.cpp: the step of the central differences
COST = (RH.PSEUDO_HUBER, 1.0)                 # the one smooth cost of the robust forms, b = 1


# ---- block constants --------------------------------------------------------------------------------------------------------
def _constant(header, name):
    text = open(os.path.join(CSRC, header)).read()
    m = re.findall(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert len(m) == 1, (header, name, m)
    return int(m[0])


BLOCKS = {"kChiBlock": _constant("pps_k4_body.h", "kChiBlock"), "kLinBlock": _constant("pps_k1_body.h", "kLinBlock"),
          "kLanesPerBlock": _constant("pps_k1_body.h", "kLanesPerBlock"), "kLaneGroup": _constant("pps_k1_body.h", "kLaneGroup"),
          "kObsLanes": _constant("pps_k1_body.h", "kObsLanes")}
# (a change of one of them moves the block edges: the count lists below follow, and whoever changes it has to look at this file)
assert BLOCKS == {"kChiBlock": 256, "kLinBlock": 128, "kLanesPerBlock": 256, "kLaneGroup": 32, "kObsLanes": 19}, BLOCKS
CHI = BLOCKS["kChiBlock"]                                                  # factors per chi2 block, nodes per retraction block
LIN = BLOCKS["kLinBlock"]                                                  # factors per block of the thread form
PER_BLOCK = BLOCKS["kLanesPerBlock"] // BLOCKS["kLaneGroup"]               # kFactorsPerBlock: 8
OBS_PER_BLOCK = (BLOCKS["kLanesPerBlock"] // 64) * (64 // BLOCKS["kObsLanes"])     # kObsPerBlock: 12
REPOP_WAVE = 64                                                            # k_linearize_repop: one wave of 64 edges per workgroup


def _around(*edges):
    return [n + k for n in edges for k in (-1, 0, 1)]


COUNTS = {
    "pp": [1] + _around(PER_BLOCK, LIN, CHI),
    "lp": [1] + _around(PER_BLOCK, LIN, CHI),
    "odo": [0] + _around(PER_BLOCK, LIN, CHI),
    "obs": _around(OBS_PER_BLOCK, CHI, 2 * CHI),
    "repop": [1] + _around(REPOP_WAVE, CHI),
}
assert COUNTS["pp"] == [1, 7, 8, 9, 127, 128, 129, 255, 256, 257] and COUNTS["obs"] == [11, 12, 13, 255, 256, 257, 511, 512, 513]
assert COUNTS["repop"] == [1, 63, 64, 65, 255, 256, 257]
N_POSE, N_PLANE, OBS_PER_POSE = 64, 14, 4                                   # the baseline the other types stay at


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def _rng(seed, tag, k=0):
    """a generator of its own per (graph seed, what is drawn, which one)"""
    return np.random.default_rng([int(seed), int(tag), int(k)])


class _Lists:
    """a GraphSpec as lists that can lose and gain factors; back to a KS.RepopSpec with spec()"""

    def __init__(self, base):
        F = len(base.f_type)
        self.base = base
        self.ft, self.fn, self.fm, self.fs = list(base.f_type), [tuple(int(v) for v in p) for p in base.f_nodes], list(base.f_meas), list(base.f_sqrtinf)
        self.after = list(base.meta["factor_after_node"])
        self.repop = list(getattr(base, "f_repop", None) if getattr(base, "f_repop", None) is not None else np.zeros(F, dtype=bool))
        self.ray = list(getattr(base, "f_ray", None) if getattr(base, "f_ray", None) is not None else np.zeros((F, 6)))

    def count(self, t, repop=None):
        return sum(1 for k in range(len(self.ft)) if self.ft[k] == t and (repop is None or bool(self.repop[k]) == repop))

    def add(self, t, a, b, meas, sq):
        m = np.zeros(6); m[:len(meas)] = meas
        s = np.zeros(21); s[:len(sq)] = sq
        self.ft.append(t); self.fn.append((int(a), int(b))); self.fm.append(m); self.fs.append(s)
        self.after.append(len(self.base.node_type) - 1); self.repop.append(False); self.ray.append(np.zeros(6))

    def drop(self, ks):
        ks = set(ks)
        for name in ("ft", "fn", "fm", "fs", "after", "repop", "ray"):
            setattr(self, name, [v for k, v in enumerate(getattr(self, name)) if k not in ks])

    def spec(self, name, node_init):
        b = self.base
        return KS.RepopSpec(name=name, node_type=b.node_type, node_init=node_init, f_type=np.array(self.ft, dtype=np.int32),
                            f_nodes=np.array(self.fn, dtype=np.int32).reshape(-1, 2), f_meas=np.array(self.fm).reshape(-1, 6),
                            f_sqrtinf=np.array(self.fs).reshape(-1, 21), truth=b.truth,
                            meta=dict(b.meta, factor_after_node=np.array(self.after, dtype=np.int64)),
                            f_repop=np.array(self.repop, dtype=bool), f_ray=np.array(self.ray).reshape(-1, 6))


def _drop_observations(L, n_drop, keep_repop=True):
    """the last n_drop plain plane observations whose plane keeps another observation or a prior"""
    seen = {}
    for k, (a, b) in enumerate(L.fn):
        if L.ft[k] in (synth.F_PLANE_OBS, synth.F_PLANE_PRIOR):
            p = b if L.ft[k] == synth.F_PLANE_OBS else a
            seen[p] = seen.get(p, 0) + 1
    out = []
    for k in range(len(L.ft) - 1, -1, -1):
        if len(out) == n_drop:
            break
        if L.ft[k] != synth.F_PLANE_OBS or (keep_repop and L.repop[k]) or seen[L.fn[k][1]] < 2:
            continue
        seen[L.fn[k][1]] -= 1
        out.append(k)
    assert len(out) == n_drop, (len(out), n_drop)
    L.drop(out)


def counted_graph(n_pp, n_odo, n_obs, n_lp, n_repop=0, n_pose=None, n_plane=None, kick=0.02, seed=11, obs_per_pose=OBS_PER_POSE,
                  meas_noise=(0.01, 0.01, 0.01, 0.0035, 0.0035, 0.0035), name=None):
    """A corridor of n_pose poses and n_plane planes with exactly n_pp pose priors, n_odo odometry edges, n_obs plane observations of which
    n_repop are Factor2 edges, and n_lp plane priors.  kick: the standard deviation of the exmap noise every node's initial value is moved
    by (a pair: poses, planes).  n_plane == 0: the pose chain alone."""
    n_pose = N_POSE if n_pose is None else n_pose
    n_plane = N_PLANE if n_plane is None else n_plane
    edge_ray = O.edge_ray                                              # (the same bits as P.edge_ray: test_edge_ray_matches_oracle)
    chain = n_plane == 0
    if n_repop:
        assert n_plane >= 11 and obs_per_pose == 6, "KS.repop_corridor puts priors on walls 1, 4 and 9 and has six observations per pose"
        base = KS.repop_corridor(n_repop, n_poses=n_pose, n_planes=n_plane, seed=seed, edge_ray=edge_ray)
    else:
        base = synth.corridor(n_pose, max(n_plane, 5), obs_per_pose=min(obs_per_pose, max(n_plane, 5)), seed=seed)
    L = _Lists(base)
    poses = [int(i) for i in np.where(base.node_type == synth.NODE_POSE)[0]]
    planes = [int(i) for i in np.where(base.node_type == synth.NODE_PLANE)[0]]
    truth = base.truth
    noise = np.asarray(meas_noise)
    if n_repop:                                                        # repop_corridor's three wall priors: the count starts from the ground's alone
        L.drop([k for k in range(len(L.ft)) if L.ft[k] == synth.F_PLANE_PRIOR and L.fn[k][0] != planes[0]])
    # -- pose priors: pose 0 has one; the others on poses 1, 2, ... in turn
    if n_pp == 0:
        L.drop([k for k in range(len(L.ft)) if L.ft[k] == synth.F_POSE_PRIOR])
    for j in range(1, n_pp):
        p = poses[j % len(poses)]
        m = synth.pose_vector(synth.pose_exmap(truth[p], _rng(seed, 1, j).normal(0.0, 1.0, 6) * noise))
        L.add(synth.F_POSE_PRIOR, p, -1, m, synth._ut_diag([0.5] * 6))
    # -- odometry: the chain has n_pose - 1; fewer: the last ones go (the observations still tie every pose down); more: k -> k + 1 again
    have = L.count(synth.F_ODOMETRY)
    if n_odo < have:
        L.drop([k for k in range(len(L.ft)) if L.ft[k] == synth.F_ODOMETRY][n_odo:])
    for j in range(max(0, n_odo - have)):
        a = j % (len(poses) - 1)
        rel = synth.pose_ominus(truth[poses[a + 1]], truth[poses[a]])
        m = synth.pose_vector(synth.pose_exmap(rel, _rng(seed, 2, j).normal(0.0, 1.0, 6) * noise))
        L.add(synth.F_ODOMETRY, poses[a], poses[a + 1], m, synth._ut_diag([0.5] * 6))
    # -- plane priors: the ground has one; the others on the walls in turn (then round again, the ground included)
    if n_lp == 0 or chain:
        L.drop([k for k in range(len(L.ft)) if L.ft[k] == synth.F_PLANE_PRIOR])
    if not chain:
        ring = planes[1:] + planes[:1]
        for j in range(1, n_lp):
            p = ring[(j - 1) % len(ring)]
            m = synth.plane_exmap(truth[p, :4], _rng(seed, 3, j).normal(0.0, 0.01, 3))
            L.add(synth.F_PLANE_PRIOR, p, -1, m, synth._ut_diag([2.0] * 3))
    # -- plane observations (after the priors: a plane may keep a prior instead of an observation)
    if chain:
        L.drop([k for k in range(len(L.ft)) if L.ft[k] == synth.F_PLANE_OBS])
    else:
        n_fixed = n_obs - n_repop
        have = L.count(synth.F_PLANE_OBS, repop=False)
        if n_fixed < have:
            _drop_observations(L, have - n_fixed)
        walls = [k for k in range(len(base.f_type)) if base.f_type[k] == synth.F_PLANE_OBS and base.f_nodes[k, 1] != planes[0]
                 and not (n_repop and base.f_repop[k])]
        for j in range(max(0, n_fixed - have)):
            k = walls[j % len(walls)]
            a, b = (int(v) for v in base.f_nodes[k])
            m = synth.plane_exmap(synth.plane_transform_to(truth[b, :4], truth[a]), _rng(seed, 4, j).normal(0.0, 0.01, 3))
            L.add(synth.F_PLANE_OBS, a, b, m, base.f_sqrtinf[k, :6])
    # -- every node's initial value leaves the place the builder derived from the measurements
    kp, kl = (kick, kick) if np.isscalar(kick) else kick
    init = base.node_init.copy()
    for i in range(len(base.node_type)):
        if base.node_type[i] == synth.NODE_POSE:
            init[i] = synth.pose_exmap(init[i], _rng(seed, 5, i).normal(0.0, kp, 6))
        else:
            init[i, :4] = synth.plane_exmap(init[i, :4], _rng(seed, 5, i).normal(0.0, kl, 3))
    spec = L.spec(name or f"counted_{n_pp}pp_{n_odo}odo_{n_obs}obs_{n_repop}f2_{n_lp}lp", init)
    if chain:
        spec = _poses_only(spec)
    spec.rays = {k: spec.f_ray[k] for k in range(len(spec.f_type)) if spec.f_repop[k]}      # (what RH.RobustGraph reads)
    c = spec.counts()
    assert (c[synth.F_POSE_PRIOR], c[synth.F_ODOMETRY], c[synth.F_PLANE_OBS], c[synth.F_PLANE_PRIOR]) == (n_pp, n_odo, 0 if chain else n_obs, 0 if chain else n_lp), (c, name)
    assert int(spec.f_repop.sum()) == n_repop
    assert spec.n_poses == n_pose and spec.n_planes == n_plane, (spec.n_poses, spec.n_planes)
    _assert_constrained(spec)
    return spec


def _poses_only(spec):
    """the same spec without its plane nodes (no factor may name one)"""
    keep = np.where(spec.node_type == synth.NODE_POSE)[0]
    new = -np.ones(len(spec.node_type) + 1, dtype=np.int64)             # (index -1 -> -1)
    new[keep] = np.arange(len(keep))
    assert not np.isin(spec.f_type, (synth.F_PLANE_OBS, synth.F_PLANE_PRIOR)).any()
    return KS.RepopSpec(name=spec.name, node_type=spec.node_type[keep], node_init=spec.node_init[keep], f_type=spec.f_type,
                        f_nodes=new[spec.f_nodes].astype(np.int32), f_meas=spec.f_meas, f_sqrtinf=spec.f_sqrtinf, truth=spec.truth[keep],
                        meta=dict(spec.meta, factor_after_node=np.full(len(spec.f_type), len(keep) - 1, dtype=np.int64)),
                        f_repop=spec.f_repop, f_ray=spec.f_ray)


def _assert_constrained(spec):
    """every node is named by a factor, and something holds the gauge: a pose prior, or priors on three planes whose normals span space"""
    named = set(int(v) for v in spec.f_nodes.ravel() if v >= 0)
    assert named == set(range(len(spec.node_type))), sorted(set(range(len(spec.node_type))) - named)
    if not (spec.f_type == synth.F_POSE_PRIOR).any():
        pl = sorted(set(int(spec.f_nodes[k, 0]) for k in np.where(spec.f_type == synth.F_PLANE_PRIOR)[0]))
        assert np.linalg.matrix_rank(spec.truth[pl, :3], tol=1e-6) == 3, "no pose prior and the planes with a prior do not span space"


def type_slots(spec):
    """factor indices per type in the order the device keeps them: {"obs": plain observations, "repop": Factor2 edges, "odo", "pp", "lp"}"""
    t, f2 = spec.f_type, spec.f_repop
    return {"obs": [int(k) for k in np.where((t == synth.F_PLANE_OBS) & ~f2)[0]], "repop": [int(k) for k in np.where((t == synth.F_PLANE_OBS) & f2)[0]],
            "odo": [int(k) for k in np.where(t == synth.F_ODOMETRY)[0]], "pp": [int(k) for k in np.where(t == synth.F_POSE_PRIOR)[0]],
            "lp": [int(k) for k in np.where(t == synth.F_PLANE_PRIOR)[0]]}


SWEEP_ORDER = ("obs", "repop", "odo", "pp", "lp")                         # the grid: observations (Factor2 slots behind the plain ones), odometry, pose priors, plane priors


# ---- cases ------------------------------------------------------------------------------------------------------------------
_BASE = dict(n_pp=1, n_odo=N_POSE - 1, n_obs=N_POSE * OBS_PER_POSE, n_lp=1)


def _repop_shape(n_repop, short):
    """(poses, fixed observations) of a Factor2 case: KS.repop_corridor turns two of every three wall observations (five per pose) into
    edges; the plain observations are cut down to 256 (or 6 short of it: the first edge then sits at slot 250 of block 0)"""
    n_pose = max(-(-(CHI + n_repop) // 6), -(-3 * n_repop // 10) + 2)
    return n_pose, CHI - (6 if short else 0)


def _case_table():
    T = {}

    def case(axis, count, is_case, seed=11, **kw):
        args = dict(_BASE); args.update(kw)
        T[f"{axis}-{count}"] = dict(axis=axis, count=count, args=args, is_case=is_case, seed=seed)

    for n in COUNTS["pp"]:
        case("pp", n, lambda s, n=n: s.counts()[synth.F_POSE_PRIOR] == n, n_pp=n)
    for n in COUNTS["lp"]:
        case("lp", n, lambda s, n=n: s.counts()[synth.F_PLANE_PRIOR] == n, n_lp=n)
    for n in COUNTS["odo"]:
        # odometry 0: every pose carries a prior
        case("odo", n, lambda s, n=n: s.counts()[synth.F_ODOMETRY] == n and (n > 0 or s.counts()[synth.F_POSE_PRIOR] == s.n_poses),
             n_odo=n, n_pp=N_POSE if n == 0 else 1)
    for n in COUNTS["obs"]:
        # the smallest graphs keep five planes: eleven observations cannot hold fourteen
        case("obs", n, lambda s, n=n: s.counts()[synth.F_PLANE_OBS] == n and not s.f_repop.any(), n_obs=n, n_plane=5 if n < 64 else N_PLANE)
    for n in COUNTS["repop"]:
        for short in (False, True):
            n_pose, n_fixed = _repop_shape(n, short)
            case("repop" + ("_short" if short else ""), n,
                 lambda s, n=n, n_fixed=n_fixed: int(s.f_repop.sum()) == n and s.counts()[synth.F_PLANE_OBS] - n == n_fixed and n_fixed % CHI == (CHI - 6 if n_fixed < CHI else 0),
                 n_pose=n_pose, n_plane=16, n_odo=n_pose - 1, n_obs=n_fixed + n, n_repop=n, obs_per_pose=6)
    # nodes: the retraction has one block and one |delta|^2 partial per 256 nodes, poses first
    for total, (n_pose, n_plane, opp) in {255: (241, 14, 3), 256: (242, 14, 3), 257: (243, 14, 3), 512: (412, 100, 2), 513: (413, 100, 2)}.items():
        case("nodes", total, lambda s, total=total: s.n_poses + s.n_planes == total, n_pose=n_pose, n_plane=n_plane, n_odo=n_pose - 1, n_obs=n_pose * opp, obs_per_pose=opp)
    case("nodes", "pose256", lambda s: s.n_poses == CHI and s.n_planes > 0, n_pose=CHI, n_plane=14, n_odo=CHI - 1, n_obs=CHI * 3, obs_per_pose=3)
    case("nodes", "pose250", lambda s: s.n_poses == CHI - 6 and s.n_poses + s.n_planes > CHI, n_pose=CHI - 6, n_plane=14, n_odo=CHI - 7, n_obs=(CHI - 6) * 3, obs_per_pose=3)
    # zero counts
    case("zero", "pp", lambda s: s.counts()[synth.F_POSE_PRIOR] == 0 and s.counts()[synth.F_PLANE_PRIOR] == 4, n_pp=0, n_lp=4)
    case("zero", "lp", lambda s: s.counts()[synth.F_PLANE_PRIOR] == 0, n_lp=0)
    case("zero", "obs", lambda s: s.counts()[synth.F_PLANE_OBS] == 0 and s.n_planes == 0 and s.counts()[synth.F_PLANE_PRIOR] == 0, n_obs=0, n_lp=0, n_plane=0)
    # only Factor2 observations: two of every three wall observations of a corridor are edges, the plain ones and the ground's are gone.
    # Nothing observes the ground then, and a single prior would be met exactly (r = 0) by the first step: every plane gets a prior and
    # the ground two, with different noise
    case("zero", "obs_fixed", lambda s: s.counts()[synth.F_PLANE_OBS] == int(s.f_repop.sum()) == 140 and s.counts()[synth.F_PLANE_PRIOR] == 17,
         n_pose=42, n_plane=16, n_odo=41, n_obs=140, n_repop=140, n_lp=17, obs_per_pose=6)
    return T


CASES = _case_table()
# the graph whose first LM trial at lambda0 is rejected, and the second one too: 256 poses, 30 planes, 3 observations per pose, kicked by 1.0 / 0.1
REJECTED = dict(n_pp=1, n_odo=255, n_obs=768, n_lp=1, n_pose=256, n_plane=30, obs_per_pose=3, kick=(1.0, 0.1))
# per-case seeds for a case whose default seed leaves some factor with too small a residual after the first accepted trial: chosen on the
# CPU, by the condition tests/test_host_sweep_counts.py asserts for every case.  None is needed today: the smallest ratio min r*'r* / bound
# is 2.9e4 at the start (nodes-513) and 16.5 after the first accepted trial (nodes-pose250; then 33 on repop-1 and nodes-255)
SEEDS = {}
_SPECS = {}


def make(name):
    """the graph of a case (built once per process; nothing modifies a spec)"""
    if name not in _SPECS:
        if name == "rejected":
            spec = counted_graph(seed=SEEDS.get(name, 11), name=name, **REJECTED)
        else:
            c = CASES[name]
            spec = counted_graph(seed=SEEDS.get(name, c["seed"]), name=name, **c["args"])
            assert c["is_case"](spec), name
        for a in (spec.node_init, spec.f_meas, spec.f_sqrtinf, spec.f_nodes, spec.f_type):
            a.setflags(write=False)
        _SPECS[name] = spec
    return _SPECS[name]


def varied_type(name):
    """the slot list (type_slots) a case varies, or None"""
    axis = CASES[name]["axis"] if name in CASES else None
    return {"pp": "pp", "lp": "lp", "odo": "odo", "obs": "obs", "repop": "repop", "repop_short": "repop"}.get(axis)


# ---- reference --------------------------------------------------------------------------------------------------------------
class Reference:
    """the oracle and the numpy restatement of one spec.  State: (poses [n_pose, 7], planes [n_plane, 4]) in node order."""

    def __init__(self, spec, cost=None):
        self.spec, self.cost = spec, cost
        self.o = O.OracleGraph()
        self.nid, self.fid = spec.replay(self.o)
        self.np_graph = RH.RobustGraph(spec, *(cost or (RH.NONE, 1.0)))
        self.pose_nodes = [int(i) for i in np.where(spec.node_type == synth.NODE_POSE)[0]]
        self.plane_nodes = [int(i) for i in np.where(spec.node_type == synth.NODE_PLANE)[0]]
        self.start = self.state()

    def state(self):
        o = self.o
        return (np.array([o.get_pose(int(self.nid[i])) for i in self.pose_nodes]).reshape(-1, 7),
                np.array([o.get_plane(int(self.nid[i])) for i in self.plane_nodes]).reshape(-1, 4))

    def set_state(self, poses, planes):
        for j, i in enumerate(self.pose_nodes):
            self.o.set_pose(int(self.nid[i]), poses[j])
        for j, i in enumerate(self.plane_nodes):
            self.o.set_plane(int(self.nid[i]), planes[j])

    def _phi(self, r):
        return r if self.cost is None else RH.phi(self.cost[0], self.cost[1], r)

    def residuals(self):
        """r* of every factor at the oracle's state"""
        return [self._phi(self.o.factor_error(int(f))) for f in self.fid]

    @staticmethod
    def chi2_of(res):
        return math.fsum(float(v) * float(v) for r in res for v in r)

    def numpy_residuals(self):
        """the second CPU statement at the same state"""
        poses, planes = self.state()
        x = [None] * len(self.spec.node_type)
        for j, i in enumerate(self.pose_nodes):
            x[i] = poses[j]
        for j, i in enumerate(self.plane_nodes):
            x[i] = planes[j]
        return [self.np_graph.error(k, x) for k in range(len(self.spec.f_type))]

    def yardstick(self, res=None):
        """(chi2*, d, worst |r*_oracle - r*_numpy|)"""
        res = self.residuals() if res is None else res
        rn = self.numpy_residuals()
        c, cn = self.chi2_of(res), self.chi2_of(rn)
        return c, abs(c - cn) / c, max(float(np.abs(a - b).max()) for a, b in zip(res, rn))

    def jacobian(self, k, analytic=0):
        """(J*, r*) of factor k at the oracle's state.  With a cost function: the central differences of phi(r) through the oracle's exmaps
        (numericalDiff.cpp: eps = 1e-4, (y+ - y-) / (eps + eps)), columns of the first node, then of the second."""
        o, f = self.o, int(self.fid[k])
        if self.cost is None:
            return o.factor_jacobian(f, analytic=analytic)
        assert not analytic
        r0 = self._phi(o.factor_error(f))
        cols = []
        for n in (int(v) for v in self.spec.f_nodes[k] if v >= 0):
            pose = self.spec.node_type[n] == synth.NODE_POSE
            nid = int(self.nid[n])
            x0 = o.get_pose(nid) if pose else o.get_plane(nid)
            for j in range(6 if pose else 3):
                y = []
                for s in (1.0, -1.0):
                    d = np.zeros(6 if pose else 3); d[j] = s * NUM_DIFF_EPS
                    if pose:
                        o.set_pose(nid, O.pose_exmap(x0, d))
                    else:
                        o.set_plane(nid, O.plane_exmap(x0, d))
                    y.append(self._phi(o.factor_error(f)))
                cols.append((y[0] - y[1]) / (NUM_DIFF_EPS + NUM_DIFF_EPS))
            if pose:
                o.set_pose(nid, x0)
            else:
                o.set_plane(nid, x0)
        return np.array(cols).T, r0

    def retracted(self, state, delta, lay):
        """state (+) delta through the oracle's pose_exmap / plane_exmap; lay: node -> (offset in delta, dim)"""
        poses, planes = state
        return (np.array([O.pose_exmap(poses[j], delta[lay[i][0]:lay[i][0] + 6]) for j, i in enumerate(self.pose_nodes)]).reshape(-1, 7),
                np.array([O.plane_exmap(planes[j], delta[lay[i][0]:lay[i][0] + 3]) for j, i in enumerate(self.plane_nodes)]).reshape(-1, 4))

    def sensitivity(self):
        """S = sum over the factors of 2 |r*|' |J*| 1 at the oracle's state: what chi2 can move by per unit of |dx|_inf, to first order"""
        return math.fsum(2.0 * float(np.abs(r) @ np.abs(J).sum(axis=1)) for J, r in (self.jacobian(k) for k in range(len(self.fid))))


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def bound_exact(chi2, d):
    """a chi2 at a state both sides hold bit for bit"""
    return max(16.0 * d, 1e-12) * max(1.0, chi2)


def eta(delta, state):
    """how far the device's x (+) delta may lie from the oracle's retraction by the hook's delta: the two figures of
    test_the_hook_measures_the_shipped_path (the shipped step against the hook's, the retraction against the reference's)"""
    xinf = max([float(np.abs(a).max()) for a in state if a.size] + [0.0])
    return 1e-13 * float(np.abs(delta).max()) + 64.0 * EPS * max(1.0, xinf)


def bound_retracted(chi2, d, S, delta, state):
    """a chi2 at a state the device does not hand out (a rejected trial): bound_exact + the first-order term S eta"""
    return bound_exact(chi2, d) + S * eta(delta, state)


def assert_visible(label, res, bound):
    """the visibility condition; returns min r*'r* / bound"""
    least = min(float(r @ r) for r in res)
    assert least >= 8.0 * bound, (label, "a factor's r'r is too small for the bound to see it", least, bound, least / bound)
    return least / bound


MUTATIONS = ("drop_last", "drop_after_256", "next_twice", "drop_tail", "drop_last_repop")


def mutated_sums(spec, res, which):
    """{mutation: the sum of squares with ONE mistake a sweep could make at the edges of type `which` (a key of type_slots)}: the last
    factor of the type left out, the first one after a multiple of 256 left out, factor 0 of the next type counted twice, the whole tail
    [256 floor(n / 256), n) left out, the last Factor2 edge left out.  A mutation that does not apply at this count is absent."""
    slots = type_slots(spec)
    sq = [float(r @ r) for r in res]
    total = [sq[k] for k in range(len(sq))]
    out = {}

    def without(ks, twice=()):
        ks = set(ks)
        return math.fsum([v for k, v in enumerate(total) if k not in ks] + [total[k] for k in twice])

    mine = slots[which]
    # (the Factor2 slots continue the observations' numbering: their block edges are those of n_obs_fixed + k)
    first = len(slots["obs"]) if which == "repop" else 0
    n = first + len(mine)
    if mine:
        out["drop_last"] = without([mine[-1]])
        edge = CHI * ((n - 1) // CHI)
        if edge >= first and edge > 0:
            out["drop_after_256"] = without([mine[edge - first]])
        tail = mine[max(0, CHI * (n // CHI) - first):] if n % CHI else []
        if tail and len(tail) < len(sq):
            out["drop_tail"] = without(tail)
    later = [t for t in SWEEP_ORDER[SWEEP_ORDER.index(which) + 1:] if slots[t]]      # (an empty type hands its blocks to the next one that has any)
    if later:
        out["next_twice"] = without([], twice=[slots[later[0]][0]])
    if slots["repop"]:
        out["drop_last_repop"] = without([slots["repop"][-1]])
    return out
