"""One edit script, three consumers: what decides which bytes the kernels read.

upload_all / flush_uploads (csrc/pps_upload.cpp) and the frame tables (csrc/pps_frames.cpp) form a state machine of more than ten flags
(grown_only_upload, kept-prefix hints, incr_pack and the pk_* arrays, pk_meas_ok, keep_meas, up_unknown, up_unknown_meas, dev_values_newer,
dev_meas_newer, host_values_newer, meas_dirty).  A script here is a list of API calls with every argument spelled out, a pure function of
its seed: new pose estimates come from the script's own dead-reckoned model and never from a handle, so the same script drives

  * two handles without a device -- incremental analysis against analysis from scratch (tests/test_host_upload_states.py),
  * twin handles on the device, one of them rebuilding everything -- bit for bit -- and the oracle (tests/test_gpu_upload_states.py).

Ops are tuples.  Nodes and factors are named by their creation index in the script; every consumer keeps its own id tables.
  ("pose", tq) ("plane", abcd) ("pp", n, m6, ut21) ("odo", a, b, m6, ut21) ("obs", pose, plane, m4, ut6) ("obs2", pose, plane, m4, ray6, ut6)
  ("lp", plane, m4, ut6) ("rmf", f) ("rmn", n) ("set_pose", n, tq) ("set_plane", n, abcd) ("set_meas", f, m4) ("set_meas_bulk", [f], M)
  ("calib", invK) ("frame", pose, seg2d, [f | -1]) ("refresh",) ("analyze",) ("save",) ("restore",) ("cost", kind, b)
  ("solve", kind, pull, arg)   kind in SOLVE_KINDS; pull: also read every pose and plane back afterwards
  ("cov", [n, n, n])           cov_recover + cov_marginals

Reads that bring device-side data home (get_measurement, the getters) are part of the script and not of every check: a consumer that
read every measurement after every call would take keep_meas and dev_meas_newer out of the states under test."""
import collections

import numpy as np

import pop_up_slam_amd as P
from oracle import oracle_py as O
from pop_up_slam_amd import synth

INVK = np.linalg.inv(synth.K_TUM).astype(np.float32)
DUMMY = np.array([0.0, 0.0, -1.0, 0.5])              # what a registered frame's observations hold until the first refresh
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
POSE_UT = synth._ut_diag([0.5] * 6)
OBS_UT = synth._ut_diag([0.1] * 3)
FRAME_UT = synth._ut_diag([1.0] * 3)

EDIT_KINDS = ("grow", "grow_many", "new_landmark", "drop_obs", "merge", "set_measurement", "loop_closure",      # the seven of test_gpu_fuzz.py
              "set_pose", "set_plane", "set_measurements", "pose_prior", "frame_refresh", "plane_obs2", "remove_newest_pose",
              "analyze_twice", "save_restore")
SOLVE_KINDS = ("update", "batch", "chi2", "eval", "dsolve", "getm")
# The seeds both legs run, chosen on the host so that every seeded script meets the coverage conditions of tests/test_host_upload_states.py
# (seeds divisible by three start from a corridor) and that no LM run of the oracle takes more than 20 iterations (a merge of two unlike
# landmarks can leave a valley so flat that the iteration count of a second implementation is not pinned to +-1); 16-24 steps as in
# test_gpu_fuzz.py.
SEEDS = (0, 12, 15, 24, 4, 5, 7, 8, 10, 13, 14, 17)
STEPS = 18
HUBER_SEED = 7                # this script also switches a Huber cost on and off again (the uploads of the one-step LM loop)


def j_capacity(n):
    """capacity of a Jacobian slab (csrc/pps_upload.cpp): powers of two from 16"""
    c = 16
    while c < n:
        c *= 2
    return c


def unit4(v):
    v = np.asarray(v, dtype=float)
    return v / np.linalg.norm(v)


class Script:
    def __init__(self, name):
        self.name = name
        self.ops = []
        self.log = []                 # (edit kind, applied?) per drawn edit
        self.solves = collections.Counter()
        self.crossed = False          # a plane-observation or odometry slab outgrew its capacity after the start graph

    def skipped(self):
        return sum(1 for _, ok in self.log if not ok)


class _Gen:
    """the script's own model of the graph: dead-reckoned poses, landmark planes, live factors"""

    def __init__(self, rng, name, local=None):
        self.rng = rng
        self.s = Script(name)
        self.local = local            # corridors: edits stay within this many poses of the newest one (long kept prefixes)
        self.poses, self.planes, self.fac = [], [], {}
        self.nn = self.nf = 0
        self.cnt = {"obs": 0, "odo": 0}
        self.started = False
        self.ground = self.L = self.R = None
        self.calibrated = False

    # ---- emission ----
    def op(self, *t):
        self.s.ops.append(t)

    def add_pose(self, value, est=None):
        self.op("pose", np.array(value[:7], dtype=float))
        self.poses.append(dict(node=self.nn, est=np.array(value[:7] if est is None else est[:7], dtype=float), live=True))
        self.nn += 1
        return len(self.poses) - 1

    def add_plane(self, value, val=None, frame=False):
        self.op("plane", np.array(value[:4], dtype=float))
        self.planes.append(dict(node=self.nn, val=unit4(value[:4] if val is None else val[:4]), live=True, frame=frame))
        self.nn += 1
        return len(self.planes) - 1

    def _count(self, t, d):
        before = self.cnt[t]
        self.cnt[t] += d
        if d > 0 and self.started and j_capacity(self.cnt[t]) > j_capacity(before):
            self.s.crossed = True

    def add_factor(self, kind, pose=None, plane=None, meas=None, extra=(), ut=None, other=None, frame=False):
        pn = None if pose is None else self.poses[pose]["node"]
        ln = None if plane is None else self.planes[plane]["node"]
        if kind == "pp": self.op("pp", pn, meas, ut)
        elif kind == "odo": self.op("odo", self.poses[other]["node"], pn, meas, ut)
        elif kind == "obs": self.op("obs", pn, ln, meas, ut)
        elif kind == "obs2": self.op("obs2", pn, ln, meas, extra, ut)
        else: self.op("lp", ln, meas, ut)
        f = self.nf
        self.nf += 1
        self.fac[f] = dict(kind=kind, pose=pose, plane=plane, other=other, meas=None if meas is None else np.array(meas, dtype=float), live=True, frame=frame)
        if kind in ("obs", "obs2"): self._count("obs", 1)
        elif kind == "odo": self._count("odo", 1)
        return f

    def _dead(self, f):
        r = self.fac[f]
        if not r["live"]:
            return
        r["live"] = False
        if r["kind"] in ("obs", "obs2"): self._count("obs", -1)
        elif r["kind"] == "odo": self._count("odo", -1)

    def remove_factor(self, f):
        self.op("rmf", f)
        self._dead(f)

    def remove_node(self, pose=None, plane=None):
        self.op("rmn", self.poses[pose]["node"] if pose is not None else self.planes[plane]["node"])
        for f, r in self.fac.items():
            if pose is not None and (r["pose"] == pose or r["other"] == pose): self._dead(f)
            if plane is not None and r["plane"] == plane: self._dead(f)
        (self.poses[pose] if pose is not None else self.planes[plane])["live"] = False

    # ---- queries on the model ----
    def live_poses(self):
        return [k for k, p in enumerate(self.poses) if p["live"]]

    def live_obs(self, plane=None, pose=None):
        return [f for f, r in self.fac.items() if r["live"] and r["kind"] in ("obs", "obs2") and (plane is None or r["plane"] == plane) and
                (pose is None or r["pose"] == pose)]

    def recent_planes(self, n_poses=3):
        out = []
        for k in self.live_poses()[-n_poses:]:
            for f in self.live_obs(pose=k):
                if self.fac[f]["plane"] not in out:
                    out.append(self.fac[f]["plane"])
        return out

    def model_meas(self, plane, pose, sigma):
        m = synth.plane_transform_to(self.planes[plane]["val"], self.poses[pose]["est"])
        return synth.plane_exmap(m, self.rng.normal(0, sigma, 3))

    # ---- the start graph ----
    def start(self, spec):
        order = spec.meta["factor_after_node"]
        idx = {}
        nf = 0
        for i in range(len(spec.node_type)):
            if spec.node_type[i] == synth.NODE_POSE:
                idx[i] = self.add_pose(spec.node_init[i], spec.truth[i])
            else:
                idx[i] = self.add_plane(spec.node_init[i], spec.truth[i])
                if self.ground is None and np.allclose(unit4(spec.truth[i, :4]), unit4(synth.GROUND)):
                    self.ground = idx[i]
            while nf < len(spec.f_type) and order[nf] <= i:
                t = spec.f_type[nf]
                a, b = (int(x) for x in spec.f_nodes[nf])
                if t == synth.F_POSE_PRIOR: self.add_factor("pp", pose=idx[a], meas=spec.f_meas[nf, :6].copy(), ut=spec.f_sqrtinf[nf, :21].copy())
                elif t == synth.F_ODOMETRY: self.add_factor("odo", pose=idx[b], other=idx[a], meas=spec.f_meas[nf, :6].copy(), ut=spec.f_sqrtinf[nf, :21].copy())
                elif t == synth.F_PLANE_OBS: self.add_factor("obs", pose=idx[a], plane=idx[b], meas=spec.f_meas[nf, :4].copy(), ut=spec.f_sqrtinf[nf, :6].copy())
                else: self.add_factor("lp", plane=idx[a], meas=spec.f_meas[nf, :4].copy(), ut=spec.f_sqrtinf[nf, :6].copy())
                nf += 1
        assert nf == len(spec.f_type) and self.ground is not None
        self.started = True

    # ---- edits: True when applied, False when a precondition is not met (nothing emitted) ----
    def _new_pose(self):
        prev = self.live_poses()[-1]
        odo = synth.pose_exmap(IDENT, self.rng.normal(0, 1, 6) * np.array([0.05, 0.05, 0.1, 0.01, 0.01, 0.01]))
        est = synth.pose_oplus(self.poses[prev]["est"], odo)
        k = self.add_pose(est)
        self.add_factor("odo", pose=k, other=prev, meas=synth.pose_vector(odo), ut=POSE_UT)
        return k

    def grow(self):
        cand = [k for k in (self.recent_planes() if self.local else [j for j, p in enumerate(self.planes) if p["live"]]) if not self.planes[k]["frame"]]
        k = self._new_pose()
        for j in self.rng.choice(cand, size=min(len(cand), int(self.rng.integers(2, 4))), replace=False):
            self.add_factor("obs", pose=k, plane=int(j), meas=self.model_meas(int(j), k, 0.01), ut=OBS_UT)
        return True

    def grow_many(self):
        for _ in range(int(self.rng.integers(2, 5))):
            self.grow()
        return True

    def new_landmark(self):
        lp = self.live_poses()
        if len(lp) < 2:
            return False
        n = self.rng.normal(0, 1, 3); n[2] *= 0.1; n /= np.linalg.norm(n)
        w = unit4([*n, self.rng.uniform(1.0, 4.0)])
        j = self.add_plane(w)
        for k in (lp[-1], lp[-2]):
            self.add_factor("obs", pose=k, plane=j, meas=self.model_meas(j, k, 0.01), ut=OBS_UT)
        return True

    def _plane_pool(self):
        pool = self.recent_planes(10) if self.local else [j for j, p in enumerate(self.planes) if p["live"]]
        return [j for j in pool if j != self.ground and not self.planes[j]["frame"]]

    def drop_obs(self):
        cand = [fs[1] for fs in (self.live_obs(plane=j) for j in self._plane_pool() + [self.ground]) if len(fs) >= 4]
        if not cand:
            return False
        self.remove_factor(cand[int(self.rng.integers(0, len(cand)))])
        return True

    def merge(self):
        pool = [j for j in self._plane_pool() if all(self.fac[f]["kind"] == "obs" for f in self.live_obs(plane=j))]
        if len(pool) < 3:
            return False
        A, B = (int(x) for x in self.rng.choice(pool, size=2, replace=False))
        seen = {self.fac[f]["pose"] for f in self.live_obs(plane=A)}
        for f in self.live_obs(plane=B):
            r = self.fac[f]
            self.remove_factor(f)
            if r["pose"] not in seen:
                seen.add(r["pose"])
                self.add_factor("obs", pose=r["pose"], plane=A, meas=r["meas"], ut=OBS_UT)
        self.remove_node(plane=B)
        return True

    def _some_obs(self, n):
        fs = self.live_obs()
        if self.local:
            recent = set(self.live_poses()[-self.local:])
            fs = [f for f in fs if self.fac[f]["pose"] in recent]
        if not fs:
            return []
        return [int(f) for f in self.rng.choice(fs, size=min(n, len(fs)), replace=False)]

    def _new_meas(self, f):
        r = self.fac[f]
        r["meas"] = self.model_meas(r["plane"], r["pose"], 0.02)
        return r["meas"]

    def set_measurement(self):
        fs = self._some_obs(1)
        if not fs:
            return False
        self.op("set_meas", fs[0], self._new_meas(fs[0]))
        return True

    def set_measurements(self):
        fs = self._some_obs(int(self.rng.integers(3, 7)))
        if len(fs) < 2:
            return False
        self.op("set_meas_bulk", fs, np.array([self._new_meas(f) for f in fs]))
        return True

    def _old_pose(self):
        lp = self.live_poses()
        lo = max(0, len(lp) - self.local) if self.local else 0
        return lp[int(self.rng.integers(lo, len(lp) - 3))] if len(lp) - 3 > lo else None

    def loop_closure(self):
        lp = self.live_poses()
        old = self._old_pose()
        if len(lp) < 6 or old is None:
            return False
        new = lp[-1]
        rel = synth.pose_ominus(self.poses[new]["est"], self.poses[old]["est"])
        self.add_factor("odo", pose=new, other=old, meas=synth.pose_vector(rel), ut=POSE_UT)
        return True

    def set_pose(self):
        old = self._old_pose()
        if old is None:
            return False
        d = self.rng.normal(0, 1, 6) * np.array([0.01, 0.01, 0.01, 0.002, 0.002, 0.002])
        self.op("set_pose", self.poses[old]["node"], synth.pose_exmap(self.poses[old]["est"], d))
        return True

    def set_plane(self):
        pool = self._plane_pool()
        if not pool:
            return False
        j = pool[int(self.rng.integers(0, len(pool)))]
        self.op("set_plane", self.planes[j]["node"], synth.plane_exmap(self.planes[j]["val"], self.rng.normal(0, 0.005, 3)))
        return True

    def pose_prior(self):
        old = self._old_pose()
        if old is None:
            return False
        self.add_factor("pp", pose=old, meas=synth.pose_vector(self.poses[old]["est"]), ut=POSE_UT)
        return True

    def _frame_view(self, k):
        """the ground segments a camera at pose k sees of a corridor section, and the planes they pop up to (sensor frame, unit)"""
        est = self.poses[k]["est"]
        seg, _polys, _T = synth.corridor_frame(est)
        pl = O.popup_planes(seg, INVK, synth.T_from_pose(est).astype(np.float32)).astype(np.float64)
        pl /= np.linalg.norm(pl, axis=1, keepdims=True)
        if self.L is None:
            self.L = self.add_plane(synth.plane_transform_from(pl[1], est), frame=True)
            self.R = self.add_plane(synth.plane_transform_from(pl[3], est), frame=True)
        return seg, pl

    def frame_refresh(self, n_obs=3, refresh=True):
        """a new pose whose observations are registered as a frame: dummies until the refresh re-derives them on the device"""
        if not self.calibrated:
            self.op("calib", INVK.copy())
            self.calibrated = True
        k = self._new_pose()
        seg, _pl = self._frame_view(k)
        fids = [-1, -1, -1, -1]                                    # ground | left | front (never observed: it moves with the camera) | right
        for slot, plane in ((0, self.ground), (1, self.L), (3, self.R))[:n_obs]:
            fids[slot] = self.add_factor("obs", pose=k, plane=plane, meas=DUMMY.copy(), ut=FRAME_UT, frame=True)
        self.op("frame", self.poses[k]["node"], seg.copy(), fids)
        if refresh:
            self.op("refresh")
        return True

    def plane_obs2(self):
        """a new pose that sees the ground, the right wall, and the left wall through a re-popping edge (Pose3d_Plane3d_Factor2)"""
        k = self._new_pose()
        seg, pl = self._frame_view(k)
        self.add_factor("obs", pose=k, plane=self.ground, meas=self.model_meas(self.ground, k, 0.01), ut=OBS_UT)
        self.add_factor("obs", pose=k, plane=self.R, meas=pl[3].copy(), ut=FRAME_UT)
        self.add_factor("obs2", pose=k, plane=self.L, meas=pl[1].copy(), extra=np.array(P.edge_ray(INVK, seg[0]), dtype=float), ut=FRAME_UT)
        return True

    def remove_newest_pose(self):
        lp = self.live_poses()
        if len(lp) < 4:
            return False
        k = lp[-1]
        for f in self.live_obs(pose=k):
            if len(self.live_obs(plane=self.fac[f]["plane"])) < 3:      # every landmark keeps two observations
                return False
        self.remove_node(pose=k)
        return True

    def analyze_twice(self):
        self.op("analyze"); self.op("analyze")
        return True

    def save_restore(self):
        self.op("save")
        self.solve("batch" if self.rng.random() < 0.5 else "update", pull=False)
        self.op("restore")
        return True

    # ---- solves and reads ----
    def solve(self, kind, pull=None, arg=None):
        if pull is None:
            pull = bool(self.rng.random() < 0.5)
        if kind == "eval" and arg is None:
            fs = [f for f, r in self.fac.items() if r["live"]]
            arg = int(fs[int(self.rng.integers(0, len(fs)))])
        if kind == "dsolve" and arg is None:
            arg = float(10.0 ** self.rng.integers(-4, 1))
        self.op("solve", kind, bool(pull), arg)
        self.s.solves[kind] += 1

    def cov(self):
        lp = self.live_poses()
        nodes = [self.poses[lp[-1]]["node"], self.poses[lp[len(lp) // 2]]["node"], self.planes[self.ground]["node"]]
        self.op("cov", nodes)

    def edit(self, kind):
        ok = getattr(self, kind)()
        self.s.log.append((kind, bool(ok)))
        return ok


def _start_spec(rng, corridor):
    """a start graph one of whose slabs (plane observations, odometry) outgrows its capacity within a few new frames"""
    while True:
        if corridor:
            n = int(rng.integers(120, 301)); per = 5
            spec_args = (n, max(12, n // 5))
        else:
            n = int(rng.integers(6, 31)); walls = int(rng.integers(3, 9)); opp = int(rng.integers(2, 5))
            per = 2 + min(walls - 2, max(0, opp - 2))            # ground, the wall every pose must see, opp - 2 of the other walls - 2
            spec_args = (n, walls, opp)
        n_obs, n_odo = n * per, n - 1
        room = min((j_capacity(n_obs) - n_obs) // 3, j_capacity(n_odo) - n_odo)
        if room <= 3:
            return spec_args


def make_script(seed, steps=18, huber=False):
    """the seeded script: a start graph (a corridor of 120-300 poses for seed % 3 == 0, else a small world of 6-30), then `steps` drawn edits,
    each followed by a solve and now and then another read"""
    rng = np.random.default_rng(7000 + seed)
    corridor = seed % 3 == 0
    g = _Gen(rng, f"seed{seed}", local=40 if corridor else None)
    args = _start_spec(rng, corridor)
    if corridor:
        spec = synth.corridor(args[0], args[1], seed=300 + seed)
    else:
        spec = synth.small_world(args[0], args[1], seed=100 + seed, obs_per_pose=args[2])
    g.start(spec)
    g.solve("batch", pull=True)
    cov_at = int(rng.integers(2, steps))
    huber_at = int(rng.integers(2, steps))                # (drawn either way: the flag changes nothing else of the script)
    if not huber:
        huber_at = -1
    for step in range(steps):
        # until a slab has outgrown its capacity, every other edit appends (the kept-prefix path with moved offsets needs pure growth)
        if not g.s.crossed and step % 2 == 0:
            kind = ("grow", "grow_many", "frame_refresh")[int(rng.integers(0, 3))]
        else:
            kind = EDIT_KINDS[int(rng.integers(0, len(EDIT_KINDS)))]
        g.edit(kind)
        r = rng.random()
        g.solve("chi2" if r < 0.2 else ("batch" if step % 3 == 0 else "update"))
        if rng.random() < 0.5:
            g.solve(("chi2", "eval", "dsolve", "getm")[int(rng.integers(0, 4))])
        if step == cov_at:
            g.cov()
        if step == huber_at:
            g.op("cost", P.COST_HUBER, 1.0)
            g.solve("batch", pull=False); g.solve("update", pull=False)
            g.op("cost", P.COST_NONE, 1.0)
            g.solve("update", pull=True)
    g.solve("getm", pull=True)
    return g.s


# ---- directed scripts: one per upload path ----
def _directed_base(name, n_frames, last_obs=3, rng_seed=1):
    """a small world, solved, then n_frames registered frames (the last one with last_obs observations), refreshed and solved"""
    g = _Gen(np.random.default_rng(rng_seed), name)
    g.start(synth.small_world(6, 4, seed=41, obs_per_pose=3))
    g.solve("batch", pull=False)
    for k in range(n_frames):
        g.frame_refresh(n_obs=last_obs if k == n_frames - 1 else 3, refresh=False)
    g.op("refresh")                                                     # (no LM solve ever sees the dummies)
    g.solve("update", pull=False)
    return g


def directed_scripts():
    out = []
    # 1. refresh, an append-only frame, chi2: keep_meas leaves the refreshed rows on the device and sends the new rows as exact pieces
    g = _directed_base("keep_meas", 3)
    g.op("refresh"); g.frame_refresh(refresh=False); g.solve("chi2", pull=False); g.solve("getm", pull=True)
    out.append(g.s)
    # 2. refresh, remove a factor, chi2: the measurements come home before the slots move
    g = _directed_base("refresh_remove", 3)
    g.op("refresh"); g.remove_factor(g.live_obs(plane=g.ground)[1]); g.solve("chi2", pull=False); g.solve("getm", pull=True)
    out.append(g.s)
    # 3. refresh, a re-popping edge, solve: keep_meas is off, the re-popping slots sit behind the fixed ones and move with the next fixed one
    g = _directed_base("refresh_obs2", 3)
    g.op("refresh"); g.plane_obs2(); g.solve("update", pull=False); g.solve("getm", pull=False)
    g.op("refresh"); g.frame_refresh(refresh=False); g.solve("chi2", pull=False); g.solve("getm", pull=True)
    out.append(g.s)
    # 4. set_measurement between a refresh and the next upload: the host is newer for one row, the device for all others
    g = _directed_base("set_after_refresh", 3)
    g.op("refresh")
    f = g.live_obs(plane=g.L)[0]
    g.op("set_meas", f, g._new_meas(f))
    g.frame_refresh(refresh=False); g.solve("chi2", pull=False); g.solve("getm", pull=True)
    out.append(g.s)
    # 5. set_pose while the device holds the newer estimate
    g = _directed_base("set_pose_device_newer", 2)
    g.solve("batch", pull=False); g.set_pose(); g.solve("chi2", pull=False); g.solve("update", pull=True)
    out.append(g.s)
    # 6. removal directly after growth: grown_only_upload falls, the kept-prefix hints must be dropped
    g = _directed_base("remove_after_growth", 2)
    g.grow(); g.solve("update", pull=False); g.grow(); g.remove_factor(g.live_obs(plane=g.ground)[2]); g.solve("update", pull=False)
    g.grow(); g.solve("batch", pull=True)
    out.append(g.s)
    # 7. refreshed rows present while the plane observations cross 16 -> 32 -- and, one frame earlier, fill the capacity of 16 exactly with an
    # odd number of new rows: a new-row piece rounded up to the 16-byte copy unit would reach into the next row's first (refreshed) entry
    # (the registered observations take the first slots: the entry behind a row's end is a refreshed one)
    g = _Gen(np.random.default_rng(7), "capacity_16_32")
    p0 = synth.pose_from_Rt(synth.CAM_R0, np.array([0.0, 0.0, 1.0]))
    k0 = g.add_pose(p0)
    g.add_factor("pp", pose=k0, meas=synth.pose_vector(p0), ut=POSE_UT)
    g.ground = g.add_plane(synth.GROUND)
    g.add_factor("lp", plane=g.ground, meas=np.array(synth.GROUND, dtype=float), ut=synth._ut_diag([20.0] * 3))
    g.started = True
    for n_obs in (3, 3, 3, 3, 1):
        g.frame_refresh(n_obs=n_obs, refresh=False)                     # 13 plane observations
    g.op("refresh")
    g.solve("batch", pull=False)
    assert g.cnt["obs"] == 13, g.cnt
    g.op("refresh"); g.frame_refresh(refresh=False)                     # 16 = capacity: three new rows behind thirteen kept ones
    g.solve("chi2", pull=False); g.solve("getm", pull=False)
    g.op("refresh"); g.frame_refresh(refresh=False)                     # 19: the slab outgrows its capacity
    g.solve("chi2", pull=False); g.solve("getm", pull=True)
    assert g.cnt["obs"] == 19 and g.s.crossed
    out.append(g.s)
    # 8. an unchanged graph solved twice
    g = _directed_base("unchanged_twice", 2)
    g.solve("batch", pull=False); g.solve("batch", pull=True)
    out.append(g.s)
    # 9. the first re-popping edge of a graph that has only grown: obs_ray is uploaded for the first time and every array behind it lands one
    # slot further on -- in the slot of another array, about whose previous content the kept-prefix and packed-row hints say nothing (found by
    # these tests: odo_a kept the leading entries of odo_b, the index arrays those of their neighbours)
    g = _Gen(np.random.default_rng(9), "first_repop_edge")
    g.start(synth.small_world(6, 4, seed=41, obs_per_pose=3))
    g.solve("batch", pull=False)
    g.grow(); g.solve("update", pull=False)
    g.plane_obs2(); g.solve("update", pull=False); g.solve("getm", pull=True)
    g.grow(); g.solve("batch", pull=True)
    out.append(g.s)
    return out


# ---- consumers ----
def apply_edit(g, op, nid, fid):
    """a construction op on any backend (P.Graph, the oracle); False: not a construction op"""
    k = op[0]
    if k == "pose": nid.append(int(g.add_pose(op[1])))
    elif k == "plane": nid.append(int(g.add_plane(op[1])))
    elif k == "pp": fid.append(int(g.add_pose_prior(nid[op[1]], op[2], op[3])))
    elif k == "odo": fid.append(int(g.add_odometry(nid[op[1]], nid[op[2]], op[3], op[4])))
    elif k == "obs": fid.append(int(g.add_plane_obs(nid[op[1]], nid[op[2]], op[3], op[4])))
    elif k == "obs2": fid.append(int(g.add_plane_obs2(nid[op[1]], nid[op[2]], op[3], op[4], op[5])))
    elif k == "lp": fid.append(int(g.add_plane_prior(nid[op[1]], op[2], op[3])))
    elif k == "rmf": g.remove_factor(fid[op[1]])
    elif k == "rmn": g.remove_node(nid[op[1]])
    elif k == "set_pose": g.set_pose(nid[op[1]], op[2])
    elif k == "set_plane": g.set_plane(nid[op[1]], op[2])
    elif k == "set_meas": g.set_measurement(fid[op[1]], op[2])
    elif k == "set_meas_bulk":
        if hasattr(g, "set_measurements"): g.set_measurements([fid[f] for f in op[1]], op[2])
        else:
            for f, m in zip(op[1], op[2]): g.set_measurement(fid[f], m)
    elif k == "calib":
        if hasattr(g, "frames_set_calibration"): g.frames_set_calibration(op[1])
    elif k == "frame":
        if hasattr(g, "frames_add"): g.frames_add(nid[op[1]], op[2], [fid[f] if f >= 0 else -1 for f in op[3]])
    else:
        return False
    return True


class Ledger:
    """what a consumer must know of the script's graph: live nodes and factors, frames, and the expected measurement of every plane
    observation -- last writer wins: a set value is what was set (normalised); a refreshed value is oracle_py.popup_planes at the float32
    cast of the pose the handle reports, normalised; a ray that misses the ground keeps the old value"""

    def __init__(self):
        self.node_kind, self.node_live = [], []
        self.f_kind, self.f_nodes, self.f_live = [], [], []
        self.expect = {}
        self.frames = []              # (pose node, seg2d, [f | -1])

    def note(self, op):
        k = op[0]
        if k in ("pose", "plane"): self.node_kind.append(k); self.node_live.append(True)
        elif k in ("pp", "odo", "obs", "obs2", "lp"):
            self.f_kind.append(k); self.f_live.append(True)
            self.f_nodes.append(tuple(op[1:3]) if k in ("odo", "obs", "obs2") else (op[1],))
            if k in ("obs", "obs2"): self.expect[len(self.f_kind) - 1] = unit4(op[3])
        elif k == "rmf": self.f_live[op[1]] = False
        elif k == "rmn":
            self.node_live[op[1]] = False
            for f, ns in enumerate(self.f_nodes):
                if op[1] in ns: self.f_live[f] = False
        elif k == "set_meas": self.expect[op[1]] = unit4(op[2])
        elif k == "set_meas_bulk":
            for f, m in zip(op[1], op[2]): self.expect[f] = unit4(m)
        elif k == "frame": self.frames.append((op[1], op[2], list(op[3])))

    def live_nodes(self, kind):
        return [n for n, (k, ok) in enumerate(zip(self.node_kind, self.node_live)) if ok and k == kind]

    def live_factors(self, kinds=None):
        return [f for f, (k, ok) in enumerate(zip(self.f_kind, self.f_live)) if ok and (kinds is None or k in kinds)]

    def refresh(self, get_pose):
        """every registered item whose factor and pose are live and whose edge does not re-pop; returns the factors it rewrote"""
        done = []
        for pose, seg, fids in self.frames:
            if not self.node_live[pose]:
                continue
            T32 = synth.T_from_pose(get_pose(pose)).astype(np.float32)
            ref = O.popup_planes(seg, INVK, T32).astype(np.float64)
            for j, f in enumerate(fids):
                if f < 0 or not self.f_live[f] or self.f_kind[f] != "obs":
                    continue
                nrm = np.linalg.norm(ref[j])
                if not np.isfinite(nrm) or nrm == 0:
                    continue
                self.expect[f] = ref[j] / nrm
                done.append(f)
        return done


# ---- the device consumer: twin handles and the oracle ----
def twin_handles(setenv, delenv):
    """I (default switches) and S (every analysis from scratch, compacted tables rebuilt: no analysis cache, no append-only compaction and
    with them no kept-prefix hints), both verifying their uploads.  S is no rebuild of everything: upload_all's incremental packing (pk_*,
    pk_meas_ok), keep_meas and the cached frame slot tables run in S exactly as in I.  Those shortcuts are pinned by the verification switch
    (the packed arrays and the frame tables rebuilt from the host records) and by the expected measurements, not by the twin.
    The switches are read once, when a handle is created: they are set around the creation only."""
    setenv("PPS_DEBUG_VERIFY_UPLOAD", "1")
    gi = P.Graph()
    setenv("PPS_NO_INCREMENTAL", "1"); setenv("PPS_NO_INCR_COMPACT", "1")
    gs = P.Graph()
    for k in ("PPS_NO_INCREMENTAL", "PPS_NO_INCR_COMPACT", "PPS_DEBUG_VERIFY_UPLOAD"):
        delenv(k)
    return gi, gs


def _bits(x):
    return np.ascontiguousarray(x).tobytes()


class TwinRun:
    """A script on I, S and the oracle.  After every solve or read: I against S bit for bit (both run the same kernels on arrays that must be
    equal, so any difference is a finding), I against the expected measurements to 1e-15, I against the oracle at the tolerances of
    test_gpu_fuzz.py (chi2 1e-7 relative, poses 1e-6, LM iterations +-1; no oracle while a robust cost is set: it has none)."""

    def __init__(self, script, gi, gs, oracle=True):
        self.script, self.I, self.S = script, gi, gs
        self.o = O.OracleGraph() if oracle else None
        self.idI, self.idS, self.ido = ([], []), ([], []), ([], [])
        self.led = Ledger()
        self.robust = False
        self.snap = None
        self.where = script.name
        self.n_checks = 0
        self.n_cov_blocks = 0         # marginal covariance blocks compared between the twins
        self.cov_form = None

    def same(self, a, b, what):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and _bits(a) == _bits(b), f"{self.where}: {what} differs between the twins: {a} / {b}"

    def run(self):
        for k, op in enumerate(self.script.ops):
            self.where = f"{self.script.name} op {k} {op[0]}"
            H_I = apply_edit(self.I, op, *self.idI); apply_edit(self.S, op, *self.idS)
            if self.o is not None:
                apply_edit(self.o, op, *self.ido)
            self.led.note(op)
            if not H_I:
                getattr(self, "op_" + op[0])(*op[1:])
        assert self.idI == self.idS
        return self

    # ---- ops that are not construction ----
    def op_refresh(self):
        self.I.refresh_measurements(); self.S.refresh_measurements()
        def pose_of(n):
            a, b = self.I.get_pose(self.idI[0][n]), self.S.get_pose(self.idS[0][n])
            self.same(a, b, f"pose {n} at the refresh")
            return a
        for f in self.led.refresh(pose_of):
            if self.o is not None:
                self.o.set_measurement(self.ido[1][f], self.led.expect[f])

    def op_analyze(self):
        self.I.analyze(); self.S.analyze()
        self.dumps()

    def op_save(self):
        self.I.save_state(); self.S.save_state()
        if self.o is not None:
            self.snap = [(n, k, (self.o.get_pose if k == "pose" else self.o.get_plane)(self.ido[0][n]))
                         for n, (k, ok) in enumerate(zip(self.led.node_kind, self.led.node_live)) if ok]

    def op_restore(self):
        self.I.restore_state(); self.S.restore_state()
        if self.o is not None:
            for n, k, v in self.snap:
                (self.o.set_pose if k == "pose" else self.o.set_plane)(self.ido[0][n], v)

    def op_cost(self, kind, b):
        self.I.set_cost_function(kind, b); self.S.set_cost_function(kind, b)
        self.robust = kind != P.COST_NONE
        if not self.robust and self.o is not None:          # the oracle did not follow the robust solves: it takes I's estimate from here on
            for kd, setter, getI, getS in (("pose", self.o.set_pose, self.I.get_pose, self.S.get_pose), ("plane", self.o.set_plane, self.I.get_plane, self.S.get_plane)):
                for n in self.led.live_nodes(kd):
                    v = getI(self.idI[0][n])
                    self.same(v, getS(self.idS[0][n]), f"{kd} {n} after the robust solves")
                    setter(self.ido[0][n], v)

    def op_cov(self, nodes):
        """cov_recover and three marginal blocks on both twins.  One refusal is taken, by its text and from both twins alike: cov_recover is
        limited to graphs whose fronts fit the wave-per-front kernels, and a graph with loop closures then goes through cov_select, which
        takes both forms.  Every other error -- an upload verification above all, which carries the same code -- fails the run."""
        res = []
        for g, ids in ((self.I, self.idI), (self.S, self.idS)):
            try:
                g.cov_recover()
                form = "recover"
            except P.PpsError as e:
                if e.code != P.PPS_ESTATE or "covariance recovery is limited to graphs whose fronts all fit" not in str(e):
                    raise
                g.cov_select()
                form = "select"
            res.append((form, g.cov_marginals([ids[0][n] for n in nodes])))
        assert res[0][0] == res[1][0], (self.where, res[0][0], res[1][0])
        assert len(res[0][1]) == len(res[1][1]) == len(nodes) == 3
        for n, a, b in zip(nodes, res[0][1], res[1][1]):
            assert a.shape in ((6, 6), (3, 3)) and np.all(np.isfinite(a)) and np.all(np.diag(a) > 0), (self.where, n, a)
            self.same(a, b, f"marginal covariance of node {n}")
            self.n_cov_blocks += 1
        self.cov_form = res[0][0]

    def dumps(self):
        a, b = self.I.analysis_dump(), self.S.analysis_dump()
        assert a.keys() == b.keys()
        for key in b:
            np.testing.assert_array_equal(np.atleast_1d(a[key]), np.atleast_1d(b[key]), err_msg=f"{self.where}: analysis_dump {key}")

    def op_solve(self, kind, pull, arg):
        I, S, o = self.I, self.S, (None if self.robust else self.o)
        if kind == "update":
            I.update(); S.update()
            if o is not None: o.update()
        elif kind == "batch":
            it, its = I.batch_optimize(), S.batch_optimize()
            assert it == its, (self.where, it, its)
            if o is not None:
                ito = o.batch_optimize()
                assert abs(it - ito) <= 1, (self.where, it, ito)
        elif kind == "eval":
            (J, r), (Js, rs) = I.eval_factor(self.idI[1][arg]), S.eval_factor(self.idS[1][arg])
            self.same(J, Js, f"eval_factor J of factor {arg}"); self.same(r, rs, f"eval_factor r of factor {arg}")
        elif kind == "dsolve":
            (d, _d2, form, bad), (ds, _d2s, forms, bads) = I.debug_solve(arg), S.debug_solve(arg)
            self.same(d, ds, f"debug_solve({arg}) delta"); assert (form, bad) == (forms, bads), (self.where, form, bad, forms, bads)
        elif kind == "getm":
            for f in self.led.live_factors(("obs", "obs2")):
                m, ms = I.get_measurement(self.idI[1][f]), S.get_measurement(self.idS[1][f])
                self.same(m, ms, f"measurement of factor {f}")
                np.testing.assert_allclose(m, self.led.expect[f], rtol=0, atol=1e-15, err_msg=f"{self.where}: measurement of factor {f}")
        else:
            assert kind == "chi2", kind
        # chi2() is called before the dumps are taken: analysis_dump() of a changed graph analyses it, and pps_analyze brings the estimate and
        # the measurements home first -- ahead of a chi2 step's upload that would take keep_meas out of every "edit, then chi2" sequence.
        # The dumps are still compared first.
        c, cs = I.chi2(), S.chi2()
        self.dumps()
        self.same(c, cs, "chi2")
        self.same(np.array(I.trace(), dtype=float).reshape(-1, 3), np.array(S.trace(), dtype=float).reshape(-1, 3), "the LM trace")
        st, sts = I.stats(), S.stats()
        for key in ("lm_iterations", "chi2_final", "last_delta_norm"):
            self.same(st[key], sts[key], f"stats {key}")
        if o is not None:
            co = o.chi2()
            assert abs(c - co) <= 1e-7 * max(co, 1e-9), (self.where, c, co)
        if pull:
            poses, planes = self.led.live_nodes("pose"), self.led.live_nodes("plane")
            vp = I.get_poses([self.idI[0][n] for n in poses]); vl = I.get_planes([self.idI[0][n] for n in planes])
            self.same(vp, S.get_poses([self.idS[0][n] for n in poses]), "the poses")
            self.same(vl, S.get_planes([self.idS[0][n] for n in planes]), "the planes")
            if o is not None:
                for n, v in list(zip(poses, vp))[-3:]:
                    np.testing.assert_allclose(v, o.get_pose(self.ido[0][n]), rtol=0, atol=1e-6, err_msg=f"{self.where}: pose {n} against the oracle")
        self.n_checks += 1


def run_all(setenv, delenv, names=None, oracle=True):
    """every seeded and every directed script (or those named) on fresh twins; returns {script name: [checks, covariance blocks compared]}"""
    scripts = [make_script(seed, STEPS, huber=seed == HUBER_SEED) for seed in SEEDS] + directed_scripts()
    out = {}
    for s in scripts:
        if names is not None and s.name not in names:
            continue
        gi, gs = twin_handles(setenv, delenv)
        run = TwinRun(s, gi, gs, oracle=oracle).run()
        out[s.name] = [run.n_checks, run.n_cov_blocks]
        gi.close(); gs.close()
    return out
