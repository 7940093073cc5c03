"""Shared by tests/test_host_linsolve.py and tests/test_gpu_linear_solve.py: the CPU side of the linear-solve tests.  Nothing in here is
code under test: graphs, shape contracts and a dense reference.

  loop_graph / CASES / front_shapes / assert_case_shapes
                       the pose-chain graphs of the tests (loop closures, optional planes) and, per graph, the front shapes it
                       exists for -- asserted from pps_analysis_dump alone, so that a change of the ordering cannot empty a test
  assemble_normal_equations
                       H = sum J'J and b = -sum J'r in numpy float64 from pps_eval_factor of every factor, indexed by node_voff
  damped               H + lambda diag(H)                                    (Cholesky.cpp:94-97)
  reference_solves     x1 = np.linalg.solve (LU), x2 = scipy cho_solve (Cholesky): two solves that share no code path;
                       d = |x1 - x2| / |x1| is the yardstick of every comparison
  check_step           e = |delta - x1| / |x1| <= max(16 d, 1e-12), whole vector and per node block

Sign of delta (stated here once): the solver's step is the one the retraction applies, x <- x (+) delta, so it solves
(H + lambda diag H) delta = -J'r with r the whitened residual pps_eval_factor returns (tests/test_host_analysis.py::_dense_and_jbuf).
"""
import numpy as np

from cov_helpers import node_layout
from pop_up_slam_amd import synth

LAMBDAS = (0.0, 1e-3, 10.0)


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def _curve_pose(k):
    """pose k of a gentle 3-D curve with unit spacing: a wide arc that climbs, with yaw along the arc and some pitch and roll"""
    R = 25.0
    a = k / R
    t = np.array([R * np.sin(a), R * (1.0 - np.cos(a)), 0.15 * k])
    rot = np.array([0.10 * np.sin(0.31 * k), 0.08 * np.cos(0.23 * k), a])
    return synth.pose_exmap(np.concatenate([t, [0, 0, 0, 1.0]]), np.concatenate([np.zeros(3), rot]))


def loop_graph(n_poses, loops, n_planes=0, seen=0, seed=1, prior=True):
    """A pose chain with a prior on pose 0, odometry between neighbours, `loops` random loop-closing odometry edges between poses at
    least 2 apart and `n_planes` planes, each seen from `seen` random poses.  Measurements are the true relative poses / planes plus
    small noise, the initial values are the truth plus a larger perturbation (b != 0), and the sqrt-information differs between
    translation and rotation.  Nodes: the poses, then the planes; every factor after the nodes."""
    rng = np.random.default_rng(seed)
    pairs = []
    while len(pairs) < loops:
        i, j = (int(v) for v in rng.integers(0, n_poses, 2))
        if abs(i - j) >= 2:
            pairs.append((min(i, j), max(i, j)))
    views = [sorted(int(v) for v in rng.choice(n_poses, seen, replace=False)) for _ in range(n_planes)]
    truth = [_curve_pose(k) for k in range(n_poses)]
    planes = []
    for _ in range(n_planes):
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        pl = np.concatenate([n, [rng.uniform(2.0, 9.0)]])
        planes.append(pl / np.linalg.norm(pl))
    nt, ni, ft, fn, fm, fs = [], [], [], [], [], []

    def factor(t, a, b, meas, sq):
        m = np.zeros(6); m[:len(meas)] = meas
        s = np.zeros(21); s[:len(sq)] = sq
        ft.append(t); fn.append((a, b)); fm.append(m); fs.append(s)

    def rel(i, j):
        d = synth.pose_exmap(synth.pose_ominus(truth[j], truth[i]), rng.normal(0.0, 1.0, 6) * np.array([.01, .01, .01, .003, .003, .003]))
        return synth.pose_vector(d)

    for k in range(n_poses):
        nt.append(synth.NODE_POSE)
        ni.append(synth.pose_exmap(truth[k], rng.normal(0.0, 1.0, 6) * np.array([.03, .03, .03, .01, .01, .01])))
    for pl in planes:
        nt.append(synth.NODE_PLANE)
        v = np.zeros(7); v[:4] = synth.plane_exmap(pl, rng.normal(0.0, 0.01, 3)); ni.append(v)
    if prior:
        factor(synth.F_POSE_PRIOR, 0, -1, synth.pose_vector(truth[0]), synth._ut_diag([10.0, 10.0, 10.0, 40.0, 40.0, 40.0]))
    for k in range(n_poses - 1):
        factor(synth.F_ODOMETRY, k, k + 1, rel(k, k + 1), synth._ut_diag([4.0, 4.0, 4.0, 20.0, 20.0, 20.0]))
    for i, j in pairs:
        factor(synth.F_ODOMETRY, i, j, rel(i, j), synth._ut_diag([1.5, 1.5, 1.5, 8.0, 8.0, 8.0]))
    for q, vs in enumerate(views):
        for k in vs:
            m = synth.plane_exmap(synth.plane_transform_to(planes[q], truth[k]), rng.normal(0.0, 0.005, 3))
            factor(synth.F_PLANE_OBS, k, n_poses + q, m, synth._ut_diag([6.0, 9.0, 12.0]))
    return synth.GraphSpec(name=f"loops_{n_poses}p_{loops}l_{n_planes}x{seen}", node_type=np.array(nt, dtype=np.int32), node_init=np.array(ni),
                           f_type=np.array(ft, dtype=np.int32), f_nodes=np.array(fn, dtype=np.int32), f_meas=np.array(fm),
                           f_sqrtinf=np.array(fs), truth=None, meta={})


def front_shapes(A):
    """(p, b) of every front, from the analysis dump"""
    return [(int(p), int(b)) for p, b in zip(A["f_p"], A["f_b"])]


# The contract of every case: what the analysis of its graph must show.  `dense` cases leave the band kernels (a front beyond 127 rows)
# and must report form 2 on the device; the others report one of `forms`.
def _shape_dense_64_200(A):
    fr = front_shapes(A)
    assert A["max_front"] > 127
    assert any(b + 1 > 128 for _, b in fr), "no update matrix of three or more 64-tiles per side (k_dense_trailing)"
    assert any(b == 0 for _, b in fr), "no front without a boundary"


def _shape_dense_100_400(A):
    fr = front_shapes(A)
    assert A["max_front"] > 127
    assert any(b >= 256 for _, b in fr), "no front whose rows below the pivots reach a second 256-row slab (k_dense_panel)"


def _shape_dense_100_100_planes(A):
    fr = front_shapes(A)
    assert A["max_front"] > 127
    pmax = max(p for p, _ in fr)
    assert any(p == 63 for p, _ in fr) or pmax % 4 != 0, "the widest pivot block is a multiple of the 4-column panel step"
    assert any(p % 4 == 3 for p, _ in fr) and any(p % 4 in (1, 2) for p, _ in fr), "not every tail of the 4-column panel loop is present"
    rem = {(b + 1) % 64 for _, b in fr}
    assert 0 in rem and 1 in rem, "tile edge of the trailing update ((b + 1) % 64 == 0 and == 1) not present"


def _shape_dense_48_150_planes(A):
    assert A["max_front"] > 127


def _shape_band_60_40(A):
    assert 64 <= A["max_front"] <= 127, A["max_front"]


def _shape_any(A):
    assert A["max_front"] <= 127


CASES = {
    # name: (maker, shape contract, forms allowed, jacobian modes)
    "dense_48p_150l_10x5": (lambda: loop_graph(48, 150, 10, 5), _shape_dense_48_150_planes, (2,), (1,)),
    "dense_64p_200l": (lambda: loop_graph(64, 200), _shape_dense_64_200, (2,), (1,)),
    "dense_100p_400l": (lambda: loop_graph(100, 400), _shape_dense_100_400, (2,), (1,)),
    "dense_100p_100l_30x8": (lambda: loop_graph(100, 100, 30, 8), _shape_dense_100_100_planes, (2,), (1,)),
    "band_60p_40l": (lambda: loop_graph(60, 40), _shape_band_60_40, (0, 1), (1,)),
    "corridor_300_60": (lambda: synth.corridor(300, 60, seed=4), _shape_any, (1,), (1, 0)),
    "small_world_50_10": (lambda: synth.small_world(50, 10, seed=3), _shape_any, (0, 1), (1, 0)),
}
CASE_ORDER = list(CASES)                      # the smallest dense case first: a failure there is the cheapest to read


def assert_case_shapes(name, A):
    CASES[name][1](A)


def spec_layout(spec, A):
    """node id -> (offset in delta, dim) for a replayed GraphSpec (ids are the positions in the spec: nothing was removed)"""
    dims = [6 if t == synth.NODE_POSE else 3 for t in spec.node_type]
    return node_layout(A, dims)


# ---- reference -------------------------------------------------------------------------------------------------------------
def assemble_normal_equations(g, spec, A, mode, fids=None):
    """H = sum J'J, b = -sum J'r over the live factors, from pps_eval_factor (at the estimate), indexed like delta (node_voff)"""
    lay = spec_layout(spec, A)
    N = int(A["n_scalars"])
    H = np.zeros((N, N)); b = np.zeros(N)
    fids = range(len(spec.f_type)) if fids is None else fids
    for fid in fids:
        a, c = (int(v) for v in spec.f_nodes[fid])
        J, r = g.eval_factor(int(fid), mode)
        cols = list(range(lay[a][0], lay[a][0] + lay[a][1]))
        if c >= 0:
            cols += list(range(lay[c][0], lay[c][0] + lay[c][1]))
        assert J.shape[1] == len(cols)
        H[np.ix_(cols, cols)] += J.T @ J
        b[cols] -= J.T @ r
    return H, b, lay


def damped(H, lam):
    Hl = H.copy()
    Hl[np.diag_indices(len(H))] *= (1.0 + lam)
    return Hl


def reference_solves(Hl, b):
    """(x1, x2, d): LU solve, Cholesky solve, and their relative disagreement"""
    from scipy.linalg import cho_factor, cho_solve
    x1 = np.linalg.solve(Hl, b)
    x2 = cho_solve(cho_factor(Hl, lower=True), b)
    return x1, x2, float(np.linalg.norm(x1 - x2) / np.linalg.norm(x1))


def cond_spd(Hl):
    """2-norm condition number of a symmetric positive definite matrix (for the report only)"""
    ev = np.linalg.eigvalsh(Hl)
    return float(ev[-1] / ev[0])


def step_errors(delta, x1, lay):
    """e = |delta - x1|_2 / |x1|_2, and the worst node block: max |delta - x1| over the block / |x1|_inf of the WHOLE vector"""
    e = float(np.linalg.norm(delta - x1) / np.linalg.norm(x1))
    xinf = float(np.max(np.abs(x1)))
    worst, worst_node = 0.0, -1
    for nid, (off, dim) in lay.items():
        eb = float(np.max(np.abs(delta[off:off + dim] - x1[off:off + dim])) / xinf)
        if not eb <= worst:                                        # (a NaN block is the worst block)
            worst, worst_node = eb, nid
    return e, worst, worst_node


def check_step(label, delta, Hl, b, lay, form, refs=None, cond=None):
    """the bound of the linear-solve tests; prints cond, d, e and form; returns (x1, d, e, bound)"""
    x1, x2, d = refs if refs is not None else reference_solves(Hl, b)
    bound = max(16.0 * d, 1e-12)
    e, eb, node = step_errors(delta, x1, lay)
    _, db, _ = step_errors(x2, x1, lay)
    print(f"LINSOLVE {label}: form {form} n {len(b)} cond {cond_spd(Hl) if cond is None else cond:.3e} d {d:.3e} e {e:.3e} bound {bound:.3e} | worst node block "
          f"{eb:.3e} (node {node}; the two CPU solves: {db:.3e})")
    assert np.all(np.isfinite(delta)), label
    assert e <= bound, (label, "whole step", e, d)
    assert eb <= bound, (label, "node block", node, eb, d)
    return x1, d, e, bound
