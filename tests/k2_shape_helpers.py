"""Shared by tests/test_host_k2_shapes.py and tests/test_gpu_k2_shapes.py: the CPU side of the K2 (csrc/pps_k2.hip) shape tests.  Nothing
in here is code under test: graphs, shape contracts and a sparse reference.

  CASES / assert_case_shapes
                       corridor graphs that put K2's H blocks at the counts where its control flow changes -- a landmark of 16, 17, 24
                       and 33 segments (the chunks of sixteen and k_hfinish), a pose block with a second and a third batch of product
                       records, one of exactly 64 and one of 65 contributions (one segment / two), Factor2 edges next to product records
                       -- and, per graph, what the analysis must show.  The contract is asserted from pps_analysis_dump alone
                       (blk_size, blk_nseg, seg_blk, seg_cnt, contrib), so that a change of the ordering or of seg_len cannot empty a test.
  repop_corridor       a corridor whose wall observations are turned into Pose3d_Plane3d_Factor2 edges until an exact count is reached
  assemble_sparse / sparse_reference_solves
                       H = sum J'J as a scipy.sparse matrix for the graphs a dense H is too slow for, and two sparse LU solves of it
                       that do not share their elimination order (SuperLU under COLAMD and under MMD_AT_PLUS_A); d = |x1 - x2| / |x1| is
                       the yardstick, as in tests/linsolve_helpers.py.  A third solve (SuperLU's symmetric mode) is what the device
                       is compared with: see sparse_reference_solves
  refine_extended      iterative refinement with a np.longdouble residual, which pins that third solve
  check_step_sparse    LH.check_step's bound and report for those graphs (cond is not computed: "-")
  jbuf_and_pbuf        the J and product-record buffers of tests/mf_emulator.py from the oracle's Jacobians (Factor2 edges write no record)
"""
from dataclasses import dataclass

import numpy as np

import linsolve_helpers as LH
from pop_up_slam_amd import synth

PRODUCT_FLAG = 256                            # kProductFlag: the contribution names a product record
POSE_BLOCK, PLANE_BLOCK = 42, 12              # entries of a diagonal block: 6 x 6 + 6 and 3 x 3 + 3
INVK = np.linalg.inv(synth.K_TUM).astype(np.float32)


# ---- graphs ----------------------------------------------------------------------------------------------------------------
@dataclass
class RepopSpec(synth.GraphSpec):
    """a GraphSpec some of whose plane observations are Factor2 edges (f_repop), with their ground-edge rays (f_ray)"""
    f_repop: np.ndarray = None
    f_ray: np.ndarray = None

    def _add_factor(self, g, k, nid):
        if self.f_repop[k]:
            a, b = self.f_nodes[k]
            return g.add_plane_obs2(int(nid[a]), int(nid[b]), self.f_meas[k, :4], self.f_ray[k], self.f_sqrtinf[k, :6])
        return super()._add_factor(g, k, nid)


def _ground_edge_ray(wall, tq, rng, edge_ray):
    """the rays of two pixels on the line where `wall` meets the ground, seen from pose tq, half a pixel of noise on each"""
    pl = synth.plane_transform_to(wall, tq); gs = synth.plane_transform_to(synth.GROUND, tq)
    dv = np.cross(pl[:3], gs[:3]); dv /= np.linalg.norm(dv)
    p0 = np.linalg.lstsq(np.array([pl[:3], gs[:3]]), -np.array([pl[3], gs[3]]), rcond=None)[0]   # the point of the line nearest the camera
    if abs(dv[2]) > 0.5:                       # a side wall: the line runs along the view, take it at 2 m and 4 m of depth
        pts = [p0 + dv * ((z - p0[2]) / dv[2]) for z in (2.0, 4.0)]
    else:                                      # a cross wall: the line runs across the view
        pts = [p0 - dv, p0 + dv]
    assert all(p[2] > 0.5 for p in pts), pts
    px = [(synth.K_TUM @ (p / p[2]))[:2] + rng.normal(0.0, 0.5, 2) for p in pts]
    return edge_ray(INVK, np.concatenate(px).astype(np.float32))


def repop_corridor(n_repop, n_poses=70, n_planes=16, seed=4, edge_ray=None):
    """synth.corridor(n_poses, n_planes, obs_per_pose=6) whose wall observations -- two of every three, in factor order -- are
    Factor2 edges until exactly n_repop are; walls 1, 4 and 9 get a prior.  edge_ray: P.edge_ray or the oracle's (the same bits:
    tests/test_gpu_factor2.py::test_edge_ray_matches_oracle)."""
    if edge_ray is None:
        import pop_up_slam_amd as P
        edge_ray = P.edge_ray
    base = synth.corridor(n_poses, n_planes, obs_per_pose=6, seed=seed)
    rng = np.random.default_rng(seed)
    ground = int(np.where(base.node_type == synth.NODE_PLANE)[0][0])
    F = len(base.f_type)
    repop = np.zeros(F, dtype=bool); ray = np.zeros((F, 6))
    seen = 0
    for k in range(F):
        a, b = base.f_nodes[k]
        if base.f_type[k] != synth.F_PLANE_OBS or b == ground or repop.sum() == n_repop:
            continue
        seen += 1
        if seen % 3 == 0:
            continue
        repop[k] = True
        ray[k] = _ground_edge_ray(base.truth[b, :4], base.truth[a], rng, edge_ray)
    assert repop.sum() == n_repop, (repop.sum(), n_repop)
    walls = [int(i) for i in np.where(base.node_type == synth.NODE_PLANE)[0] if i != ground]
    ft, fn, fm, fs = list(base.f_type), list(base.f_nodes), list(base.f_meas), list(base.f_sqrtinf)
    after = list(base.meta["factor_after_node"])
    for w in (walls[1], walls[4], walls[9]):
        m = np.zeros(6); m[:4] = base.truth[w, :4]
        s = np.zeros(21); s[:6] = synth._ut_diag([2.0] * 3)
        ft.append(synth.F_PLANE_PRIOR); fn.append((w, -1)); fm.append(m); fs.append(s); after.append(len(base.node_type) - 1)
    extra = len(ft) - F
    return RepopSpec(name=f"repop_{n_repop}", node_type=base.node_type, node_init=base.node_init, f_type=np.array(ft, dtype=np.int32),
                     f_nodes=np.array(fn, dtype=np.int32), f_meas=np.array(fm), f_sqrtinf=np.array(fs), truth=base.truth,
                     meta=dict(base.meta, factor_after_node=np.array(after, dtype=np.int64)),
                     f_repop=np.concatenate([repop, np.zeros(extra, dtype=bool)]), f_ray=np.vstack([ray, np.zeros((extra, 6))]))


def repeat_corridor(pose=20, total=65, n_poses=40, n_planes=12, seed=4):
    """synth.corridor(n_poses, n_planes, obs_per_pose=6) in which one pose observes its five walls again and again (each time with other
    noise) until its diagonal block has `total` contributions: a pose block of two segments whose fronts stay within the wave-per-front
    kernels -- with 63 different planes, as in pose_65, a front has 195 rows and pps_multi refuses the graph"""
    base = synth.corridor(n_poses, n_planes, obs_per_pose=6, seed=seed)
    rng = np.random.default_rng(seed)
    pn = int(np.where(base.node_type == synth.NODE_POSE)[0][pose])
    ground = int(np.where(base.node_type == synth.NODE_PLANE)[0][0])
    have = int((base.f_nodes == pn).any(axis=1).sum())
    mine = [k for k in range(len(base.f_type)) if base.f_type[k] == synth.F_PLANE_OBS and base.f_nodes[k, 0] == pn and base.f_nodes[k, 1] != ground]
    ft, fn, fm, fs = list(base.f_type), list(base.f_nodes), list(base.f_meas), list(base.f_sqrtinf)
    after = list(base.meta["factor_after_node"])
    for i in range(total - have):
        k = mine[i % len(mine)]
        m = np.zeros(6); m[:4] = synth.plane_exmap(base.f_meas[k, :4], rng.normal(0.0, 0.01, 3))
        ft.append(synth.F_PLANE_OBS); fn.append(tuple(base.f_nodes[k])); fm.append(m); fs.append(base.f_sqrtinf[k]); after.append(len(base.node_type) - 1)
    return synth.GraphSpec(name=f"repeat_{total}", node_type=base.node_type, node_init=base.node_init, f_type=np.array(ft, dtype=np.int32),
                           f_nodes=np.array(fn, dtype=np.int32), f_meas=np.array(fm), f_sqrtinf=np.array(fs), truth=base.truth,
                           meta=dict(base.meta, factor_after_node=np.array(after, dtype=np.int64)))


# ---- what the analysis shows ------------------------------------------------------------------------------------------------
def block_table(A):
    """per H block: (size, nseg, [(contributions, product records) of every segment])"""
    flags = A["contrib"].reshape(-1, 4)[:, 3]
    segs = [[] for _ in range(A["n_blocks"])]
    for s in range(A["n_segs"]):
        c0, cnt = int(A["seg_c0"][s]), int(A["seg_cnt"][s])
        segs[int(A["seg_blk"][s])].append((cnt, int((flags[c0:c0 + cnt] >= PRODUCT_FLAG).sum())))
    out = []
    for blk in range(A["n_blocks"]):
        assert len(segs[blk]) == A["blk_nseg"][blk], blk
        out.append((int(A["blk_size"][blk]), int(A["blk_nseg"][blk]), segs[blk]))
    return out


def _count(segs):
    return sum(c for c, _ in segs)


def _shape_ground(nseg, cnt=None):
    def check(A, spec):
        T = block_table(A)
        size, ns, segs = max(T, key=lambda t: _count(t[2]))
        assert size == PLANE_BLOCK, "the longest block is not a plane's diagonal block"
        assert ns == nseg, (ns, nseg)
        if cnt is not None:
            assert _count(segs) == cnt, (_count(segs), cnt)
        assert all(c == 64 for c, _ in segs[:-1]) and 1 <= segs[-1][0] <= 64        # (what the chunk arithmetic of the case assumes)
        assert sum(1 for t in T if t[1] > 4) == 1, "a second long block"
        # every contribution but the prior is a product record
        assert sum(p for _, p in segs) == _count(segs) - 1
    return check


def _shape_pose_products(lo, hi):
    def check(A, spec):
        best = max((p for size, ns, segs in block_table(A) if size == POSE_BLOCK for _, p in segs), default=0)
        assert lo <= best <= hi, f"no 42-entry block with a segment of {lo} .. {hi} product records (most: {best})"
    return check


def _shape_pose_64(A, spec):
    T = [t for t in block_table(A) if t[0] == POSE_BLOCK]
    assert any(_count(segs) == 64 and ns == 1 for _, ns, segs in T), "no 42-entry block of exactly 64 contributions"
    assert all(ns == 1 for _, ns, _ in T), "a 42-entry block of two segments"


def _shape_pose_65(A, spec):
    T = [t for t in block_table(A) if t[0] == POSE_BLOCK]
    assert any(_count(segs) == 65 and ns == 2 for _, ns, segs in T), "no 42-entry block of 65 contributions in two segments"


def _shape_pose_65_band(A, spec):
    _shape_pose_65(A, spec)
    assert A["max_front"] <= 127, "fronts beyond the wave-per-front kernels: pps_multi refuses the graph"


def _shape_repop(n_repop):
    def check(A, spec):
        assert int(spec.f_repop.sum()) == n_repop
        assert int(((spec.f_type == synth.F_PLANE_OBS) & ~spec.f_repop).sum()) > 0
        for size, what in ((POSE_BLOCK, "pose"), (PLANE_BLOCK, "wall")):
            mixes = [(c - p, p) for sz, ns, segs in block_table(A) if sz == size for c, p in segs]
            assert any(j % 2 == 1 and p >= 1 for j, p in mixes), f"no {what} block with an odd number of Jacobian-slice contributions next to a product record"
    return check


CASES = {
    # name: (maker, shape contract, lambdas, jacobian modes, dense reference)
    "ground_16seg": (lambda: synth.corridor(1023, 206, seed=4), _shape_ground(16, 1024), LH.LAMBDAS, (1,), False),
    "ground_17seg": (lambda: synth.corridor(1024, 206, seed=4), _shape_ground(17, 1025), LH.LAMBDAS, (1, 0), False),
    "ground_24seg": (lambda: synth.corridor(1500, 300, seed=4), _shape_ground(24), (1e-3,), (1,), False),
    "ground_33seg": (lambda: synth.corridor(2048, 410, seed=4), _shape_ground(33), (1e-3,), (1,), False),
    "pose_18": (lambda: synth.corridor(60, 40, obs_per_pose=18, seed=4), _shape_pose_products(17, 32), LH.LAMBDAS, (1, 0), True),
    "pose_34": (lambda: synth.corridor(60, 80, obs_per_pose=34, seed=4), _shape_pose_products(33, 64), LH.LAMBDAS, (1,), True),
    "pose_64": (lambda: synth.corridor(40, 90, obs_per_pose=62, seed=4), _shape_pose_64, LH.LAMBDAS, (1,), True),
    "pose_65": (lambda: synth.corridor(40, 90, obs_per_pose=63, seed=4), _shape_pose_65, LH.LAMBDAS, (1, 0), True),
    "mixed_repop_129": (lambda: repop_corridor(129), _shape_repop(129), LH.LAMBDAS, (1, 0), True),
}
# the graphs that take part in the batch and wave-boundary tests only: exactly one and exactly two full waves of k_linearize_repop, and a
# two-segment pose block in a graph that pps_multi accepts
BATCH_ONLY = {
    "repop_64": (lambda: repop_corridor(64, n_poses=40, n_planes=12), _shape_repop(64)),
    "repop_128": (lambda: repop_corridor(128), _shape_repop(128)),
    "pose_65_repeat": (repeat_corridor, _shape_pose_65_band),
}
CASE_ORDER = list(CASES)
SMALL = [name for name in CASE_ORDER if CASES[name][4]]
THREAD_FORM = ("ground_17seg", "pose_18", "pose_65")         # repeated with PPS_K1_THREAD_FORM=1: K2 multiplies Jacobian slices throughout
_SPECS = {}


def make(name):
    """the graph of a case (built once per process: the generators are deterministic and nothing modifies a spec)"""
    if name not in _SPECS:
        _SPECS[name] = (CASES[name] if name in CASES else BATCH_ONLY[name])[0]()
    return _SPECS[name]


def assert_case_shapes(name, A, spec):
    (CASES[name] if name in CASES else BATCH_ONLY[name])[1](A, spec)


# ---- sparse reference -------------------------------------------------------------------------------------------------------
def assemble_sparse(g, spec, A, mode):
    """LH.assemble_normal_equations with H as a scipy.sparse CSC matrix: the same J and r, the same indexing (node_voff)"""
    from scipy import sparse
    lay = LH.spec_layout(spec, A)
    N = int(A["n_scalars"])
    ri, ci, vv = [], [], []
    b = np.zeros(N)
    for fid in range(len(spec.f_type)):
        a, c = (int(v) for v in spec.f_nodes[fid])
        J, r = g.eval_factor(int(fid), mode)
        cols = np.arange(lay[a][0], lay[a][0] + lay[a][1])
        if c >= 0:
            cols = np.concatenate([cols, np.arange(lay[c][0], lay[c][0] + lay[c][1])])
        assert J.shape[1] == len(cols)
        JtJ = J.T @ J
        ri.append(np.repeat(cols, len(cols))); ci.append(np.tile(cols, len(cols))); vv.append(JtJ.ravel())
        b[cols] -= J.T @ r
    H = sparse.coo_matrix((np.concatenate(vv), (np.concatenate(ri), np.concatenate(ci))), shape=(N, N)).tocsc()   # (duplicates are summed)
    H.sum_duplicates()
    return H, b, lay


def damped_sparse(H, lam):
    """H + lambda diag(H), as LH.damped"""
    Hl = H.copy()
    Hl.setdiag(H.diagonal() * (1.0 + lam))                      # (every diagonal entry is stored: the pattern does not change)
    return Hl


def sparse_reference_solves(Hl, b):
    """(x0, x1, x2, d).  x1 and x2: SuperLU with partial pivoting under two column orderings that share no elimination order (COLAMD,
    MMD on A' + A); d = |x1 - x2| / |x1| is the yardstick, as in LH.reference_solves.  x0 is what a step is compared WITH: SuperLU in its
    symmetric mode (pivots on the diagonal, MMD on A' + A -- the elimination a sparse Cholesky does).  On these graphs the two pivoting
    solves are each accurate to about d in the 2-norm, but their errors sit in a few node blocks, where they reach or pass 16 d in the
    maximum norm (measured against an extended-precision refinement at lambda = 1e-3, ground_17seg: 9e-13 / 1.5e-11 and 1e-12 / 1.3e-11
    with 16 d = 1.7e-11; the symmetric mode: 7e-15 / 2.5e-14) -- the exact solution itself would fail the node-block bound against x1.
    tests/test_host_k2_shapes.py pins x0 against that refinement."""
    from scipy.sparse.linalg import splu
    x1 = splu(Hl, permc_spec="COLAMD").solve(b)
    x2 = splu(Hl, permc_spec="MMD_AT_PLUS_A").solve(b)
    x0 = splu(Hl, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True)).solve(b)
    return x0, x1, x2, float(np.linalg.norm(x1 - x2) / np.linalg.norm(x1))


def refine_extended(Hl, b, x, steps=4):
    """iterative refinement of x with the residual b - H x in np.longdouble (corrections from a symmetric-mode SuperLU factor): the
    higher-precision opinion the sparse reference is pinned with.  Returns the refined x (longdouble) and the size of every correction."""
    from scipy.sparse.linalg import splu
    lu = splu(Hl, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    Hr = Hl.tocsr()
    data, rows = Hr.data.astype(np.longdouble), np.repeat(np.arange(Hr.shape[0]), np.diff(Hr.indptr))
    x = x.astype(np.longdouble); bl = b.astype(np.longdouble)
    sizes = []
    for _ in range(steps):
        Ax = np.zeros(len(b), dtype=np.longdouble)
        np.add.at(Ax, rows, data * x[Hr.indices])
        dx = lu.solve(np.asarray(bl - Ax, dtype=np.float64))
        x = x + dx
        sizes.append(float(np.linalg.norm(dx) / np.linalg.norm(np.asarray(x, dtype=np.float64))))
    return x, sizes


def check_step_sparse(label, delta, refs, lay, form):
    """the bound of LH.check_step for a step whose reference came from sparse_reference_solves: e = |delta - x0| / |x0| <= max(16 d, 1e-12),
    whole vector and per node block, with d the disagreement of the two pivoting solves; prints d, e and form; returns (d, e, bound)"""
    x0, x1, x2, d = refs
    bound = max(16.0 * d, 1e-12)
    e, eb, node = LH.step_errors(delta, x0, lay)
    e1, db1, _ = LH.step_errors(x1, x0, lay)
    e2, db2, _ = LH.step_errors(x2, x0, lay)
    print(f"LINSOLVE {label}: form {form} n {len(x0)} cond - (sparse reference) d {d:.3e} e {e:.3e} bound {bound:.3e} | worst node block "
          f"{eb:.3e} (node {node}; the two pivoting CPU solves against the symmetric one: {e1:.3e} / {db1:.3e} and {e2:.3e} / {db2:.3e})")
    assert np.all(np.isfinite(delta)), label
    assert e <= bound, (label, "whole step", e, d)
    assert eb <= bound, (label, "node block", node, eb, d)
    return d, e, bound


# ---- the buffers of tests/mf_emulator.py ------------------------------------------------------------------------------------
def jbuf_and_pbuf(spec, A, o):
    """J buffer and product-record buffer in the device layout from the oracle's Jacobians (analytic; Factor2 numeric, as on the device),
    and the dense J and -r of the whole graph in node order.  A product record -- [J_a'J_a | -J_a'r] then the same for node b -- is
    written for plain plane observations only, the factors whose contributions carry kProductFlag."""
    dims = [o.node_dim(i) for i in range(o.num_nodes())]
    starts = np.concatenate([[0], np.cumsum(dims)])
    ncol = int(starts[-1])
    Jbuf = np.zeros(A["J_size"]); Pbuf = np.zeros(A["P_size"])
    repop = getattr(spec, "f_repop", np.zeros(len(spec.f_type), dtype=bool))
    rows, rhs = [], []
    for k in range(o.num_factors()):
        Hk, rk = o.factor_jacobian(k, 1)
        m = Hk.shape[0]; a, b = spec.f_nodes[k]; da = dims[a]; db = dims[b] if b >= 0 else 0
        off = A["factor_joff"][k]
        Jbuf[off:off + m * da] = Hk[:, :da].ravel()
        Jbuf[off + m * da:off + m * (da + db)] = Hk[:, da:].ravel()
        Jbuf[off + m * (da + db):off + m * (da + db) + m] = rk
        if spec.f_type[k] == synth.F_PLANE_OBS and not repop[k]:
            po = A["factor_poff"][k]
            Ja = Hk[:, :da]; Pbuf[po:po + da * da] = (Ja.T @ Ja).ravel(); Pbuf[po + da * da:po + da * da + da] = -Ja.T @ rk
            pb_ = po + da * da + da; Jb = Hk[:, da:]
            Pbuf[pb_:pb_ + db * db] = (Jb.T @ Jb).ravel(); Pbuf[pb_ + db * db:pb_ + db * db + db] = -Jb.T @ rk
        R = np.zeros((m, ncol)); R[:, starts[a]:starts[a] + da] = Hk[:, :da]
        if b >= 0:
            R[:, starts[b]:starts[b] + db] = Hk[:, da:]
        rows.append(R); rhs.append(-rk)
    return Jbuf, Pbuf, np.vstack(rows), np.concatenate(rhs), starts, dims
