"""Shared by tests/test_gpu_merge_gate.py and tests/test_gpu_merge_gate_facade.py: the pair index, the numpy reference of the merge gate and
the corridor with one wall split in two."""
import numpy as np

from pop_up_slam_amd import synth

IDENT3 = np.array([1.0, 0, 0, 1, 0, 1])          # identity sqrt information, packed upper triangle
CHI2_3_095 = 7.815


def pair_index(i, j, n):
    return i * n - i * (i + 1) // 2 + (j - i - 1)


def pairs_of(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def reference_d2(Ja, Jb, e, planes, S, blk, floor_var):
    """d2 (n x n, NaN where np.linalg.cholesky refuses S) and the largest condition number of S, from J_a, J_b, e per pair (linear pair order)
    and the dense Sigma: S = [J_a J_b] Sigma_(a, b) [J_a J_b]' + floor_var I, d2 = e' S^-1 e by np.linalg.solve"""
    n = len(planes)
    out = np.zeros((n, n)); cond = 0.0
    for i, j in pairs_of(n):
        p = pair_index(i, j, n)
        a, b = planes[i], planes[j]
        Jab = np.hstack([Ja[p], Jb[p]])
        Sig = np.block([[blk(S, a, a), blk(S, a, b)], [blk(S, b, a), blk(S, b, b)]])
        Sm = Jab @ Sig @ Jab.T + floor_var * np.eye(3)
        try:
            np.linalg.cholesky(Sm)
            cond = max(cond, float(np.linalg.cond(Sm)))
            out[i, j] = out[j, i] = e[p] @ np.linalg.solve(Sm, e[p])
        except np.linalg.LinAlgError:
            out[i, j] = out[j, i] = np.nan
    return out, cond


def best_of(d2):
    """per row the first index of the smallest finite off-diagonal entry, -1 if none"""
    n = len(d2)
    m = np.where(np.isfinite(d2) & ~np.eye(n, dtype=bool), d2, np.inf)
    return [int(np.argmin(m[i])) if np.isfinite(m[i]).any() else -1 for i in range(n)]


def pairs_below(d2, threshold):
    return [(i, j) for i, j in pairs_of(len(d2)) if np.isfinite(d2[i, j]) and d2[i, j] < threshold]


def split_wall(spec, wall):
    """`spec` with the plane node `wall` split in two: its observations from the second half of the poses that see it go to a NEW plane
    node (appended last), initialised from the first of them (the measurement carried to the world by that pose's initial value).
    Returns (spec, id of the new node).  All nodes are added before all factors."""
    obs = [k for k in range(len(spec.f_type)) if spec.f_type[k] == synth.F_PLANE_OBS and spec.f_nodes[k][1] == wall]
    assert len(obs) >= 4, "the wall is seen too rarely to be split"
    moved = obs[len(obs) // 2:]
    new = len(spec.node_type)
    first = moved[0]
    init = np.zeros(7); init[:4] = synth.plane_transform_from(spec.f_meas[first, :4], spec.node_init[spec.f_nodes[first][0]])
    f_nodes = spec.f_nodes.copy()
    for k in moved:
        f_nodes[k][1] = new
    out = synth.GraphSpec(name=spec.name + "_split", node_type=np.append(spec.node_type, synth.NODE_PLANE).astype(np.int32),
                          node_init=np.vstack([spec.node_init, init]), f_type=spec.f_type.copy(), f_nodes=f_nodes, f_meas=spec.f_meas.copy(),
                          f_sqrtinf=spec.f_sqrtinf.copy(), meta={})
    return out, new


def twin_wall(spec, wall, weight=None):
    """`spec` with the plane node `wall` listed twice: a second node with the same initial value and a copy of every observation of the
    first (same pose, same measurement, same sqrt information -- or diag(weight) on both copies).  Returns (spec, id of the twin)."""
    obs = [k for k in range(len(spec.f_type)) if spec.f_type[k] == synth.F_PLANE_OBS and spec.f_nodes[k][1] == wall]
    new = len(spec.node_type)
    f_nodes = np.vstack([spec.f_nodes, [[spec.f_nodes[k][0], new] for k in obs]]).astype(np.int32)
    f_sq = np.vstack([spec.f_sqrtinf, spec.f_sqrtinf[obs]])
    if weight is not None:
        w = np.zeros(21); w[:6] = synth._ut_diag([weight] * 3)
        for k in obs + list(range(len(spec.f_type), len(f_nodes))):
            f_sq[k] = w
    out = synth.GraphSpec(name=spec.name + "_twin", node_type=np.append(spec.node_type, synth.NODE_PLANE).astype(np.int32),
                          node_init=np.vstack([spec.node_init, spec.node_init[wall]]), f_type=np.append(spec.f_type, spec.f_type[obs]).astype(np.int32),
                          f_nodes=f_nodes, f_meas=np.vstack([spec.f_meas, spec.f_meas[obs]]), f_sqrtinf=f_sq, meta={})
    return out, new
