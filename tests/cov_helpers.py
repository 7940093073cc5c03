"""Shared by tests/test_host_cov.py and tests/test_gpu_cov.py: the CPU side of the covariance tests.

  emulate_selected_inverse   the recursion of csrc/pps_cov.hip in numpy, driven ONLY by the arrays pps_analysis_dump exports (fronts,
                             pidx, bidx, cmap, parents).  (tests/mf_emulator.py keeps its per-front panels to itself; the panels here are
                             cut out of one dense Cholesky factor of the permuted H, which is the same thing.)
  locate_block               node pair -> (front, local row, local column, transposed): the look-up of csrc/pps_cov.cpp
  dense_h_from_device        H = J'J from pps_eval_factor of every factor, in node order
"""
import numpy as np


def node_layout(A, node_dims):
    """per graph node id: (delta offset, dim); deleted nodes (compact id -1) are left out"""
    out = {}
    for i, dim in enumerate(node_dims):
        c = int(A["node_compact"][i])
        if c >= 0:
            out[i] = (int(A["node_voff"][c]), int(dim))
    return out


def emulate_selected_inverse(A, H):
    """H: dense, indexed like delta (node_voff).  Returns per front its full block [S_AA S_BA'; S_BA S_BB] over (pivots, boundary)."""
    F = A["n_fronts"]
    pidx = np.asarray(A["pidx"])
    n = len(pidx)
    assert sorted(pidx) == list(range(n))
    Lg = np.linalg.cholesky(H[np.ix_(pidx, pidx)])
    epos = np.empty(n, dtype=np.int64); epos[pidx] = np.arange(n)
    full = [None] * F
    for s in range(F - 1, -1, -1):                      # post-order: a parent has a larger index than its children
        p, b, po = int(A["f_p"][s]), int(A["f_b"][s]), int(A["f_poff"][s])
        piv = np.arange(po, po + p)
        bnd = epos[A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]]]
        assert len(bnd) == b
        LA = Lg[np.ix_(piv, piv)]; LB = Lg[np.ix_(bnd, piv)]
        X = np.linalg.inv(LA)
        G = LB @ X
        if b:
            q = int(A["f_parent"][s])
            assert q > s
            cm = A["cmap"][A["f_cmap_off"][s]:A["f_cmap_off"][s + 1]]
            assert len(cm) == b + 1 and cm[b] == A["f_p"][q] + A["f_b"][q]       # last entry: the rhs row
            SBB = full[q][np.ix_(cm[:b], cm[:b])]
        else:
            SBB = np.zeros((0, 0))
        SBA = -SBB @ G
        SAA = X.T @ X - G.T @ SBA
        SAA = np.tril(SAA) + np.tril(SAA, -1).T
        full[s] = np.block([[SAA, SBA.T], [SBA, SBB]])
    return full, epos


def locate_block(A, epos, lay, r, c):
    """Sigma(node r, node c) -> (front, local row offset, local col offset, transposed) or None when outside the pattern"""
    (vr, dr), (vc, dc) = lay[r], lay[c]
    er, ec = int(epos[vr]), int(epos[vc])
    first = er <= ec
    (ve, de, ee), (vo, do, eo) = ((vr, dr, er), (vc, dc, ec)) if first else ((vc, dc, ec), (vr, dr, er))
    poff = np.asarray(A["f_poff"])
    s = int(np.searchsorted(poff, ee, side="right")) - 1
    p = int(A["f_p"][s])
    assert poff[s] <= ee and ee + de <= poff[s] + p
    le = ee - int(poff[s])
    if poff[s] <= eo < poff[s] + p:
        lo = eo - int(poff[s])
    else:
        bi = list(A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]])
        if vo not in bi:
            return None
        lo = p + bi.index(vo)
        assert bi[lo - p:lo - p + do] == list(range(vo, vo + do))
    return s, lo, le, first and er != ec


def block_from_fronts(full, loc, dr, dc):
    s, lo, le, tr = loc
    if tr:
        return full[s][lo:lo + dc, le:le + dr].T
    return full[s][lo:lo + dr, le:le + dc]


def factor_pairs(f_nodes):
    return sorted({(int(a), int(b)) for a, b in f_nodes if b >= 0})


def rel_err(got, ref):
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def dense_h_from_device(g, n_nodes, node_dims, fids, f_nodes, mode):
    """H = J'J from pps_eval_factor (at the estimate) of every live factor; returns H and the start column of every node"""
    starts = np.concatenate([[0], np.cumsum(node_dims)]).astype(np.int64)
    N = int(starts[-1])
    H = np.zeros((N, N))
    for fid, (a, b) in zip(fids, f_nodes):
        J, _ = g.eval_factor(int(fid), mode)
        cols = list(range(starts[a], starts[a] + node_dims[a]))
        if b >= 0:
            cols += list(range(starts[b], starts[b] + node_dims[b]))
        assert J.shape[1] == len(cols)
        H[np.ix_(cols, cols)] += J.T @ J
    return H, starts


def cpu_inverses(H):
    """two CPU inverses of H that share no code path, and their disagreement per block is the yardstick of the device comparison"""
    from scipy.linalg import cho_factor, cho_solve
    S1 = np.linalg.inv(H)
    S2 = cho_solve(cho_factor(H), np.eye(len(H)))
    return S1, S2
