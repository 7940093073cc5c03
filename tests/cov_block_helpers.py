"""Shared by tests/test_host_cov_block.py and tests/test_gpu_cov_block.py: the CPU side of the tests of pps_cov_block.

  emulate_block     the path walk and the suffix Gram product of csrc/pps_cov.hip (k_cov_path, k_cov_gram) in numpy, driven ONLY by the
                    arrays pps_analysis_dump exports (f_parent, f_p, f_b, f_poff, pidx, bidx, cmap).  The panels are cut out of one dense
                    Cholesky factor of the permuted H, like emulate_selected_inverse (tests/cov_helpers.py) cuts its own.
  request_tables    the request of a query as csrc/pps_query.cpp builds it (CovWalk / CovStep / CovPair of csrc/pps_cov.h), for the kernel
                    source compiled for the host (tests/cpp/cov_block_emu.cpp)
  block_err         |M - M0|_F / sqrt(|S0(r, r)|_F |S0(c, c)|_F): a small cross block between distant nodes is measured against the
                    reference's diagonal blocks, not against its own near-zero norm
"""
import numpy as np
from scipy.linalg import solve_triangular

WALK = np.dtype([("strip", "<i8"), ("step0", "<i4"), ("n_steps", "<i4"), ("local", "<i4"), ("dim", "<i4")])
STEP = np.dtype([("front", "<i4"), ("row", "<i4")])
PAIR = np.dtype([("yi", "<i8"), ("yj", "<i8"), ("dst", "<i8"), ("dst_t", "<i8"), ("di", "<i4"), ("dj", "<i4"), ("len", "<i4"), ("ld", "<i4")])


def elimination_positions(A):
    pidx = np.asarray(A["pidx"])
    epos = np.empty(len(pidx), dtype=np.int64); epos[pidx] = np.arange(len(pidx))
    return pidx, epos


def node_front(A, epos, v):
    """delta offset of a node -> (its front, the local index of its first pivot)"""
    poff = np.asarray(A["f_poff"])
    e = int(epos[v])
    s = int(np.searchsorted(poff, e, side="right")) - 1
    assert poff[s] <= e < poff[s] + A["f_p"][s]
    return s, e - int(poff[s])


def path_to_root(A, s):
    out = []
    while s >= 0:
        out.append(int(s)); s = int(A["f_parent"][s])
        assert len(out) <= A["n_fronts"]
    return out


def root_lengths(A):
    """per front: the pivots of the front and of all its ancestors"""
    return np.array([sum(int(A["f_p"][t]) for t in path_to_root(A, s)) for s in range(A["n_fronts"])], dtype=np.int64)


def common_suffix(A, pa, pb):
    """pivots of the fronts two paths (leaf -> root) end with in common"""
    n = 0
    for x, y in zip(reversed(pa), reversed(pb)):
        if x != y:
            break
        n += int(A["f_p"][x])
    return n


def walk(A, Lg, epos, v, dim):
    """Y = the rows of L^-1 E_node on the pivots of the node's path, leaf -> root: (path, Y of shape (pivots on the path, dim))"""
    s, local = node_front(A, epos, v)
    path = path_to_root(A, s)
    p, b = int(A["f_p"][s]), int(A["f_b"][s])
    z = np.zeros((p + b, dim))
    z[local:local + dim] = np.eye(dim)
    ys = []
    for k, s in enumerate(path):
        p, b, po = int(A["f_p"][s]), int(A["f_b"][s]), int(A["f_poff"][s])
        piv = np.arange(po, po + p)
        bnd = epos[A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]]]
        assert len(bnd) == b and len(z) == p + b
        y = solve_triangular(Lg[np.ix_(piv, piv)], z[:p], lower=True)
        ys.append(y)
        if b:
            q = path[k + 1]
            cm = np.asarray(A["cmap"][A["f_cmap_off"][s]:A["f_cmap_off"][s] + b])
            zq = np.zeros((int(A["f_p"][q]) + int(A["f_b"][q]), dim))      # parent rows that no row of this front maps to start at zero
            assert len(set(cm.tolist())) == b and cm.min() >= 0 and cm.max() < len(zq)
            zq[cm] = z[p:] - Lg[np.ix_(bnd, piv)] @ y
            z = zq
        else:
            assert k == len(path) - 1
    return path, np.vstack(ys)


def emulate_block(A, H, lay, rows, cols=None):
    """Sigma(rows, cols) by path walks and suffix Gram products; cols None: the joint marginal (lower triangle, mirrored)"""
    pidx, epos = elimination_positions(A)
    Lg = np.linalg.cholesky(H[np.ix_(pidx, pidx)])
    joint = cols is None
    cols = rows if joint else cols
    strips = {n: walk(A, Lg, epos, lay[n][0], lay[n][1]) for n in set(rows) | set(cols)}
    K = max(len(y) for _, y in strips.values())
    right = {n: np.vstack([np.full((K - len(y), y.shape[1]), np.nan), y]) for n, (_, y) in strips.items()}     # aligned at the root end
    ro = np.concatenate([[0], np.cumsum([lay[n][1] for n in rows])]); co = np.concatenate([[0], np.cumsum([lay[n][1] for n in cols])])
    out = np.full((ro[-1], co[-1]), np.nan)
    for i, r in enumerate(rows):
        for j, c in enumerate(cols):
            if joint and j > i:
                continue
            n = common_suffix(A, strips[r][0], strips[c][0])
            blk = right[r][K - n:].T @ right[c][K - n:]
            if joint and i == j:
                blk = np.tril(blk) + np.tril(blk, -1).T
            out[ro[i]:ro[i + 1], co[j]:co[j + 1]] = blk
            if joint:
                out[co[j]:co[j + 1], ro[i]:ro[i + 1]] = blk.T
    return out


def request_tables(A, lay, rows, cols=None):
    """(walks, steps, pairs, K, n_strip, shape) of a query, as pps_cov_block lays them out"""
    _, epos = elimination_positions(A)
    rl = root_lengths(A)
    joint = cols is None
    cols = rows if joint else cols
    ids = list(dict.fromkeys(list(rows) + list(cols)))
    where = {n: node_front(A, epos, lay[n][0]) for n in ids}
    K = int(max(rl[where[n][0]] for n in ids))
    walks = np.zeros(len(ids), dtype=WALK); steps = []; paths = {}
    n_strip = 0
    for w, n in enumerate(ids):
        paths[n] = path_to_root(A, where[n][0])
        walks[w] = (n_strip, len(steps), len(paths[n]), where[n][1], lay[n][1])
        steps += [(s, K - int(rl[s])) for s in paths[n]]
        n_strip += K * lay[n][1]
    ro = np.concatenate([[0], np.cumsum([lay[n][1] for n in rows])]); co = np.concatenate([[0], np.cumsum([lay[n][1] for n in cols])])
    ld = int(co[-1])
    pairs = []
    for i, r in enumerate(rows):
        for j, c in enumerate(cols):
            if joint and j > i:
                continue
            n = common_suffix(A, paths[r], paths[c])
            a, b = ids.index(r), ids.index(c)
            pairs.append((walks[a]["strip"] + (K - n) * lay[r][1], walks[b]["strip"] + (K - n) * lay[c][1], ro[i] * ld + co[j],
                          co[j] * ld + ro[i] if joint else -1, lay[r][1], lay[c][1], n, ld))
    return walks, np.array(steps, dtype=STEP), np.array(pairs, dtype=PAIR), K, n_strip, (int(ro[-1]), ld)


def block_err(M, M0, Srr, Scc):
    return float(np.linalg.norm(M - M0) / np.sqrt(np.linalg.norm(Srr) * np.linalg.norm(Scc)))


def query_errors(got, S1, S2, rows, cols, span):
    """per node pair of a query result `got` = Sigma(rows, cols): (max e against S1, max d between S2 and S1); span(n) = the slice of
    node n in the reference matrices"""
    e = d = 0.0
    o = 0
    for r in rows:
        sr = span(r); oc = 0
        for c in cols:
            sc = span(c)
            nr, nc = sr.stop - sr.start, sc.stop - sc.start
            e = max(e, block_err(got[o:o + nr, oc:oc + nc], S1[sr, sc], S1[sr, sr], S1[sc, sc]))
            d = max(d, block_err(S2[sr, sc], S1[sr, sc], S1[sr, sr], S1[sc, sc]))
            oc += nc
        o += nr
    return e, d
