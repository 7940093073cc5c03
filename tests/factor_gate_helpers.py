"""Shared by tests/test_host_factor_gate.py and tests/test_gpu_factor_gate.py: the numpy side of the pps_factor_gate tests.

  reference_gate     d2 = r' (I - P)^-1 r, lev = trace(P) and the smallest eigenvalue of I - P, P = J Sigma_ff J', per factor from a DENSE
                     covariance (no structure is used: whatever the device does with fronts and descriptors, this is the formula)
  cpu_graph_gate     the same on the CPU reference graph of oracle/numpy_ref.py at its current estimate (J, r by its central differences,
                     Sigma = the dense inverse of J'J)
  leave_one_out_d2   what the statistic means: the factor is taken out, the rest is solved again, and the factor's residual at that
                     solution is measured against its innovation covariance there
"""
import copy

import numpy as np

CHI2_3_095 = 7.815       # chi-square 0.95 quantile, 3 degrees of freedom
CHI2_6_095 = 12.592      # ... 6 degrees of freedom
PIVOT_MIN = 1e-7         # a factor whose I - P has a smaller eigenvalue than this is untestable (include/pps.h)


def threshold_of(m):
    return CHI2_3_095 if m == 3 else CHI2_6_095


def reference_gate(J_rows, r_rows, Sigma, node_layout):
    """J_rows[k] (m x c), r_rows[k] (m) of factor k; Sigma: dense covariance; node_layout[k]: the c columns of Sigma that belong to the
    factor's nodes, in the column order of J.  Returns (d2, lev, emin) arrays; d2 by np.linalg.solve (NaN where numpy finds I - P singular)"""
    d2, lev, emin = [], [], []
    for J, r, cols in zip(J_rows, r_rows, node_layout):
        cols = np.asarray(cols)
        P = J @ Sigma[np.ix_(cols, cols)] @ J.T
        A = np.eye(len(r)) - P
        emin.append(float(np.linalg.eigvalsh(0.5 * (A + A.T))[0]))
        lev.append(float(np.trace(P)))
        try:
            d2.append(float(r @ np.linalg.solve(A, r)))
        except np.linalg.LinAlgError:
            d2.append(np.nan)
    return np.array(d2), np.array(lev), np.array(emin)


def graph_columns(G, k):
    """columns of factor k's nodes in the state vector of an oracle/numpy_ref.py Graph"""
    return np.concatenate([np.arange(G.start[n], G.start[n] + G.dim[n]) for n in G.f_nodes[k] if n >= 0])


def cpu_graph_gate(G):
    """(d2, lev, emin, Jr) of every factor of the numpy_ref Graph at G.x; Jr = [(J, r)] as used"""
    Jr = [G.factor_jacobian(k, G.x) for k in range(len(G.f_type))]
    Jd, _ = G.jacobian(G.x)
    Sigma = np.linalg.inv(Jd.T @ Jd)
    d2, lev, emin = reference_gate([j for j, _ in Jr], [r for _, r in Jr], Sigma, [graph_columns(G, k) for k in range(len(G.f_type))])
    return d2, lev, emin, Jr


def without_factor(spec, k):
    s = copy.copy(spec)
    keep = np.arange(len(spec.f_type)) != k
    s.f_type, s.f_nodes, s.f_meas, s.f_sqrtinf = spec.f_type[keep], spec.f_nodes[keep], spec.f_meas[keep], spec.f_sqrtinf[keep]
    s.meta = {}
    return s


def leave_one_out_d2(NR, spec, G, k, **lm):
    """factor k removed, the rest re-solved by LM from G's estimate; r_-' (I + J_- Sigma_- J_-')^-1 r_- of the removed factor there"""
    R = NR.Graph(without_factor(spec, k))
    R.x = [v.copy() for v in G.x]
    R.levenberg_marquardt(**lm)
    J, r = G.factor_jacobian(k, R.x)
    Jd, _ = R.jacobian(R.x)
    Sigma = np.linalg.inv(Jd.T @ Jd)
    cols = graph_columns(G, k)
    S = np.eye(len(r)) + J @ Sigma[np.ix_(cols, cols)] @ J.T
    return float(r @ np.linalg.solve(S, r))
