"""GPU: the covariance calls (pps_cov_recover, pps_cov_select, pps_cov_factor + pps_cov_block) at every front shape of the table of
tests/cov_shape_helpers.py, and at every node pair of the factor's pattern -- the pairs that share a front without sharing a factor
included, which the older covariance tests never read.

Per entry the graph is built in analytic mode (batch_optimize on the band entries, like tests/test_gpu_cov.py), every device result is read,
and only then H = sum J'J is assembled from pps_eval_factor (that call moves the linearisation point).  Reference S* =
longdouble_inverse(H) (64-bit mantissa, 2.6e-19 from a 40-digit inverse); S1 = np.linalg.inv(H).  Error of a block: the measure of
cov_block_helpers.block_err, |M - S*(r, c)|_F / sqrt(|S*(r, r)|_F |S*(c, c)|_F); e = the device against S*, d = S1 against S*, maximum
over the same blocks; bound e <= max(16 d, 1e-12), factor and floor of every covariance and linear-solve test here.  One
`COVSHAPE <entry> <call>: blocks ... (no factor: ...) e ... d ... bound ...` line per case (-s); the lines of the first full run are in
DESIGN.md, section 5b.

  recover     band entries: k_cov_level, at (48, 78) with 66 832 bytes of dynamic LDS -- beyond the 64 KB a kernel has without the raised
              ceiling.  All marginals (symmetric bit for bit, positive diagonal), pps_cov_access of every pair of the pattern in both
              orders (none outside, Sigma(r, c) the transpose of Sigma(c, r) bit for bit), pps_cov_joint of all nodes of the widest front.
  select      the dense-front pass (k_cov_dense_pre / gather / sba / saa): forced onto the band entries, plain on the dense ones.  The same
              reads against S*; on band entries also against the pps_cov_recover blocks of the same handle, with the bound and the
              normalisation of test_gpu_cov_select.py::test_dense_pass_forced_onto_a_band_graph_against_the_recovery.
  block       pps_cov_factor + pps_cov_block (k_cov_path, k_cov_gram) at about a dozen nodes chosen by role: every pairwise block in one
              call, the joint, rows x cols against cols x rows (transposes bit for bit), then the same under debug_cov_path_form(1)
              (k_cov_path_wide): byte for byte what form 0 gave.

What the first device run found (MI355X): `select` on dense_72p_400l_8x6 missed the bound -- e 5.137e-04 at d 9.722e-13 (bound 1.555e-11),
cond(H) 8.57e+07 -- from the one front with b > 256, (p, b) = (6, 258), downwards: its panel equalled, to 6e-14, the recursion with row 257
of G = L_B L_A^-1 zero (the second row of the second 256-row work item of k_cov_dense_pre), while pps_cov_block on the same factor and the
host emulation of the same source were right.  The -O3 build of that kernel spilled wave-uniform masks into the lanes of a vector register;
the same source built without such spills is right (csrc/Makefile).
"""
import numpy as np
import pytest

import cov_shape_helpers as H
from cov_block_helpers import block_err
from linsolve_helpers import assemble_normal_equations, cond_spd
from test_gpu_cov import _build

pytestmark = pytest.mark.gpu

_RUNS = {}


def _reads(g, ids, pairs, group):
    return {"marg": g.cov_marginals(), "cross": g.cov_access(pairs), "joint": g.cov_joint(group), "times": g.cov_last_times(), "ids": ids}


def _block_queries(g, sel):
    half = max(1, len(sel) // 2)
    rows, cols = sel[:half], sel[half - 1:] if len(sel) > 1 else sel
    return {"all": g.cov_block(sel, sel), "joint": g.cov_block(sel), "rc": g.cov_block(rows, cols), "cr": g.cov_block(cols, rows), "rows": rows, "cols": cols,
            "launches": g.cov_block_last()[1]}


def _run(name):
    """every device result of an entry first, then H and its two inverses; once per entry and session, shared by the tests below"""
    if name in _RUNS:
        return _RUNS[name]
    spec = H.TABLE[name][0]()
    band = name in H.BAND
    g, rec = _build(spec, jacobian_mode=1)
    if band:
        g.batch_optimize()
    else:
        g.analyze()
    A = g.analysis_dump()
    from linsolve_helpers import spec_layout
    lay = spec_layout(spec, A)
    f, sel, pairs, fill = H.assert_entry(name, A, lay, spec)
    ids = rec.node_ids()
    assert ids == sorted(lay)
    widest = max(range(A["n_fronts"]), key=lambda s: int(A["f_p"][s]) + int(A["f_b"][s]))
    piv, bnd = H.front_nodes(A, lay, widest)
    group = list(dict.fromkeys(piv + bnd))
    out = {"A": A, "lay": lay, "facts": f, "sel": sel, "pairs": pairs, "fill": set(fill), "group": group, "band": band}
    if band:
        g.cov_recover()
        out["recover"] = _reads(g, ids, pairs, group)
        g.debug_cov_select_form(1)
    g.cov_select()
    out["select"] = _reads(g, ids, pairs, group)
    g.debug_cov_select_form(0)
    g.cov_factor()
    out["factor_times"] = g.cov_last_times()
    out["block0"] = _block_queries(g, sel)
    g.debug_cov_path_form(1)
    out["block1"] = _block_queries(g, sel)
    g.debug_cov_path_form(0)
    max_p, max_rows = max(p for p, _ in f["fronts"]), max(p + b for p, b in f["fronts"])
    out["auto_wide"] = (max_p * (max_p | 1) + max_p * 6 + 2 * max_rows * 6) * 8 > 64 * 1024      # (cov_path_lds_bytes of csrc/pps_cov.hip)
    # ---- only now: H at the estimate from pps_eval_factor, and the references ----
    Hm, _, _ = assemble_normal_equations(g, spec, A, 1)
    g.close()
    out["Sref"] = H.longdouble_inverse(Hm); out["S1"] = np.linalg.inv(Hm); out["cond"] = cond_spd(Hm)
    _RUNS[name] = out
    return out


def _span(lay):
    return lambda n: slice(lay[n][0], lay[n][0] + lay[n][1])


def _selected_inverse_blocks(name, call, R, reads):
    """the shape checks of one set of reads; returns the blocks [(r, c, M)]: marginals, the pattern, the joint of the widest front"""
    lay = R["lay"]
    blocks = []
    assert len(reads["marg"]) == len(reads["ids"])
    for n, M in zip(reads["ids"], reads["marg"]):
        assert M.shape == (lay[n][1],) * 2 and np.all(np.isfinite(M)), (name, call, n)
        assert np.array_equal(M, M.T), (name, call, n, "diagonal block not symmetric bit for bit")
        assert np.all(np.diag(M) > 0), (name, call, n)
        blocks.append((n, n, M))
    got = dict(zip(R["pairs"], reads["cross"]))
    for (r, c), M in got.items():
        assert M is not None, (name, call, r, c, "a pair of the pattern is reported as outside it")
        assert M.shape == (lay[r][1], lay[c][1]) and np.all(np.isfinite(M)), (name, call, r, c)
        assert np.array_equal(M, got[(c, r)].T), (name, call, r, c, "Sigma(r, c) is not the transpose of Sigma(c, r) bit for bit")
        blocks.append((r, c, M))
    J = reads["joint"]
    assert np.all(np.isfinite(J)) and np.array_equal(J, J.T), (name, call, "joint of the widest front not symmetric bit for bit")
    jb = H.split_block(J, R["group"], R["group"], lay)
    marg = dict(zip(reads["ids"], reads["marg"]))
    for r, c, M in jb:
        assert np.array_equal(M, marg[r] if r == c else got[(r, c)]), (name, call, r, c, "joint and access disagree")
    return blocks + jb


def _report(name, call, R, blocks, note=""):
    e, d = H.block_errors(blocks, R["Sref"], R["S1"], _span(R["lay"]))
    fill = sum(1 for r, c, _ in blocks if (r, c) in R["fill"])
    bound = max(16 * d, 1e-12)
    print(f"COVSHAPE {name} {call}: scalars {R['facts']['n_scalars']} max front {R['facts']['max_front']} blocks {len(blocks)} (no factor: {fill}) "
          f"e {e:.3e} d {d:.3e} bound {bound:.3e} cond {R['cond']:.2e}{note}")
    assert e <= bound, (name, call, e, d, R["cond"])
    return e, d


# ---- 1. pps_cov_recover: k_cov_level -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.BAND)
def test_recover_every_front_shape_and_every_pair_of_the_pattern(built, name):
    R = _run(name)
    t = R["recover"]["times"]
    assert t[0] > t[1] > 0, (name, t)                       # the level pass ran (at (48, 78): under the raised LDS ceiling), no PpsError
    blocks = _selected_inverse_blocks(name, "recover", R, R["recover"])
    lds = max((2 * p * p + b * p + 2) * 8 for p, b in R["facts"]["fronts"])
    _report(name, "recover", R, blocks, f" | k_cov_level: up to {lds} bytes of dynamic LDS, pass {t[1] * 1e3:.3f} ms")


# ---- 2. pps_cov_select: the dense-front pass -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.TABLE))
def test_select_dense_front_pass_every_front_shape_and_every_pair_of_the_pattern(built, name):
    R = _run(name)
    t = R["select"]["times"]
    assert t[0] > t[1] > 0, (name, t)
    blocks = _selected_inverse_blocks(name, "select", R, R["select"])
    _report(name, "select" + (" (forced form 1)" if R["band"] else ""), R, blocks)
    if not R["band"]:
        return
    # against the recovery of the same handle: the MFMA sums differ in order from the FMA loops of k_cov_level, so no bit equality is asked
    Sref, S1, span = R["Sref"], R["S1"], _span(R["lay"])
    e = d = 0.0
    rec = _selected_inverse_blocks(name, "recover", R, R["recover"])
    assert [(r, c) for r, c, _ in rec] == [(r, c) for r, c, _ in blocks]
    for (r, c, M0), (_, _, M2) in zip(rec, blocks):
        e = max(e, block_err(M2, M0, S1[span(r), span(r)], S1[span(c), span(c)]))
        d = max(d, block_err(S1[span(r), span(c)], Sref[span(r), span(c)], S1[span(r), span(r)], S1[span(c), span(c)]))
    print(f"COVSHAPE {name} select against recover: blocks {len(blocks)} e {e:.3e} d {d:.3e} bound {max(16 * d, 1e-12):.3e}")
    assert e <= max(16 * d, 1e-12), (name, e, d)


# ---- 3. pps_cov_factor + pps_cov_block: the path walks -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.TABLE))
def test_blocks_between_the_role_nodes_in_both_path_forms(built, name):
    R = _run(name)
    lay, sel, q0, q1 = R["lay"], R["sel"], R["block0"], R["block1"]
    assert R["factor_times"][0] > 0 and R["factor_times"][1] == 0
    roles = H.roles_present(R["A"], lay, sel)
    assert all(roles.values()) or len(R["facts"]["fronts"]) == 1, (name, roles)
    for q in (q0, q1):
        assert q["launches"] == 2                           # one walk launch, one Gram launch
        for k in ("all", "joint", "rc", "cr"):
            assert np.all(np.isfinite(q[k])), (name, k)
        assert np.array_equal(q["all"], q["all"].T), (name, "Sigma(sel, sel) is not its own transpose bit for bit")
        assert np.array_equal(q["joint"], q["joint"].T) and np.all(np.diag(q["joint"]) > 0), name
        assert np.array_equal(q["rc"], q["cr"].T), (name, "Sigma(rows, cols) is not the transpose of Sigma(cols, rows) bit for bit")
    for k in ("all", "joint", "rc", "cr"):                  # the header of csrc/pps_cov_wide.hip: the bits of k_cov_path
        assert q0[k].tobytes() == q1[k].tobytes(), (name, k, "k_cov_path_wide does not write the bits of k_cov_path")
    blocks = H.split_block(q0["all"], sel, sel, lay) + H.split_block(q0["joint"], sel, sel, lay) + H.split_block(q0["rc"], q0["rows"], q0["cols"], lay)
    note = " | form 0 is already k_cov_path_wide here" if R["auto_wide"] else " | form 0 k_cov_path, form 1 k_cov_path_wide: the same bytes"
    _report(name, "block", R, blocks, f" nodes {sel}{note}")
