"""The covariance entry points interleaved on ONE handle: what pps_cov_factor, pps_cov_recover and pps_cov_select build, check and upload
for an analysis is kept in one record (pps_graph::cov_cache, pps_cov.cpp), and every other test runs each entry point mostly on a handle
of its own.

Band graph (small_world_5_3, after batch_optimize so that stats() and trace() have something to lose):
  cov_factor -> cov_block -> cov_recover -> marginals, access on the factor pairs, cov_block -> form 1, cov_select -> marginals ->
  cov_factor -> marginals (refused, PPS_ESTATE, both call names in the text) -> cov_block -> form 0, cov_select -> marginals; then one pose
  and one odometry factor are added through the handle, cov_recover, marginals.
Dense-front graph (dense_48p_150l_10x5, the smallest of DENSE):
  cov_select -> marginals -> cov_factor -> cov_block, assoc_gate -> cov_select -> marginals; cov_recover is still refused ("dense-front").

Every comparison asks for the same bytes; the commit before the record gave them on an MI355X, in all of these:
  the three cov_block results; the first and the last marginals of the band graph (both from the band level pass); the form-1 marginals
  against a fresh handle that ran form 1 alone, and that handle's form-0 marginals afterwards against the first; the marginals after the
  topology change against a fresh handle built from the grown
  graph; the first and the last marginals of the dense-front graph.
So no comparison falls back on the bound of test_dense_pass_forced_onto_a_band_graph_against_the_recovery.

After every call of a sequence: cov_block_last()[1] == 2 and assoc_gate_last()[1] == 2 once there has been such a call, and the solve
figures of stats() and trace() are those of the batch_optimize before the sequence (as tests/test_gpu_cov_factor.py checks them).
"""
import numpy as np
import pytest

import pop_up_slam_amd as P
from cov_factor_helpers import DENSE, GRAPHS
from cov_helpers import factor_pairs
from pop_up_slam_amd import synth
from test_gpu_cov import _build
from test_gpu_gate import _measurements

pytestmark = pytest.mark.gpu

SOLVE_FIGURES = ("lm_iterations", "chi2_initial", "chi2_final", "lambda_final", "n_linearize", "n_factorize", "n_launches", "t_total")


class Sequence:
    """calls on one handle, the standing checks after each"""

    def __init__(self, g):
        self.g, self.stats, self.trace, self.block, self.gate = g, g.stats(), g.trace(), False, False

    def __call__(self, name, *args):
        try:
            out = getattr(self.g, name)(*args)
        finally:
            self.block |= name == "cov_block"; self.gate |= name == "assoc_gate"
            after = self.g.stats()
            for k in SOLVE_FIGURES:
                assert after[k] == self.stats[k], (name, k)
            assert self.g.trace() == self.trace, name
            if self.block:
                assert self.g.cov_block_last()[1] == 2, name
            if self.gate:
                assert self.g.assoc_gate_last()[1] == 2, name
        return out


def _same_bytes(label, xs, ys):
    same = len(xs) == len(ys) and all(a.tobytes() == b.tobytes() for a, b in zip(xs, ys))
    print(f"COVORDER {label}: same bytes {same}")
    return same


def _grow(g, rec):
    """one pose behind the last one, joined to it by an odometry factor"""
    last = max(n for n in rec.node_ids() if rec.dims[n] == 6)
    p = g.add_pose(g.get_pose(last))
    g.add_odometry(last, p, np.zeros(6), synth._ut_diag([1.0] * 6))


def test_band_graph_every_entry_point_on_one_handle(built):
    make = lambda: synth.small_world(5, 3)
    g, rec = _build(make())
    g.batch_optimize()
    assert g.stats()["max_front"] <= 127
    ids = rec.node_ids()
    pairs = factor_pairs(list(rec.factors.values()))
    s = Sequence(g)
    s("cov_factor")
    b0 = s("cov_block", ids)
    s("cov_recover")
    m0 = s("cov_marginals")
    assert all(M is not None for M in s("cov_access", pairs))
    b1 = s("cov_block", ids)
    s("debug_cov_select_form", 1); s("cov_select")
    m1 = s("cov_marginals")
    s("cov_factor")
    with pytest.raises(P.PpsError) as e:
        s("cov_marginals")
    assert e.value.code == P.PPS_ESTATE and "pps_cov_factor" in str(e.value) and "pps_cov_recover" in str(e.value)
    b2 = s("cov_block", ids)
    s("debug_cov_select_form", 0); s("cov_select")
    m2 = s("cov_marginals")
    assert np.all(np.isfinite(b0)) and all(np.all(np.isfinite(M)) for M in m0 + m1)
    assert _same_bytes("band cov_block 1 / 2", [b0], [b1]) and _same_bytes("band cov_block 1 / 3", [b0], [b2])
    assert _same_bytes("band marginals first / last", m0, m2)

    f, _ = _build(make())
    f.batch_optimize(); f.debug_cov_select_form(1); f.cov_select()
    assert _same_bytes("band form 1 / fresh handle", m1, f.cov_marginals())
    f.debug_cov_select_form(0); f.cov_select()                  # the level pass on a handle that has prepared the dense-front pass alone
    assert _same_bytes("band form 0 after form 1 on the fresh handle / first", m0, f.cov_marginals())
    f.close()

    _grow(g, rec)
    s("cov_recover")
    m3 = s("cov_marginals")
    h, hrec = _build(make())
    h.batch_optimize(); _grow(h, hrec); h.cov_recover()
    mh = h.cov_marginals()
    assert hrec.node_ids() == rec.node_ids() and len(m3) == len(mh) == len(ids) + 1
    assert _same_bytes("band grown / fresh handle", m3, mh)
    g.close(); h.close()


def test_dense_front_graph_every_entry_point_on_one_handle(built):
    g, rec = _build(GRAPHS[DENSE[0]](), jacobian_mode=1)
    g.batch_optimize()
    assert g.stats()["max_front"] > 127
    ids = rec.node_ids()
    poses = [n for n in ids if rec.dims[n] == 6]; planes = [n for n in ids if rec.dims[n] == 3]
    meas, W, _ = _measurements(g, poses[-1], planes, seed=5, steps=(2.5, 40.0))
    s = Sequence(g)
    s("cov_select")
    m0 = s("cov_marginals")
    s("cov_factor")
    b = s("cov_block", ids[::3])
    d2, best = s("assoc_gate", poses[-1], meas, W, planes)
    s("cov_select")
    m1 = s("cov_marginals")
    assert np.all(np.isfinite(b)) and np.all(np.isfinite(d2)) and all(np.all(np.isfinite(M)) for M in m0)
    assert _same_bytes("dense marginals first / last", m0, m1)
    with pytest.raises(P.PpsError) as e:
        s("cov_recover")
    assert e.value.code == P.PPS_ESTATE and "dense-front" in str(e.value)
    g.close()
