"""GPU: the five queries on the factor -- cov_block, assoc_gate, merge_gate, loop_gate, factor_gate -- interleaved on ONE handle.  Each keeps a
state of its own on the handle (csrc/pps_query.h: result, tickets, records, status word, figures of the last call) while all five share the
request blob, the strips and the event pair.  What the per-call tests do not look at: a call after a LARGER call of the same kind (every buffer
grown, tickets of the larger call still allocated), after calls of the other four kinds in another order, and after a call that raised its
status word.  Every comparison is of the handle with itself, bit for bit (tobytes(), so NaNs compare): the calls leave the estimate alone
(the test_*_solves_are_left_alone tests assert that).

Graph: synth.corridor(60, 14, seed=7), a band graph -- one cov_recover serves all five calls.  Round 1: every call at its smallest shape.
Round 2: every call at a shape that makes its buffers grow -- 60 poses x 14 planes for cov_block, 70 measurements x 14 planes for assoc_gate
(more than the 64 tickets a ticket buffer starts with), all 14 planes for merge_gate (its 14 row tickets fit the 64 the first call allocated:
that one buffer cannot be made to grow on this graph), 70 candidates for loop_gate (no multiple of the kernel's candidates per workgroup), all
factors for factor_gate.  Round 3: round 1 again in another order; outputs, records, launch counts and not-PD / untestable counts must be
round 1's."""
import numpy as np
import pytest

import pop_up_slam_amd as P
from loop_gate_helpers import WAVES, make_candidates
from pop_up_slam_amd import synth

pytestmark = pytest.mark.gpu

ORDER_1 = ("cov_block", "assoc_gate", "merge_gate", "loop_gate", "factor_gate")
ORDER_3 = ("factor_gate", "loop_gate", "cov_block", "merge_gate", "assoc_gate")


def _bits(v):
    """a call's answer as bytes: nested tuples / lists of arrays, numbers and None"""
    if isinstance(v, (tuple, list)):
        return tuple(_bits(x) for x in v)
    return None if v is None else np.ascontiguousarray(v).tobytes()


@pytest.fixture(scope="module")
def scene(built):
    spec = synth.corridor(60, 14, seed=7)
    g = P.Graph(); nid, fid = spec.replay(g)
    g.batch_optimize()
    g.cov_recover()
    poses = [int(n) for n, t in zip(nid, spec.node_type) if t == synth.NODE_POSE]
    planes = [int(n) for n, t in zip(nid, spec.node_type) if t != synth.NODE_POSE]
    fids = [int(f) for f in fid]
    assert (len(poses), len(planes)) == (60, 14)
    rng = np.random.default_rng(3)
    x = poses[31]
    # measurements of pose x near its view of plane k % 14, 70 of them; the first is round 1's
    meas = np.array([synth.plane_exmap(synth.plane_transform_to(g.get_plane(planes[k % 14]), g.get_pose(x)), 0.02 * rng.normal(size=3)) for k in range(70)])
    sq = np.array([synth._ut_diag([30.0, 40.0, 50.0])] * 70)
    pairs = [(poses[(7 * k) % 60], poses[(7 * k + 11 + k % 5) % 60]) for k in range(70)]
    assert all(a != b for a, b in pairs) and len(pairs) % WAVES != 0
    lmeas, lsq = make_candidates({n: g.get_pose(n) for n in poses}, pairs, 17, gross=(20.0, 1.0))
    pa, pb = [a for a, _ in pairs], [b for _, b in pairs]
    small = {"cov_block": lambda: g.cov_block([poses[3], planes[2]]),
             "assoc_gate": lambda: g.assoc_gate(x, meas[:1], sq[:1], planes[4:6]),
             "merge_gate": lambda: g.merge_gate(planes[1:4]),
             "loop_gate": lambda: g.loop_gate(pa[:1], pb[:1], lmeas[:1], lsq[:1], want_S=True),
             "factor_gate": lambda: g.factor_gate(fids[5:8])}
    large = {"cov_block": lambda: g.cov_block(poses, planes),
             "assoc_gate": lambda: g.assoc_gate(x, meas, sq),
             "merge_gate": lambda: g.merge_gate(),
             "loop_gate": lambda: g.loop_gate(pa, pb, lmeas, lsq, want_S=True),
             "factor_gate": lambda: g.factor_gate()}
    last = {"cov_block": g.cov_block_last, "assoc_gate": g.assoc_gate_last, "merge_gate": g.merge_gate_last, "loop_gate": g.loop_gate_last,
            "factor_gate": g.factor_gate_last}
    # a factor_gate record is a slot of 78 doubles of which [J m x c | r m] are specified (the rest keeps what an earlier call left there)
    used = {synth.F_POSE_PRIOR: 6 * 6 + 6, synth.F_ODOMETRY: 6 * 12 + 6, synth.F_PLANE_OBS: 3 * 9 + 3, synth.F_PLANE_PRIOR: 3 * 3 + 3}
    assert list(fids) == list(range(len(fids)))           # (a factor's id is its index in the spec)
    factor_records = lambda ids: lambda: [slot[:used[int(spec.f_type[f])]] for slot, f in zip(g.factor_gate_records(), ids)]
    records = {"cov_block": lambda table: lambda: None, "assoc_gate": lambda table: g.assoc_gate_records, "merge_gate": lambda table: g.merge_gate_records,
               "loop_gate": lambda table: g.loop_gate_records, "factor_gate": lambda table: factor_records(fids[5:8] if table is small else fids)}

    def call(table, name):
        """(answer, records, launches and count of _last) of one call, as bytes and ints"""
        out = table[name]()
        return _bits(out), _bits(records[name](table)()), tuple(last[name]()[1:]), out

    yield {"g": g, "x": x, "planes": planes, "meas": meas, "sq": sq, "small": small, "large": large, "call": call}
    g.close()


def test_small_calls_repeat_bit_for_bit_after_larger_calls_in_another_order(scene):
    call, small, large = scene["call"], scene["small"], scene["large"]
    first = {name: call(small, name) for name in ORDER_1}
    grown = {name: call(large, name) for name in ORDER_1}
    again = {name: call(small, name) for name in ORDER_3}
    for name in ORDER_1:
        assert again[name][0] == first[name][0], name                # every output
        assert again[name][1] == first[name][1], name                # every record
        assert again[name][2] == first[name][2], name                # launches, not-PD / untestable entries
        assert first[name][2][0] == (1 if name == "factor_gate" else 2), name
    # the rounds did compute something, and the larger round was larger
    assert np.all(np.isfinite(first["cov_block"][3])) and first["cov_block"][3].shape == (9, 9) and grown["cov_block"][3].shape == (360, 42)
    d2, best = first["assoc_gate"][3]
    assert d2.shape == (1, 2) and np.all(np.isfinite(d2)) and grown["assoc_gate"][3][0].shape == (70, 14)
    assert first["merge_gate"][3][0].shape == (3, 3) and grown["merge_gate"][3][0].shape == (14, 14)
    assert np.isfinite(first["loop_gate"][3][0][0]) and len(grown["loop_gate"][3][0]) == 70 and np.all(np.isfinite(grown["loop_gate"][3][0]))
    assert len(first["factor_gate"][3][0]) == 3 and len(grown["factor_gate"][3][0]) > 200
    # a small call is part of the large one: same bits wherever the two overlap (an answer does not depend on the rest of its list)
    assert grown["assoc_gate"][3][0][0, 4:6].tobytes() == d2.tobytes()
    assert grown["loop_gate"][3][0][:1].tobytes() == first["loop_gate"][3][0].tobytes()
    assert grown["factor_gate"][3][0][5:8].tobytes() == first["factor_gate"][3][0].tobytes()


def test_assoc_gate_after_a_call_that_raised_its_status_word(scene):
    """PPS_ENOTPD is the one status a query raises in normal operation: a finite sqrt information of 1e200 makes the innovation covariance
    overflow (1 + Jw Sigma Jw' = inf: no finite pivot; the CPU emulation of the kernel, tests/cpp/gate_emu.cpp, raises its status word to 1
    on such a measurement in both Jacobian modes).  The call after it finds the status word set and answers as if nothing had happened."""
    g, x, planes, meas, sq = (scene[k] for k in ("g", "x", "planes", "meas", "sq"))
    call, small = scene["call"], scene["small"]
    first = call(small, "assoc_gate")
    d2_before = g.merge_gate(planes[1:4])[0]
    with pytest.raises(P.PpsError) as e:
        g.assoc_gate(x, meas[:3], np.array([synth._ut_diag([1e200] * 3)] * 3), planes[:5])
    assert e.value.code == P.PPS_ENOTPD and "association gate" in str(e.value)
    with pytest.raises(P.PpsError) as e:
        g.assoc_gate_records()                                        # records exist exactly when the last call succeeded
    assert e.value.code == P.PPS_ESTATE
    assert g.merge_gate(planes[1:4])[0].tobytes() == d2_before.tobytes()      # the other calls' states are their own
    again = call(small, "assoc_gate")
    assert again[:3] == first[:3]
