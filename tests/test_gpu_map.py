"""GPU: the dense map (pps_map_*).  Expected values never come from the code under test: the chunks are the cloud and the plane-id map of
the same run (pps_popup_download) split in numpy, the projections are pps_reproject_points (bit for bit) and a numpy fp64
Plane3d::project_to_plane (1 fp32 ulp: the fp64 arithmetic differs by rounding order only, which can move the final fp32 rounding by at
most one ulp), the selection is pps_map_select_host (itself checked against main_3d.cpp:538-562 in tests/test_host_map.py)."""
import numpy as np
import pytest

import pop_up_slam_amd as P
from map_helpers import assert_within_one_ulp, project_to_plane, raw16, split_frame, xyz_of
from pop_up_slam_amd import pipeline, synth

pytestmark = pytest.mark.gpu


def _calib(w, h):
    K = synth.K_TUM.copy(); K[0] *= w / 640.0; K[1] *= h / 480.0
    return K, np.linalg.inv(K).astype(np.float32)


def _pose(k, yaw=0.05, pitch=0.02):
    Rp = np.array([[1, 0, 0], [0, np.cos(pitch), -np.sin(pitch)], [0, np.sin(pitch), np.cos(pitch)]])
    R = synth._Rz(yaw + 0.01 * k) @ synth.CAM_R0 @ Rp
    return synth.pose_from_Rt(R, np.array([0.1, 0.3 * k, 1.0]))


def _popup(w, h, seed=0):
    K, invK = _calib(w, h)
    pp = P.Popup(w, h, invK)
    pp.set_image(np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    return pp, K


def _plane_graph(n_planes):
    """a graph that only has to know its plane nodes (compaction and capacity do not read the estimate)"""
    g = P.Graph()
    g.add_pose([0, 0, 1, 0, 0, 0, 1])
    return g, [g.add_plane([np.sin(i), np.cos(i), 0.1 * i, -1.0 - i]) for i in range(n_planes)]


def _check_store(m, frames):
    """frames: per frame (seq, ids, expected chunk per plane); the whole table and every stored record"""
    t = m.chunks(); store = m.download(0)
    rows = [(f, seq, k, ids[k], want[k]) for f, (seq, ids, want) in enumerate(frames) for k in range(len(ids)) if ids[k] >= 0]
    assert len(t) == len(rows)
    off = 0
    for c, (f, seq, k, lm, want) in zip(t, rows):
        assert (c["frame"], c["frame_seq_id"], c["frame_plane"], c["plane_id"], c["offset"], c["count"]) == (f, seq, k, lm, off, len(want))
        np.testing.assert_array_equal(raw16(store[off:off + len(want)]), raw16(want))
        off += len(want)
    info = m.info()
    assert (info["n_points"], info["n_frames"], info["n_chunks"]) == (off, len(frames), len(rows)) and len(store) == off


# 150 x 113: the width is no multiple of 64, the pixel count (16950) no multiple of 256
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("w,h", [(160, 120), (150, 113)])
def test_compaction_is_the_numpy_split_of_the_same_run(built, w, h, step):
    pp, K = _popup(w, h)
    g, pl = _plane_graph(9)
    m = P.Map(g, 6 * w * h)
    frames = []

    def add(seq, seg, T, polys, ids, depth_thre=10.0):
        nv = pp.run(seg, T, polys, step=step, depth_thre=depth_thre, ceiling_thre=2.5)
        _, cloud, _, pid = pp.download()
        want = [split_frame(cloud, pid, k) for k in range(len(ids))]
        counts = m.add_frame(pp, seq, ids)
        np.testing.assert_array_equal(counts, [len(want[k]) if ids[k] >= 0 else 0 for k in range(len(ids))])
        if all(i >= 0 for i in ids) and len(ids) == len(seg) + 1:
            assert int(counts.sum()) == nv
        frames.append((seq, list(ids), want))
        return counts

    seg, polys, T = synth.corridor_frame(_pose(0), width=w, height=h, K=K)
    c = add(3, seg, T, polys, pl[:4])
    assert np.all(c > 0)                                                 # ground and three walls, all seen
    if step == 2:
        _, cloud, _, pid = pp.download()
        odd = (np.arange(w)[None, :] % 2 == 1) | (np.arange(h)[:, None] % 2 == 1)
        assert np.all(pid[odd] == -1)                                    # (the chunks hold even pixels only)
    seg, polys, T = synth.corridor_frame(_pose(1), width=w, height=h, K=K)
    c = add(4, seg, T, polys, [pl[0], -1, pl[2], pl[3]])                 # a plane skipped by -1
    assert c[1] == 0 and len(frames[-1][2][1]) > 0                       # (it had points; they are not stored)
    seg, polys, T = synth.corridor_frame(_pose(2), width=w, height=h, K=K)
    polys = list(polys); polys[2] = np.zeros((0, 2), np.float32)
    c = add(6, seg, T, polys, pl[:4])                                    # a polygon list that leaves plane 2 empty: an empty chunk
    assert c[2] == 0 and c[1] > 0 and c[3] > 0
    seg, polys, T = synth.corridor_frame(_pose(3), width=w, height=h, K=K)
    c = add(7, seg, T, polys, pl[:4], depth_thre=0.0)                    # no valid point at all: four empty chunks
    assert not c.any()
    fr = pipeline.popup_sequence(n_frames=3, seed=7, width=w, height=h, K=K)[2]      # the frame loop's generator: 3 to 7 walls
    T = synth.T_from_pose(fr.true_pose).astype(np.float32)
    c = add(9, fr.seg2d, T, fr.polys, pl[:len(fr.seg2d) + 1])
    assert c[0] > 0 and c[1:].sum() > 0
    _check_store(m, frames)
    sec = m.last_times()
    assert 0.0 < sec[0] < 0.1 and sec[1] == 0.0


def test_capacity_is_a_hard_limit(built):
    w, h = 160, 120
    pp, K = _popup(w, h)
    g, pl = _plane_graph(4)
    views = [synth.corridor_frame(_pose(k), width=w, height=h, K=K) for k in range(3)]
    kept = []
    for seg, polys, T in views:
        kept.append(pp.run(seg, T, polys, step=1))
    assert all(k > 0 for k in kept)
    m = P.Map(g, kept[0] + kept[1])                                      # room for two frames, to the point
    frames = []
    for k, (seg, polys, T) in enumerate(views[:2]):
        pp.run(seg, T, polys, step=1)
        _, cloud, _, pid = pp.download()
        m.add_frame(pp, k, pl)
        frames.append((k, pl, [split_frame(cloud, pid, j) for j in range(4)]))
    before = (m.info(), m.chunks(), m.download(0))
    seg, polys, T = views[2]
    pp.run(seg, T, polys, step=1)
    with pytest.raises(P.PpsError) as e:
        m.add_frame(pp, 2, pl)
    assert e.value.code == P.PPS_ENOMEM
    assert m.info() == before[0]
    np.testing.assert_array_equal(m.chunks(), before[1])
    np.testing.assert_array_equal(raw16(m.download(0)), raw16(before[2]))
    _check_store(m, frames)
    # still usable: a frame that keeps nothing fits a full store
    pp.run(seg, T, polys, step=1, depth_thre=0.0)
    assert not m.add_frame(pp, 2, pl).any()
    assert m.info()["n_frames"] == 3 and m.info()["n_chunks"] == 12 and m.info()["n_points"] == kept[0] + kept[1]


def _world(n_frames=12, w=160, h=120):
    """a solved small_world graph of n_frames poses and a store of as many frames; frame plane 0 is the ground landmark, the three walls
    of a frame go to wall landmarks in rotation, one landmark is seen in a single frame"""
    spec = synth.small_world(n_frames, 6, seed=3)
    g = P.Graph(); spec.replay(g)
    g.batch_optimize()
    pl = [i for i, t in enumerate(spec.node_type) if t == synth.NODE_PLANE]
    assert len(pl) == 6
    pp, K = _popup(w, h, seed=5)
    m = P.Map(g, n_frames * w * h)
    for f in range(n_frames):
        seg, polys, T = synth.corridor_frame(_pose(f), width=w, height=h, K=K)
        pp.run(seg, T, polys, step=1 + f % 2)
        walls = [pl[1 + (f + j) % 3] for j in range(3)]
        if f == 2:
            walls[0] = pl[4]                                             # tracked once
        if f % 4 == 1:
            walls[1] = pl[5]                                             # tracked three times
        m.add_frame(pp, f, [pl[0]] + walls)
    return g, m, pl


def _expected_build(g, m, table):
    """the chunks of `table` (rows of the store's chunk table) through pps_reproject_points, back to back"""
    store = m.download(0)
    pts = np.concatenate([store[c["offset"]:c["offset"] + c["count"]] for c in table]) if len(table) else store[:0]
    ids = np.concatenate([np.full(c["count"], c["plane_id"], dtype=np.int32) for c in table]) if len(table) else np.zeros(0, np.int32)
    return pts, ids, g.reproject_points(ids, xyz_of(pts))


def _check_build(g, m, table):
    """the built map against both references; returns (raw points, landmark id per point, built points)"""
    pts, ids, want = _expected_build(g, m, table)
    got = m.download(1)
    assert len(got) == len(pts) == m.info()["built_points"]
    np.testing.assert_array_equal(xyz_of(got).view(np.uint32), want.view(np.uint32))         # bit-identical to pps_reproject_points
    np.testing.assert_array_equal(got["rgba"], pts["rgba"])
    for lm in np.unique(ids):
        s = ids == lm
        try:
            plane = g.get_plane(int(lm))
        except P.PpsError:
            np.testing.assert_array_equal(raw16(got[s]), raw16(pts[s]))                      # a landmark that is gone: untouched
            continue
        assert_within_one_ulp(xyz_of(got[s]), project_to_plane(plane, xyz_of(pts[s])))
    bt = m.built_chunks()
    assert len(bt) == len(table)
    np.testing.assert_array_equal(bt["count"], table["count"])
    np.testing.assert_array_equal(bt["offset"], np.concatenate([[0], np.cumsum(table["count"])[:-1]]) if len(table) else [])
    for name in ("frame", "frame_seq_id", "frame_plane", "plane_id"):
        np.testing.assert_array_equal(bt[name], table[name])
    return pts, ids, got


def test_build_projects_the_raw_points_onto_the_current_estimate(built):
    g, m, pl = _world()
    store0 = m.download(0).copy()
    assert m.build() == (m.info()["n_points"], m.info()["n_chunks"])
    pts, ids, b1 = _check_build(g, m, m.chunks())
    assert np.any(xyz_of(b1) != xyz_of(pts))                             # (the projection moved points: the check is not vacuous)
    np.testing.assert_array_equal(raw16(m.download(0)), raw16(store0))   # the store is not modified
    # further optimisation: a prior pulls one wall landmark to another plane; the second build projects the RAW points onto it
    old = g.get_plane(pl[1])
    new = old + np.array([0.2, 0.1, 0.0, 0.3]); new /= np.linalg.norm(new)
    g.add_plane_prior(pl[1], new, synth._ut_diag([300.0] * 3))
    g.batch_optimize()
    assert np.abs(g.get_plane(pl[1]) - old).max() > 0.05
    m.build()
    _, _, b2 = _check_build(g, m, m.chunks())
    s = ids == pl[1]
    twice = g.reproject_points(ids[s], xyz_of(b1[s]))                    # what projecting the first build's output would have given
    assert np.abs(twice - xyz_of(b2[s])).max() > 1e-3
    np.testing.assert_array_equal(raw16(m.download(0)), raw16(store0))
    assert m.last_times()[1] > 0.0


def test_selection_and_merge(built):
    g, m, pl = _world()
    t = m.chunks()
    sel = P.map_select(11)                                               # published at the last frame: gates at frames 7, 3 and 1
    keep = P.map_select_host(t, sel)
    assert 0 < keep.sum() < len(t)
    assert not keep[t["plane_id"] == pl[4]].any()                        # tracked once, frame 2 <= 11 - 4: dropped by the tracking gate
    assert m.build(sel) == (int(t["count"][keep].sum()), int(keep.sum()))
    _check_build(g, m, t[keep])
    # loopclose_merge: landmark b is merged into a (its node leaves the graph), landmark c leaves without a successor
    a, b, c = pl[1], pl[2], pl[5]
    na, nb = int((t["plane_id"] == a).sum()), int((t["plane_id"] == b).sum())
    assert na > 0 and nb > 0 and (t["plane_id"] == c).sum() == 3
    m.redirect(b, a)
    g.remove_node(b)
    g.remove_node(c)
    t2 = m.chunks()
    np.testing.assert_array_equal(t2["plane_id"], np.where(t["plane_id"] == b, a, t["plane_id"]))
    for name in ("frame", "frame_seq_id", "frame_plane", "offset", "count"):
        np.testing.assert_array_equal(t2[name], t[name])
    m.build()
    pts, ids, got = _check_build(g, m, t2)
    was_b = np.concatenate([np.full(r["count"], r["plane_id"] == b) for r in t])
    assert was_b.any() and np.all(ids[was_b] == a)
    assert_within_one_ulp(xyz_of(got[was_b]), project_to_plane(g.get_plane(a), xyz_of(pts[was_b])))   # b's chunks lie on a's plane
    gone = ids == c
    assert gone.sum() > 0
    np.testing.assert_array_equal(raw16(got[gone]), raw16(pts[gone]))    # removed and not redirected: untouched
    # the tracked counts add up: a gate of na + nb observations passes a's chunks -- all na + nb of them -- and nothing else
    gate = P.map_select(11, every_frame=1, age=(-1000, -1000, -1000), min_tracked=(na + nb,) * 3)
    assert na + nb > (t2["plane_id"] == pl[0]).sum()
    keep = P.map_select_host(t2, gate)
    np.testing.assert_array_equal(keep, t2["plane_id"] == a)
    assert m.build(gate)[1] == na + nb
    _check_build(g, m, t2[keep])


def test_refusals_leave_the_map_usable(built):
    w, h = 160, 120
    pp, K = _popup(w, h)
    g, pl = _plane_graph(4)
    m = P.Map(g, 2 * w * h)
    seg, polys, T = synth.corridor_frame(_pose(0), width=w, height=h, K=K)

    def refused(fn, code):
        with pytest.raises(P.PpsError) as e:
            fn()
        assert e.value.code == code, e.value

    refused(lambda: m.add_frame(pp, 0, pl), P.PPS_ESTATE)                # no run yet
    pp.set_outputs(depth=True, plane_id=False)
    pp.run(seg, T, polys)
    refused(lambda: m.add_frame(pp, 0, pl), P.PPS_ESTATE)                # the run had the plane-id output switched off
    pp.set_outputs(depth=True, plane_id=True)
    refused(lambda: m.add_frame(pp, 0, pl), P.PPS_ESTATE)                # (what counts is the run, not the switch)
    pp.run(seg, T, polys)
    refused(lambda: m.add_frame(pp, 0, [pl[0], 0, pl[2], pl[3]]), P.PPS_EINVAL)      # node 0 is a pose
    refused(lambda: m.add_frame(pp, 0, [pl[0], 77, pl[2], pl[3]]), P.PPS_EINVAL)
    refused(lambda: m.redirect(pl[1], 77), P.PPS_EINVAL)
    assert m.info()["n_frames"] == 0 and m.build() == (0, 0)
    _, cloud, _, pid = pp.download()
    m.add_frame(pp, 0, pl)
    _check_store(m, [(0, pl, [split_frame(cloud, pid, k) for k in range(4)])])
    refused(lambda: m.download(0, 0, m.info()["n_points"] + 1), P.PPS_EINVAL)
    refused(lambda: m.download(1, 0, 1), P.PPS_EINVAL)                   # nothing built yet
    pp.run_async(seg, T, polys, step=2)                                  # a run in flight is waited for, like every reader of a run does
    m.add_frame(pp, 1, pl)
    _, cloud2, _, pid2 = pp.download()
    _check_store(m, [(0, pl, [split_frame(cloud, pid, k) for k in range(4)]), (1, pl, [split_frame(cloud2, pid2, k) for k in range(4)])])
