"""GPU: the four builds of the dense map (pps_map_build, pps_map_build_posed, pps_map_build_grid, pps_map_build_grid_posed) called one
after another on ONE handle, so that every call meets the buffers, the selection tables and the results the calls before it left: a small
selection after a large one, a table layout after another, buffers that have to grow between two calls.

After every call everything the handle answers is compared with the statements in numpy, as raw bytes: the selection is
map_helpers.ref_select, a point of the built map map_posed_helpers.move_points in fp64 cast to fp32 once (with no motion that is
Plane3d::project_to_plane in the order of csrc/pps_project.h), a motion map_posed_helpers.motion, the grid grid_helpers.ref_grid over that
map.  numpy rounds every product and every sum once, which is what the library's files, compiled without contraction, do.  A fresh handle
of the code under test is not the reference anywhere."""
import numpy as np
import pytest

import pop_up_slam_amd as P
import map_posed_helpers as H
from grid_helpers import NEWEST, ref_grid, scan_frame
from map_helpers import raw16, ref_select, xyz_of
from test_gpu_map_posed import _graph, _poses

pytestmark = pytest.mark.gpu

PLANES = [[0.0, 0.0, -1.0, 0.2], [0.6, -0.8, 0.0, 0.7], [1.0, 0.0, 0.0, -2.0], [0.0, 2.0, 0.0, 1.0]]
# (width, height, frame planes): 1, 63, 64, 65, 257 and 300 pixels -- below, at and above a wave, above a workgroup -- in 12 chunks
FRAMES = [(1, 1, 1), (9, 7, 2), (8, 8, 3), (13, 5, 3), (257, 1, 1), (20, 15, 2)]
LATER = [(20, 15, 2), (15, 20, 2)]                                      # step 7: two more frames of 300 pixels
COUNTER, CELL = 5, 0.05
GRID_KEYS = ("n_points", "n_cells", "n_in", "n_dropped", "n_passed_through", "n_planes", "launches", "cell", "inv_cell")


class _World:
    """the handle under test and what the statements say it holds"""

    def __init__(self):
        self.rng = np.random.default_rng(31)
        self.est, self.T0 = _poses(self.rng, 3)
        self.g, self.ps, self.pl = _graph(PLANES, self.est)
        self.cap = 4096
        self.m = P.Map(self.g, self.cap)
        self.n_frames = 0
        # the last plain / posed build, the last grid, the last posed call: what the calls in between must leave alone
        self.B = np.zeros(0, dtype=P.POINT_DTYPE)
        self.bt = np.zeros(0, dtype=P.CHUNK_DTYPE)
        self.grid = None
        self.motions = (np.zeros((0, 12)), np.zeros(0, dtype=np.int32))
        self.posed_launches = 0

    def add(self, width, height, k):
        f = self.n_frames
        ids = [self.pl[(f + j) % 4] for j in range(k)]
        cloud, pid = scan_frame(self.rng, [PLANES[(f + j) % 4] for j in range(k)], width, height, (-0.4 + 0.1 * f, -0.3), 0.04,
                                p_valid=1.0 if width * height == 1 else 0.9)
        self.m.debug_add_points(cloud, pid, f, ids)
        self.m.set_frame_pose(f, self.ps[f % 3], self.T0[f % 3])         # 0.3 m / 5 degrees off the estimate of its node
        self.n_frames += 1

    def keep(self, sel):
        t = self.m.chunks()
        return np.ones(len(t), dtype=bool) if sel is None else ref_select(t, COUNTER, every_frame=False)

    def statement(self, sel, posed):
        """(B, its chunk table, motion table, moved flags) of build(sel, posed) from the store, the tables and the estimate"""
        t, fr, store = self.m.chunks(), self.m.frames(), self.m.download(0)
        kept = t[self.keep(sel)]
        bt = kept.copy()
        bt["offset"] = np.cumsum(bt["count"]) - bt["count"]
        rows, out = {}, [store[:0]]
        for c in kept:
            if c["count"] == 0:
                continue
            f = int(c["frame"])
            if posed and f not in rows:
                rows[f] = H.motion(fr[f]["T_wc"], self.g.get_pose(int(fr[f]["pose_id"])))
            seg = store[int(c["offset"]):int(c["offset"] + c["count"])].copy()
            xyz = H.move_points(rows[f] if posed else None, self.g.get_plane(int(c["plane_id"])), xyz_of(seg)).astype(np.float32)
            seg["x"], seg["y"], seg["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            out.append(seg)
        D = np.array([rows[f] for f in sorted(rows)]).reshape(-1, 12)
        return np.concatenate(out), bt, D, np.ones(len(D), dtype=np.int32)

    def build(self, sel, posed):
        B, bt, D, moved = self.statement(sel, posed)
        assert self.m.build(sel, posed=posed) == (len(B), len(bt))
        self.B, self.bt = B, bt
        if posed:
            self.motions, self.posed_launches = (D, moved), 2
        self.check()

    def build_grid(self, sel, posed):
        B, bt, D, moved = self.statement(sel, posed)
        ret = self.m.build_grid(sel, cell=CELL, rule=NEWEST, posed=posed)
        info = self.m.grid_info()
        want = ref_grid(B, bt, self.pl, self.m.grid_planes(), info["inv_cell"], NEWEST, 1)
        assert ret == (want["totals"]["n_cells"], want["totals"]["n_planes"]) and want["totals"]["n_cells"] > 0
        for p in want["planes"]:                                         # the frames ref_grid copied through: the estimate's
            n, e1, e2 = P.map_grid_frame_host(self.g.get_plane(int(p["plane_id"])))
            assert (p["n"].tobytes(), p["e1"].tobytes(), p["e2"].tobytes()) == (n.tobytes(), e1.tobytes(), e2.tobytes())
        # extent, zeroing is no launch, vote, count + scan + plane_off, emit
        want["info"] = dict(want["totals"], launches=6, cell=CELL, inv_cell=1.0 / CELL)
        self.grid = want
        if posed:
            self.motions, self.posed_launches = (D, moved), 1
        self.check()

    def check(self):
        m = self.m
        assert m.info() == dict(capacity=self.cap, n_points=len(self.store), built_points=len(self.B), n_frames=self.n_frames,
                                n_chunks=len(self.chunks), built_chunks=len(self.bt))
        assert m.built_chunks().tobytes() == self.bt.tobytes()
        assert m.download(1).tobytes() == self.B.tobytes()
        D, moved = m.frame_motions()
        assert (D.tobytes(), moved.tobytes()) == (self.motions[0].tobytes(), self.motions[1].tobytes())
        last = m.posed_last()
        assert (last["launches"], last["n_unposed_frames"]) == (self.posed_launches, 0)
        info = m.grid_info()
        if self.grid is None:
            assert len(m.grid_planes()) == 0 and info["n_cells"] == 0 and info["launches"] == 0
        else:
            assert {k: info[k] for k in GRID_KEYS} == self.grid["info"]
            assert m.grid_planes().tobytes() == np.ascontiguousarray(self.grid["planes"]).tobytes()
            pts, counts, ij, src = m.grid_download()
            assert (raw16(pts).tobytes(), counts.tobytes(), ij.tobytes(), src.tobytes()) == \
                   (raw16(self.grid["pts"]).tobytes(), self.grid["counts"].tobytes(), self.grid["ij"].tobytes(), self.grid["src"].tobytes())
        assert m.download(0).tobytes() == self.store.tobytes() and m.chunks().tobytes() == self.chunks.tobytes()

    def freeze(self):
        """the store and its table as they are now: no build may change them"""
        self.store, self.chunks = self.m.download(0), self.m.chunks()


def test_the_four_builds_one_after_another_on_one_handle(built):
    w = _World()
    for width, height, k in FRAMES:
        w.add(width, height, k)
    w.freeze()
    t = w.chunks
    assert len(t) == 12 and np.all(t["count"] > 0) and t["count"][0] == 1
    A = P.map_select(COUNTER)
    keep = w.keep(A)
    np.testing.assert_array_equal(keep, P.map_select_host(t, A))
    # A: five chunks of frames 0, 2 and 4 -- an odd number of rows in the tables, so the 8-byte pad before the frame records of a posed
    # grid is there; all chunks: an even number, no pad
    assert int(keep.sum()) == 5 and sorted(set(t["frame"][keep].tolist())) == [0, 2, 4]
    w.check()                                                            # nothing built yet
    w.build(A, posed=False)                                              # 1
    w.build_grid(None, posed=True)                                       # 2
    w.build(None, posed=False)                                           # 3
    w.build(A, posed=True)                                               # 4
    w.build_grid(A, posed=False)                                         # 5
    w.build(None, posed=True)                                            # 6
    assert len(w.motions[1]) == 6 and np.max(np.abs(xyz_of(w.B) - xyz_of(w.store))) > 0.1
    for width, height, k in LATER:                                       # 7
        w.add(width, height, k)
    w.freeze()
    assert len(w.chunks) == 16 and np.all(w.chunks["count"] > 0)
    w.check()                                                            # the new frames left the built map and the grid alone
    w.build(None, posed=False)                                           # 8
    w.build(None, posed=True)
    w.build_grid(None, posed=False)
    w.build_grid(None, posed=True)
    assert len(w.motions[1]) == 8 and w.posed_launches == 1
    w.build_grid(A, posed=True)                                          # the padded layout after the unpadded one
    assert int(w.keep(A).sum()) % 2 == 1
    w.m.close(); w.g.close()
