"""What tests/test_host_map_compare.py and tests/test_gpu_map_compare.py share: the numpy statement of the compared views (include/pps.h:
pps_map_compare), written from the header's text.  None of it calls the compare code under test, pps_map_compare_point_host included:
it reads the view's plane-id image (render_download), the plane table (grid_planes) and the plane equations the grid was built with
(grid_plane_eq), and computes every pixel with numpy, which rounds every product and every sum once.  All outputs are integers."""
import numpy as np

import pop_up_slam_amd as P
from render_helpers import frame_exact

Q_MAX = 524288
TOTAL_KEYS = ("width", "height", "nplanes", "n_rows", "n_both", "n_frame_only", "n_view_only", "n_neither", "n_bad_id", "n_pairs")


def ref_point(abcd, x, y, z, tol):
    """fp32 coordinates (arrays of one shape) against one plane -> (agree bool, e fp64, q int64)"""
    l, n, _, _ = frame_exact(abcd)
    x, y, z = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (x, y, z))
    with np.errstate(all="ignore"):
        dn = np.float64(abcd[3]) / l
        e = ((n[0] * x + n[1] * y) + n[2] * z) + dn
        agree = np.abs(e) <= tol                                         # (a NaN fails)
        s = e * 4096.0
        top = np.isnan(s) | (s >= Q_MAX)
        bottom = ~top & (s <= -Q_MAX)
        q = np.where(top, Q_MAX, np.where(bottom, -Q_MAX, np.rint(np.where(top | bottom, 0.0, s)))).astype(np.int64)
    return agree, e, q


def sides(view_id, plane_ids, cloud, frame_id, nplanes):
    """per pixel: k (nplanes: no frame), r (n_rows: no view), the bad-id flag"""
    kf = np.asarray(frame_id, dtype=np.int64).reshape(-1)
    valid_bit = ((np.asarray(cloud["rgba"]).reshape(-1) >> np.uint32(24)) & np.uint32(1)) == 1
    in_range = (kf >= 0) & (kf < nplanes)
    k = np.where(in_range & valid_bit, kf, nplanes)
    bad = ~in_range & (kf != -1)
    vid = np.asarray(view_id, dtype=np.int64).reshape(-1)
    ids = np.asarray(plane_ids, dtype=np.int64)
    n_rows = len(ids)
    r = np.full(len(vid), n_rows, dtype=np.int64)
    for row, node in enumerate(ids):
        r[vid == node] = row
    assert np.all((r < n_rows) | (vid == -1)), "the view shows a plane id the plane table does not have"
    return k, r, bad


def ref_compare(view_id, planes, plane_eq, cloud, frame_id, nplanes, tol):
    """The statement.  view_id: the plane-id image of render_download; planes: grid_planes(); plane_eq: grid_plane_eq(); cloud
    (POINT_DTYPE) and frame_id: the frame, one record per pixel.  -> dict(planes, rows, pairs: structured arrays; totals: dict)"""
    view_id = np.asarray(view_id)
    height, width = view_id.shape
    cloud = np.asarray(cloud).reshape(-1)
    n_rows = len(planes)
    k, r, bad = sides(view_id, planes["plane_id"], cloud, frame_id, nplanes)
    assert len(k) == len(cloud) == width * height
    n = np.zeros((nplanes + 1, n_rows + 1), dtype=np.int64)
    ag, sq, sq2 = np.zeros_like(n), np.zeros_like(n), np.zeros_like(n)
    np.add.at(n, (k, r), 1)
    for row in range(n_rows):
        px = (r == row) & (k < nplanes)
        if not px.any():
            continue
        agree, _, q = ref_point(plane_eq[row], cloud["x"][px], cloud["y"][px], cloud["z"][px], tol)
        np.add.at(ag[:, row], k[px], agree.astype(np.int64))
        np.add.at(sq[:, row], k[px], q)
        np.add.at(sq2[:, row], k[px], q * q)
    rec = np.zeros(nplanes, dtype=P.MAP_COMPARE_PLANE_DTYPE)
    pairs = []
    for f in range(nplanes):
        rec["n_valid"][f], rec["n_new"][f] = n[f].sum(), n[f, n_rows]
        best = -1
        for row in range(n_rows):
            if ag[f, row] >= 1 and (best < 0 or (ag[f, row], n[f, row]) > (ag[f, best], n[f, best])):
                best = row
            if n[f, row] >= 1:
                pairs.append((f, row, int(planes["plane_id"][row]), 0, n[f, row], ag[f, row], sq[f, row], sq2[f, row]))
        rec["best_row"][f] = best
        rec["best_plane_id"][f] = planes["plane_id"][best] if best >= 0 else -1
        rec["best_n"][f], rec["best_agree"][f] = (n[f, best], ag[f, best]) if best >= 0 else (0, 0)
    rows = np.zeros(n_rows, dtype=P.MAP_COMPARE_ROW_DTYPE)
    rows["n_view"], rows["n_unseen"] = n[:, :n_rows].sum(axis=0), n[nplanes, :n_rows]
    totals = dict(width=width, height=height, nplanes=nplanes, n_rows=n_rows, n_both=int(n[:nplanes, :n_rows].sum()),
                  n_frame_only=int(n[:nplanes, n_rows].sum()), n_view_only=int(n[nplanes, :n_rows].sum()), n_neither=int(n[nplanes, n_rows]),
                  n_bad_id=int(bad.sum()), n_pairs=len(pairs))
    assert totals["n_both"] + totals["n_frame_only"] + totals["n_view_only"] + totals["n_neither"] == width * height
    return dict(planes=rec, rows=rows, pairs=np.array(pairs, dtype=P.MAP_COMPARE_PAIR_DTYPE).reshape(-1), totals=totals)


def assert_compare_equal(got, want):
    """every field of every output, exactly"""
    for name in ("planes", "rows", "pairs"):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        for f in want[name].dtype.names:
            np.testing.assert_array_equal(got[name][f], want[name][f], err_msg=f"{name}.{f}")
    assert {k: got["totals"][k] for k in TOTAL_KEYS} == want["totals"]
    t = want["totals"]
    assert t["n_both"] + t["n_frame_only"] + t["n_view_only"] + t["n_neither"] == t["width"] * t["height"]


def read_compare(m, plane_records):
    """every output of the last comparison of map m, as ref_compare returns them"""
    return dict(planes=plane_records, rows=m.compare_rows(), pairs=m.compare_pairs(), totals=m.compare_info())


# ---- made-up frames ------------------------------------------------------------------------------------------------------------------
VALID = np.uint32(1 << 24)


def rows_of(view_id, planes):
    """per pixel the row of the plane table the view shows, -1 where it shows none"""
    r = np.full(np.shape(view_id), -1, dtype=np.int64)
    for row, node in enumerate(planes["plane_id"]):
        r[np.asarray(view_id) == node] = row
    return r


def shifted(cloud, r, plane_eq, offset, rgba=0x01c0ffee):
    """a frame cloud: every point of `cloud` whose pixel shows row r >= 0 moved by `offset` metres (per pixel) along that row's normal,
    in fp64 and cast once; the valid bit set everywhere"""
    out = np.zeros(np.shape(cloud), dtype=P.POINT_DTYPE)
    xyz = np.stack([np.asarray(cloud[k], dtype=np.float64) for k in "xyz"], axis=-1)
    off = np.broadcast_to(np.asarray(offset, dtype=np.float64), np.shape(cloud))
    for row in range(len(plane_eq)):
        n = frame_exact(plane_eq[row])[1]
        at = np.asarray(r) == row
        xyz[at] += off[at][:, None] * n
    for i, k in enumerate("xyz"):
        out[k] = xyz[..., i].astype(np.float32)
    out["rgba"] = np.uint32(rgba) | VALID
    return out


def made_up_view(rng, r, planes, plane_eq, spread=3.0):
    """a view nobody rendered: the plane-id image of the rows r (-1: none) and a point on the shown plane for every pixel"""
    r = np.asarray(r, dtype=np.int64)
    ids = np.append(np.asarray(planes["plane_id"], dtype=np.int64), -1)  # (r = -1 reads the last entry)
    view_id = ids[r].astype(np.int32)
    cloud = np.zeros(r.shape, dtype=P.POINT_DTYPE)
    xyz = rng.uniform(-spread, spread, size=r.shape + (3,))
    for row in range(len(plane_eq)):
        l, n, e1, e2 = frame_exact(plane_eq[row])
        at = r == row
        uv = rng.uniform(-spread, spread, size=(int(at.sum()), 2))
        xyz[at] = -(plane_eq[row][3] / l) * n + uv[:, :1] * e1 + uv[:, 1:] * e2
    for i, k in enumerate("xyz"):
        cloud[k] = xyz[..., i].astype(np.float32)
    return view_id, cloud


def plane_table(ids):
    """a plane table as grid_planes returns it, of which the comparison reads the ids alone"""
    t = np.zeros(len(ids), dtype=P.GRID_PLANE_DTYPE)
    t["plane_id"] = ids
    return t


def mixed_frame(rng, on, r, plane_eq, nplanes, tol, junk=True):
    """a frame for the view (on: a point on the shown plane per pixel, r: the shown row or -1) with pixels of all four classes, distances
    on both sides of tol and far beyond it, and (junk) plane ids and points of no use -> (cloud, frame ids)"""
    shape = np.shape(r)
    off = rng.choice([0.0, 0.4, 0.9, 1.1, -0.9, -1.1, 3.0, -40.0, 700.0, -1500.0], size=shape) * rng.uniform(0.95, 1.05, size=shape) * tol
    cloud = shifted(on, r, plane_eq, off)
    fid = rng.integers(-1, nplanes, size=shape).astype(np.int32)
    if junk:
        npx = fid.size
        flat_id, flat_c = fid.reshape(-1), cloud.reshape(-1)
        pick = rng.permutation(npx)
        for i, bad in zip(pick[:6], (-2, nplanes, 2 ** 31 - 1, -2 ** 31, nplanes + 7, -100)):
            flat_id[i] = bad
        flat_c["rgba"][pick[6:6 + max(2, npx // 10)]] &= ~VALID          # the valid bit clear, whatever the id says
        for i, v in zip(pick[-6:], (np.inf, -np.inf, np.nan, 1e30, -1e30, 3e38)):
            flat_c["z"][i] = v; flat_c["rgba"][i] |= VALID
    return cloud, fid


# per (frame plane, row): (pixels that agree, pixels that do not).  The best landmark of plane 0 is decided by n_agree, of plane 1 by n,
# of plane 2 by the row; plane 3 agrees nowhere.
TIES_PLAN = {(0, 0): (3, 5), (0, 1): (4, 0), (0, 2): (2, 9), (1, 0): (3, 0), (1, 1): (3, 2), (1, 2): (3, 1), (2, 0): (1, 4), (2, 1): (2, 2),
             (2, 2): (2, 2), (3, 0): (0, 3), (3, 2): (0, 2)}


def ties_frame(rng, on, r, plane_eq, tol):
    """a frame for a view of three rows (at least 20 pixels each) after TIES_PLAN; every other pixel has no frame -> (cloud, frame ids)"""
    r = np.asarray(r)
    fid = np.full(r.shape, -1, dtype=np.int32)
    off = np.zeros(r.shape)
    free = {row: list(rng.permutation(np.flatnonzero(r.reshape(-1) == row))) for row in range(3)}
    for (k, row), (a, d) in TIES_PLAN.items():
        for j in range(a + d):
            i = free[row].pop()
            fid.reshape(-1)[i] = k
            off.reshape(-1)[i] = (0.5 if j < a else 3.0) * tol
    return shifted(on, r, plane_eq, off), fid


def check_ties(want, plane_ids):
    assert want["planes"]["best_row"].tolist() == [1, 1, 1, -1] and want["planes"]["best_plane_id"].tolist() == [plane_ids[1]] * 3 + [-1]
    assert want["planes"]["best_agree"].tolist() == [4, 3, 2, 0] and want["planes"]["best_n"].tolist() == [4, 5, 4, 0]
    assert want["planes"]["n_valid"][3] == 5 and want["planes"]["n_new"][3] == 0
