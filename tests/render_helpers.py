"""What tests/test_host_map_render.py and tests/test_gpu_map_render.py share: the numpy statement of the rendered view (include/pps.h:
pps_map_render), written from the header's text.  None of it calls the render code under test, the two _host entry points included: it
reads the plane equations the grid was built with, the boxes of the plane table and what pps_map_grid_download returns (the lattice
cells that were emitted, in the order of the grid map, and their colours), and computes every pixel with numpy, which rounds every product
and every sum once."""
import numpy as np

from grid_helpers import LIMIT, POINT_DTYPE

EMPTY_ID = -1


def frame_exact(abcd):
    """(l, n, e1, e2) of a plane's four doubles in the operations and the order of the grid statement (grid_helpers.frame_fp64 goes through
    np.cross, whose subtractions are ordered differently: equal to 4 ulp, not bit for bit)"""
    p = np.asarray(abcd, dtype=np.float64)
    l = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    n = np.array([p[0] / l, p[1] / l, p[2] / l])
    c = np.array([-n[1], n[0], 0.0]) if abs(n[2]) <= 0.7 else np.array([0.0, -n[2], n[1]])
    lc = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    e1 = np.array([c[0] / lc, c[1] / lc, c[2] / lc])
    e2 = np.array([n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]])
    return l, n, e1, e2


def ref_rays(col, row, invK, T_wc):
    """(o (3,), ds, dw: lists of three arrays shaped like col) of the pixels (col, row)"""
    iK = np.asarray(invK, dtype=np.float32).reshape(9).astype(np.float64)
    T = np.asarray(T_wc, dtype=np.float32).reshape(16).astype(np.float64)
    x, y = np.asarray(col).astype(np.float64), np.asarray(row).astype(np.float64)
    with np.errstate(all="ignore"):
        ds = [(iK[3 * k] * x + iK[3 * k + 1] * y) + iK[3 * k + 2] for k in range(3)]
        dw = [(T[4 * k] * ds[0] + T[4 * k + 1] * ds[1]) + T[4 * k + 2] * ds[2] for k in range(3)]
    return np.array([T[3], T[7], T[11]]), ds, dw


def _cell(xf, e, inv_cell):
    """grid statement: floor(((x*e0 + y*e1) + z*e2) * inv_cell) of fp32 coordinates, and the kept flag"""
    x, y, z = (v.astype(np.float64) for v in xf)
    with np.errstate(all="ignore"):
        u = (x * e[0] + y * e[1]) + z * e[2]
        t = np.floor(u * inv_cell)
        ok = np.isfinite(u) & (np.abs(t) < LIMIT)
    return np.where(ok, t, 0.0).astype(np.int64), ok


def ref_hit(o, ds, dw, abcd, inv_cell, z_near=0.0, z_far=np.inf):
    """one landmark against the rays (arrays of any one shape): (hit flag, z fp64, Xf: three fp32 arrays, i, j int64)"""
    l, n, e1, e2 = frame_exact(abcd)
    p = np.asarray(abcd, dtype=np.float64)
    with np.errstate(all="ignore"):
        dn = p[3] / l
        den = (n[0] * dw[0] + n[1] * dw[1]) + n[2] * dw[2]
        h = ((n[0] * o[0] + n[1] * o[1]) + n[2] * o[2]) + dn
        ok = (den != 0.0) & np.isfinite(den)
        t = (-h) / den
        ok = ok & (t > 0.0)
        z = t * ds[2]
        ok = ok & (z >= z_near) & (z <= z_far)
        xf = [(o[k] + t * dw[k]).astype(np.float32) for k in range(3)]
        ok = ok & np.isfinite(xf[0]) & np.isfinite(xf[1]) & np.isfinite(xf[2])
    i, oki = _cell(xf, e1, inv_cell)
    j, okj = _cell(xf, e2, inv_cell)
    return ok & oki & okj, z, xf, i, j


def ring_order(reach):
    """the (di, dj) a cell lookup visits, in order"""
    return [(di, dj) for k in range(reach + 1) for dj in range(-k, k + 1) for di in range(-k, k + 1) if max(abs(di), abs(dj)) == k]


def slot_boxes(planes, grid_ij):
    """per row of the plane table its box as an (nj, ni) int64 array: the index of the cell in the grid map, -1 where none was emitted"""
    boxes = []
    for p in planes:
        box = np.full((int(p["nj"]), int(p["ni"])), -1, dtype=np.int64)
        a, k = int(p["offset"]), int(p["count"])
        ij = np.asarray(grid_ij[a:a + k], dtype=np.int64).reshape(-1, 2)
        box[ij[:, 1] - int(p["j0"]), ij[:, 0] - int(p["i0"])] = np.arange(a, a + k)
        boxes.append(box)
    return boxes


def ref_render(width, height, invK, T_wc, planes, plane_eq, inv_cell, grid_pts, grid_ij, reach=1, z_near=0.0, z_far=np.inf):
    """The statement.  planes: rows with plane_id, i0, j0, ni, nj, offset, count (grid_planes); plane_eq: (rows, 4); grid_pts, grid_ij:
    the grid map.  -> dict(cloud, depth, plane_id, cell: (height, width); n_hit)"""
    row, col = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    o, ds, dw = ref_rays(col, row, invK, T_wc)
    shape = (height, width)
    has = np.zeros(shape, dtype=bool)
    best_z = np.zeros(shape)
    cloud = np.zeros(shape, dtype=POINT_DTYPE)
    pid = np.full(shape, EMPTY_ID, dtype=np.int32)
    cell = np.full(shape, -1, dtype=np.int64)
    boxes = slot_boxes(planes, grid_ij)
    order = ring_order(reach)
    for r, p in enumerate(planes):
        ni, nj = int(p["ni"]), int(p["nj"])
        if ni * nj == 0:
            continue
        ok, z, xf, i, j = ref_hit(o, ds, dw, plane_eq[r], inv_cell, z_near, z_far)
        ri, rj = i - int(p["i0"]), j - int(p["j0"])
        ans = np.full(shape, -1, dtype=np.int64)
        for di, dj in order:
            ci, cj = ri + di, rj + dj
            ask = ok & (ans < 0) & (ci >= 0) & (ci < ni) & (cj >= 0) & (cj < nj)
            ans[ask] = boxes[r][cj[ask], ci[ask]]
        with np.errstate(invalid="ignore"):
            win = (ans >= 0) & (~has | (z < best_z))                     # among equal z the earlier row keeps the pixel
        has |= win
        best_z[win] = z[win]
        for k, name in enumerate("xyz"):
            cloud[name][win] = xf[k][win]
        cloud["rgba"][win] = grid_pts["rgba"][ans[win]]
        pid[win] = int(p["plane_id"])
        cell[win] = ans[win]
    depth = np.where(has, best_z, 0.0).astype(np.float32)
    return dict(cloud=cloud, depth=depth, plane_id=pid, cell=cell, n_hit=int(has.sum()))


def assert_view_equal(got, want):
    """every pixel of the four images, exactly (the cloud as raw 16-byte records), and the hit count"""
    np.testing.assert_array_equal(got["plane_id"], want["plane_id"])
    np.testing.assert_array_equal(got["cell"], want["cell"])
    np.testing.assert_array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1, 16)
    np.testing.assert_array_equal(raw(got["cloud"]), raw(want["cloud"]))
    assert got["n_hit"] == want["n_hit"] == int(np.count_nonzero(want["plane_id"] >= 0))


# ---- cameras -------------------------------------------------------------------------------------------------------------------------
def pinhole_invK(width, height, f=None):
    """inverse of K = [[f, 0, cx], [0, f, cy], [0, 0, 1]] as fp32"""
    f = float(f if f is not None else 0.8 * width)
    cx, cy = 0.5 * (width - 1), 0.5 * (height - 1)
    return np.array([[1 / f, 0, -cx / f], [0, 1 / f, -cy / f], [0, 0, 1]], dtype=np.float32)


def rot_xyz(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(R, t):
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T.astype(np.float32)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """sensor -> world with the optical axis (sensor z) from eye to target, sensor y pointing down"""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    zc = target - eye; zc /= np.linalg.norm(zc)
    xc = np.cross(zc, up); xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    return pose(np.stack([xc, yc, zc], axis=1), eye)
