"""What tests/test_host_map_grid.py and tests/test_gpu_map_grid.py share: the numpy statement of the grid map (include/pps.h:
pps_map_build_grid), an fp64 frame of a plane, and the flat frames the kernels are fed.  None of it calls the grid code under test: the
statement reads the map pps_map_build wrote (Map.download(1), Map.built_chunks()), the ids of the live plane nodes, the frames the library
published (grid_planes) and its inv_cell (grid_info), so it computes with the library's own doubles."""
import numpy as np

POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
PLANE_DTYPE = np.dtype([("plane_id", "<i4"), ("n_chunks", "<i4"), ("i0", "<i4"), ("j0", "<i4"), ("ni", "<i4"), ("nj", "<i4"),
                        ("offset", "<i8"), ("count", "<i8"), ("n_in", "<i8"), ("n", "<f8", 3), ("e1", "<f8", 3), ("e2", "<f8", 3)])
NEWEST, OLDEST = 0, 1
LIMIT = 2.0 ** 30
VALID = np.uint32(1 << 24)


def frame_fp64(abcd):
    """n, e1, e2 of a plane (a, b, c, d): n = abc / |abc|; a = z if |n_z| <= 0.7 else x; e1 = (a x n) / |a x n|; e2 = n x e1"""
    p = np.asarray(abcd, dtype=np.float64)
    n = p[:3] / np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    a = np.array([0.0, 0.0, 1.0]) if abs(n[2]) <= 0.7 else np.array([1.0, 0.0, 0.0])
    c = np.cross(a, n)
    e1 = c / np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    return n, e1, np.cross(n, e1)


def cell_index(pts, e, inv_cell):
    """(floor(((x*e0 + y*e1) + z*e2) * inv_cell) as int64 (0 where dropped), kept flag) of fp32 points along the axis e: numpy rounds every
    product and every sum once"""
    x, y, z = (pts[k].astype(np.float64) for k in "xyz")
    with np.errstate(all="ignore"):
        u = (x * e[0] + y * e[1]) + z * e[2]
        t = np.floor(u * inv_cell)
        ok = np.isfinite(u) & (np.abs(t) < LIMIT)
    return np.where(ok, t, 0.0).astype(np.int64), ok


def ref_grid(B, built_chunks, live_ids, frames, inv_cell, rule=NEWEST, min_count=1):
    """The statement.  B: the built map; built_chunks: its chunk table; live_ids: ids of the live plane nodes; frames: rows with plane_id,
    e1, e2 (and n, copied through).  -> dict(planes, pts, counts, ij, src, totals)"""
    B = np.ascontiguousarray(B)
    pid = np.repeat(built_chunks["plane_id"], built_chunks["count"]).astype(np.int64)
    assert len(pid) == len(B)
    live = np.isin(pid, np.asarray(live_ids, dtype=np.int64))
    ids = sorted(set(int(c["plane_id"]) for c in built_chunks if int(c["plane_id"]) in set(int(v) for v in live_ids)))
    by_id = {int(f["plane_id"]): f for f in frames}
    planes = np.zeros(len(ids), dtype=PLANE_DTYPE)
    out = dict(pts=[], counts=[], ij=[], src=[])
    n_cells = n_in_all = n_dropped = 0
    for r, lm in enumerate(ids):
        f = by_id[lm]
        row = planes[r]
        row["plane_id"] = lm
        row["n_chunks"] = int(np.count_nonzero(built_chunks["plane_id"] == lm))
        row["n"], row["e1"], row["e2"] = f["n"], f["e1"], f["e2"]
        idx = np.flatnonzero(pid == lm)
        i, oki = cell_index(B[idx], f["e1"], inv_cell)
        j, okj = cell_index(B[idx], f["e2"], inv_cell)
        ok = oki & okj
        n_dropped += int(np.count_nonzero(~ok))
        idx, i, j = idx[ok], i[ok], j[ok]
        row["n_in"] = len(idx); n_in_all += len(idx)
        row["offset"] = n_cells
        if len(idx) == 0:
            continue
        row["i0"], row["j0"] = i.min(), j.min()
        row["ni"], row["nj"] = i.max() - i.min() + 1, j.max() - j.min() + 1
        cell = (j - j.min()) * int(row["ni"]) + (i - i.min())           # raster order of the box: j ascending, then i
        order = np.lexsort((idx, cell))                                  # by cell, inside a cell by index in B
        cell_s, idx_s = cell[order], idx[order]
        first = np.flatnonzero(np.concatenate([[True], cell_s[1:] != cell_s[:-1]]))
        last = np.concatenate([first[1:], [len(cell_s)]]) - 1
        count = last - first + 1
        win = idx_s[last] if rule == NEWEST else idx_s[first]
        emit = count >= min_count
        c = cell_s[first][emit]
        out["pts"].append(B[win[emit]]); out["counts"].append(count[emit].astype(np.uint32)); out["src"].append(win[emit].astype(np.int64))
        out["ij"].append(np.stack([c % int(row["ni"]) + i.min(), c // int(row["ni"]) + j.min()], axis=1).astype(np.int32))
        row["count"] = int(emit.sum()); n_cells += int(emit.sum())
    cat = lambda k, empty: np.concatenate(out[k]) if out[k] else empty
    totals = dict(n_points=len(B), n_cells=n_cells, n_in=n_in_all, n_dropped=n_dropped, n_passed_through=int(np.count_nonzero(~live)),
                  n_planes=len(ids))
    return dict(planes=planes, pts=cat("pts", B[:0]), counts=cat("counts", np.zeros(0, np.uint32)),
                ij=cat("ij", np.zeros((0, 2), np.int32)), src=cat("src", np.zeros(0, np.int64)), totals=totals)


# ---- flat frames ---------------------------------------------------------------------------------------------------------------------
def points(xyz, rng=None):
    """records from (n, 3) coordinates: every valid bit set, random colours"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    pts = np.zeros(len(xyz), dtype=POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0].astype(np.float32), xyz[:, 1].astype(np.float32), xyz[:, 2].astype(np.float32)
    pts["rgba"] = (rng.integers(0, 1 << 24, size=len(xyz), dtype=np.uint32) if rng is not None else np.arange(len(xyz), dtype=np.uint32)) | VALID
    return pts


def on_plane(abcd, uv, lift=0.0):
    """world points at plane coordinates uv (n, 2) of the frame frame_fp64 gives, lifted off the plane by `lift` metres along n (the
    projection takes that away again)"""
    n, e1, e2 = frame_fp64(abcd)
    foot = -abcd[3] / np.linalg.norm(abcd[:3]) * n                       # the foot of the origin: n . x = -d / |abc|
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    return foot + uv[:, :1] * e1 + uv[:, 1:] * e2 + np.reshape(lift, (-1, 1)) * n


def scan_frame(rng, abcds, width, height, origin, pitch, p_valid=0.9, noise=0.01):
    """flat frame of width x height pixels over len(abcds) planes: the rows are cut into equal bands, band k shows plane k; a pixel's point
    lies at plane coordinates origin + (column, row) * pitch, a little off the plane -- neighbouring pixels fall into the same or adjacent
    cells, like a camera's.  Some pixels are invalid, some carry no plane."""
    npx = width * height
    col, row = np.arange(npx) % width, np.arange(npx) // width
    band = np.minimum(row * len(abcds) // height, len(abcds) - 1)
    uv = np.stack([origin[0] + col * pitch, origin[1] + row * pitch], axis=1)
    xyz = np.zeros((npx, 3))
    for k, abcd in enumerate(abcds):
        s = band == k
        xyz[s] = on_plane(np.asarray(abcd, dtype=np.float64), uv[s], rng.normal(size=int(s.sum())) * noise)
    cloud = points(xyz, rng)
    pid = band.astype(np.int32)
    pid[rng.random(npx) < 0.03] = -1
    invalid = rng.random(npx) >= p_valid
    cloud["rgba"][invalid] &= np.uint32(0x00FFFFFF)
    return cloud, pid


def one_point_frame(rng, n_slots, spread=2.0):
    """n_slots pixels, pixel k the only point of frame plane k: chunks of one point"""
    return points(rng.normal(size=(n_slots, 3)) * spread, rng), np.arange(n_slots, dtype=np.int32)
