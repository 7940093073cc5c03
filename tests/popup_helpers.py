"""Inputs and float64 references for the pop-up pixel tests (test_host_popup_ref.py, test_gpu_popup_pixels.py).  CPU only; nothing in
here is under test.

ref64 and planes64 state K5 / K6 from the geometry -- pixel ray, ray-plane intersection, rigid transform -- in float64 numpy, with no
line taken from the kernel or the C oracle; the only things shared with them are the conventions a caller sees: T maps sensor to world,
planes are (n, d) with n.p + d = 0, and a wall's normal is (G1 - G0) x (0, 0, -1) (seg_to_plane)."""
import functools

import numpy as np

from pop_up_slam_amd import synth
from oracle import numpy_raster as NR
from oracle import oracle_py as O

DEPTH_THRE, CEILING_THRE, GROUND_THRE = 10.0, 2.5, -0.2
POSE = (0.3, 0.05, 0.03)                           # yaw, pitch, roll of the generic pose
MORE_POSES = ((-0.5, -0.08, 0.06), (0.45, 0.1, -0.05), (-0.2, -0.04, -0.08))      # planes64 only: |yaw| <= 0.5, both signs of pitch / roll
HORIZON_SEG = 3                                    # the ground segment replaced by one above the horizon (plane 4: inside npl = 9 too)

# size -> the k_popup_frame instantiation a run with polygons takes (pps_popup.hip, popup_enqueue)
SIZES = {(640, 480): "<2,true>", (321, 243): "<2,true>", (258, 6): "<2,true>", (2, 2): "<2,true>",
         (642, 480): "<2,false>", (800, 601): "<2,false>", (1283, 819): "<8,false>"}
NPLS, STEPS = (9, 64), (1, 2)
# the seed is the image width, as in the random-polygon test of test_gpu_popup.py, except where that leaves a class of test_branches_are_populated
# short of pixels (258 x 6 at step 2 holds 387 pixels a run)
SEEDS = {(258, 6): 260, (2, 2): 12}     # (2 x 2: pixel (0, 0) has a depth at step 2, for k_depth_fill)
# 2 x 2 holds 4 pixels: it cannot hold 20 pixels of each of five classes, and is in the list for hw == hh == 1 of k_depth_fill alone
POPULATED = [s for s in SIZES if s != (2, 2)]
MIN_PER_CLASS = 20
CLASSES = ("behind", "far", "below", "ceiling", "kept", "below_only")

# Tolerances: 4 x the largest value measured on the CPU oracle (fp32) against ref64 / planes64 over every run of test_host_popup_ref.py;
# the measured values are listed in that module's docstring.  e = max |fp32 - ref64| / max(1, |Pw|inf) (planes: / max(1, |d|)).
E_CLOUD_MEASURED, E_DEPTH_MEASURED, E_PLANES_MEASURED = 7.21e-6, 8.41e-6, 1.69e-5
E_CLOUD, E_DEPTH, E_PLANES = 4 * E_CLOUD_MEASURED, 4 * E_DEPTH_MEASURED, 4 * E_PLANES_MEASURED
BAND_REL, BAND_MAX_FRACTION = 1e-4, 1e-3


def expected_form(w, h, nplanes):
    """restates the dispatch of popup_enqueue from the size and the number of polygons alone"""
    npx = w * h
    if npx <= 640 * 480 and nplanes > 0:
        return "<2,true>"
    return "<8,false>" if npx >= 1 << 20 else "<2,false>"


def pose_T(yaw, pitch, roll, t=(0.1, 0.3, 1.0)):
    """camera 1 m above the ground, looking along world y turned by yaw, nose down by pitch, rolled about the optical axis"""
    cp, sp, cr, sr = np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rr = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1.0]])
    T = np.eye(4)
    T[:3, :3] = synth._Rz(yaw) @ synth.CAM_R0 @ Rx @ Rr
    T[:3, 3] = t
    return T


def scene(w, h, seed, npl, pose=POSE):
    """-> dict(K float64, invK fp32, T fp32, seg (63, 4) fp32, polys: list of npl vertex arrays, bgr (h, w, 3) uint8)"""
    rng = np.random.default_rng(seed)
    K = synth.K_TUM.copy()
    K[0] *= w / 640.0; K[1] *= h / 480.0
    invK = np.linalg.inv(K).astype(np.float32)
    T = pose_T(*pose).astype(np.float32)
    seg = rng.uniform([0, 0.5 * h, 0, 0.5 * h], [w, h, w, h], size=(63, 4)).astype(np.float32)     # 63 ground segments -> 64 planes
    seg[HORIZON_SEG] = rng.uniform([0, 0.05 * h, 0, 0.05 * h], [w, 0.3 * h, w, 0.3 * h]).astype(np.float32)   # above the horizon
    polys = []
    for p in range(npl):
        n = int(rng.integers(0, 9))
        if n == 0:
            polys.append(np.zeros((0, 2), np.float32))
        elif p % 3 == 2 or min(w, h) < 4:          # (random_convex needs room for a 2-pixel radius)
            polys.append(rng.uniform([-0.2 * w, -0.2 * h], [1.2 * w, 1.2 * h], size=(n, 2)).astype(np.float32))
        else:
            polys.append(NR.random_convex(rng, w, h, max(3, n), spill=0.2))
    bgr = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return dict(K=K, invK=invK, T=T, seg=seg, polys=polys, bgr=bgr, w=w, h=h)


def ceiling_plane(T, ceiling_thre=CEILING_THRE):
    """fp32 T^T (0, 0, -1, ceiling): the operand O.popup_depth takes"""
    T = np.asarray(T, dtype=np.float32).reshape(4, 4)
    return (T.T @ np.array([0, 0, -1, ceiling_thre], np.float32)).astype(np.float32)


def _rays(K, w, h):
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    px = np.stack([x, y, np.ones_like(x)], axis=-1)
    return np.linalg.solve(np.asarray(K, dtype=np.float64), px.reshape(-1, 3).T).T.reshape(h, w, 3)


def ref64(pid, K, T, planes, depth_thre=DEPTH_THRE, ceiling_thre=CEILING_THRE):
    """K6 in float64.  pid (h, w) plane per pixel (-1: none), K 3 x 3, T 4 x 4 sensor -> world, planes (n, 4) in the sensor frame."""
    pid = np.asarray(pid); h, w = pid.shape
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    R, t = T[:3, :3], T[:3, 3]
    cls = pid >= 0
    ray = _rays(K, w, h)
    pl = planes[np.where(cls, pid, 0)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # the point on the ray s * ray with n . (s * ray) + d = 0, taken to the world
        s = -pl[..., 3] / np.einsum("hwk,hwk->hw", pl[..., :3], ray)
        Ps = s[..., None] * ray
        Pw = Ps @ R.T + t
        # the horizontal plane z_world = ceiling, seen from the sensor: (R^T n_w, n_w . t + d_w) with (n_w, d_w) = (0, 0, -1, ceiling)
        cs = T.T @ np.array([0.0, 0.0, -1.0, ceiling_thre])
        zc = (-cs[3] / (ray @ cs[:3])) * ray[..., 2]
    Psz, Pwz = Ps[..., 2], Pw[..., 2]
    behind, far, below, ceil = cls & (Psz < 0), cls & (Psz > depth_thre), cls & (Pwz < GROUND_THRE), cls & ~(Pwz < ceiling_thre)
    valid = cls & ~behind & ~far & ~below
    xyz = np.where(valid[..., None], np.concatenate([Pw[..., :2], np.minimum(Pwz, ceiling_thre)[..., None]], axis=-1), 0.0)
    dz = np.where(ceil, zc, Psz)
    depth = np.where(cls & ~(dz < 0), dz, 0.0)
    fin = np.isfinite(Psz) & np.isfinite(Pw).all(-1)
    rel = lambda v, thr: np.abs(v - thr) < BAND_REL * max(1.0, abs(thr))
    with np.errstate(invalid="ignore"):
        band = cls & (~fin | rel(Psz, 0.0) | rel(Psz, depth_thre) | rel(Pwz, GROUND_THRE) | rel(Pwz, ceiling_thre))
        scale = np.maximum(1.0, np.abs(np.where(fin[..., None], Pw, 0.0)).max(-1))
    return dict(Psz=Psz, Pw=Pw, classified=cls, behind=behind, far=far, below=below, ceiling=ceil, valid=valid, xyz=xyz, depth=depth,
                band=band, scale=scale)


def branch_counts(classified, behind, far, below, ceiling):
    """pixels per class.  behind: Ps.z < 0; far: Ps.z > depth_thre; below: in front of the camera and under the ground, too far or not;
    below_only: rejected by that filter alone; kept: passes all three; ceiling: kept and clamped to the ceiling"""
    classified, behind, far, below, ceiling = (np.asarray(a, dtype=bool) for a in (classified, behind, far, below, ceiling))
    b = classified & behind
    f = classified & far
    g = classified & ~b & below
    kept = classified & ~b & ~f & ~g
    return dict(behind=int(b.sum()), far=int(f.sum()), below=int(g.sum()), ceiling=int((kept & ceiling).sum()), kept=int(kept.sum()),
                below_only=int((g & ~f).sum()))


def oracle_classes(o, sc):
    """the predicates of branch_counts read off the oracle's outputs alone: popup_depth without a ceiling is Ps.z where the point is in
    front of the camera and 0 behind it, which gives `behind` and `far`; what popup_cloud without a depth threshold rejects in front of the
    camera is `below`"""
    pid = o["pid"]; cls = pid >= 0
    inf = np.float32(np.inf)
    psz = O.popup_depth(pid, sc["invK"], sc["T"], o["planes"], np.zeros(4, np.float32), inf)
    _, valid_inf = O.popup_cloud(pid, sc["invK"], sc["T"], o["planes"], inf, CEILING_THRE)
    behind = cls & (psz == 0)
    far = cls & (psz > np.float32(DEPTH_THRE))
    below = cls & ~behind & ~valid_inf.astype(bool)
    ceiling = o["valid"].astype(bool) & (o["xyz"][..., 2] == np.float32(CEILING_THRE))
    return dict(classified=cls, behind=behind, far=far, below=below, ceiling=ceiling)


def errors_vs_ref64(xyz, valid, depth, r):
    """fp32 outputs against ref64 outside its guard band -> (flag mismatches, e of the cloud, e of the depth, band fraction); e is taken
    over the kept pixels: a rejected pixel has no point, and its depth can lie at any distance"""
    cls, band = r["classified"], r["band"]
    use = cls & ~band
    valid = np.asarray(valid).astype(bool)
    mism = int((use & (valid != r["valid"])).sum())
    both = use & valid & r["valid"]
    e_xyz = e_dep = 0.0
    if both.any():
        e_xyz = float((np.abs(np.asarray(xyz, dtype=np.float64) - r["xyz"]).max(-1)[both] / r["scale"][both]).max())
        e_dep = float((np.abs(np.asarray(depth, dtype=np.float64) - r["depth"])[both] / r["scale"][both]).max())
    frac = float(band.sum()) / max(1, int(cls.sum()))
    return mism, e_xyz, e_dep, frac


def planes64(seg, K, T):
    """K5 in float64 -> (planes (n + 1, 4) in the sensor frame, plane 0 the ground; ground points (n, 2, 3); in front of the camera (n, 2))"""
    seg = np.asarray(seg, dtype=np.float64).reshape(-1, 4)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    R, c = T[:3, :3], T[:3, 3]
    px = np.concatenate([seg.reshape(-1, 2), np.ones((2 * len(seg), 1))], axis=1)
    d = (R @ np.linalg.solve(np.asarray(K, dtype=np.float64), px.T)).T       # world direction of every end point's ray from the camera centre c
    with np.errstate(divide="ignore", invalid="ignore"):
        s = -c[2] / d[:, 2]                                                  # c + s d meets z = 0
    G = (c + s[:, None] * d).reshape(-1, 2, 3)
    G[..., 2] = 0.0
    front = (s > 0).reshape(-1, 2)               # the ray's third sensor component is 1 (last row of K): s is the depth along the optical axis
    t1 = G[:, 1] - G[:, 0]
    nw = np.cross(t1, np.array([0.0, 0.0, -1.0]))                            # vertical plane through both ground points
    world = np.concatenate([nw, -np.einsum("nk,nk->n", nw, G[:, 0])[:, None]], axis=1)
    world = np.concatenate([[[0.0, 0.0, -1.0, 0.0]], world], axis=0)
    return world @ T, G, front                                               # sensor plane = T^T world plane (rows)


def planes_error(planes, seg, K, T):
    """planes (n + 1, 4) fp32 against planes64, both divided by the norm of their normal: max |difference| / max(1, |d|) over the ground
    and the segments whose ground points are more than 1 cm apart and in front of the camera; -> (e, segments measured)"""
    ref, G, front = planes64(seg, K, T)
    use = np.concatenate([[True], front.all(1) & (np.linalg.norm(G[:, 1] - G[:, 0], axis=1) > 0.01)])
    a = np.asarray(planes, dtype=np.float64)[use]; b = ref[use]
    a = a / np.linalg.norm(a[:, :3], axis=1, keepdims=True); b = b / np.linalg.norm(b[:, :3], axis=1, keepdims=True)
    return float((np.abs(a - b).max(1) / np.maximum(1.0, np.abs(b[:, 3]))).max()), int(use.sum()) - 1


def depth_fill64(sparse):
    """the half-resolution tail of the depth map in float64: 2 x 2 block sums (one pixel of four is set), then a bilinear spread over the
    full frame -- source coordinate (X + 0.5) / 2 - 0.5, taps clamped at the borders: weights 0.25 / 0.75 inside, 1 at the rim.
    -> (map, largest |tap| per pixel: the scale of the fp32 rounding)"""
    a = np.asarray(sparse, dtype=np.float64); h, w = a.shape
    half = a.reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3))

    def taps(n, m):
        f = (np.arange(n) + 0.5) / 2 - 0.5
        i0 = np.floor(f).astype(int); fr = f - i0
        i1 = i0 + 1
        return np.clip(i0, 0, m - 1), np.clip(i1, 0, m - 1), fr

    y0, y1, fy = taps(h, h // 2); x0, x1, fx = taps(w, w // 2)
    fy, fx = fy[:, None], fx[None, :]
    c = [half[np.ix_(y0, x0)], half[np.ix_(y0, x1)], half[np.ix_(y1, x0)], half[np.ix_(y1, x1)]]
    out = (c[0] * (1 - fx) + c[1] * fx) * (1 - fy) + (c[2] * (1 - fx) + c[3] * fx) * fy
    return out, np.max(np.abs(c), axis=0)


@functools.lru_cache(maxsize=None)
def scene_cached(w, h, npl, pose=POSE):
    return scene(w, h, SEEDS.get((w, h), w), npl, pose)


@functools.lru_cache(maxsize=None)
def oracle_run(w, h, npl, step):
    """what the fp32 C oracle gives for scene_cached(w, h, npl): computed once, shared, never modified (arrays are read-only)"""
    sc = scene_cached(w, h, npl)
    planes = O.popup_planes(sc["seg"], sc["invK"], sc["T"])
    pid = O.popup_mask(sc["polys"], w, h, step)
    xyz, valid = O.popup_cloud(pid, sc["invK"], sc["T"], planes, DEPTH_THRE, CEILING_THRE)
    depth = O.popup_depth(pid, sc["invK"], sc["T"], planes, ceiling_plane(sc["T"]), CEILING_THRE)
    out = dict(planes=planes, pid=pid, xyz=xyz, valid=valid, depth=depth)
    for v in out.values():
        v.setflags(write=False)
    return out
