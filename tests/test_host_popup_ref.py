"""CPU: the float64 statements of the pop-up geometry (tests/popup_helpers.py: ref64, planes64, depth_fill64) against the fp32 C oracle,
and the inputs of test_gpu_popup_pixels.py -- so that the GPU comparison with either cannot be vacuous.

Measured on the CPU oracle, scenes of popup_helpers.scene (seed = image width; 258 x 6: seed 260, 2 x 2: seed 12), npl in (9, 64), step in (1, 2):

  branch population, summed over npl, (step 1 / step 2).  behind: Ps.z < 0; far: Ps.z > 10; below: in front and Pw.z < -0.2; below_only:
  rejected by that filter alone; ceiling: kept and clamped to 2.5
    size        behind            far               below             below_only       ceiling           kept
    640x480     47853 / 12064     58498 / 14678     70907 / 17674     19047 / 4755     27762 / 7005      271704 / 67994
    321x243     19410 / 4738      17493 / 4477      11031 / 2804      4008 / 981       13358 / 3360      77196 / 19736
    258x6       424 / 72          706 / 202         262 / 47          71 / 0           370 / 198         1630 / 482
    642x480     141066 / 35386    49055 / 12137     41085 / 10306     31542 / 7912     28577 / 7243      298033 / 75075
    800x601     194305 / 49219    345250 / 86367    129888 / 32474    26899 / 6743     52115 / 13003     224157 / 55678
    1283x819    216995 / 81106    154975 / 41369    198754 / 48631    125661 / 30558   181381 / 43185    1167274 / 264742
  (2 x 2 holds 4 pixels and is not asked to populate anything.  258 x 6 at step 2 has rows 0, 2, 4 only, and its 6.7-pixel focal length
  leaves a wall point in front of the camera, nearer than 10 m and more than 0.2 m under the ground a band of about 0.1 pixel rows: of 42
  seeds tried none had a single such pixel, so below_only is asked for everywhere else.)

  e = max |oracle - ref64| / max(1, |Pw|inf) over the kept pixels outside the guard band, ref64 fed the oracle's fp32 plane equations;
  per run (cloud / depth), smallest and largest of the four runs of a size:
    640x480   2.4e-7 .. 6.3e-7 / 1.8e-7 .. 4.5e-7        642x480   5.6e-7 .. 4.4e-6 / 4.8e-7 .. 4.1e-6
    321x243   3.5e-7 .. 7.2e-7 / 2.5e-7 .. 5.9e-7        800x601   2.5e-7 .. 7.2e-6 / 2.2e-7 .. 8.4e-6
    258x6     2.3e-7 .. 6.2e-7 / 1.9e-7 .. 6.7e-7        1283x819  6.2e-7 .. 8.8e-7 / 5.8e-7 .. 7.9e-7
    2x2       9.0e-8 .. 1.3e-7 / 2.3e-8 .. 6.4e-8
  largest: cloud 7.21e-6, depth 8.41e-6 (both 800x601, npl 64: a ray that meets its plane at a grazing angle).  No valid flag differed in
  any run, guard band or not; the band held at most 2.5e-4 of the classified pixels of a run.

  planes: max |oracle / |n| - planes64 / |n|| / max(1, |d|) over the ground and the segments whose ground points are more than 1 cm
  apart and in front of the camera (27 to 62 of 63), four poses per size: 5.7e-7 .. 1.68e-5, largest at 642x480, pose (-0.2, -0.04, -0.08).

The assertions take 4 x the largest measured value (popup_helpers.E_CLOUD, E_DEPTH, E_PLANES): the fp32 rounding moves with the seed."""
import numpy as np
import pytest

import popup_helpers as H
from oracle import oracle_py as O

RUNS = [(w, h, npl, step) for (w, h) in H.SIZES for npl in H.NPLS for step in H.STEPS]


@pytest.fixture(scope="module", autouse=True)
def _oracle_lib():
    O.build()


@pytest.mark.parametrize("size", H.POPULATED, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("step", H.STEPS)
def test_branches_are_populated(size, step):
    """a condition on the inputs, not a measurement: every filter branch of K6 sees at least 20 pixels at every size, at both steps"""
    w, h = size
    tot = dict.fromkeys(H.CLASSES, 0)
    for npl in H.NPLS:
        sc, o = H.scene_cached(w, h, npl), H.oracle_run(w, h, npl, step)
        for k, v in H.branch_counts(**H.oracle_classes(o, sc)).items():
            tot[k] += v
        assert (o["pid"].max() >= npl // 2) and (o["pid"] == -1).any()        # late polygons show, and some pixels have none
    print(size, step, tot)
    for k in H.CLASSES:
        if k == "below_only" and size == (258, 6):
            continue                                  # (module docstring)
        assert tot[k] >= H.MIN_PER_CLASS, (size, step, k, tot)


@pytest.mark.parametrize("size", list(H.SIZES), ids=lambda s: "%dx%d" % s)
def test_forms(size):
    """the table of sizes names the kernel form each size was chosen for"""
    w, h = size
    for npl in H.NPLS:
        assert H.expected_form(w, h, npl) == H.SIZES[size]
    assert H.expected_form(w, h, 0) in ("<2,false>", "<8,false>")
    assert sorted(set(H.SIZES.values())) == ["<2,false>", "<2,true>", "<8,false>"]
    assert H.SIZES[(1283, 819)] == "<8,false>" and 819 % 8 == 3 and 1283 % 256 == 3 and 1283 * 819 >= 1 << 20


@pytest.mark.parametrize("w,h,npl,step", RUNS)
def test_oracle_cloud_and_depth_against_ref64(w, h, npl, step):
    sc, o = H.scene_cached(w, h, npl), H.oracle_run(w, h, npl, step)
    r = H.ref64(o["pid"], sc["K"], sc["T"], o["planes"])
    mism, e_xyz, e_dep, frac = H.errors_vs_ref64(o["xyz"], o["valid"], o["depth"], r)
    print("%dx%d npl %d step %d: e_cloud %.3g e_depth %.3g band %.3g mismatches %d" % (w, h, npl, step, e_xyz, e_dep, frac, mism))
    assert frac <= H.BAND_MAX_FRACTION
    assert mism == 0
    assert e_xyz <= H.E_CLOUD and e_dep <= H.E_DEPTH
    # the two readings of the classes -- ref64's predicates, the oracle's outputs -- count the same pixels outside the band
    a = H.oracle_classes(o, sc)
    for k in ("behind", "far", "below", "ceiling"):
        rk = r[k] if k != "below" else r["below"] & ~r["behind"]
        rk = rk if k != "ceiling" else rk & r["valid"]
        assert not ((a[k] != rk) & ~r["band"]).any(), k


def test_ref64_on_a_hand_worked_view():
    """ref64 itself, at a pose where the answer is known on paper: camera at the origin's height 1 m looking along world y, no rotation
    besides the axis swap; the ground pixel straight below the principal point at 45 degrees lies 1 m ahead"""
    K = np.array([[100.0, 0, 50.0], [0, 100.0, 50.0], [0, 0, 1]])
    T = H.pose_T(0.0, 0.0, 0.0, t=(0.0, 0.0, 1.0))
    ground_s = T.T @ np.array([0, 0, -1.0, 0])                         # sensor-frame ground plane
    wall_s = T.T @ np.array([0, -1.0, 0, 4.0])                         # the wall y = 4
    pid = np.full((151, 101), -1); pid[150, 50] = 0; pid[50, 70] = 1; pid[10, 50] = 1; pid[49, 50] = 0; pid[55, 50] = 0
    r = H.ref64(pid, K, T, np.stack([ground_s, wall_s]))
    np.testing.assert_allclose(r["Pw"][150, 50], [0, 1, 0], atol=1e-12)
    np.testing.assert_allclose(r["Pw"][50, 70], [0.8, 4, 1], atol=1e-12)               # x = 0.2 * depth 4 to the right, at camera height
    np.testing.assert_allclose(r["Pw"][10, 50], [0, 4, 2.6], atol=1e-12)               # above the ceiling: clamped, depth from the ceiling
    assert r["valid"][10, 50] and r["ceiling"][10, 50]
    np.testing.assert_allclose(r["xyz"][10, 50], [0, 4, 2.5], atol=1e-12)
    np.testing.assert_allclose(r["depth"][10, 50], 1.5 / 0.4, atol=1e-12)
    assert r["behind"][49, 50] and not r["valid"][49, 50] and r["depth"][49, 50] == 0  # a ground pixel above the horizon
    assert r["far"][55, 50] and not r["valid"][55, 50] and r["Psz"][55, 50] == pytest.approx(20.0) and r["depth"][55, 50] == pytest.approx(20.0)
    assert r["depth"][150, 50] == pytest.approx(1.0) and r["Psz"][50, 70] == pytest.approx(4.0)


POSES = (H.POSE,) + H.MORE_POSES


@pytest.mark.parametrize("size", list(H.SIZES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pose", POSES, ids=lambda p: "yaw%+.2f" % p[0])
def test_oracle_planes_against_planes64(size, pose):
    w, h = size
    sc = H.scene(w, h, H.SEEDS.get(size, w), 9, pose)
    planes = O.popup_planes(sc["seg"], sc["invK"], sc["T"])
    e, n = H.planes_error(planes, sc["seg"], sc["K"], sc["T"])
    print("%dx%d pose %s: e_planes %.3g over %d segments" % (w, h, pose, e, n))
    assert n >= 20
    assert e <= H.E_PLANES
    # the segment above the horizon meets the ground behind the camera
    _, _, front = H.planes64(sc["seg"], sc["K"], sc["T"])
    assert not front[H.HORIZON_SEG].any()


def test_planes64_on_a_hand_worked_view():
    K = np.array([[100.0, 0, 50.0], [0, 100.0, 50.0], [0, 0, 1]])
    T = H.pose_T(0.0, 0.0, 0.0, t=(0.0, 0.0, 1.0))
    # pixels (30, 75) and (70, 75): 0.25 below the axis -> 4 m ahead, 0.8 m to either side: the wall y = 4, seen from the front
    planes, G, front = H.planes64([[30.0, 75.0, 70.0, 75.0]], K, T)
    np.testing.assert_allclose(G[0], [[-0.8, 4, 0], [0.8, 4, 0]], atol=1e-12)
    assert front.all()
    world = np.linalg.inv(T).T @ planes[1]                  # back to the world: sensor = T^T world
    np.testing.assert_allclose(world / np.linalg.norm(world[:3]), [0, 1, 0, -4], atol=1e-12)     # (G1 - G0) x (0, 0, -1) = +y
    np.testing.assert_allclose(planes[0], T.T @ np.array([0, 0, -1.0, 0]), atol=1e-15)


@pytest.mark.parametrize("size", [s for s in H.SIZES if s[0] % 2 == 0 and s[1] % 2 == 0], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("npl", H.NPLS)
def test_oracle_depth_fill_against_float64(size, npl):
    """every value passes four fp32 roundings on its way (product, sum, product, sum), the weights are exact and add up to 1:
    |fp32 - float64| <= 4 u (1 + u)^3 max |tap| with u = 2^-24; 5 u is asked"""
    w, h = size
    sparse = H.oracle_run(w, h, npl, 2)["depth"]
    assert sparse[0, 0] > 0 if size == (2, 2) else (sparse > 0).sum() >= 100
    got = O.depth_fill_half(sparse)
    ref, tap = H.depth_fill64(sparse)
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= 5 * 2.0 ** -24 * tap).all(), float((err / np.maximum(tap, 1e-30)).max())
    # the rim repeats the outermost half-resolution sample, and the interior weights are 0.25 / 0.75
    np.testing.assert_array_equal(got[0, 0], sparse[0, 0])
    np.testing.assert_array_equal(got[h - 1, w - 1], sparse[h - 2, w - 2])
    if w >= 6:
        np.testing.assert_allclose(ref[0, 3], 0.75 * sparse[0, 2].astype(np.float64) + 0.25 * sparse[0, 4], rtol=1e-15)
