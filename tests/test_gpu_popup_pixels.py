"""GPU: every per-pixel output of the pop-up run (pps_popup_run: K5 + K6, k_depth_fill) in each of its kernel forms, at image sizes whose
last row block and last column block are partial, with every filter branch populated (tests/test_host_popup_ref.py holds the counts):
bit for bit against the fp32 C oracle, and -- independently of it -- against the float64 statement of the geometry in popup_helpers."""
import ctypes as C
import functools

import numpy as np
import pytest

import pop_up_slam_amd as P
import popup_helpers as H
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

ALL = list(H.SIZES)
EVEN = [s for s in ALL if s[0] % 2 == 0 and s[1] % 2 == 0]
BIG = [s for s in ALL if H.SIZES[s] != "<2,true>"]
_id = lambda s: "%dx%d" % s
_fp = C.POINTER(C.c_float)


def _handle(w, h, sc, image=True, outputs=True):
    pp = P.Popup(w, h, sc["invK"])
    if image:
        pp.set_image(sc["bgr"])
    if not outputs:
        pp.set_outputs(depth=False, plane_id=False)
    return pp


def _run(pp, sc, step, w, h, polys=None, run_async=False):
    polys = sc["polys"] if polys is None else polys
    # which kernel form this run takes follows from the size and the number of polygons alone: a moved threshold must not empty a case
    want = H.SIZES[(w, h)]
    assert H.expected_form(w, h, len(polys)) == (want if len(polys) or want == "<8,false>" else "<2,false>")
    fn = pp.run_async if run_async else pp.run
    return fn(sc["seg"], sc["T"], polys, step=step, depth_thre=H.DEPTH_THRE, ceiling_thre=H.CEILING_THRE)


def _planes_and_cloud(pp):
    """pps_popup_download asked for the plane equations and the cloud alone (Popup.download asks for everything)"""
    planes = np.zeros((pp.n + 1, 4), dtype=np.float32)
    cloud = np.zeros(pp.w * pp.h_, dtype=P.POINT_DTYPE)
    pp._ck(pp.L.pps_popup_download(pp.h, planes.ctypes.data_as(_fp), cloud.ctypes.data_as(C.c_void_p), None, None))
    return planes, cloud.reshape(pp.h_, pp.w)


def _flag(cloud):
    return ((cloud["rgba"] >> 24) & 1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _device_run(w, h, npl, step):
    """one synchronous run with image and all outputs on a fresh handle, downloaded; shared by the tests below, never modified"""
    sc = H.scene_cached(w, h, npl)
    pp = _handle(w, h, sc)
    nv = _run(pp, sc, step, w, h)
    planes, cloud, depth, pid = pp.download()
    pp.close()
    for a in (planes, cloud, depth, pid):
        a.setflags(write=False)
    return dict(nv=nv, planes=planes, cloud=cloud, depth=depth, pid=pid)


def _same_bits(a, b, colour=True):
    """two downloads (planes, cloud, ...) hold the same bits; colour=False: but for the colour of the cloud"""
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    for f in ("x", "y", "z"):
        np.testing.assert_array_equal(a[1][f].view(np.uint32), b[1][f].view(np.uint32))
    mask = np.uint32(0xFFFFFFFF if colour else 0xFF000000)
    np.testing.assert_array_equal(a[1]["rgba"] & mask, b[1]["rgba"] & mask)
    for x, y in zip(a[2:], b[2:]):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def _check_against_oracle(got, sc, o, nv):
    planes, cloud, depth, pid = got
    np.testing.assert_array_equal(planes, o["planes"])
    np.testing.assert_array_equal(pid, o["pid"])
    valid = o["valid"].astype(bool)
    np.testing.assert_array_equal(_flag(cloud), o["valid"])
    for k, f in enumerate(("x", "y", "z")):
        np.testing.assert_array_equal(cloud[f][valid], o["xyz"][..., k][valid])
    for f in ("x", "y", "z", "rgba"):
        assert not cloud[f][~valid].view(np.uint32).any(), f            # a pixel without a point is the all-zero record
    assert nv == int(valid.sum())
    if depth is not None:
        np.testing.assert_array_equal(depth, o["depth"])


@pytest.mark.parametrize("size", ALL, ids=_id)
def test_outputs_match_oracle(built, size):
    """planes, mask, cloud, valid flag, n_valid, colour and depth of every run, bit for bit"""
    w, h = size
    for npl in H.NPLS:
        sc = H.scene_cached(w, h, npl)
        bgr = sc["bgr"].astype(np.uint32)
        rgb = (bgr[..., 2] << 16) | (bgr[..., 1] << 8) | bgr[..., 0]
        for step in H.STEPS:
            d, o = _device_run(w, h, npl, step), H.oracle_run(w, h, npl, step)
            _check_against_oracle((d["planes"], d["cloud"], d["depth"], d["pid"]), sc, o, d["nv"])
            v = o["valid"].astype(bool)
            np.testing.assert_array_equal(d["cloud"]["rgba"][v], rgb[v] | np.uint32(1 << 24))       # 0x00RRGGBB under the flag
            if step == 2:
                odd = (np.arange(w)[None, :] % 2 == 1) | (np.arange(h)[:, None] % 2 == 1)
                assert np.all(d["pid"][odd] == -1) and not d["depth"][odd].any()


@pytest.mark.parametrize("size", ALL, ids=_id)
def test_run_without_an_image(built, size):
    """bgr == nullptr in the kernel: the colour is 0, everything else has the bits of the run with an image"""
    w, h = size
    for npl in H.NPLS:
        sc = H.scene_cached(w, h, npl)
        pp = _handle(w, h, sc, image=False)
        for step in H.STEPS:
            d = _device_run(w, h, npl, step)
            nv = _run(pp, sc, step, w, h)
            got = pp.download()
            assert nv == d["nv"]
            assert not (got[1]["rgba"] & np.uint32(0xFFFFFF)).any()
            _same_bits(got, (d["planes"], d["cloud"], d["depth"], d["pid"]), colour=False)
        pp.close()


@pytest.mark.parametrize("size", ALL, ids=_id)
def test_outputs_switched_off(built, size):
    """pps_popup_set_outputs(0, 0) -- what the frame loops and the benchmark run: depth == nullptr and plane_id == nullptr in the kernel;
    cloud and n_valid keep their bits"""
    w, h = size
    for npl in H.NPLS:
        sc = H.scene_cached(w, h, npl)
        pp = _handle(w, h, sc, outputs=False)
        for step in H.STEPS:
            d = _device_run(w, h, npl, step)
            nv = _run(pp, sc, step, w, h)
            assert nv == d["nv"]
            _same_bits(_planes_and_cloud(pp), (d["planes"], d["cloud"]))
            with pytest.raises(P.PpsError) as ei:
                pp.download()
            assert ei.value.code == P.PPS_ESTATE
            with pytest.raises(P.PpsError) as ei:
                pp.fill_depth()
            assert ei.value.code == P.PPS_ESTATE
        pp.close()


@pytest.mark.parametrize("size", EVEN, ids=_id)
def test_fill_depth(built, size):
    """k_depth_fill after a half-resolution run: border clamps at every even size, hw == hh == 1 at 2 x 2"""
    w, h = size
    for npl in H.NPLS:
        sc, o = H.scene_cached(w, h, npl), H.oracle_run(w, h, npl, 2)
        pp = _handle(w, h, sc)
        _run(pp, sc, 2, w, h)
        pp.fill_depth()
        filled = pp.download()[2]
        np.testing.assert_array_equal(filled, O.depth_fill_half(o["depth"]))
        assert filled[0, 0] > 0 if size == (2, 2) else (filled[:, w - 1] > 0).any() and (filled[h - 1, :] > 0).any()
        # float64 statement of the same map; the bound is derived in test_host_popup_ref.py
        ref, tap = H.depth_fill64(o["depth"])
        assert (np.abs(filled.astype(np.float64) - ref) <= 5 * 2.0 ** -24 * tap).all()
        pp.close()


def test_fill_depth_refuses_an_odd_size(built):
    w, h = 321, 243
    sc = H.scene_cached(w, h, 9)
    pp = _handle(w, h, sc)
    _run(pp, sc, 2, w, h)
    with pytest.raises(P.PpsError) as ei:
        pp.fill_depth()
    assert ei.value.code == P.PPS_EINVAL
    nv = _run(pp, sc, 2, w, h)                          # the handle still runs
    _check_against_oracle(pp.download(), sc, H.oracle_run(w, h, 9, 2), nv)
    pp.close()


@pytest.mark.parametrize("size", BIG, ids=_id)
def test_run_async(built, size):
    """pps_popup_run_async on the frames that launch k_popup_rows in front: the same bits as the synchronous run"""
    w, h = size
    for npl in H.NPLS:
        sc = H.scene_cached(w, h, npl)
        pp = _handle(w, h, sc)
        for step in H.STEPS:
            d = _device_run(w, h, npl, step)
            assert _run(pp, sc, step, w, h, run_async=True) is None
            np.testing.assert_array_equal(pp.planes_wait().view(np.uint32), d["planes"].view(np.uint32))
            _same_bits(pp.download(), (d["planes"], d["cloud"], d["depth"], d["pid"]))       # (no wait(): the download settles the run)
            assert pp.wait() == d["nv"]
        pp.close()


@pytest.mark.parametrize("size", [(640, 480), (1283, 819)], ids=_id)
def test_no_polygons_after_a_run_with_polygons(built, size):
    """nplanes == 0: no k_popup_rows launch, and the frame kernel must not read the row intervals the run before left in device memory"""
    w, h = size
    sc = H.scene_cached(w, h, 64)
    pp = _handle(w, h, sc)
    for step in H.STEPS:
        assert _run(pp, sc, step, w, h) == _device_run(w, h, 64, step)["nv"] > 0
        assert _run(pp, sc, step, w, h, polys=[]) == 0
        planes, cloud, depth, pid = pp.download()
        np.testing.assert_array_equal(planes, H.oracle_run(w, h, 64, step)["planes"])      # the planes are still published
        assert np.all(pid == -1) and not depth.any()
        assert not cloud.view(np.uint32).any()
    pp.close()


@pytest.mark.parametrize("size", ALL, ids=_id)
def test_handle_reused_across_steps_and_polygon_counts(built, size):
    """step 1 -> 2 -> 1 and 64 -> 9 polygons on one handle: nothing of the run before shows"""
    w, h = size
    pp = _handle(w, h, H.scene_cached(w, h, 64))
    for npl, step in ((64, 1), (64, 2), (9, 1), (9, 2), (64, 1)):
        sc = H.scene_cached(w, h, npl)
        pp.set_image(sc["bgr"])
        d = _device_run(w, h, npl, step)
        assert _run(pp, sc, step, w, h) == d["nv"]
        got = pp.download()
        _same_bits(got, (d["planes"], d["cloud"], d["depth"], d["pid"]))
        if step == 2:
            odd = (np.arange(w)[None, :] % 2 == 1) | (np.arange(h)[:, None] % 2 == 1)
            assert np.all(got[3][odd] == -1) and not got[1][odd].view(np.uint32).any() and not got[2][odd].any()
    pp.close()


@pytest.mark.parametrize("size", ALL, ids=_id)
def test_kernel_against_float64(built, size):
    """the device's own outputs against ref64 / planes64 -- not through the oracle: ref64 is fed the kernel's plane equations and mask"""
    w, h = size
    for npl in H.NPLS:
        sc = H.scene_cached(w, h, npl)
        for step in H.STEPS:
            d = _device_run(w, h, npl, step)
            r = H.ref64(d["pid"], sc["K"], sc["T"], d["planes"])
            xyz = np.stack([d["cloud"]["x"], d["cloud"]["y"], d["cloud"]["z"]], axis=-1)
            mism, e_xyz, e_dep, frac = H.errors_vs_ref64(xyz, _flag(d["cloud"]), d["depth"], r)
            print("%dx%d npl %d step %d: e_cloud %.3g e_depth %.3g band %.3g mismatches %d" % (w, h, npl, step, e_xyz, e_dep, frac, mism))
            assert frac <= H.BAND_MAX_FRACTION and mism == 0
            assert e_xyz <= H.E_CLOUD and e_dep <= H.E_DEPTH
            assert d["nv"] == int(_flag(d["cloud"]).sum())
        e, n = H.planes_error(d["planes"], sc["seg"], sc["K"], sc["T"])
        print("%dx%d: e_planes %.3g over %d segments" % (w, h, e, n))
        assert n >= 20 and e <= H.E_PLANES


@pytest.mark.parametrize("pose", H.MORE_POSES, ids=lambda p: "yaw%+.2f" % p[0])
def test_planes_against_float64_at_more_poses(built, pose):
    for (w, h) in ((640, 480), (1283, 819)):
        sc = H.scene(w, h, w, 9, pose)
        for planes in (P.popup_planes(sc["seg"], sc["invK"], sc["T"]),):
            np.testing.assert_array_equal(planes, O.popup_planes(sc["seg"], sc["invK"], sc["T"]))
            e, n = H.planes_error(planes, sc["seg"], sc["K"], sc["T"])
            assert n >= 20 and e <= H.E_PLANES
