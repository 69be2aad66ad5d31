"""tests/keypoints_3d_model.py on hand-made cases with hand-computed values, and the host mirror (rtabmap_amd/host/Keypoints3D.cpp, through
c_shim.cpp) against the model, bit for bit.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import keypoints_3d_inputs as I
import keypoints_3d_model as M

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_computed_window():
    """a 3 x 3 f32 window around 2.0: two edge neighbours and one corner inside the band, one edge neighbour outside it, the rest holes"""
    d = np.array([[2.02, 2.01, 0.0],
                  [2.05, 2.00, np.nan],
                  [np.inf, 1.99, -2.0]], np.float32)
    cam = [M.camera(2.0, 4.0, 1.0, 1.0)]
    im = M.image(d, cam)
    p, defined = M.point_of(im, (1.0, 1.0))
    # visited uu-major: (0,0) corner 2.02, (0,1) edge 2.05 (|0.05| >= 0.04: out), (0,2) inf, (1,0) edge 2.01, (1,2) edge 1.99, (2,0) 0, (2,1) NaN, (2,2) < 0
    sums = F(2.02)
    sums = sums + F(2.01) * F(2)
    sums = sums + F(1.99) * F(2)
    z = (F(2.0) * F(4) + sums) / F(9)
    assert defined and p[2] == z and p[0] == 0 and p[1] == 0
    assert abs(float(z) - (8 + 2.02 + 4.02 + 3.98) / 9) < 1e-6
    # half a pixel right and down: the same centre pixel (1.49 + 0.5 truncates to 1), X and Y from the fraction
    p2 = M.point_of(im, (1.49, 1.25))[0]
    assert p2[2] == z and p2[0] == (F(1.49) - F(1)) * z / F(2) and p2[1] == (F(1.25) - F(1)) * z / F(4)
    # u16: millimetres, 0 and 65535 are holes
    d16 = np.array([[0, 1000, 65535], [1010, 1000, 990], [1000, 1030, 1000]], np.uint16)
    z16 = M.point_of(M.image(d16, cam), (1.0, 1.0))[0][2]
    m = lambda v: F(v) * F(0.001)
    s = m(1010) * F(2)                                   # (0,1)
    s = s + m(1000)                                      # (0,2)
    s = s + m(1000) * F(2)                               # (1,0)
    s = s + m(990) * F(2)                                # (2,1); (1,2) = 1030 is out of the band, (2,2) counts
    s = s + m(1000)
    assert z16 == (m(1000) * F(4) + s) / F(12)


def test_hand_computed_cameras_factors_and_transform():
    """two cameras side by side on a 4 x 2 image, the colour image twice as large: keypoint (5, 2) is depth pixel (2.5, 1) -> camera 1, its
    column 0.5 -> u = 1; the transform is applied left to right"""
    d = np.zeros((2, 4), np.float32)
    d[1, 3] = 2.0                                        # camera 1, its pixel (1, 1)
    t = [0, 0, 1, 0.5, -1, 0, 0, 0.25, 0, -1, 0, -0.125]
    cams = [M.camera(8.0, 8.0, 2.0, 2.0, 4, 4), M.camera(4.0, 8.0, 1.0, 1.0, 4, 4, transform=t)]
    im = M.image(d, cams)
    assert M.factors(im) == (2, F(2), F(0.5), F(0.5))
    reads = []
    p, defined = M.point_of(im, (5.0, 2.0), reads=reads)
    assert defined and reads[0] == (3, 1) and all(c >= 2 for c, _ in reads)
    X = (F(0.5) - F(0.5)) * F(2) / F(2)                  # cx = 1 * 0.5, fx = 4 * 0.5
    Y = (F(1.0) - F(0.5)) * F(2) / F(4)                  # cy = 1 * 0.5, fy = 8 * 0.5
    assert X == 0 and Y == F(0.25)
    np.testing.assert_array_equal(p, np.array([2 + 0.5, 0.25, -0.25 - 0.125], np.float32))
    # camera 0 has no transform and nothing to see at its pixel (1, 1)
    assert np.isnan(M.point_of(im, (2.0, 2.0))[0]).all()
    assert (I.bits(M.point_of(im, (2.0, 2.0))[0]) == M.QUIET_NAN_BITS).all()


def test_hand_computed_filters():
    d = np.array([[1000, 3000, 0, 65535, 500]], np.uint16)
    im = M.image(d, [M.camera(1.0, 1.0, 0.5, 0.5)])
    pts = [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (3.0, 0.0), (4.0, 0.0), (4.4, 0.4), (4.5, 0.0), (0.0, 0.5)]
    assert M.frame(im, pts, M.FILTER_PIXEL, 0.5, 3.0, with_xyz=False)[0] == [0]             # 1.0 in range; 3.0 is not < 3.0; 0.5 is not > 0.5
    assert M.frame(im, pts, M.FILTER_PIXEL, 0.0, 0.0, with_xyz=False)[0] == [0, 1, 3, 4, 5]  # 65.535 m stands, 0 does not; (4.5, 0) and (0, 0.5) are outside
    kept, xyz = M.frame(im, pts[:5], M.FILTER_3D, 0.0, 0.0)
    assert kept == [0, 1, 4] and np.isnan(xyz[2]).all() and np.isnan(xyz[3]).all()
    kept = M.frame(im, pts[:5], M.FILTER_3D, 0.75, 2.0)[0]
    assert kept == [0]                                   # 0.5 m is below Kp/MinDepth, 3 m above Kp/MaxDepth: bad points already
    for lo, hi, flt in ((-1.0, 0.0, M.FILTER_3D), (-1.0, 0.0, M.FILTER_PIXEL), (2.0, 2.0, M.KEEP_ALL), (2.0, 1.0, M.FILTER_3D), (float("nan"), 0.0, M.KEEP_ALL)):
        with pytest.raises(M.Refused):
            M.frame(im, pts[:5], flt, lo, hi)
    assert M.frame(im, pts[:5], M.KEEP_ALL, -1.0, 0.0)[0] == [0, 1, 2, 3, 4]                 # without a filter min_depth < 0 switches the lower test off


def test_abi_of_the_new_structs():
    from rtabmap_amd import capi
    assert ctypes.sizeof(capi.LcdCamera) == 80 and ctypes.sizeof(capi.LcdDepthImage) == 40 and ctypes.sizeof(capi.LcdKeypoints3dArgs) == 128
    assert ctypes.sizeof(capi.LcdSelectArgs) == 120 and ctypes.sizeof(capi.LcdExpandArgs) == 64
    assert capi.LcdSelectArgs.n_in.offset == 112 and capi.LcdExpandArgs.n_features.offset == 56
    src = open(os.path.join(ROOT, "rtabmap_amd", "csrc", "keypoints_3d.hip")).read()
    assert re.search(r"static_assert\(sizeof\(lcd_keypoints_3d_args\) == 128\b", src)
    sel = open(os.path.join(ROOT, "rtabmap_amd", "csrc", "feature_select.hip")).read()
    assert re.search(r"static_assert\(sizeof\(lcd_select_args\) == 120\b", sel) and re.search(r"static_assert\(sizeof\(lcd_expand_args\) == 64\b", sel)
    header = open(os.path.join(ROOT, "include", "lcd.h")).read()
    assert int(re.search(r"#define LCD_ABI_VERSION (\d+)", header).group(1)) == 7
    assert "block_rank" not in sel.replace("block_rank(flag", "").replace("block_rank(id", "")   # the scan is shared, not copied


# ---------------------------------------------------------------------------------------------------------------- the host mirror
def _mirror_frame(im, pts, filter, lo, hi):
    """the host mirror's three functions chained as MemoryHip chains them -> (kept or None, xyz or None)"""
    from rtabmap_amd import vwdictionary as V
    if filter == M.FILTER_PIXEL:
        return V.filter_keypoints_by_depth_pixel(pts, im["data"], lo, hi, width=im["width"]), None
    xyz = V.generate_keypoints_3d_depth(pts, im["data"], im["cameras"], lo, hi, width=im["width"])
    if xyz is None:
        return None, None
    if filter == M.KEEP_ALL:
        return list(range(len(pts))), xyz
    return V.filter_keypoints_by_depth_3d(xyz, lo, hi), xyz


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("width,height", I.SHAPES)
def test_host_mirror_equals_the_model(dtype, width, height):
    rng = np.random.default_rng(width)
    for n_cameras in (1, 2, 4):
        if width % n_cameras:
            continue
        for kw in (dict(), dict(transform=I.TILT, image_size=(width // n_cameras * 3 + 1, height * 2)), dict(pad=3, zero_principal=True)):
            im, pts = I.random_frame(rng, dtype, width, height, n_cameras, 300, host_ok=True, **kw)
            for flt, lo, hi in ((M.KEEP_ALL, -1.0, 0.0), (M.KEEP_ALL, 0.0, 0.0), (M.FILTER_3D, 0.0, 0.0), (M.FILTER_3D, 1.5, 3.0), (M.FILTER_PIXEL, 1.5, 3.0)):
                kept, xyz = M.frame(im, pts, flt, lo, hi, with_xyz=False)
                got_kept, got_xyz = _mirror_frame(im, pts, flt, lo, hi)
                assert list(got_kept) == kept, (n_cameras, kw.keys(), flt)
                if xyz is not None:
                    np.testing.assert_array_equal(I.bits(got_xyz), I.bits(xyz))


def test_host_mirror_on_the_single_property_inputs():
    from rtabmap_amd import vwdictionary as V
    rng = np.random.default_rng(9)
    exact, inside, pts = I.band_edge_case()
    order, opts = I.loop_order_case(rng)
    for data, p in ((exact, pts), (inside, pts), (order, opts)):
        im = M.image(data, I.cameras_for(3, 3, 1))
        np.testing.assert_array_equal(I.bits(V.generate_keypoints_3d_depth(p, data, im["cameras"])), I.bits(M.frame(im, p)[1]))
    d, cams, p = I.fma_transform_case(rng)
    np.testing.assert_array_equal(I.bits(V.generate_keypoints_3d_depth(p, d, cams)), I.bits(M.frame(M.image(d, cams), p)[1]))
    d, cams, p, lo, hi = I.fma_dist_case(rng)
    xyz = V.generate_keypoints_3d_depth(p, d, cams, lo, hi)
    assert V.filter_keypoints_by_depth_3d(xyz, lo, hi).tolist() == [0]
    for n_cameras in (2, 4):
        d, p = I.seam_case(rng, np.uint16, n_cameras)
        im = M.image(d, I.cameras_for(d.shape[1] // n_cameras, d.shape[0], n_cameras))
        np.testing.assert_array_equal(I.bits(V.generate_keypoints_3d_depth(p, d, im["cameras"])), I.bits(M.frame(im, p)[1]))


def test_host_mirror_refuses_what_the_reference_asserts_on():
    from rtabmap_amd import vwdictionary as V
    d = np.full((12, 16), 2.0, np.float32)
    cams = I.cameras_for(16, 12, 1)
    for pt in list(I.wild_points()) + [(16.0, 1.0)]:
        assert V.generate_keypoints_3d_depth([pt], d, cams) is None
    for pt in I.wild_points()[:6]:
        assert V.filter_keypoints_by_depth_pixel([pt], d) is None
    assert V.generate_keypoints_3d_depth([(1.0, 1.0)], d, I.cameras_for(5, 12, 3)) is None      # 16 % 3 != 0
    assert V.filter_keypoints_by_depth_3d(np.zeros((1, 3), np.float32), -1.0, 0.0) is None
    assert V.filter_keypoints_by_depth_3d(np.zeros((1, 3), np.float32), 2.0, 1.0) is None
    assert V.filter_keypoints_by_depth_pixel([(1.0, 1.0)], d, 2.0, 2.0) is None
    assert V.generate_keypoints_3d_depth(np.zeros((0, 2), np.float32), d, cams).shape == (0, 3)


def test_memory_hip_depth_stage_keeps_what_the_model_keeps():
    """MemoryHip::update with a depth image and cameras: the features that pass Kp/MinDepth and Kp/MaxDepth and their points are the
    model's, with or without a device (without one Keypoints3D's host code runs the stage; the word ids need the engine and are the GPU
    suite's)"""
    from rtabmap_amd.vwdictionary import MemoryHip
    from helpers import unit_rows
    rng = np.random.default_rng(31)
    h = MemoryHip(max_features=100, min_depth=1.5, max_depth=3.4)
    for t, (n, dtype, nc) in enumerate(((300, np.uint16, 2), (120, np.float32, 1), (300, np.uint16, 4))):
        im, p = I.random_frame(rng, dtype, 64, 48, nc, n, transform=I.TILT if t % 2 else None, host_ok=True, border=t == 2)
        kept, xyz = M.frame(im, p, M.FILTER_3D, 1.5, 3.4)
        sid, ids, got_xyz, got_kept = h.update_depth(unit_rows(n, 64, seed=40 + t), np.ones(n, np.float32), p, (64, 48), im["data"], im["cameras"], width=im["width"])
        assert sid == t + 1 and len(ids) == len(kept) and 0 < len(kept) < n
        assert got_kept.tolist() == kept
        np.testing.assert_array_equal(I.bits(got_xyz), I.bits(xyz[kept]))
    bad = np.array([[np.nan, 1.0]] * 3, np.float32)
    assert h.update_depth(unit_rows(3, 64, seed=50), np.ones(3, np.float32), bad, (64, 48), im["data"], im["cameras"])[0] == 0 and "keypoint" in h.select_error()
    h.close()
