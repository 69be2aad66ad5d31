"""The rule of lcd_keypoints_3d_stereo without a GPU: hand-computed pyramid and derivative values, the host mirror
(rtabmap_amd/host/Stereo.cpp) and MemoryHip's stereo stage against tests/stereo_flow_model.py bit for bit, the ABI of the new structs, and
the tracker's accuracy against an independent float64 tracker."""
import ctypes
import os
import re

import numpy as np
import pytest

import stereo_flow_inputs as I
import stereo_flow_model as M
import stereo_flow_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_computed_pyramid_and_derivative():
    img = np.array([[10, 20, 30, 40, 50, 60],
                    [20, 30, 40, 50, 60, 70],
                    [30, 40, 50, 60, 70, 80],
                    [40, 50, 60, 70, 80, 90],
                    [50, 60, 70, 80, 90, 100]], np.uint8)
    down = M.pyr_down(img)
    assert down.shape == (3, 3)
    # a plane a + 10 x + 10 y is reproduced where no tap is reflected: level(1, 1) = src(2, 2)
    assert down[1, 1] == 50
    # level(0, 0): columns -2 .. 2 reflect to 2, 1, 0, 1, 2 -> 10 + 10 * (2 + 4 + 0 + 4 + 2) / 16 = 17.5 per axis offset: 10 + 7.5 + 7.5 = 25
    assert down[0, 0] == (25 * 256 + 128) >> 8
    # level(2, 2) is centred on src(4, 4) = 90; rows 2 .. 6 reflect to 2, 3, 4, 3, 2: (-20 - 40 - 40 - 20) / 16 = -7.5; columns 2 .. 6 reflect to
    # 2, 3, 4, 5, 4: (-20 - 40 + 40 + 0) / 16 = -1.25; (81.25 * 256 + 128) >> 8 = 81
    assert down[2, 2] == 81
    dx, dy = M.scharr(img)
    assert dx[2, 2] == 16 * 20 and dy[2, 2] == 16 * 20                   # a unit step of 10 per pixel: (3 + 10 + 3) * (I(x+1) - I(x-1))
    assert dx[2, 0] == 0 and dx[2, 5] == 0 and dy[0, 2] == 0 and dy[4, 2] == 0      # the reflected taps cancel
    assert dy[2, 0] == 16 * 20 and dx[0, 2] == 16 * 20
    L = M.Level(img, img, 3, 3)
    assert (L.dx[:L.py] == 0).all() and (L.dx[:, :L.px] == 0).all()       # the derivative's border is zero, the image's reflected
    assert L.I[L.py, L.px - 1] == img[0, 1] and L.I[L.py - 2, L.px] == img[2, 0]
    assert M.reflect101(np.array([-7, -1, 6, 9, 13]), 6).tolist() == [3, 1, 4, 1, 3]


def test_abi_of_the_new_structs():
    from rtabmap_amd import capi
    assert ctypes.sizeof(capi.LcdStereoCamera) == 104 and ctypes.sizeof(capi.LcdStereoImage) == 48
    assert ctypes.sizeof(capi.LcdStereoParams) == 56 and ctypes.sizeof(capi.LcdKeypoints3dStereoArgs) == 152
    src = open(os.path.join(ROOT, "rtabmap_amd", "csrc", "keypoints_3d_stereo.hip")).read()
    assert re.search(r"static_assert\(sizeof\(lcd_keypoints_3d_stereo_args\) == 152\b", src)
    assert "gather_kept_rows" in src and "block_rank(keep" in src and "stand_and_transform" not in src      # shared, not copied
    rule = open(os.path.join(ROOT, "rtabmap_amd", "csrc", "stereo_flow_rule.h")).read()
    assert "kp3d::stand_and_transform" in rule and "fp contract(off)" in rule
    L = capi.load()
    assert L.lcd_keypoints_3d_stereo and L.lcd_keypoints_3d_stereo_dev


def _mirror_frame(pr, pts, P, filter, lo, hi):
    """the host mirror's functions chained as MemoryHip chains them"""
    from rtabmap_amd import vwdictionary as V
    got = V.stereo_correspondences(pr["left"], pr["right"], pts, P, width=pr["width"])
    if got is None:
        return None
    right, status = got
    xyz = V.generate_keypoints_3d_stereo(pts, right, pr["camera"], status, lo, hi)
    kept = list(range(len(pts))) if filter == M.KEEP_ALL else V.filter_keypoints_by_depth_3d(xyz, lo, hi).tolist()
    return dict(right=right, status=status, xyz=xyz, kept=kept)


def _assert_mirror(pr, pts, P, filter=M.KEEP_ALL, lo=0.0, hi=0.0, what=""):
    want = M.frame(pr, pts, P, filter, lo, hi)
    got = _mirror_frame(pr, pts, P, filter, lo, hi)
    np.testing.assert_array_equal(got["status"], want["status"], err_msg=what)
    np.testing.assert_array_equal(I.bits(got["right"]), I.bits(want["right"]), err_msg=what)
    np.testing.assert_array_equal(I.bits(got["xyz"]), I.bits(want["xyz"]), err_msg=what)
    assert got["kept"] == want["kept"], what
    return want


@pytest.mark.parametrize("max_level", [0, 2, 5])
@pytest.mark.parametrize("width,height,win_w,win_h", I.SHAPES)
def test_host_mirror_equals_the_model(width, height, win_w, win_h, max_level):
    from rtabmap_amd import vwdictionary as V
    rng = np.random.default_rng(width + max_level)
    tracked = 0
    for kw in (dict(), dict(transform=I.TILT), dict(right_cx=0.0, pad=5)):
        pr, pts = I.random_frame(rng, width, height, 250, win_w, win_h, **kw)
        for mode in (1, 0):
            P = M.params(win_width=win_w, win_height=win_h, max_level=max_level, use_min_eigenvals=mode)
            for flt, lo, hi in ((M.KEEP_ALL, -1.0, 0.0), (M.FILTER_3D, 1.0, 4.0)):
                tracked += int(_assert_mirror(pr, pts, P, flt, lo, hi, what=str((kw.keys(), mode, flt)))["status"].sum())
        w = pr["width"]
        want = M.build_pyramid(pr["left"][:, :w], win_w, win_h, max_level)
        got = V.stereo_pyramid(pr["left"], win_w, win_h, max_level, width=w)
        assert len(got) == len(want) and all((a == b).all() for a, b in zip(got, want))
        dx, dy = M.scharr(want[-1])
        gx, gy = V.stereo_derivative(want[-1])
        assert (dx == gx).all() and (dy == gy).all()
    assert tracked > 500


def test_host_mirror_on_the_single_property_inputs_and_the_largest_window():
    for k, c in enumerate(I.all_cases(np.random.default_rng(5))):
        _assert_mirror(c["pair"], c["points"], c["P"], c.get("filter", M.KEEP_ALL), c.get("min_depth", 0.0), c.get("max_depth", 0.0), what="case %d" % k)
    pr, pts = I.random_frame(np.random.default_rng(31), 96, 80, 70, 31, 31)
    _assert_mirror(pr, pts, M.params(win_width=31, win_height=31, max_level=2), what="31 x 31")


def test_host_mirror_refuses_what_the_engine_refuses():
    from rtabmap_amd import vwdictionary as V
    pr, pts = I.random_frame(np.random.default_rng(2), 64, 48, 5)
    for pt in I.wild_points():
        assert V.stereo_correspondences(pr["left"], pr["right"], [pt]) is None
        with pytest.raises(M.Refused):
            M.frame(pr, [pt])
        assert M.frame(pr, [pt], device=True)["status"].tolist() == [0]
    for change in (dict(win_width=2), dict(win_height=32), dict(max_level=9), dict(max_level=-1), dict(win_width=64), dict(min_disparity=-1.0),
                   dict(min_disparity=3.0, max_disparity=2.0), dict(eps=float("nan")), dict(max_disparity=float("nan"))):
        assert V.stereo_correspondences(pr["left"], pr["right"], pts, change) is None, change
        with pytest.raises(M.Refused):
            M.frame(pr, pts, M.params(**change))
    for change in (dict(baseline=0.0), dict(fx=-1.0), dict(cx=float("nan"))):
        assert V.generate_keypoints_3d_stereo(pts, pts, dict(pr["camera"], **change)) is None
        with pytest.raises(M.Refused):
            M.frame(dict(pr, camera=dict(pr["camera"], **change)), pts)
    assert V.stereo_correspondences(pr["left"], pr["right"], np.zeros((0, 2), np.float32))[0].shape == (0, 2)
    # the clamps of util2d.cpp:493-501: 150 iterations are 100, eps 20 is 10, negative ones are 0
    for a, b in ((dict(iterations=150, eps=0.0), dict(iterations=100, eps=0.0)), (dict(eps=20.0), dict(eps=10.0)), (dict(iterations=-3), dict(iterations=0)),
                 (dict(eps=-1.0, iterations=3), dict(eps=0.0, iterations=3))):
        np.testing.assert_array_equal(I.bits(M.frame(pr, pts, M.params(**a))["right"]), I.bits(M.frame(pr, pts, M.params(**b))["right"]))
        _assert_mirror(pr, pts, M.params(**a))


def test_memory_hip_stereo_stage_keeps_what_the_model_keeps():
    """MemoryHip::update with a left and a right image and a stereo camera: the features that pass the tracker, the disparity gate, Kp/MinDepth
    and Kp/MaxDepth and their points are the model's, with or without a device (without one StereoOpticalFlowHip's host code runs the stage;
    the word ids need the engine and are the GPU suite's)"""
    from rtabmap_amd.vwdictionary import MemoryHip
    from helpers import unit_rows
    rng = np.random.default_rng(31)
    h = MemoryHip(max_features=100, min_depth=1.0, max_depth=4.0)
    for t, (n, kw, P) in enumerate(((300, dict(), None), (120, dict(transform=I.TILT), dict(win_width=5, win_height=5, max_level=2, max_disparity=4.0)),
                                    (300, dict(pad=3), dict(iterations=3, eps=0.1, min_disparity=2.5)))):
        pr, p = I.random_frame(rng, 64, 48, n, **kw)
        h.set_stereo_params(P)
        fr = M.frame(pr, p, M.params(**(P or {})), M.FILTER_3D, 1.0, 4.0)
        kept = fr["kept"]
        sid, ids, got_xyz, got_kept = h.update_stereo(unit_rows(n, 64, seed=40 + t), np.ones(n, np.float32), p, (64, 48), pr["left"], pr["right"], pr["camera"], width=pr["width"])
        assert sid == t + 1 and len(ids) == len(kept) and 0 < len(kept) < n, h.select_error()
        assert got_kept.tolist() == kept
        np.testing.assert_array_equal(I.bits(got_xyz), I.bits(fr["xyz"][kept]))
    bad = np.array([[np.nan, 1.0]] * 3, np.float32)
    assert h.update_stereo(unit_rows(3, 64, seed=50), np.ones(3, np.float32), bad, (64, 48), pr["left"], pr["right"], pr["camera"], width=pr["width"])[0] == 0
    assert "keypoint" in h.select_error()
    h.close()


def test_accuracy_against_the_float64_yardstick():
    """Smooth random textures whose right image is resampled at a known disparity (integer and fractional, 64 x 48 and 160 x 120).  The
    yardstick is an independent float64 tracker (tests/stereo_flow_yardstick.py); its largest error against the truth is recorded in DESIGN.md
    4q (0.0566 pixels, at disparity 6.7 on 160 x 120; the rule's is 0.0566 too).  The rule's largest error over the points both trackers keep
    stays within 4 x the recorded value, and the rule keeps at least 90 % of the points."""
    worst_yardstick = worst_rule = 0.0
    for width, height, disparity in Y.SCENES:
        left, right, pts, truth = Y.scene(width, height, disparity)
        rx, kept = Y.track(left, right, pts)
        assert kept.mean() >= 0.95
        fr = M.frame(M.pair(left, right, I.camera_for(width, height)), pts, M.params(min_disparity=0.0))
        tracked = fr["status"] == 1
        assert tracked.mean() >= 0.90, (width, height, disparity)
        both = kept & tracked
        worst_yardstick = max(worst_yardstick, float(np.abs(rx - truth)[kept].max()))
        worst_rule = max(worst_rule, float(np.abs(fr["right"][:, 0].astype(np.float64) - truth)[both].max()))
    print("yardstick %.6f rule %.6f recorded %.4f" % (worst_yardstick, worst_rule, Y.YARDSTICK_ERROR))
    assert 0.5 * Y.YARDSTICK_ERROR <= worst_yardstick <= 1.25 * Y.YARDSTICK_ERROR
    assert worst_rule <= Y.FACTOR * Y.YARDSTICK_ERROR
