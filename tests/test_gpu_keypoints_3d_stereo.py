"""GPU tests of lcd_keypoints_3d_stereo and lcd_keypoints_3d_stereo_dev (rtabmap_amd/csrc/keypoints_3d_stereo.hip) against
tests/stereo_flow_model.py.  Every comparison is exact: status, right corners, NaN positions and all other bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import feature_select_inputs as FS
import stereo_flow_inputs as I
import stereo_flow_model as M

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
MODES = ((M.KEEP_ALL, -1.0, 0.0), (M.FILTER_3D, 1.0, 4.0))


def _refused(status, call, *args, **kw):
    from rtabmap_amd import capi
    with pytest.raises(capi.LcdError) as err:
        call(*args, **kw)
    assert err.value.status == status, err.value


def _batch(rng, width, height, win_w, win_h, sizes):
    """one frame per size; a local transform, no right_cx and a pitch larger than the row take turns"""
    pairs, points = [], []
    for k, n in enumerate(sizes):
        kw = [dict(), dict(transform=I.TILT), dict(right_cx=0.0), dict(pad=5)][k % 4]
        pr, pts = I.random_frame(rng, width, height, n, win_w, win_h, **kw)
        pairs.append(pr)
        points.append(pts)
    return pairs, points


@pytest.mark.parametrize("max_level", [0, 2, 5])
@pytest.mark.parametrize("width,height,win_w,win_h", I.SHAPES)
def test_both_entries_equal_the_model(width, height, win_w, win_h, max_level):
    """frames of 0, 1, 63, 64, 65 and 1100 keypoints in ONE batch, both filter modes, responses, rows and a 12-byte payload carried along"""
    import rtabmap_amd
    rng = np.random.default_rng(width + max_level)
    P = M.params(win_width=win_w, win_height=win_h, max_level=max_level)
    pairs, points = _batch(rng, width, height, win_w, win_h, I.FRAME_SIZES)
    n_all = sum(I.FRAME_SIZES)
    resp = rng.standard_normal(n_all).astype(np.float32)
    rows = FS.rows_of(rng, "f32", 64, n_all)
    aux = rng.integers(0, 256, (n_all, 12), dtype=np.uint8)
    eng = rtabmap_amd.Engine("f32", 64)
    for flt, lo, hi in MODES:
        kw = dict(response=resp, rows=rows, aux=aux)
        want = M.batch(pairs, points, P, flt, lo, hi)
        I.assert_same(I.run_dev(eng, pairs, points, P, flt, lo, hi, **kw), pairs, points, P, flt, lo, hi, device=True, what=flt + " dev", want=want, **kw)
        I.assert_same(I.run_host(eng, pairs, points, P, flt, lo, hi, **kw), pairs, points, P, flt, lo, hi, what=flt + " host", want=want, **kw)
    assert sum(int(s.sum()) for s in want["status"]) > 300                  # the tracker did track
    got = I.run_dev(eng, pairs, points, P, M.FILTER_3D, 1.0, 4.0, tracks=False)      # out_right and out_status NULL
    I.assert_same(got, pairs, points, P, M.FILTER_3D, 1.0, 4.0, device=True, tracks=False, what="no tracks", want=want)
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


def test_largest_window():
    """31 x 31: sixteen window pixels per lane, the most LDS a workgroup asks for"""
    import rtabmap_amd
    rng = np.random.default_rng(31)
    P = M.params(win_width=31, win_height=31, max_level=2)
    pr, pts = I.random_frame(rng, 96, 80, 70, 31, 31)
    eng = rtabmap_amd.Engine("f32", 64)
    I.assert_same(I.run_dev(eng, [pr], [pts], P), [pr], [pts], P, device=True, what="dev")
    I.assert_same(I.run_host(eng, [pr], [pts], P), [pr], [pts], P, what="host")
    eng.close()


@pytest.mark.parametrize("kind,dim", FS.KINDS)
def test_rows_of_every_kind_and_payloads(kind, dim):
    """rows of each kind with payloads of 12 and 32 bytes (the last copied as 16-byte vectors); a padded handle's device entry refuses rows
    and serves the rest, its host entry serves rows"""
    import rtabmap_amd
    rng = np.random.default_rng(dim)
    P = M.params(win_width=5, win_height=3)
    pairs, points = _batch(rng, 40, 24, 5, 3, [65, 130, 0, 64])
    n_all = 65 + 130 + 64
    rows = FS.rows_of(rng, kind, dim, n_all)
    padded = kind == "u8" and dim % 4 != 0
    eng = rtabmap_amd.Engine(kind, dim)
    flt, lo, hi = M.FILTER_3D, 1.0, 4.0
    want = M.batch(pairs, points, P, flt, lo, hi)
    for aux_bytes in (12, 32):
        aux = rng.integers(0, 256, (n_all, aux_bytes), dtype=np.uint8)
        I.assert_same(I.run_host(eng, pairs, points, P, flt, lo, hi, rows=rows, aux=aux), pairs, points, P, flt, lo, hi, rows=rows, aux=aux, what="host", want=want)
        if padded:
            _refused(LCD_ERR_UNSUPPORTED, I.run_dev, eng, pairs, points, P, flt, lo, hi, rows=rows, aux=aux)
            I.assert_same(I.run_dev(eng, pairs, points, P, flt, lo, hi, aux=aux), pairs, points, P, flt, lo, hi, aux=aux, device=True, what="dev, no rows", want=want)
        else:
            I.assert_same(I.run_dev(eng, pairs, points, P, flt, lo, hi, rows=rows, aux=aux), pairs, points, P, flt, lo, hi, rows=rows, aux=aux, device=True, what="dev", want=want)
    eng.close()


def test_keypoints_the_reference_asserts_on():
    """NaN, inf, 1e20 among ordinary keypoints: the device entry gives them status 0, the right corner (NaN, NaN) and the bad point and is
    otherwise unaffected; the host entry refuses the call"""
    import rtabmap_amd
    rng = np.random.default_rng(3)
    eng = rtabmap_amd.Engine("f32", 64)
    pr, pts = I.random_frame(rng, 64, 48, 100)
    pts = np.concatenate([pts, I.wild_points()])[rng.permutation(108)]
    for flt, lo, hi in MODES:
        got = I.run_dev(eng, [pr], [pts], None, flt, lo, hi)
        I.assert_same(got, [pr], [pts], None, flt, lo, hi, device=True, what=flt)
        _refused(LCD_ERR_INVALID, I.run_host, eng, [pr], [pts], None, flt, lo, hi)
    wild = ~np.isfinite(pts).all(1) | (np.abs(pts) >= 2.0 ** 31).any(1)
    assert wild.sum() == 8 and (got["status"][wild] == 0).all() and np.isnan(got["right"][wild]).all()
    eng.close()


def test_single_property_inputs():
    """the inputs whose properties tests/test_stereo_flow_inputs.py proves, each through both entries"""
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    for k, c in enumerate(I.all_cases(np.random.default_rng(5))):
        args = ([c["pair"]], [c["points"]], c["P"], c.get("filter", M.KEEP_ALL), c.get("min_depth", 0.0), c.get("max_depth", 0.0))
        want = M.batch(*args)
        I.assert_same(I.run_dev(eng, *args), *args, device=True, what="case %d dev" % k, want=want)
        I.assert_same(I.run_host(eng, *args), *args, what="case %d host" % k, want=want)
    eng.close()


def test_70_frames_over_three_shared_pairs():
    import rtabmap_amd
    rng = np.random.default_rng(7)
    shared = [I.random_frame(rng, w, h, 0, **kw)[0] for w, h, kw in ((64, 48, dict()), (96, 40, dict(transform=I.TILT)), (64, 48, dict(pad=3)))]
    pools = [I.random_points(rng, 200, p["width"], p["left"].shape[0]) for p in shared]
    pairs, points = [], []
    for f in range(70):
        k = int(rng.integers(0, 9))
        a = int(rng.integers(0, 200 - k))
        pairs.append(shared[f % 3])
        points.append(pools[f % 3][a:a + k])
    eng = rtabmap_amd.Engine("f32", 64)
    want = M.batch(pairs, points, None, M.FILTER_3D, 1.0, 4.0)
    assert (want["count"] == 0).sum() > 5 and (want["count"] > 2).sum() > 5
    I.assert_same(I.run_dev(eng, pairs, points, None, M.FILTER_3D, 1.0, 4.0), pairs, points, None, M.FILTER_3D, 1.0, 4.0, device=True, what="dev", want=want)
    I.assert_same(I.run_host(eng, pairs, points, None, M.FILTER_3D, 1.0, 4.0), pairs, points, None, M.FILTER_3D, 1.0, 4.0, what="host", want=want)
    eng.close()


def test_a_filter_that_keeps_nothing_and_one_that_keeps_everything():
    import rtabmap_amd
    rng = np.random.default_rng(8)
    eng = rtabmap_amd.Engine("f32", 64)
    pr, _ = I.random_frame(rng, 64, 48, 0, disparity=3.0)
    pts = np.stack([rng.uniform(12, 50, 300), rng.uniform(4, 43, 300)], 1).astype(np.float32)
    want = M.batch([pr], [pts], None, M.FILTER_3D, 0.5, 0.0)
    assert want["count"].tolist() == [300]                                 # every keypoint is tracked and in range
    flat = M.pair(np.full((48, 64), 90, np.uint8), np.full((48, 64), 90, np.uint8), pr["camera"], 64)
    got = I.run_dev(eng, [pr, flat, pr], [pts, pts, pts[:70]], None, M.FILTER_3D, 0.5, 0.0)
    assert got["count"].tolist() == [300, 0, 70]
    assert (got["index"][300:600] == -1).all() and (got["index"][:300] == np.arange(300)).all()
    I.assert_same(got, [pr, flat, pr], [pts, pts, pts[:70]], None, M.FILTER_3D, 0.5, 0.0, device=True)
    got = I.run_dev(eng, [pr], [pts], None, M.FILTER_3D, 50.0, 0.0)      # everything is nearer than Kp/MinDepth
    assert got["count"].tolist() == [0] and (got["index"] == -1).all()
    eng.close()


def test_unsynchronised_back_to_back_calls():
    """three device calls in a row without a synchronisation in between (they alternate between the two job-table slots and share the
    pyramid scratch, which the stream orders); the scratch is counted in lcd_stats.bytes_device and reused"""
    import rtabmap_amd
    rng = np.random.default_rng(9)
    a = _batch(rng, 40, 24, 15, 3, [65])
    b = _batch(rng, 160, 120, 15, 3, [130, 200, 64])
    eng = rtabmap_amd.Engine("f32", 64)
    bytes0 = eng.stats()["bytes_device"]
    staged = [I.stage_dev(*x) for x in (b, a, b)]
    for st in staged:
        I.launch_dev(eng, st, None, M.FILTER_3D, 1.0, 4.0)
    for st, x in zip(staged, (b, a, b)):
        I.assert_same(I.to_host(eng, st), x[0], x[1], None, M.FILTER_3D, 1.0, 4.0, device=True)
    bytes1 = eng.stats()["bytes_device"]
    assert bytes1 > bytes0                                                 # the job table and the pyramids
    I.run_dev(eng, a[0], a[1])
    assert eng.stats()["bytes_device"] == bytes1                           # ... reused
    I.assert_same(I.run_host(eng, b[0], b[1], None, M.FILTER_3D, 1.0, 4.0), b[0], b[1], None, M.FILTER_3D, 1.0, 4.0)
    assert eng.stats()["bytes_device"] > bytes1                            # the staged inputs and results
    eng.close()


def test_error_table():
    """every refusal of include/lcd.h's list; after each of them nothing was written and the handle still serves a call"""
    import rtabmap_amd
    from rtabmap_amd import capi
    rng = np.random.default_rng(12)
    eng = rtabmap_amd.Engine("f32", 64)
    pr, pts = I.random_frame(rng, 64, 48, 100)
    images = I.api_images([pr])
    off = [0, 100]
    call = eng.keypoints_3d_stereo
    ok = dict(filter=M.FILTER_3D, min_depth=0.5, max_depth=3.0)
    # limits
    _refused(LCD_ERR_UNSUPPORTED, call, np.zeros((0, 2), np.float32), np.zeros(65537, np.int64), images, **ok)
    # offsets
    _refused(LCD_ERR_INVALID, call, pts, [1, 100], images, **ok)
    _refused(LCD_ERR_INVALID, call, pts, [0, 60, 50, 100], images * 3, **ok)
    # filter, bounds, aux_bytes
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter=3)
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter="filter_pixel", min_depth=0.5)
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter=M.FILTER_3D, min_depth=-1.0)
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter=M.KEEP_ALL, min_depth=2.0, max_depth=2.0)
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter=M.KEEP_ALL, min_depth=float("nan"))
    _refused(LCD_ERR_INVALID, call, pts, off, images, aux=np.zeros((100, 6), np.uint8), **ok)
    _refused(LCD_ERR_INVALID, call, pts, off, images, aux=np.zeros((100, 68), np.uint8), **ok)
    # the parameters
    for change in (dict(win_width=2), dict(win_width=32), dict(win_height=2), dict(win_height=33), dict(max_level=-1), dict(max_level=9),
                   dict(win_width=64), dict(win_width=63, win_height=48), dict(eps=float("nan")), dict(min_eig_threshold=float("nan")),
                   dict(error_threshold=float("nan")), dict(min_disparity=float("nan")), dict(max_disparity=float("nan")), dict(min_disparity=-0.5),
                   dict(min_disparity=3.0, max_disparity=2.0)):
        _refused(LCD_ERR_INVALID, call, pts, off, images, params=change, **ok)
    _refused(LCD_ERR_INVALID, call, pts, off, [dict(images[0], width=15)], **ok)                  # width <= win_width
    _refused(LCD_ERR_INVALID, call, pts, off, [dict(images[0], height=3)], **ok)
    # the images and the camera
    for change in (dict(left_pitch_bytes=63), dict(right_pitch_bytes=10), dict(left=None), dict(right=None), dict(camera=None)):
        _refused(LCD_ERR_INVALID, call, pts, off, [dict(images[0], **change)], **ok)
    for change in (dict(baseline=0.0), dict(baseline=-1.0), dict(fx=0.0), dict(fx=float("nan")), dict(cy=float("nan")), dict(right_cx=float("nan"))):
        _refused(LCD_ERR_INVALID, call, pts, off, [dict(images[0], camera=dict(pr["camera"], **change))], **ok)
    # struct_size and NULL pointers, checking that nothing is written
    o = np.array(off, np.int64)
    count, index = np.full(1, I.CANARY, np.int32), np.full(100, I.CANARY, np.int32)
    xyz, out_pts = np.full((100, 3), I.CANARY, np.float32), np.full((100, 2), I.CANARY, np.float32)
    arr, keep = eng._stereo_images(images, lambda a: a.ctypes.data)
    sp = capi.stereo_params()
    full = C.sizeof(capi.LcdKeypoints3dStereoArgs)
    a = capi.LcdKeypoints3dStereoArgs(full, 1, capi.LCD_KP3D_FILTER_3D, 0, 0.5, 3.0)
    a.offsets, a.images, a.params, a.points = o.ctypes.data, arr, C.pointer(sp), pts.ctypes.data
    a.out_count, a.out_index, a.out_xyz, a.out_points = count.ctypes.data, index.ctypes.data, xyz.ctypes.data, out_pts.ctypes.data
    for field, value in (("struct_size", full - 8), ("out_index", None), ("out_xyz", None), ("out_points", None), ("points", None), ("out_count", None),
                         ("response", pts.ctypes.data), ("rows", pts.ctypes.data), ("offsets", None)):
        before = getattr(a, field)
        setattr(a, field, value)
        assert eng.L.lcd_keypoints_3d_stereo(eng.h, C.byref(a)) == LCD_ERR_INVALID, field
        setattr(a, field, before)
    a.images = None
    assert eng.L.lcd_keypoints_3d_stereo(eng.h, C.byref(a)) == LCD_ERR_INVALID
    a.images = arr
    a.params = None
    assert eng.L.lcd_keypoints_3d_stereo(eng.h, C.byref(a)) == LCD_ERR_INVALID
    for buf in (count, index, xyz, out_pts):
        assert (buf == I.CANARY).all()
    # the device entry refuses the same before anything is enqueued
    st = I.stage_dev([pr], [pts])
    dev = eng.keypoints_3d_stereo_dev
    _refused(LCD_ERR_INVALID, dev, st["pts"], off, st["images"], st["count"], st["index"], st["xyz"], filter=7, d_out_points=st["points"])
    _refused(LCD_ERR_INVALID, dev, st["pts"], off, st["images"], st["count"], None, st["xyz"], d_out_points=st["points"])
    _refused(LCD_ERR_INVALID, dev, st["pts"], off, st["images"], st["count"], st["index"], None)
    _refused(LCD_ERR_INVALID, dev, st["pts"], off, st["images"], st["count"], st["index"], st["xyz"], filter=M.FILTER_3D)
    _refused(LCD_ERR_INVALID, dev, st["pts"], off, [dict(st["images"][0], left_pitch_bytes=2)], st["count"], st["index"], st["xyz"])
    _refused(LCD_ERR_UNSUPPORTED, dev, st["pts"], np.zeros(65537, np.int64), st["images"], st["count"], st["index"], st["xyz"])
    eng.synchronize()
    got = I.to_host(eng, st)
    assert all((got[k] == I.CANARY).all() for k in ("count", "index", "xyz", "points", "right")) and (got["status"] == 249).all()
    # n_frames == 0 is LCD_OK, and the handle still works
    assert call(np.zeros((0, 2), np.float32), [0], [])["count"].shape == (0,)
    I.assert_same(I.run_host(eng, [pr], [pts], None, M.FILTER_3D, 0.5, 3.0), [pr], [pts], None, M.FILTER_3D, 0.5, 3.0)
    I.assert_same(I.run_dev(eng, [pr], [pts], None, M.FILTER_3D, 0.5, 3.0), [pr], [pts], None, M.FILTER_3D, 0.5, 3.0, device=True)
    eng.close()
