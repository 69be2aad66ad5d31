"""GPU tests of lcd_keypoints_3d and lcd_keypoints_3d_dev (rtabmap_amd/csrc/keypoints_3d.hip) against tests/keypoints_3d_model.py.  Every
comparison is exact: NaN positions and all other bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import feature_select_inputs as FS
import keypoints_3d_inputs as I
import keypoints_3d_model as M

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
MODES = ((M.KEEP_ALL, -1.0, 0.0), (M.FILTER_3D, 1.5, 3.0), (M.FILTER_PIXEL, 1.5, 3.0))


def _refused(status, call, *args, **kw):
    from rtabmap_amd import capi
    with pytest.raises(capi.LcdError) as err:
        call(*args, **kw)
    assert err.value.status == status, err.value


def _batch(rng, dtype, width, height, sizes, host_ok):
    """one frame per size; the cameras (1, 2, 4 where the width divides), a local transform, a colour image of another size, a pitch larger
    than the row and a principal point that is not given take turns"""
    cams = [c for c in (1, 2, 4) if width % c == 0]
    images, points = [], []
    for k, n in enumerate(sizes):
        nc = cams[k % len(cams)]
        kw = [dict(), dict(transform=I.TILT), dict(image_size=(width // nc * 3 + 1, height * 2)), dict(pad=3, zero_principal=True)][k % 4]
        im, pts = I.random_frame(rng, dtype, width, height, nc, n, host_ok=host_ok, **kw)
        images.append(im)
        points.append(pts)
    return images, points


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("width,height", I.SHAPES)
def test_both_entries_equal_the_model(dtype, width, height):
    """frames of 0, 1, 63, 64, 65, 255, 256, 257 and 1100 keypoints in ONE batch, every filter mode, responses and a 12-byte payload carried along"""
    import rtabmap_amd
    rng = np.random.default_rng(width + (0 if dtype == np.uint16 else 1))
    images, points = _batch(rng, dtype, width, height, I.FRAME_SIZES, host_ok=True)
    n_all = sum(I.FRAME_SIZES)
    resp = rng.standard_normal(n_all).astype(np.float32)
    rows = FS.rows_of(rng, "f32", 64, n_all)
    aux = rng.integers(0, 256, (n_all, 12), dtype=np.uint8)
    eng = rtabmap_amd.Engine("f32", 64)
    for flt, lo, hi in MODES:
        kw = dict(response=resp, rows=rows, aux=aux)
        want = M.batch(images, points, flt, lo, hi)                         # no keypoint here is one the two entries differ on
        I.assert_same(I.run_dev(eng, images, points, flt, lo, hi, **kw), images, points, flt, lo, hi, device=True, what=flt + " dev", want=want, **kw)
        I.assert_same(I.run_host(eng, images, points, flt, lo, hi, **kw), images, points, flt, lo, hi, what=flt + " host", want=want, **kw)
    got = I.run_dev(eng, images, points, M.FILTER_PIXEL, 1.5, 3.0, with_xyz=False)              # the pixel filter alone: no point is computed
    I.assert_same(got, images, points, M.FILTER_PIXEL, 1.5, 3.0, device=True, with_xyz=False, what="pixel, no xyz")
    assert eng.vocab_count() == (0, 0) and eng.sig_count() == (0, 0)
    eng.close()


@pytest.mark.parametrize("kind,dim", FS.KINDS)
def test_rows_of_every_kind_and_payloads(kind, dim):
    """rows of each kind with payloads of 12, 28 and 32 bytes (the last copied as 16-byte vectors); a padded handle's device entry refuses
    rows and serves the rest, its host entry serves rows"""
    import rtabmap_amd
    rng = np.random.default_rng(dim)
    images, points = _batch(rng, np.uint16, 16, 12, [65, 257, 0, 64], host_ok=True)
    n_all = 65 + 257 + 64
    rows = FS.rows_of(rng, kind, dim, n_all)
    padded = kind == "u8" and dim % 4 != 0
    eng = rtabmap_amd.Engine(kind, dim)
    for aux_bytes in (12, 28, 32):
        aux = rng.integers(0, 256, (n_all, aux_bytes), dtype=np.uint8)
        flt, lo, hi = M.FILTER_3D, 1.5, 3.0
        I.assert_same(I.run_host(eng, images, points, flt, lo, hi, rows=rows, aux=aux), images, points, flt, lo, hi, rows=rows, aux=aux, what="host")
        if padded:
            _refused(LCD_ERR_UNSUPPORTED, I.run_dev, eng, images, points, flt, lo, hi, rows=rows, aux=aux)
            I.assert_same(I.run_dev(eng, images, points, flt, lo, hi, aux=aux), images, points, flt, lo, hi, aux=aux, device=True, what="dev, no rows")
        else:
            I.assert_same(I.run_dev(eng, images, points, flt, lo, hi, rows=rows, aux=aux), images, points, flt, lo, hi, rows=rows, aux=aux, device=True, what="dev")
    eng.close()


def test_keypoints_the_reference_asserts_on():
    """NaN, inf, 1e20 and out-of-camera coordinates among ordinary ones: the device entry gives them the bad point, keeps them under no
    filter and is otherwise unaffected; the host entry refuses the call and writes nothing"""
    import rtabmap_amd
    rng = np.random.default_rng(3)
    eng = rtabmap_amd.Engine("f32", 64)
    for dtype, nc in ((np.uint16, 1), (np.float32, 2), (np.uint16, 4)):
        im, pts = I.random_frame(rng, dtype, 16, 12, nc, 300)
        pts = np.concatenate([pts, I.wild_points()])[rng.permutation(308)]
        bad = [not M.point_of(im, p, device=True)[1] for p in pts]
        assert sum(bad) > 10
        for flt, lo, hi in MODES:
            I.assert_same(I.run_dev(eng, [im], [pts], flt, lo, hi), [im], [pts], flt, lo, hi, device=True, what=flt)
            _refused(LCD_ERR_INVALID, I.run_host, eng, [im], [pts], flt, lo, hi)
    eng.close()


def test_single_property_inputs():
    """the inputs whose properties tests/test_keypoints_3d_inputs.py proves: the strict band edge, the loop order, the seams, the principal
    point fallback, the range bounds met exactly, and the two inputs on which a fused multiply-add is told from the rule"""
    import rtabmap_amd
    rng = np.random.default_rng(5)
    eng = rtabmap_amd.Engine("f32", 64)
    cases = []
    exact, inside, pts = I.band_edge_case()
    order, opts = I.loop_order_case(rng)
    for data, p in ((exact, pts), (inside, pts), (order, opts)):
        cases.append((M.image(data, I.cameras_for(3, 3, 1)), p, M.KEEP_ALL, 0.0, 0.0))
    for dtype in (np.uint16, np.float32):
        for nc in (2, 4):
            d, p = I.seam_case(rng, dtype, nc)
            cases.append((M.image(d, I.cameras_for(d.shape[1] // nc, d.shape[0], nc)), p, M.KEEP_ALL, 0.0, 0.0))
    d, cams, p = I.fma_transform_case(rng)
    cases.append((M.image(d, cams), p, M.KEEP_ALL, 0.0, 0.0))
    d, cams, p, lo, hi = I.fma_dist_case(rng)
    cases.append((M.image(d, cams), p, M.FILTER_3D, lo, hi))
    one = np.zeros((3, 3), np.float32)
    ident = I.cameras_for(3, 3, 1)
    centre = [(ident[0]["cx"], ident[0]["cy"])]
    for pixel in (3.0, float(I.down(3.0)), float(I.up(3.0, 2))):
        e = one.copy()
        e[1, 1] = pixel
        for lo, hi in ((3.0, 0.0), (0.0, 3.0), (float(I.down(3.0)), 0.0)):
            cases.append((M.image(e, ident), centre, M.FILTER_3D, lo, hi))               # Z against Kp/MinDepth and Kp/MaxDepth
        for shift, lo, hi in ((-1.0, 2.0, 0.0), (1.0, 0.0, 4.0)):
            t = list(I.IDENTITY)
            t[11] = shift
            cam = [M.camera(ident[0]["fx"], ident[0]["fy"], ident[0]["cx"], ident[0]["cy"], transform=t)]
            cases.append((M.image(e, cam), centre, M.FILTER_3D, lo, hi))                  # d2 against the squared bounds
    cases.append((M.image(np.full((12, 16), 2.0, np.float32), I.cameras_for(16, 12, 1, zero_principal=True)), [(7.5, 5.5), (8.5, 5.5), (0.0, 0.0)], M.KEEP_ALL, 0.0, 0.0))
    counts = set()
    for k, (im, p, flt, lo, hi) in enumerate(cases):
        p = np.asarray(p, np.float32).reshape(-1, 2)
        got = I.run_dev(eng, [im], [p], flt, lo, hi)
        I.assert_same(got, [im], [p], flt, lo, hi, device=True, what="case %d dev" % k)
        I.assert_same(I.run_host(eng, [im], [p], flt, lo, hi), [im], [p], flt, lo, hi, what="case %d host" % k)
        counts.add((flt, int(got["count"][0])))
    assert (M.FILTER_3D, 0) in counts and (M.FILTER_3D, 1) in counts
    eng.close()


def test_700_frames_over_shared_images():
    import rtabmap_amd
    rng = np.random.default_rng(7)
    shared = [I.random_frame(rng, dt, w, h, nc, 0, host_ok=True)[0] for dt, w, h, nc in
              ((np.uint16, 16, 12, 1), (np.float32, 16, 12, 2), (np.uint16, 64, 48, 4), (np.float32, 5, 4, 1), (np.uint16, 16, 12, 4))]
    images, points = [], []
    pools = [I.random_frame(rng, im["data"].dtype.type, im["width"], im["data"].shape[0], len(im["cameras"]), 400, host_ok=True)[1] for im in shared]
    for f in range(700):
        k = int(rng.integers(0, 9))
        a = int(rng.integers(0, 400 - k))
        images.append(shared[f % 5])
        points.append(pools[f % 5][a:a + k])
    eng = rtabmap_amd.Engine("f32", 64)
    want = M.batch(images, points, M.FILTER_3D, 1.5, 3.0)
    assert (want["count"] == 0).sum() > 50 and (want["count"] > 2).sum() > 50
    I.assert_same(I.run_dev(eng, images, points, M.FILTER_3D, 1.5, 3.0), images, points, M.FILTER_3D, 1.5, 3.0, device=True, what="dev", want=want)
    I.assert_same(I.run_host(eng, images, points, M.FILTER_3D, 1.5, 3.0), images, points, M.FILTER_3D, 1.5, 3.0, what="host", want=want)
    eng.close()


def test_a_filter_that_keeps_nothing_and_one_that_keeps_everything():
    import rtabmap_amd
    rng = np.random.default_rng(8)
    eng = rtabmap_amd.Engine("f32", 64)
    pts = np.stack([rng.uniform(0, 15, 600), rng.uniform(0, 11, 600)], 1).astype(np.float32)
    for dtype, value in ((np.uint16, 2000), (np.float32, 2.0)):
        full = M.image(np.full((12, 16), value, dtype), I.cameras_for(16, 12, 1))
        empty = M.image(np.zeros((12, 16), dtype), I.cameras_for(16, 12, 1))
        for flt in (M.FILTER_3D, M.FILTER_PIXEL):
            got = I.run_dev(eng, [full, empty, full], [pts, pts, pts[:70]], flt, 0.5, 0.0)
            assert got["count"].tolist() == [600, 0, 70]
            assert (got["index"][600:1200] == -1).all() and (got["index"][:600] == np.arange(600)).all()
            I.assert_same(got, [full, empty, full], [pts, pts, pts[:70]], flt, 0.5, 0.0, device=True)
            got = I.run_dev(eng, [full], [pts], flt, 2.5, 0.0)                          # everything is nearer than Kp/MinDepth
            assert got["count"].tolist() == [0] and (got["index"] == -1).all()
    eng.close()


def test_unsynchronised_back_to_back_calls():
    """three device calls in a row without a synchronisation in between (they alternate between the two job-table slots); the scratch is
    counted in lcd_stats.bytes_device and reused"""
    import rtabmap_amd
    rng = np.random.default_rng(9)
    a = _batch(rng, np.uint16, 16, 12, [65], host_ok=True)
    b = _batch(rng, np.float32, 64, 48, [257, 300, 64], host_ok=True)
    eng = rtabmap_amd.Engine("f32", 64)
    bytes0 = eng.stats()["bytes_device"]
    staged = [I.stage_dev(*x) for x in (a, b, a)]
    for st in staged:
        I.launch_dev(eng, st, M.FILTER_3D, 1.5, 3.0)
    for st, x in zip(staged, (a, b, a)):
        I.assert_same(I.to_host(eng, st), x[0], x[1], M.FILTER_3D, 1.5, 3.0, device=True)
    bytes1 = eng.stats()["bytes_device"]
    assert bytes1 > bytes0                                                 # the job table
    I.run_dev(eng, a[0], a[1], M.KEEP_ALL, 0.0, 0.0)
    assert eng.stats()["bytes_device"] == bytes1                           # ... reused
    I.assert_same(I.run_host(eng, b[0], b[1], M.FILTER_3D, 1.5, 3.0), b[0], b[1], M.FILTER_3D, 1.5, 3.0)
    assert eng.stats()["bytes_device"] > bytes1                            # the staged inputs and results
    eng.close()


def test_error_table():
    """every refusal of include/lcd.h's list; after each of them nothing was written and the handle still serves a call"""
    import rtabmap_amd
    from rtabmap_amd import capi
    rng = np.random.default_rng(12)
    eng = rtabmap_amd.Engine("f32", 64)
    im, pts = I.random_frame(rng, np.uint16, 16, 12, 2, 100, host_ok=True)
    images = I.api_images([im])
    off = [0, 100]
    call = eng.keypoints_3d
    ok = dict(filter=M.FILTER_3D, min_depth=0.5, max_depth=3.0)
    # limits
    _refused(LCD_ERR_UNSUPPORTED, call, np.zeros((0, 2), np.float32), np.zeros(65537, np.int64), images, **ok)          # (refused before an image is read)
    # offsets
    _refused(LCD_ERR_INVALID, call, pts, [1, 100], images, **ok)
    _refused(LCD_ERR_INVALID, call, pts, [0, 60, 50, 100], images * 3, **ok)
    # filter, bounds, aux_bytes
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter=3)
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter=M.FILTER_3D, min_depth=-1.0)
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter=M.FILTER_PIXEL, min_depth=-0.5)
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter=M.KEEP_ALL, min_depth=2.0, max_depth=2.0)
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter=M.FILTER_3D, min_depth=2.0, max_depth=1.0)
    _refused(LCD_ERR_INVALID, call, pts, off, images, filter=M.KEEP_ALL, min_depth=float("nan"))
    _refused(LCD_ERR_INVALID, call, pts, off, images, aux=np.zeros((100, 6), np.uint8), **ok)
    _refused(LCD_ERR_INVALID, call, pts, off, images, aux=np.zeros((100, 68), np.uint8), **ok)
    # the image
    for change in (dict(n_cameras=3, cameras=im["cameras"] * 2), dict(type=2), dict(pitch_bytes=30), dict(pitch_bytes=33), dict(width=0), dict(height=0), dict(n_cameras=0)):
        _refused(LCD_ERR_INVALID, call, pts, off, [dict(images[0], **change)], **ok)
    # struct_size and NULL pointers, checking that nothing is written
    o = np.array(off, np.int64)
    count, index = np.full(1, I.CANARY, np.int32), np.full(100, I.CANARY, np.int32)
    xyz, out_pts = np.full((100, 3), I.CANARY, np.float32), np.full((100, 2), I.CANARY, np.float32)
    arr, keep = eng._kp3d_images(images, lambda a: a.ctypes.data)
    a = capi.LcdKeypoints3dArgs(C.sizeof(capi.LcdKeypoints3dArgs) - 8, 1, capi.LCD_KP3D_FILTER_3D, 0, 0.5, 3.0)
    a.offsets, a.images, a.points = o.ctypes.data, arr, pts.ctypes.data
    a.out_count, a.out_index, a.out_xyz, a.out_points = count.ctypes.data, index.ctypes.data, xyz.ctypes.data, out_pts.ctypes.data
    full = C.sizeof(capi.LcdKeypoints3dArgs)
    for field, value in (("struct_size", full - 8), ("out_index", None), ("out_xyz", None), ("out_points", None), ("points", None), ("out_count", None),
                         ("response", pts.ctypes.data), ("rows", pts.ctypes.data), ("offsets", None)):
        before = getattr(a, field)
        setattr(a, field, value)
        if field != "struct_size":
            a.struct_size = full
        assert eng.L.lcd_keypoints_3d(eng.h, C.byref(a)) == LCD_ERR_INVALID, field
        setattr(a, field, before)
    a.images = None
    assert eng.L.lcd_keypoints_3d(eng.h, C.byref(a)) == LCD_ERR_INVALID
    a.images = arr
    a.filter, a.out_xyz = capi.LCD_KP3D_KEEP_ALL, None
    assert eng.L.lcd_keypoints_3d(eng.h, C.byref(a)) == LCD_ERR_INVALID                       # only the pixel filter goes without out_xyz
    for buf in (count, index, xyz, out_pts):
        assert (buf == I.CANARY).all()
    # the device entry refuses the same before anything is enqueued
    st = I.stage_dev([im], [pts])
    _refused(LCD_ERR_INVALID, eng.keypoints_3d_dev, st["pts"], off, st["images"], st["count"], st["index"], st["xyz"], filter=7, d_out_points=st["points"])
    _refused(LCD_ERR_INVALID, eng.keypoints_3d_dev, st["pts"], off, st["images"], st["count"], None, st["xyz"], d_out_points=st["points"])
    _refused(LCD_ERR_INVALID, eng.keypoints_3d_dev, st["pts"], off, st["images"], st["count"], st["index"], st["xyz"], filter=M.FILTER_3D)
    _refused(LCD_ERR_INVALID, eng.keypoints_3d_dev, st["pts"], off, [dict(st["images"][0], pitch_bytes=2)], st["count"], st["index"], st["xyz"])
    _refused(LCD_ERR_UNSUPPORTED, eng.keypoints_3d_dev, st["pts"], np.zeros(65537, np.int64), st["images"], st["count"], st["index"], st["xyz"])
    eng.synchronize()
    got = I.to_host(eng, st)
    assert all((got[k] == I.CANARY).all() for k in ("count", "index", "xyz", "points"))
    # n_frames == 0 is LCD_OK, and the handle still works
    assert call(np.zeros((0, 2), np.float32), [0], [])["count"].shape == (0,)
    I.assert_same(I.run_host(eng, [im], [pts], M.FILTER_3D, 0.5, 3.0), [im], [pts], M.FILTER_3D, 0.5, 3.0)
    I.assert_same(I.run_dev(eng, [im], [pts], M.FILTER_3D, 0.5, 3.0), [im], [pts], M.FILTER_3D, 0.5, 3.0, device=True)
    eng.close()
