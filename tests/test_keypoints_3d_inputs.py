"""The generators of tests/keypoints_3d_inputs.py produce what they promise: every input has, on the model, the property it is there for.
No GPU."""
import numpy as np
import pytest

import keypoints_3d_inputs as I
import keypoints_3d_model as M

F = np.float32


def _one(data, cams=None, width=None):
    return M.image(data, cams or I.cameras_for(data.shape[1] if width is None else width, data.shape[0], 1), width)


def _flat(dtype, width, height, value=2.0):
    return np.full((height, width), 2000 if dtype == np.uint16 else value, dtype)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_rounding_and_clamp_at_the_borders(dtype):
    """x + 0.5f == cols with x < cols is clamped onto the last column, x == cols is outside; (-1.5, -0.5) lands on pixel 0, -1.5 is outside"""
    cols, rows = 16, 12
    im = _one(_flat(dtype, cols, rows))
    seen = lambda x, y: (lambda r: (M.point_of(im, (x, y), reads=r), r))([])
    for x, y, centre in ((cols - 0.5, 3.0, (cols - 1, 3)), (float(I.down(cols)), 3.0, (cols - 1, 3)), (3.0, rows - 0.5, (3, rows - 1)),
                         (3.0, float(I.down(rows)), (3, rows - 1)), (-1.0, 3.0, (0, 3)), (-0.75, 3.0, (0, 3)), (3.0, -1.0, (3, 0)), (-1.0, -1.0, (0, 0))):
        assert F(x) < cols and F(y) < rows
        (p, defined), reads = seen(x, y)
        assert defined and np.isfinite(p).all() and reads[0] == centre, (x, y)
    assert int(F(cols - 0.5) + F(0.5)) == cols and int(F(-1.0) + F(0.5)) == 0
    for x, y in ((3.0, float(rows)), (-1.5, 3.0), (3.0, -1.5), (3.0, rows + 0.5)):
        (p, defined), reads = seen(x, y)
        assert defined and np.isnan(p).all() and reads == [], (x, y)
    # x == cols is the next camera's first column: with a next camera its pixel 0, without one the reference's assertion
    with pytest.raises(M.Refused):
        M.point_of(im, (float(cols), 3.0))
    assert not M.point_of(im, (float(cols), 3.0), device=True)[1]
    two = M.image(_flat(dtype, 2 * cols, rows), I.cameras_for(cols, rows, 2))
    reads = []
    assert np.isfinite(M.point_of(two, (float(cols), 3.0), reads=reads)[0]).all() and reads[0] == (cols, 3)
    pts = I.border_points(cols, rows)
    for x, y in ((cols - 0.5, rows - 0.5), (float(cols), 0.0), (-1.0, -1.0), (-1.5, 0.0), (0.0, -1.5), (0.0, float(rows))):
        assert ((pts[:, 0] == F(x)) & (pts[:, 1] == F(y))).any(), (x, y)


def test_corners_and_edges_have_clipped_windows():
    cols, rows = 5, 4
    im = _one(_flat(np.float32, cols, rows))
    sizes = {}
    for x in (0.0, 2.0, cols - 1.0):
        for y in (0.0, 2.0, rows - 1.0):
            r = []
            M.point_of(im, (x, y), reads=r)
            sizes[(x, y)] = len(r)
            assert all(0 <= c < cols and 0 <= v < rows for c, v in r)
    assert sorted(set(sizes.values())) == [4, 6, 9] and sizes[(0.0, 0.0)] == 4 and sizes[(2.0, 0.0)] == 6 and sizes[(2.0, 2.0)] == 9
    pts = I.border_points(cols, rows)
    for x, y in ((0.0, 0.0), (cols - 1.0, 0.0), (0.0, rows - 1.0), (cols - 1.0, rows - 1.0), (cols / 2, 0.0), (0.0, rows / 2), (cols - 1.0, rows / 2)):
        assert ((pts[:, 0] == F(x)) & (pts[:, 1] == F(y))).any(), (x, y)


def test_wild_coordinates_are_refused_on_the_host_and_bad_points_on_the_device():
    im = _one(_flat(np.float32, 16, 12))
    for pt in I.wild_points():
        with pytest.raises(M.Refused):
            M.point_of(im, pt)
        r = []
        p, defined = M.point_of(im, pt, device=True, reads=r)
        assert not defined and np.isnan(p).all() and r == []
        assert M.frame(im, [pt], M.FILTER_3D, device=True)[0] == [] and M.frame(im, [pt], M.KEEP_ALL, device=True)[0] == [0]
    for pt in I.wild_points()[:6]:
        with pytest.raises(M.Refused):
            M.keep_pixel(im, pt, 0.0, 0.0)
        assert M.keep_pixel(im, pt, 0.0, 0.0, device=True) == (False, False)
    # a keypoint of a camera that does not exist: x / subW >= n_cameras
    two = M.image(_flat(np.float32, 16, 12), I.cameras_for(8, 12, 2))
    assert M.point_of(two, (15.9, 1.0))[1]
    with pytest.raises(M.Refused):
        M.point_of(two, (16.0, 1.0))
    with pytest.raises(M.Refused):
        M.point_of(two, (-8.0, 1.0))
    assert M.point_of(two, (-7.9, 1.0), device=True)[1]                      # int(-0.98) == 0: camera 0, outside its sub-image


def test_pixels_that_are_no_measurement():
    """u16 0 and 65535, f32 0, NaN, inf and a negative depth: at the centre there is no point, among the neighbours they do not count"""
    for dtype, bad_values in ((np.uint16, [0, 65535]), (np.float32, [0.0, np.nan, np.inf, -1.5])):
        for bad in bad_values:
            d = _flat(dtype, 5, 4)
            d[1, 1] = 2010 if dtype == np.uint16 else 2.01
            d[2, 2] = bad
            im = _one(d)
            assert np.isnan(M.point_of(im, (2.0, 2.0))[0]).all(), bad                       # the centre
            full = M.point_of(_one(_flat(dtype, 5, 4)), (1.0, 2.0))[0]
            assert np.isfinite(M.point_of(im, (1.0, 2.0))[0]).all()
            d2 = _flat(dtype, 5, 4)
            d2[2, 2] = 2030 if dtype == np.uint16 else 2.03                                 # ... where a valid neighbour changes Z
            assert M.point_of(_one(d2), (1.0, 2.0))[0][2] != full[2]
            d3 = _flat(dtype, 5, 4)
            d3[2, 2] = bad                                                                  # ... and this one leaves the sums alone
            centre = F(2000) * F(0.001) if dtype == np.uint16 else F(2.0)
            assert M.point_of(_one(d3), (1.0, 2.0))[0][2] == (centre * F(4) + (centre * F(2)) * F(3) + centre * F(4)) / F(14)
    # the surfaces of the GPU tests contain all of them, at centres and among neighbours
    rng = np.random.default_rng(1)
    s16, s32 = I.surface(rng, np.uint16, 64, 48), I.surface(rng, np.float32, 64, 48)
    assert (s16 == 0).any() and (s16 == 65535).any()
    assert (s32 == 0).any() and np.isnan(s32).any() and np.isinf(s32).any() and (s32 < 0).any()
    # the pixel filter reads u16 0 and 65535 as 0 and 65.535 metres: no 0 / 65535 test there
    d = np.array([[0, 65535, 1000]], np.uint16)
    im = _one(d)
    assert [M.keep_pixel(im, (x, 0.0), 0.0, 0.0)[0] for x in (0.0, 1.0, 2.0)] == [False, True, True]
    assert M.keep_pixel(im, (1.0, 0.0), 0.0, 65.0)[0] is False
    # a negative f32 depth passes no range: depth > 0 is required even with min_depth < 0
    neg = _one(np.full((3, 3), -2.0, np.float32))
    assert np.isnan(M.point_of(neg, (1.0, 1.0), min_depth=-1.0)[0]).all()


def test_band_edge_is_strict():
    exact, inside, pts = I.band_edge_case()
    D, d = exact[1, 1], exact[1, 2]
    assert d - D == F(0.02) * D and inside[1, 2] == I.down(d)
    z_exact = M.point_of(_one(exact), pts[0])[0][2]
    z_inside = M.point_of(_one(inside), pts[0])[0][2]
    assert z_exact == D                                                       # (4 D + 0) / 4: the neighbour at the edge does not count
    assert z_inside == (D * F(4) + inside[1, 2] * F(2)) / F(6) and z_inside != D


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("n_cameras", [2, 4])
def test_windows_stop_at_the_seam(dtype, n_cameras):
    """on the first and last column of every sub-image the pixel across the seam is valid and would change the result if it were read"""
    rng = np.random.default_rng(n_cameras)
    d, pts = I.seam_case(rng, dtype, n_cameras)
    sub = d.shape[1] // n_cameras
    im = M.image(d, I.cameras_for(sub, d.shape[0], n_cameras))
    changed = 0
    for pt in pts:
        reads = []
        p, defined = M.point_of(im, pt, reads=reads)
        cam = int(pt[0] // sub)
        assert defined and np.isfinite(p).all()
        assert all(cam * sub <= c < (cam + 1) * sub for c, _ in reads), pt
        u = int(F(pt[0]) - F(cam * sub) + F(0.5))
        across = cam * sub - 1 if u == 0 else (cam + 1) * sub
        assert u in (0, sub - 1)
        if not 0 <= across < d.shape[1]:
            continue                                                            # the image's own border: nothing lies beyond
        whole = M.get_depth(im, 0, d.shape[1], F(pt[0]), F(pt[1]))             # the window clipped to the whole image instead
        assert M.pixel(im, across, int(pt[1])) > 0
        assert whole != p[2], pt
        changed += 1
    assert changed >= 6 * (n_cameras - 1)


def test_loop_order_matters():
    a, pts = I.loop_order_case(np.random.default_rng(3))
    im = _one(a)
    assert M.point_of(im, pts[0])[0][2] != M.point_of(im, pts[0], order="vu")[0][2]


def test_principal_point_fallback():
    d = _flat(np.float32, 16, 12)
    im = _one(d, I.cameras_for(16, 12, 1, zero_principal=True))
    assert im["cameras"][0]["cx"] == 0.0 and im["cameras"][0]["cy"] < 0
    p = M.point_of(im, (7.5, 5.5))[0]
    assert p[0] == 0 and p[1] == 0 and p[2] == 2                               # cols / 2 - 0.5, rows / 2 - 0.5
    assert M.point_of(im, (8.5, 5.5))[0][0] == F(2.0) / F(0.91 * 16)


def test_range_bounds_are_met_exactly():
    """Z == min_depth goes (strict), Z == max_depth stays; d2 == min^2 and d2 == max^2 both stay, one float beyond goes"""
    d = np.zeros((3, 3), np.float32)
    d[1, 1] = 3.0
    ident = I.cameras_for(3, 3, 1)
    im = _one(d, ident)
    assert np.isnan(M.point_of(im, (1.0, 1.0), min_depth=3.0)[0]).all()
    assert np.isfinite(M.point_of(im, (1.0, 1.0), min_depth=float(I.down(3.0)))[0]).all()
    assert np.isfinite(M.point_of(im, (1.0, 1.0), max_depth=3.0)[0]).all()
    assert np.isnan(M.point_of(im, (1.0, 1.0), max_depth=float(I.down(3.0)))[0]).all()
    cx, cy = ident[0]["cx"], ident[0]["cy"]
    for shift, lo, hi in ((-1.0, 2.0, 0.0), (1.0, 0.0, 4.0)):
        t = list(I.IDENTITY)
        t[11] = shift
        for pixel, kept in ((3.0, [0]), (float(I.down(3.0) if shift < 0 else I.up(3.0, 2)), [])):
            e = d.copy()
            e[1, 1] = pixel
            cam = [M.camera(ident[0]["fx"], ident[0]["fy"], cx, cy, transform=t)]
            got, xyz = M.frame(M.image(e, cam), [(cx, cy)], M.FILTER_3D, lo, hi)
            assert xyz[0][0] == 0 and xyz[0][1] == 0 and np.isfinite(xyz[0][2])        # the range test passed: the filter decides
            assert got == kept, (shift, pixel)
            if kept:
                assert M.dist_sqr(xyz[0]) == F(max(lo, hi)) ** 2


def test_a_fused_multiply_add_is_told_from_the_rule():
    rng = np.random.default_rng(5)
    d, cams, pts = I.fma_transform_case(rng)
    im = M.image(d, cams)
    assert (I.bits(M.frame(im, pts)[1]) != I.bits(M.frame(im, pts, fma=True)[1])).any()
    d, cams, pts, lo, hi = I.fma_dist_case(rng)
    im = M.image(d, cams)
    assert M.frame(im, pts, M.FILTER_3D, lo, hi)[0] == [0] and M.frame(im, pts, M.FILTER_3D, lo, hi, fma=True)[0] == []


def test_factors_and_pitch():
    """an image_width that is not the depth image's width scales keypoints and intrinsics; columns behind the row are never read"""
    rng = np.random.default_rng(6)
    im, pts = I.random_frame(rng, np.uint16, 16, 12, 2, 200, image_size=(20, 30))
    sub_cols, sub_w, fx, fy = M.factors(im)
    assert sub_cols == 8 and fx == F(1) / (F(20) / F(8)) and fy == F(1) / (F(30) / F(12))
    assert pts[:, 0].max() > 16 and pts[:, 1].max() > 12                       # in the colour image's coordinates
    kept, xyz = M.frame(im, pts, M.KEEP_ALL, device=True)
    assert np.isfinite(xyz).all(1).sum() > 50
    padded, pts2 = I.random_frame(rng, np.float32, 16, 12, 1, 200, pad=3)
    assert padded["data"].shape == (12, 19) and padded["width"] == 16 and np.isfinite(padded["data"][:, 16:]).all()
    for pt in pts2:
        reads = []
        M.point_of(padded, pt, device=True, reads=reads)
        assert all(c < 16 for c, _ in reads)
    tight = M.image(np.ascontiguousarray(padded["data"]), padded["cameras"])   # the same array read as 19 columns wide: other results
    a = M.frame(padded, pts2, device=True)[1]
    b = M.frame(tight, pts2, device=True)[1]
    assert (I.bits(a) != I.bits(b)).any()


def test_random_frames_hold_every_outcome():
    rng = np.random.default_rng(7)
    for dtype in (np.uint16, np.float32):
        im, pts = I.random_frame(rng, dtype, 64, 48, 4, 1100, transform=I.TILT)
        kept, xyz = M.frame(im, pts, M.FILTER_3D, 0.5, 3.0, device=True)
        assert 100 < len(kept) < 1000
        ok = np.isfinite(xyz).all(1)
        assert (np.isnan(xyz).all(1) | ok).all()                               # a point is whole or three NaNs
        assert (I.bits(xyz[~ok]) == M.QUIET_NAN_BITS).all()
        kp = M.frame(im, pts, M.FILTER_PIXEL, 0.5, 3.0, device=True)[0]
        assert kp != kept and 100 < len(kp) < 1000
