"""The rule of lcd_keypoints_3d (include/lcd.h) in NumPy float32, written from the reference's text -- util3d::generateKeypoints3DDepth
(util3d_features.cpp:67-120), util2d::getDepth (util2d.cpp:947-1111), util3d::projectDepthTo3D (util3d.cpp:215-244), util3d::transformPoint
(util3d_transforms.cpp:211-220) and both Feature2D::filterKeypointsByDepth overloads (Features2d.cpp:105-212) -- one operation per statement,
every intermediate a numpy.float32, so that nothing is fused and nothing is computed wider.  `device=True` switches to the device entry's
definition of what the reference asserts on: a bad point that no filter keeps.  `order="vu"` and `fma=True` are deliberately WRONG variants:
the input tests use them to prove that an input tells the rule from them."""
import math

import numpy as np

F = np.float32
U16_MM, F32_M = 0, 1
KEEP_ALL, FILTER_3D, FILTER_PIXEL = "keep_all", "filter_3d", "filter_pixel"
NAN3 = np.full(3, np.nan, np.float32)
QUIET_NAN_BITS = 0x7FC00000


class Refused(Exception):
    """what the host entry answers with LCD_ERR_INVALID"""


def camera(fx, fy, cx, cy, image_width=0, image_height=0, transform=None):
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, image_width=image_width, image_height=image_height, transform=transform)


def image(data, cameras, width=None):
    """data: 2-D uint16 (millimetres) or float32 (metres), possibly wider than `width` (a pitch larger than the row)"""
    assert data.dtype in (np.uint16, np.float32) and data.ndim == 2
    return dict(data=data, cameras=list(cameras), width=int(data.shape[1] if width is None else width))


def convertible(v):
    """int(v) is defined"""
    v = float(v)
    return math.isfinite(v) and -2147483648.0 < v < 2147483648.0


def fused(a, b, c):
    """a * b + c rounded ONCE to float32, as a fused multiply-add does.  The exact value is rounded to double first; where that could change
    the float32 result (the double next to a float32 tie) ValueError is raised and the caller looks for another input."""
    from fractions import Fraction
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    d = float(exact)
    if Fraction(d) != exact and not (F(np.nextafter(d, -np.inf)) == F(d) == F(np.nextafter(d, np.inf))):
        raise ValueError("double rounding")
    return F(d)


def factors(im):
    if "_factors" not in im:                             # (an image is not changed once it is made)
        im["_factors"] = _factors(im)
    return im["_factors"]


def _factors(im):
    sub_cols = im["width"] // len(im["cameras"])
    sub_w = F(sub_cols)
    c0 = im["cameras"][0]
    rx = F(c0["image_width"]) / sub_w if c0["image_width"] > 0 else F(1)
    ry = F(c0["image_height"]) / F(im["data"].shape[0]) if c0["image_height"] > 0 else F(1)
    return sub_cols, sub_w, F(1) / rx, F(1) / ry


def pixel(im, col, row, checked=True):
    p = im["data"][row, col]
    if im["data"].dtype == np.uint16:
        if checked and (p == 0 or p == 65535):
            return F(0)
        return F(p) * F(0.001)
    return F(p)


def get_depth(im, col0, cols, x, y, order="uv", reads=None):
    """getDepth in the sub-image [col0, col0 + cols); reads: a list that receives the (col, row) of every pixel looked at"""
    rows = im["data"].shape[0]
    u = int(x + F(0.5))
    v = int(y + F(0.5))
    if u == cols and x < F(cols):
        u = cols - 1
    if v == rows and y < F(rows):
        v = rows - 1
    if not (0 <= u < cols and 0 <= v < rows):
        return F(0)
    look = lambda uu, vv: (reads.append((col0 + uu, vv)) if reads is not None else None, pixel(im, col0 + uu, vv))[1]
    depth = look(u, v)
    if depth == 0 or not np.isfinite(depth):
        return F(0)
    u_range = range(max(u - 1, 0), min(u + 1, cols - 1) + 1)
    v_range = range(max(v - 1, 0), min(v + 1, rows - 1) + 1)
    window = [(uu, vv) for uu in u_range for vv in v_range] if order == "uv" else [(uu, vv) for vv in v_range for uu in u_range]
    sum_weights, sum_depths = F(0), F(0)
    depth_error = F(0.02) * depth
    for uu, vv in window:
        if uu == u and vv == v:
            continue
        d = look(uu, vv)
        if d == 0 or not np.isfinite(d):
            continue
        if not (abs(d - depth) < depth_error):
            continue
        if uu == u or vv == v:
            sum_weights = sum_weights + F(2)
            d = d * F(2)
        else:
            sum_weights = sum_weights + F(1)
        sum_depths = sum_depths + d
    depth = depth * F(4)
    sum_weights = sum_weights + F(4)
    total = depth + sum_depths
    return total / sum_weights


def transform_point(t, p, fma=False):
    out = []
    for r in range(3):
        a, b, c, d = (F(v) for v in t[4 * r:4 * r + 4])
        if fma:
            s = a * p[0]
            s = fused(b, p[1], s)
            s = fused(c, p[2], s)
            out.append(s + d)
        else:
            s = a * p[0]
            s = s + b * p[1]
            s = s + c * p[2]
            out.append(s + d)
    return np.array(out, np.float32)


def point_of(im, pt, min_depth=0.0, max_depth=0.0, device=False, order="uv", fma=False, reads=None):
    """-> (the 3-D point [3] float32, defined)"""
    with np.errstate(all="ignore"):
        sub_cols, sub_w, fx_, fy_ = factors(im)
        x = F(pt[0]) * fx_
        y = F(pt[1]) * fy_
        q = x / sub_w
        if not (convertible(x + F(0.5)) and convertible(y + F(0.5)) and convertible(q)):
            if not device:
                raise Refused("a coordinate that is not finite or beyond int")
            return NAN3.copy(), False
        cam = int(q)
        if not 0 <= cam < len(im["cameras"]):
            if not device:
                raise Refused("camera index outside")
            return NAN3.copy(), False
        C = im["cameras"][cam]
        xs = x - sub_w * F(cam)
        depth = get_depth(im, sub_cols * cam, sub_cols, xs, y, order, reads)
        if not depth > 0:
            return NAN3.copy(), True
        cx = F(C["cx"]) * fx_
        cy = F(C["cy"]) * fy_
        fx = F(C["fx"]) * fx_
        fy = F(C["fy"]) * fy_
        if not cx > 0:
            cx = F(sub_cols // 2) - F(0.5)
        if not cy > 0:
            cy = F(im["data"].shape[0] // 2) - F(0.5)
        X = (xs - cx) * depth
        X = X / fx
        Y = (y - cy) * depth
        Y = Y / fy
        p = np.array([X, Y, depth], np.float32)
        mn, mx = F(min_depth), F(max_depth)
        if not (np.isfinite(p).all() and (mn < 0 or p[2] > mn) and (mx <= 0 or p[2] <= mx)):
            return NAN3.copy(), True
        if C["transform"] is not None:
            p = transform_point(C["transform"], p, fma)
        return p, True


def dist_sqr(p, fma=False):
    if fma:
        return fused(p[2], p[2], fused(p[1], p[1], p[0] * p[0]))
    s = p[0] * p[0]
    s = s + p[1] * p[1]
    return s + p[2] * p[2]


def keep_3d(p, min_depth, max_depth, fma=False):
    with np.errstate(all="ignore"):
        if not np.isfinite(p).all():
            return False
        mn, mx = F(min_depth) * F(min_depth), F(max_depth) * F(max_depth)
        d2 = dist_sqr(p, fma)
        return bool(d2 >= mn and (mx == 0 or d2 <= mx))


def keep_pixel(im, pt, min_depth, max_depth, device=False):
    """-> (kept, defined)"""
    with np.errstate(all="ignore"):
        fu, fv = F(pt[0]) + F(0.5), F(pt[1]) + F(0.5)
        if not (convertible(fu) and convertible(fv)):
            if not device:
                raise Refused("a coordinate that is not finite or beyond int")
            return False, False
        u, v = int(fu), int(fv)
        if not (0 <= u < im["width"] and 0 <= v < im["data"].shape[0]):
            return False, True
        d = pixel(im, u, v, checked=False)
        mn, mx = F(min_depth), F(max_depth)
        return bool(np.isfinite(d) and d > mn and (mx <= 0 or d < mx)), True


def check_bounds(filter, min_depth, max_depth):
    if math.isnan(min_depth) or math.isnan(max_depth) or (filter != KEEP_ALL and min_depth < 0) or (0 < max_depth <= min_depth):
        raise Refused("depth bounds")


def frame(im, points, filter=KEEP_ALL, min_depth=0.0, max_depth=0.0, device=False, with_xyz=True, order="uv", fma=False):
    """-> (kept indices (a list, ascending), xyz of ALL keypoints [n x 3] or None)"""
    check_bounds(filter, min_depth, max_depth)
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    need_xyz = with_xyz or filter != FILTER_PIXEL
    xyz = np.zeros((pts.shape[0], 3), np.float32)
    kept = []
    for i, pt in enumerate(pts):
        defined = True
        if need_xyz:
            xyz[i], defined = point_of(im, pt, min_depth, max_depth, device, order, fma)
        if filter == KEEP_ALL:
            keep = True
        elif filter == FILTER_3D:
            keep = defined and keep_3d(xyz[i], min_depth, max_depth, fma)
        else:
            keep = keep_pixel(im, pt, min_depth, max_depth, device)[0] and defined
        if keep:
            kept.append(i)
    return kept, (xyz if need_xyz else None)


def batch(images, frames_points, filter=KEEP_ALL, min_depth=0.0, max_depth=0.0, device=False, with_xyz=True):
    """-> dict(count [n_frames], index [N] with -1 behind each frame's count, kept: per frame the list, xyz: per frame [n x 3] of all keypoints)"""
    count, index, kept_all, xyz_all = [], [], [], []
    for im, pts in zip(images, frames_points):
        kept, xyz = frame(im, pts, filter, min_depth, max_depth, device, with_xyz)
        n = len(pts)
        count.append(len(kept))
        index += kept + [-1] * (n - len(kept))
        kept_all.append(kept)
        xyz_all.append(xyz)
    return dict(count=np.array(count, np.int32), index=np.array(index, np.int32).reshape(-1), kept=kept_all, xyz=xyz_all)
