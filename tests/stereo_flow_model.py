"""The rule of lcd_keypoints_3d_stereo (include/lcd.h) in NumPy, written from the reference's text -- util2d::calcOpticalFlowPyrLKStereo
(util2d.cpp:371-736), StereoOpticalFlow::updateStatus (Stereo.cpp:240-268), util3d::projectDisparityTo3D (util3d.cpp:2806-2825) and
util3d::generateKeypoints3DStereo (util3d_features.cpp:158-203) -- and from the engine's pyramid rule: int32 and float32, one operation per
statement, float64 where the rule says so.  Unlike the engine's code it MATERIALISES the padded pyramid and the padded derivative images, as
OpenCV lays them out, and cuts the windows out of them.

Three deliberately WRONG variants, which the input tests use to prove that an input tells the rule from them:
    variant="plain_lk"        the y correction kept (cv::calcOpticalFlowPyrLK)
    variant="half_up"         weights rounded half up instead of half to even
    variant="reflect_deriv"   the derivative image's border reflected instead of zero"""
import math

import numpy as np

import keypoints_3d_model as K3

F = np.float32
D = np.float64
I32 = np.int32
NAN3 = K3.NAN3
KEEP_ALL, FILTER_3D = K3.KEEP_ALL, K3.FILTER_3D
INT_MIN = -2 ** 31
FLT_EPSILON = F(1.1920928955078125e-07)
FLT_SCALE = F(1.0 / (1 << 20))

DEFAULTS = dict(win_width=15, win_height=3, max_level=5, iterations=30, eps=0.01, use_min_eigenvals=1, min_eig_threshold=1e-4,
                error_threshold=50.0, min_disparity=0.5, max_disparity=128.0)


class Refused(Exception):
    """what the host entry answers with LCD_ERR_INVALID"""


def params(**kw):
    return dict(DEFAULTS, **kw)


def camera(fx, fy, cx, cy, baseline, right_cx=0.0, transform=None):
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, right_cx=right_cx, baseline=baseline, transform=transform)


def pair(left, right, cam, width=None):
    """left, right: 2-D uint8, possibly wider than `width` (a pitch larger than the row)"""
    assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.shape == right.shape
    return dict(left=left, right=right, camera=cam, width=int(left.shape[1] if width is None else width))


def check_params(P, width, height):
    bad = (not 3 <= P["win_width"] <= 31 or not 3 <= P["win_height"] <= 31 or not 0 <= P["max_level"] <= 8 or width <= P["win_width"] or
           height <= P["win_height"] or any(math.isnan(P[k]) for k in ("eps", "min_eig_threshold", "error_threshold", "min_disparity", "max_disparity")) or
           P["min_disparity"] < 0 or P["min_disparity"] > P["max_disparity"])
    if bad:
        raise Refused("parameters")


def check_camera(C):
    if any(math.isnan(C[k]) for k in ("fx", "fy", "cx", "cy", "right_cx", "baseline")) or not C["baseline"] > 0 or not C["fx"] > 0:
        raise Refused("camera")


# ---- the pyramid and the derivative (the engine's rule)
def reflect101(p, n):
    p = np.array(p, np.int64)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)
    return p


def padded(img, px, py):
    """the image with px columns and py rows of BORDER_REFLECT_101 around it"""
    h, w = img.shape
    return img[reflect101(np.arange(-py, h + py), h)][:, reflect101(np.arange(-px, w + px), w)]


def pyr_down(img):
    h, w = img.shape
    src = padded(img, 2, 2).astype(I32)
    k = (1, 4, 6, 4, 1)
    nw, nh = (w + 1) // 2, (h + 1) // 2
    acc = np.zeros((nh, nw), I32)
    for i in range(5):
        for j in range(5):
            acc += I32(k[i] * k[j]) * src[i:i + 2 * nh:2, j:j + 2 * nw:2]
    return ((acc + I32(128)) >> 8).astype(np.uint8)


def build_pyramid(img, win_w, win_h, max_level):
    levels = [np.ascontiguousarray(img)]
    while len(levels) <= max_level:
        h, w = levels[-1].shape
        if (w + 1) // 2 <= win_w or (h + 1) // 2 <= win_h:
            break
        levels.append(pyr_down(levels[-1]))
    return levels


def scharr(img):
    """(dx, dy) int32 at every pixel inside, reflect101 on the taps"""
    h, w = img.shape
    p = padded(img, 1, 1).astype(I32)
    t0 = (p[:-2, :] + p[2:, :]) * I32(3) + p[1:-1, :] * I32(10)          # [h x (w + 2)]
    dx = t0[:, 2:] - t0[:, :-2]
    t1 = p[2:, :] - p[:-2, :]
    dy = (t1[:, :-2] + t1[:, 2:]) * I32(3) + t1[:, 1:-1] * I32(10)
    return dx, dy


class Level:
    """one level of both pyramids, padded by the window as OpenCV pads it: I, J with the reflected border, dx, dy with a zero border"""

    def __init__(self, left, right, win_w, win_h, variant=None):
        self.rows, self.cols = left.shape
        self.px, self.py = win_w + 1, win_h + 1
        self.I = padded(left, self.px, self.py).astype(I32)
        self.J = padded(right, self.px, self.py).astype(I32)
        dx, dy = scharr(left)
        if variant == "reflect_deriv":
            self.dx, self.dy = padded(dx, self.px, self.py), padded(dy, self.px, self.py)
        else:
            self.dx, self.dy = np.pad(dx, ((self.py, self.py), (self.px, self.px))), np.pad(dy, ((self.py, self.py), (self.px, self.px)))

    def window(self, a, x0, y0, w, h):
        """the (h + 1) x (w + 1) pixels whose first is (x0, y0)"""
        return a[y0 + self.py:y0 + self.py + h + 1, x0 + self.px:x0 + self.px + w + 1]


def levels_of(P, left, right, variant=None):
    lp = build_pyramid(left, P["win_width"], P["win_height"], P["max_level"])
    rp = build_pyramid(right, P["win_width"], P["win_height"], P["max_level"])
    assert len(lp) == len(rp)
    return [Level(l, r, P["win_width"], P["win_height"], variant) for l, r in zip(lp, rp)]


# ---- the tracker
def floor_int(v):
    if not K3.convertible(v):
        return INT_MIN
    return int(math.floor(float(v)))


def cv_round(v, variant=None):
    if variant == "half_up":
        return int(math.floor(float(v) + 0.5))
    return int(np.rint(F(v)))


def weights(a, b, variant=None):
    na = F(1) - a
    nb = F(1) - b
    w00 = na * nb
    w01 = a * nb
    w10 = na * b
    iw00 = cv_round(w00 * F(16384), variant)
    iw01 = cv_round(w01 * F(16384), variant)
    iw10 = cv_round(w10 * F(16384), variant)
    return I32(iw00), I32(iw01), I32(iw10), I32(16384 - iw00 - iw01 - iw10)


def interpolate(win, iw, bits):
    s = win[:-1, :-1] * iw[0] + win[:-1, 1:] * iw[1] + win[1:, :-1] * iw[2] + win[1:, 1:] * iw[3]
    return (s + I32(1 << (bits - 1))) >> bits


def ordered_sum(terms):
    """fp32, one window pixel at a time, row-major"""
    return np.add.accumulate(terms.astype(np.float32).reshape(-1), dtype=np.float32)[-1]


def outside(ix, iy, w, h, cols, rows):
    return ix < -w or ix >= cols or iy < -h or iy >= rows


def track(levels, P, pt, variant=None, trace=None):
    """one keypoint -> (right corner (x, y) float32, status, err float32).  trace: a dict that receives what happened (for the input tests)"""
    trace = {} if trace is None else trace
    with np.errstate(all="ignore"):
        ptx, pty = F(pt[0]), F(pt[1])
        if not (K3.convertible(ptx) and K3.convertible(pty)):
            return (F(np.nan), F(np.nan)), 0, F(0)
        w, h = P["win_width"], P["win_height"]
        iterations = min(max(int(P["iterations"]), 0), 100)
        eps = min(max(float(P["eps"]), 0.0), 10.0)
        eps2 = eps * eps
        hx, hy = F(w - 1) * F(0.5), F(h - 1) * F(0.5)
        status, err = 1, F(0)
        nx, ny = F(0), F(0)
        top = len(levels) - 1
        for level in range(top, -1, -1):
            L = levels[level]
            ev = trace.setdefault(level, [])
            scale = F(1.0 / (1 << level))
            px, py = ptx * scale, pty * scale
            if level == top:
                qx, qy = px, py
            else:
                qx, qy = nx * F(2), ny * F(2)
            nx, ny = qx, qy
            px, py = px - hx, py - hy
            ipx, ipy = floor_int(px), floor_int(py)
            if outside(ipx, ipy, w, h, L.cols, L.rows):
                ev.append("prev_outside")
                if level == 0:
                    status = 0
                continue
            ev.append(("origin", ipx, ipy))
            a, b = px - F(ipx), py - F(ipy)
            iw = weights(a, b, variant)
            ev.append(("weights", float(a), float(b)))
            Iw = interpolate(L.window(L.I, ipx, ipy, w, h), iw, 9)
            dxw = interpolate(L.window(L.dx, ipx, ipy, w, h), iw, 14)
            dyw = interpolate(L.window(L.dy, ipx, ipy, w, h), iw, 14)
            A11 = ordered_sum(dxw * dxw) * FLT_SCALE
            A12 = ordered_sum(dxw * dyw) * FLT_SCALE
            A22 = ordered_sum(dyw * dyw) * FLT_SCALE
            t1 = A11 * A22
            t2 = A12 * A12
            Dt = t1 - t2
            s = A22 + A11
            d = A11 - A22
            dd = d * d
            f4 = F(4) * A12
            ff = f4 * A12
            r = dd + ff
            root = np.sqrt(r)
            num = s - root
            min_eig = num / F(2 * w * h)
            ev.append(("min_eig", float(min_eig), float(Dt)))
            if float(min_eig) < P["min_eig_threshold"] or Dt < FLT_EPSILON:
                ev.append("eig_fail" if float(min_eig) < P["min_eig_threshold"] else "det_fail")
                if level == 0:
                    status = 0
                continue
            inv = F(1) / Dt
            qx, qy = qx - hx, qy - hy
            pdx, pdy = F(0), F(0)
            exit_ = "cap"
            for j in range(iterations):
                inx, iny = floor_int(qx), floor_int(qy)
                if outside(inx, iny, w, h, L.cols, L.rows):
                    exit_ = "next_outside"
                    if level == 0:
                        status = 0
                    break
                iw = weights(qx - F(inx), qy - F(iny), variant)
                diff = interpolate(L.window(L.J, inx, iny, w, h), iw, 9) - Iw
                b1 = ordered_sum(diff * dxw) * FLT_SCALE
                b2 = ordered_sum(diff * dyw) * FLT_SCALE
                u1 = A12 * b2
                u2 = A22 * b1
                u3 = u1 - u2
                dx = u3 * inv
                if variant == "plain_lk":
                    v1 = A12 * b1
                    v2 = A11 * b2
                    v3 = v1 - v2
                    dy = v3 * inv
                else:
                    dy = F(0)
                qx, qy = qx + dx, qy + dy
                nx, ny = qx + hx, qy + hy
                if D(dx) * D(dx) + D(dy) * D(dy) <= eps2:
                    exit_ = "eps"
                    break
                if j > 0 and float(abs(dx + pdx)) < 0.01 and float(abs(dy + pdy)) < 0.01:
                    nx = nx - dx * F(0.5)
                    ny = ny - dy * F(0.5)
                    exit_ = "oscillation"
                    break
                pdx, pdy = dx, dy
            ev.append(exit_)
            if status and level == 0 and not P["use_min_eigenvals"]:
                ex, ey = nx - hx, ny - hy
                iex, iey = floor_int(ex), floor_int(ey)
                if outside(iex, iey, w, h, L.cols, L.rows):
                    status = 0
                    continue
                iw = weights(ex - F(iex), ey - F(iey), variant)
                diff = interpolate(L.window(L.J, iex, iey, w, h), iw, 9) - Iw
                errval = ordered_sum(np.abs(diff))
                err = errval / F(32 * w * h)
        return (nx, ny), status, err


def update_status(P, left_x, right_x, status, err):
    if not status:
        return 0
    if not P["use_min_eigenvals"] and not float(err) < P["error_threshold"]:
        return 1                                             # counted as rejected by the reference, but the status stays
    d = F(left_x) - F(right_x)
    if d <= F(P["min_disparity"]) or d > F(P["max_disparity"]):
        return 0
    return 1


def point_of(C, status, pt, right_x, min_depth=0.0, max_depth=0.0):
    with np.errstate(all="ignore"):
        if not status:
            return NAN3.copy()
        d = F(pt[0]) - F(right_x)
        if not d != 0 or not d > 0:
            return NAN3.copy()
        c = F(0)
        if C["right_cx"] > 0 and C["cx"] > 0:
            c = F(D(C["right_cx"]) - D(C["cx"]))
        dc = d + c
        W = F(D(C["baseline"]) / D(dc))
        ux = D(F(pt[0])) - D(C["cx"])
        X = F(ux * D(W))
        uy = D(F(pt[1])) - D(C["cy"])
        uy = uy * D(C["fx"])
        uy = uy / D(C["fy"])
        Y = F(uy * D(W))
        Z = F(D(C["fx"]) * D(W))
        p = np.array([X, Y, Z], np.float32)
        mn, mx = F(min_depth), F(max_depth)
        if not (np.isfinite(p).all() and (mn < 0 or p[2] > mn) and (mx <= 0 or p[2] <= mx)):
            return NAN3.copy()
        if C["transform"] is not None:
            p = K3.transform_point(C["transform"], p)
        return p


_LEVELS = {}


def cached_levels(P, pr, variant=None):
    """(a pair is not changed once it is made)"""
    key = (id(pr["left"]), id(pr["right"]), pr["width"], P["win_width"], P["win_height"], P["max_level"], variant)
    if key not in _LEVELS:
        w = pr["width"]
        _LEVELS[key] = (pr, levels_of(P, pr["left"][:, :w], pr["right"][:, :w], variant))
    return _LEVELS[key][1]


def frame(pr, points, P=None, filter=KEEP_ALL, min_depth=0.0, max_depth=0.0, device=False, variant=None):
    """-> dict(kept: the indices (ascending), xyz of ALL keypoints [n x 3], right [n x 2], status [n])"""
    P = params() if P is None else P
    check_params(P, pr["width"], pr["left"].shape[0])
    check_camera(pr["camera"])
    if filter not in (KEEP_ALL, FILTER_3D):
        raise Refused("filter")
    K3.check_bounds(filter, min_depth, max_depth)
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    levels = cached_levels(P, pr, variant)
    n = pts.shape[0]
    xyz, right, status, kept = np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), []
    for i, pt in enumerate(pts):
        if not device and not (K3.convertible(pt[0]) and K3.convertible(pt[1])):
            raise Refused("a coordinate that is not finite or beyond int")
        (rx, ry), st, err = track(levels, P, pt, variant)
        st = update_status(P, pt[0], rx, st, err)
        right[i], status[i] = (rx, ry), st
        xyz[i] = point_of(pr["camera"], st, pt, rx, min_depth, max_depth)
        if filter == KEEP_ALL or K3.keep_3d(xyz[i], min_depth, max_depth):
            kept.append(i)
    return dict(kept=kept, xyz=xyz, right=right, status=status)


def batch(pairs, frames_points, P=None, filter=KEEP_ALL, min_depth=0.0, max_depth=0.0, device=False):
    """-> dict(count [n_frames], index [N] with -1 behind each frame's count, kept / xyz / right / status: per frame)"""
    out = dict(count=[], index=[], kept=[], xyz=[], right=[], status=[])
    for pr, pts in zip(pairs, frames_points):
        fr = frame(pr, pts, P, filter, min_depth, max_depth, device)
        out["count"].append(len(fr["kept"]))
        out["index"] += fr["kept"] + [-1] * (len(pts) - len(fr["kept"]))
        for k in ("kept", "xyz", "right", "status"):
            out[k].append(fr[k])
    out["count"] = np.array(out["count"], np.int32)
    out["index"] = np.array(out["index"], np.int32).reshape(-1)
    return out
