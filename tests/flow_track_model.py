"""The rule of lcd_track_flow (include/lcd.h) in NumPy: the 2-D pyramidal Lucas-Kanade tracker and the keep step of RegistrationVis
(RegistrationVis.cpp:709-724).  The pyramid, the derivative, the fixed-point patch and the bounds tests are tests/stereo_flow_model.py's
(the rule takes them from lcd_keypoints_3d_stereo by reference); this file states what differs: the lane-tree order of every float sum,
the step, the stop and the oscillation test on both axes, the start from a caller's position, minEig as the error, the keep test.  Like the
stereo model it MATERIALISES the padded pyramid and cuts the windows out of it, int32 and float32, one operation per statement.

Four deliberately WRONG variants, which the input tests use to prove that an input tells the rule from them:
    variant="x_only"      the stereo tracker's step: delta.y = 0
    variant="row_major"   the stereo rule's sequential row-major sums instead of the lane tree
    variant="osc_x"       the oscillation test on x alone
    variant="stop_float"  the stop test evaluated in float32 instead of float64"""
import math

import numpy as np

import keypoints_3d_model as K3
import stereo_flow_model as S

F = np.float32
D = np.float64
I32 = np.int32
LANES = 64
FLT_SCALE = S.FLT_SCALE
FLT_EPSILON = S.FLT_EPSILON

DEFAULTS = dict(win_width=16, win_height=16, iterations=30, eps=0.01, use_min_eigenvals=1, min_eig_threshold=1e-4, error_threshold=20.0)
Refused = S.Refused


def params(**kw):
    return dict(DEFAULTS, **kw)


def pair(image_from, image_to, width=None, max_level=3, use_initial=0):
    """image_from, image_to: 2-D uint8, possibly wider than `width` (a pitch larger than the row)"""
    assert image_from.dtype == np.uint8 and image_to.dtype == np.uint8 and image_from.shape == image_to.shape
    return {"from": image_from, "to": image_to, "width": int(image_from.shape[1] if width is None else width), "max_level": int(max_level),
            "use_initial": int(use_initial)}


def check(P, pr):
    height = pr["from"].shape[0]
    bad = (not 3 <= P["win_width"] <= 31 or not 3 <= P["win_height"] <= 31 or not 0 <= pr["max_level"] <= 8 or pr["width"] <= P["win_width"] or
           height <= P["win_height"] or any(math.isnan(P[k]) for k in ("eps", "min_eig_threshold", "error_threshold")))
    if bad:
        raise Refused("parameters")


def lane_tree_sum(terms):
    """fp32: part p % 64 adds its terms in ascending p from +0, then the halving tree.  (The zeros that fill the last pass change no bit:
    a part is never -0.)"""
    t = terms.astype(np.float32).reshape(-1)
    n = t.shape[0]
    t = np.concatenate([t, np.zeros(-n % LANES, np.float32)]).reshape(-1, LANES)
    part = np.zeros(LANES, np.float32)
    for row in t:
        part = part + row
    s = LANES // 2
    while s >= 1:
        part = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def levels_of(P, pr):
    w = pr["width"]
    fp = S.build_pyramid(pr["from"][:, :w], P["win_width"], P["win_height"], pr["max_level"])
    tp = S.build_pyramid(pr["to"][:, :w], P["win_width"], P["win_height"], pr["max_level"])
    assert len(fp) == len(tp)
    return [S.Level(a, b, P["win_width"], P["win_height"]) for a, b in zip(fp, tp)]


_LEVELS = {}


def cached_levels(P, pr):
    """(a pair's images are not changed once they are made)"""
    key = (id(pr["from"]), id(pr["to"]), pr["width"], P["win_width"], P["win_height"], pr["max_level"])
    if key not in _LEVELS:
        _LEVELS[key] = (pr["from"], pr["to"], levels_of(P, pr))
    return _LEVELS[key][2]


def trackable(pt, start):
    ok = K3.convertible(F(pt[0])) and K3.convertible(F(pt[1]))
    return ok and (start is None or (K3.convertible(F(start[0])) and K3.convertible(F(start[1]))))


def track(levels, P, pt, start=None, variant=None, trace=None):
    """one corner -> (tracked corner (x, y) float32, status, err float32).  start: the initial position (use_initial) or None.  trace: a dict
    that receives what happened at each level (for the input tests)"""
    trace = {} if trace is None else trace
    total = S.ordered_sum if variant == "row_major" else lane_tree_sum
    with np.errstate(all="ignore"):
        if not trackable(pt, start):
            return (F(np.nan), F(np.nan)), 0, F(0)
        ptx, pty = F(pt[0]), F(pt[1])
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
                if start is not None:
                    qx, qy = F(start[0]) * scale, F(start[1]) * scale
                else:
                    qx, qy = px, py
            else:
                qx, qy = nx * F(2), ny * F(2)
            nx, ny = qx, qy
            px, py = px - hx, py - hy
            ipx, ipy = S.floor_int(px), S.floor_int(py)
            if S.outside(ipx, ipy, w, h, L.cols, L.rows):
                ev.append("prev_outside")
                if level == 0:
                    status = 0
                continue
            ev.append(("origin", ipx, ipy))
            a, b = px - F(ipx), py - F(ipy)
            iw = S.weights(a, b)
            ev.append(("weights", float(a), float(b)))
            Iw = S.interpolate(L.window(L.I, ipx, ipy, w, h), iw, 9)
            dxw = S.interpolate(L.window(L.dx, ipx, ipy, w, h), iw, 14)
            dyw = S.interpolate(L.window(L.dy, ipx, ipy, w, h), iw, 14)
            A11 = total(dxw * dxw) * FLT_SCALE
            A12 = total(dxw * dyw) * FLT_SCALE
            A22 = total(dyw * dyw) * FLT_SCALE
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
            if P["use_min_eigenvals"]:
                err = min_eig
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
                inx, iny = S.floor_int(qx), S.floor_int(qy)
                if S.outside(inx, iny, w, h, L.cols, L.rows):
                    exit_ = "next_outside"
                    if level == 0:
                        status = 0
                    break
                iw = S.weights(qx - F(inx), qy - F(iny))
                diff = S.interpolate(L.window(L.J, inx, iny, w, h), iw, 9) - Iw
                b1 = total(diff * dxw) * FLT_SCALE
                b2 = total(diff * dyw) * FLT_SCALE
                u1 = A12 * b2
                u2 = A22 * b1
                u3 = u1 - u2
                dx = u3 * inv
                v1 = A12 * b1
                v2 = A11 * b2
                v3 = v1 - v2
                dy = v3 * inv
                if variant == "x_only":
                    dy = F(0)
                ev.append(("delta", dx, dy))
                qx, qy = qx + dx, qy + dy
                nx, ny = qx + hx, qy + hy
                if variant == "stop_float":
                    stop = dx * dx + dy * dy <= F(eps2)
                else:
                    stop = D(dx) * D(dx) + D(dy) * D(dy) <= eps2
                if stop:
                    exit_ = "eps"
                    break
                if j > 0 and float(abs(dx + pdx)) < 0.01 and (variant == "osc_x" or float(abs(dy + pdy)) < 0.01):
                    nx = nx - dx * F(0.5)
                    ny = ny - dy * F(0.5)
                    exit_ = "oscillation"
                    break
                pdx, pdy = dx, dy
            ev.append(exit_)
            if status and level == 0 and not P["use_min_eigenvals"]:
                ex, ey = nx - hx, ny - hy
                iex, iey = S.floor_int(ex), S.floor_int(ey)
                if S.outside(iex, iey, w, h, L.cols, L.rows):
                    ev.append("err_outside")
                    status = 0
                    continue
                iw = S.weights(ex - F(iex), ey - F(iey))
                diff = S.interpolate(L.window(L.J, iex, iey, w, h), iw, 9) - Iw
                errval = total(np.abs(diff))
                err = errval / F(32 * w * h)
        return (nx, ny), status, F(err)


def keep(P, to, status, err, cols, rows):
    """RegistrationVis.cpp:709-724 with uIsInBounds(v, low, high) = !(v < low) && !(v >= high) on a finite v"""
    x, y = F(to[0]), F(to[1])
    if not status:
        return False
    if not np.isfinite(x) or x < F(0) or x >= F(cols):
        return False
    if not np.isfinite(y) or y < F(0) or y >= F(rows):
        return False
    return bool(P["use_min_eigenvals"]) or bool(F(err) < F(P["error_threshold"]))


def run_pair(pr, points, P=None, initial=None, device=False, variant=None):
    """-> dict(kept: the indices (ascending), track [n x 2], status [n], err [n]) of one pair; initial: [n x 2], read only with use_initial"""
    P = params() if P is None else P
    check(P, pr)
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    if pr["use_initial"] and initial is None:
        raise Refused("use_initial without initial")
    ini = None if not pr["use_initial"] else np.asarray(initial, np.float32).reshape(-1, 2)
    levels = cached_levels(P, pr)
    n = pts.shape[0]
    rows, cols = pr["from"].shape[0], pr["width"]
    trk, status, err, kept = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32), []
    for i, pt in enumerate(pts):
        start = None if ini is None else ini[i]
        if not device and not trackable(pt, start):
            raise Refused("a coordinate that is not finite or beyond int")
        (tx, ty), st, e = track(levels, P, pt, start, variant)
        trk[i], status[i], err[i] = (tx, ty), st, e
        if keep(P, (tx, ty), st, e, cols, rows):
            kept.append(i)
    return dict(kept=kept, track=trk, status=status, err=err)


def batch(pairs, pair_points, P=None, initials=None, device=False):
    """-> dict(count [n_pairs], index [N] with -1 behind each pair's count, kept / track / status / err: per pair)"""
    out = dict(count=[], index=[], kept=[], track=[], status=[], err=[])
    for k, (pr, pts) in enumerate(zip(pairs, pair_points)):
        fr = run_pair(pr, pts, P, None if initials is None else initials[k], device)
        out["count"].append(len(fr["kept"]))
        out["index"] += fr["kept"] + [-1] * (len(pts) - len(fr["kept"]))
        for key in ("kept", "track", "status", "err"):
            out[key].append(fr[key])
    out["count"] = np.array(out["count"], np.int32)
    out["index"] = np.array(out["index"], np.int32).reshape(-1)
    return out
