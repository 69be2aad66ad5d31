"""The yardstick of the stereo tracker's accuracy check: an independent float64 tracker -- float Gaussian pyramid, float bilinear sampling, the
same x-only Gauss-Newton step, no fixed point anywhere -- and the textures with a known disparity it is measured on.  It shares no code with
tests/stereo_flow_model.py."""
import numpy as np

import stereo_flow_inputs as I

# width, height, disparity: integer and fractional disparities at both sizes
SCENES = [(64, 48, 3.0), (64, 48, 2.4), (160, 120, 5.0), (160, 120, 6.7)]
# The yardstick's largest error against the truth over SCENES, in pixels, measured on the CPU (DESIGN.md 4q records it); the rule's must stay
# within FACTOR times it (4n's factor, for the 5-bit patch quantisation the yardstick lacks)
YARDSTICK_ERROR = 0.0566
FACTOR = 4.0


def _reflect(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _down(a):
    h, w = a.shape
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    rows = _reflect(np.arange(-2, h + 2), h)
    cols = _reflect(np.arange(-2, w + 2), w)
    p = a[rows][:, cols]
    nh, nw = (h + 1) // 2, (w + 1) // 2
    v = sum(k[i] * p[i:i + 2 * nh:2, :] for i in range(5))
    return sum(k[j] * v[:, j:j + 2 * nw:2] for j in range(5))


def _gradient(a):
    """Scharr's derivative over 32 (a unit ramp gives 1)"""
    h, w = a.shape
    p = a[_reflect(np.arange(-1, h + 1), h)][:, _reflect(np.arange(-1, w + 1), w)]
    gx = (3 * (p[:-2, 2:] - p[:-2, :-2]) + 10 * (p[1:-1, 2:] - p[1:-1, :-2]) + 3 * (p[2:, 2:] - p[2:, :-2])) / 32.0
    gy = (3 * (p[2:, :-2] - p[:-2, :-2]) + 10 * (p[2:, 1:-1] - p[:-2, 1:-1]) + 3 * (p[2:, 2:] - p[:-2, 2:])) / 32.0
    return gx, gy


def _sample(a, x, y):
    """bilinear, the coordinates clamped to the image"""
    h, w = a.shape
    x = np.clip(x, 0, w - 1.000001)
    y = np.clip(y, 0, h - 1.000001)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = x - x0, y - y0
    return a[y0, x0] * (1 - fx) * (1 - fy) + a[y0, x0 + 1] * fx * (1 - fy) + a[y0 + 1, x0] * (1 - fx) * fy + a[y0 + 1, x0 + 1] * fx * fy


def track(left, right, points, win_w=15, win_h=3, max_level=5, iterations=30, eps=0.01, min_eig=1e-4):
    """-> (right x [n] float64, kept [n] bool)"""
    L, R = [left.astype(np.float64)], [right.astype(np.float64)]
    while len(L) <= max_level and (L[-1].shape[1] + 1) // 2 > win_w and (L[-1].shape[0] + 1) // 2 > win_h:
        L.append(_down(L[-1]))
        R.append(_down(R[-1]))
    G = [_gradient(a) for a in L]
    wx, wy = np.meshgrid(np.arange(win_w) - (win_w - 1) / 2.0, np.arange(win_h) - (win_h - 1) / 2.0)
    out, kept = np.zeros(len(points)), np.zeros(len(points), bool)
    for i, (px, py) in enumerate(np.asarray(points, np.float64)):
        ok, q = True, None
        for level in range(len(L) - 1, -1, -1):
            s = 1.0 / (1 << level)
            x, y = px * s, py * s
            q = x if q is None else q * 2.0
            h, w = L[level].shape
            ok = -win_w / 2 <= x < w + win_w / 2 and -win_h / 2 <= y < h + win_h / 2
            if not ok:
                continue
            Iw = _sample(L[level], x + wx, y + wy)
            gx, gy = _sample(G[level][0], x + wx, y + wy), _sample(G[level][1], x + wx, y + wy)
            a11, a12, a22 = (gx * gx).sum(), (gx * gy).sum(), (gy * gy).sum()
            det = a11 * a22 - a12 * a12
            eig = (a22 + a11 - np.sqrt((a11 - a22) ** 2 + 4 * a12 * a12)) / (2 * win_w * win_h)
            ok = eig / 1024.0 >= min_eig and det > 1e-12                    # the rule's scale: its derivatives are 32 x, its sums x 2^-20
            if not ok:
                continue
            prev = 0.0
            for j in range(iterations):
                ok = -win_w <= q < w + win_w
                if not ok:
                    break
                diff = _sample(R[level], q + wx, y + wy) - Iw
                b1, b2 = (diff * gx).sum(), (diff * gy).sum()
                d = (a12 * b2 - a22 * b1) / det
                q += d
                if d * d <= eps * eps:
                    break
                if j > 0 and abs(d + prev) < 0.01:
                    q -= d * 0.5
                    break
                prev = d
        out[i], kept[i] = q, ok
    return out, kept


def scene(width, height, disparity, seed=0, tries=20):
    """-> (left, right, points, true right x): a smooth random texture and its right image resampled at the disparity; the points lie more
    than win_width from the border; a texture is accepted only if the yardstick keeps at least 95 % of them"""
    rng = np.random.default_rng(1000 * width + int(disparity * 10) + seed)
    xs, ys = np.meshgrid(np.arange(17, width - 17, 5) + 0.3, np.arange(17, height - 17, 5) + 0.6)
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    for _ in range(tries):
        left, right = I.shifted_pair(I.texture(rng, width, height), width, disparity)
        rx, kept = track(left, right, pts)
        if kept.mean() >= 0.95:
            return left, right, pts, pts[:, 0].astype(np.float64) - disparity
    raise AssertionError("no texture the yardstick keeps")
