"""The yardstick of the 2-D tracker's accuracy check: an independent float64 tracker -- float Gaussian pyramid, float bilinear sampling, the
Gauss-Newton step on both axes, plain sums, no fixed point anywhere -- and the textures with a known 2-D shift it is measured on.  It shares
no code with tests/flow_track_model.py or tests/stereo_flow_model.py."""
import numpy as np

import flow_track_inputs as I

# width, height, (shift x, shift y): integer and fractional shifts on both axes at both sizes
SCENES = [(64, 48, (2.0, 1.0)), (64, 48, (-1.4, 0.7)), (64, 48, (0.0, -2.3)), (160, 120, (3.0, -2.0)), (160, 120, (-2.6, 1.8)), (160, 120, (4.3, 3.1))]
# The yardstick's largest error against the truth over SCENES (the distance in pixels), measured on the CPU (DESIGN.md 4u records it); the
# rule's must stay within FACTOR times it (4n's factor as 4q applied it, for the 5-bit patch quantisation the yardstick lacks)
YARDSTICK_ERROR = 0.0433
FACTOR = 4.0
WIN = 16
MARGIN = 20          # the points lie more than the window from the border


def _reflect(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _down(a):
    h, w = a.shape
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    p = a[_reflect(np.arange(-2, h + 2), h)][:, _reflect(np.arange(-2, w + 2), w)]
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


def track(image_from, image_to, points, win=WIN, max_level=3, iterations=30, eps=0.01, min_eig=1e-4):
    """-> (tracked corners [n x 2] float64, kept [n] bool)"""
    A, B = [image_from.astype(np.float64)], [image_to.astype(np.float64)]
    while len(A) <= max_level and (A[-1].shape[1] + 1) // 2 > win and (A[-1].shape[0] + 1) // 2 > win:
        A.append(_down(A[-1]))
        B.append(_down(B[-1]))
    G = [_gradient(a) for a in A]
    wx, wy = np.meshgrid(np.arange(win) - (win - 1) / 2.0, np.arange(win) - (win - 1) / 2.0)
    out, kept = np.zeros((len(points), 2)), np.zeros(len(points), bool)
    for i, (px, py) in enumerate(np.asarray(points, np.float64)):
        ok, q = True, None
        for level in range(len(A) - 1, -1, -1):
            s = 1.0 / (1 << level)
            x, y = px * s, py * s
            q = np.array([x, y]) if q is None else q * 2.0
            h, w = A[level].shape
            ok = -win / 2 <= x < w + win / 2 and -win / 2 <= y < h + win / 2
            if not ok:
                continue
            Iw = _sample(A[level], x + wx, y + wy)
            gx, gy = _sample(G[level][0], x + wx, y + wy), _sample(G[level][1], x + wx, y + wy)
            a11, a12, a22 = (gx * gx).sum(), (gx * gy).sum(), (gy * gy).sum()
            det = a11 * a22 - a12 * a12
            eig = (a22 + a11 - np.sqrt((a11 - a22) ** 2 + 4 * a12 * a12)) / (2 * win * win)
            ok = eig / 1024.0 >= min_eig and det > 1e-12                    # the rule's scale: its derivatives are 32 x, its sums x 2^-20
            if not ok:
                continue
            prev = np.zeros(2)
            for j in range(iterations):
                ok = -win <= q[0] < w + win and -win <= q[1] < h + win
                if not ok:
                    break
                diff = _sample(B[level], q[0] + wx, q[1] + wy) - Iw
                b1, b2 = (diff * gx).sum(), (diff * gy).sum()
                d = np.array([a12 * b2 - a22 * b1, a12 * b1 - a11 * b2]) / det
                q = q + d
                if (d * d).sum() <= eps * eps:
                    break
                if j > 0 and (np.abs(d + prev) < 0.01).all():
                    q = q - d * 0.5
                    break
                prev = d
        h, w = A[0].shape
        out[i] = q
        kept[i] = ok and 0 <= q[0] < w and 0 <= q[1] < h
    return out, kept


def scene(width, height, shift, seed=0, tries=20):
    """-> (from, to, points, true tracked corners): a smooth random texture and the same scene moved by `shift`; the points lie more than
    the window from the border; a texture is accepted only if the yardstick keeps at least 95 % of them"""
    rng = np.random.default_rng(1000 * width + int(shift[0] * 10) * 31 + int(shift[1] * 10) + seed)
    xs, ys = np.meshgrid(np.arange(MARGIN, width - MARGIN, 4) + 0.3, np.arange(MARGIN, height - MARGIN, 4) + 0.6)
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    for _ in range(tries):
        a, b = I.shifted_images(I.texture(rng, width, height), width, height, shift)
        _, kept = track(a, b, pts)
        if kept.mean() >= 0.95:
            return a, b, pts, pts.astype(np.float64) + np.array(shift)
    raise AssertionError("no texture the yardstick keeps")
