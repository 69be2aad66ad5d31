"""The rule of lcd_estimate_motion_mono (include/lcd.h) in Python, operation for operation: rtabmap_amd/csrc/motion_mono_rule.h is the
normative order, and this file follows it statement by statement.  fp64 values are Python floats (IEEE doubles, every operation rounded on
its own), fp32 values numpy.float32 scalars.  model() returns what the entry writes for one pair and a trace of the branches taken.

yardstick() is a float64 five-point estimate of the same samples with numpy.linalg.svd and numpy.roots, for the accuracy comparison: it
shares the draws and the scoring, and nothing of the solver.
"""
import math

import numpy as np

BISECT = 56
MAX_DRAWS = 32
MIN_PAIRS = 9
ROOTS = 10
ST_OK, ST_FEW_FEATURES, ST_FEW_PAIRS, ST_NO_MODEL, ST_FEW_INLIERS, ST_HIGH_VARIANCE = 0, 1, 2, 3, 4, 5
WS_M, WS_B, WS_MINOR, WS_D, WS_RA, WS_RB, WS_BASIS, WS_T, WS_Q = 0, 0, 40, 60, 170, 181, 200, 236, 246
QUAD = [[0, 3, 4, 6], [3, 1, 5, 7], [4, 5, 2, 8], [6, 7, 8, 9]]
CUBIC = [[0, 2, 4, 5], [3, 1, 6, 7], [10, 13, 16, 17], [2, 3, 8, 9], [4, 8, 10, 11], [8, 6, 13, 14], [5, 9, 11, 12], [9, 7, 14, 15], [11, 14, 17, 18],
         [12, 15, 18, 19]]
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
f32 = np.float32
INF = float("inf")


def mix(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def finite(v):
    return not (math.isinf(v) or math.isnan(v))


def ddiv(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def dsqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


def draw5(seed, h, m):
    base = (mix(seed + h) * 8) & 0xFFFFFFFF
    idx = []
    for k in range(MAX_DRAWS):
        d = mix(base + k) % m
        if d in idx:
            continue
        idx.append(d)
        if len(idx) == 5:
            return idx
    return None


def null_space(ws):
    perm = list(range(9))
    for k in range(5):
        top, pr, pc = -1.0, k, k
        for r in range(k, 5):
            for c in range(k, 9):
                a = abs(ws[9 * r + c])
                if a > top:
                    top, pr, pc = a, r, c
        for c in range(9):
            ws[9 * k + c], ws[9 * pr + c] = ws[9 * pr + c], ws[9 * k + c]
        for r in range(5):
            ws[9 * r + k], ws[9 * r + pc] = ws[9 * r + pc], ws[9 * r + k]
        perm[k], perm[pc] = perm[pc], perm[k]
        piv = ws[9 * k + k]
        if piv == 0.0 or not finite(piv):
            return False
        for c in range(k + 1, 9):
            ws[9 * k + c] = ws[9 * k + c] / piv
        ws[9 * k + k] = 1.0
        for r in range(5):
            if r == k:
                continue
            f = ws[9 * r + k]
            for c in range(k + 1, 9):
                ws[9 * r + c] = ws[9 * r + c] - f * ws[9 * k + c]
            ws[9 * r + k] = 0.0
    for b in range(4):
        for j in range(9):
            ws[WS_BASIS + 9 * b + perm[j]] = -ws[9 * j + 5 + b] if j < 5 else (1.0 if j == 5 + b else 0.0)
    return True


def quad_mac(ws, ea, eb, neg):
    for i in range(4):
        a = ws[WS_BASIS + 9 * i + ea]
        for j in range(4):
            p = a * ws[WS_BASIS + 9 * j + eb]
            q = WS_Q + QUAD[i][j]
            ws[q] = ws[q] - p if neg else ws[q] + p


def quad_zero(ws):
    for q in range(10):
        ws[WS_Q + q] = 0.0


def cubic_mac(ws, row, e, neg):
    for q in range(10):
        a = ws[WS_Q + q]
        for l in range(4):
            p = a * ws[WS_BASIS + 9 * l + e]
            c = WS_M + 20 * row + CUBIC[q][l]
            ws[c] = ws[c] - p if neg else ws[c] + p


def constraints(ws):
    for c in range(200):
        ws[c] = 0.0
    quad_zero(ws); quad_mac(ws, 4, 8, False); quad_mac(ws, 5, 7, True); cubic_mac(ws, 0, 0, False)
    quad_zero(ws); quad_mac(ws, 3, 8, False); quad_mac(ws, 5, 6, True); cubic_mac(ws, 0, 1, True)
    quad_zero(ws); quad_mac(ws, 3, 7, False); quad_mac(ws, 4, 6, True); cubic_mac(ws, 0, 2, False)
    quad_zero(ws)
    for e in range(9):
        quad_mac(ws, e, e, False)
    for q in range(10):
        ws[WS_T + q] = 0.5 * ws[WS_Q + q]
    for i in range(3):
        for j in range(3):
            for k in range(3):
                quad_zero(ws)
                for n in range(3):
                    quad_mac(ws, 3 * i + n, 3 * k + n, False)
                if k == i:
                    for q in range(10):
                        ws[WS_Q + q] = ws[WS_Q + q] - ws[WS_T + q]
                cubic_mac(ws, 1 + 3 * i + j, 3 * k + j, False)


def eliminate(ws):
    for k in range(10):
        top, pr = -1.0, k
        for r in range(k, 10):
            a = abs(ws[20 * r + k])
            if a > top:
                top, pr = a, r
        for c in range(k, 20):
            ws[20 * k + c], ws[20 * pr + c] = ws[20 * pr + c], ws[20 * k + c]
        piv = ws[20 * k + k]
        if piv == 0.0 or not finite(piv):
            return False
        for c in range(k + 1, 20):
            ws[20 * k + c] = ws[20 * k + c] / piv
        ws[20 * k + k] = 1.0
        for r in range(10):
            if r == k:
                continue
            f = ws[20 * r + k]
            for c in range(k + 1, 20):
                ws[20 * r + c] = ws[20 * r + c] - f * ws[20 * k + c]
            ws[20 * r + k] = 0.0
    return True


def b_rows(ws):
    for r in range(3):
        a, b, o = 20 * (4 + 2 * r), 20 * (5 + 2 * r), WS_B + 13 * r
        v = [ws[a + 12], ws[a + 11] - ws[b + 12], ws[a + 10] - ws[b + 11], -ws[b + 10],
             ws[a + 15], ws[a + 14] - ws[b + 15], ws[a + 13] - ws[b + 14], -ws[b + 13],
             ws[a + 19], ws[a + 18] - ws[b + 19], ws[a + 17] - ws[b + 18], ws[a + 16] - ws[b + 17], -ws[b + 16]]
        ws[o:o + 13] = v


def upoly_mac(ws, dst, a, na, b, nb, neg):
    for i in range(na):
        x = ws[a + i]
        for j in range(nb):
            p = x * ws[b + j]
            ws[dst + i + j] = ws[dst + i + j] - p if neg else ws[dst + i + j] + p


def det_polynomial(ws):
    x0, y0, c0, x1, y1, c1, x2, y2, c2 = 0, 4, 8, 13, 17, 21, 26, 30, 34
    for k in range(110):
        ws[WS_D + k] = 0.0
    ws[WS_MINOR:WS_MINOR + 8] = [0.0] * 8
    upoly_mac(ws, WS_MINOR, y1, 4, c2, 5, False); upoly_mac(ws, WS_MINOR, c1, 5, y2, 4, True)
    upoly_mac(ws, WS_D, x0, 4, WS_MINOR, 8, False)
    ws[WS_MINOR:WS_MINOR + 8] = [0.0] * 8
    upoly_mac(ws, WS_MINOR, x1, 4, c2, 5, False); upoly_mac(ws, WS_MINOR, c1, 5, x2, 4, True)
    upoly_mac(ws, WS_D, y0, 4, WS_MINOR, 8, True)
    ws[WS_MINOR:WS_MINOR + 8] = [0.0] * 8
    upoly_mac(ws, WS_MINOR, x1, 4, y2, 4, False); upoly_mac(ws, WS_MINOR, y1, 4, x2, 4, True)
    upoly_mac(ws, WS_D, c0, 5, WS_MINOR, 7, False)
    if ws[WS_D + 10] == 0.0 or not all(finite(ws[WS_D + k]) for k in range(11)):
        return False
    for k in range(1, 10):
        for i in range(0, 11 - k):
            ws[WS_D + 11 * k + i] = ws[WS_D + 11 * (k - 1) + i + 1] * float(i + 1)
    return True


def horner(ws, at, d, z):
    v = ws[at + d]
    for i in range(d - 1, -1, -1):
        v = v * z + ws[at + i]                                         # (two roundings: Python fuses nothing)
    return v


def bisect(ws, at, d, lo, hi):
    plo, phi = horner(ws, at, d, lo), horner(ws, at, d, hi)
    neg_lo = plo < 0.0
    if neg_lo == (phi < 0.0):
        return None
    a, b = lo, hi
    for _ in range(BISECT):
        mid = 0.5 * (a + b)
        if (horner(ws, at, d, mid) < 0.0) == neg_lo:
            a = mid
        else:
            b = mid
    return 0.5 * (a + b)


def real_roots(ws):
    lead = ws[WS_D + 10]
    mx = 0.0
    for i in range(10):
        a = abs(ws[WS_D + i] / lead)
        if a > mx:
            mx = a
    B = 1.0 + mx
    if not finite(B):
        return -1
    n_prev, frm, into = 0, WS_RA, WS_RB
    for d in range(1, 11):
        at = WS_D + 11 * (10 - d)
        n = 0
        for i in range(d):
            if i > n_prev:
                continue
            lo = -B if i == 0 else ws[frm + i - 1]
            hi = B if i == n_prev else ws[frm + i]
            x = bisect(ws, at, d, lo, hi)
            if x is not None:
                ws[into + n] = x
                n += 1
        frm, into = into, frm
        n_prev = n
    return n_prev


def solve(ws, x1, y1, x2, y2, trace=None):
    """-> the number of real roots, 0 for an invalid hypothesis; trace (a list) gets the branch's name"""
    note = trace.append if trace is not None else (lambda s: None)
    for j in range(5):
        x, y, xp, yp = float(x1[j]), float(y1[j]), float(x2[j]), float(y2[j])
        ws[9 * j:9 * j + 9] = [xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, 1.0]
    if not null_space(ws):
        note("null_space")
        return 0
    constraints(ws)
    if not eliminate(ws):
        note("eliminate")
        return 0
    b_rows(ws)
    if not det_polynomial(ws):
        note("polynomial")
        return 0
    n = real_roots(ws)
    if n < 0:
        note("bound")
        return 0
    note("roots%d" % n)
    return n


def make_model(ws, r):
    z = ws[WS_RA + r]
    b = [[horner(ws, WS_B + 13 * i, 3, z), horner(ws, WS_B + 13 * i + 4, 3, z), horner(ws, WS_B + 13 * i + 8, 4, z)] for i in range(3)]
    top, v = -1.0, (0.0, 0.0, 0.0)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        cx = b[i][1] * b[j][2] - b[i][2] * b[j][1]
        cy = b[i][2] * b[j][0] - b[i][0] * b[j][2]
        cz = b[i][0] * b[j][1] - b[i][1] * b[j][0]
        n = (cx * cx + cy * cy) + cz * cz
        if n > top:
            top, v = n, (cx, cy, cz)
    x, y = ddiv(v[0], v[2]), ddiv(v[1], v[2])
    ok = finite(x) and finite(y)
    E = []
    for e in range(9):
        E.append(((x * ws[WS_BASIS + e] + y * ws[WS_BASIS + 9 + e]) + z * ws[WS_BASIS + 18 + e]) + ws[WS_BASIS + 27 + e])
        ok = ok and finite(E[e])
    return E if ok else None


def sampson(E, x1, y1, x2, y2):
    """E: nine float32; the coordinates float32"""
    with np.errstate(all="ignore"):
        ex = (E[0] * x1 + E[1] * y1) + E[2]
        ey = (E[3] * x1 + E[4] * y1) + E[5]
        ez = (E[6] * x1 + E[7] * y1) + E[8]
        tx = (E[0] * x2 + E[3] * y2) + E[6]
        ty = (E[1] * x2 + E[4] * y2) + E[7]
        dot = (x2 * ex + y2 * ey) + ez
        den = ((ex * ex + ey * ey) + tx * tx) + ty * ty
        return (dot * dot) / den


def count_inliers(E32, X, thr2):
    """vectorised over the correspondences: the same float32 operations element by element"""
    with np.errstate(all="ignore"):
        return sampson(E32, X[0], X[1], X[2], X[3]) <= thr2


def decompose(E):
    G = [[(E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1]) + E[3 * i + 2] * E[3 * j + 2] for j in range(3)] for i in range(3)]
    h = 0.5 * ((G[0][0] + G[1][1]) + G[2][2])
    M = [[(h - G[i][j]) if i == j else -G[i][j] for j in range(3)] for i in range(3)]
    top, col = M[0][0], 0
    if M[1][1] > top:
        top, col = M[1][1], 1
    if M[2][2] > top:
        top, col = M[2][2], 2
    root = dsqrt(top)
    b = [ddiv(M[i][col], root) for i in range(3)]
    bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    nb = dsqrt(bb)
    C = []
    for i in range(3):
        p, q = (i + 1) % 3, (i + 2) % 3
        C += [E[3 * p + 1] * E[3 * q + 2] - E[3 * p + 2] * E[3 * q + 1], E[3 * p + 2] * E[3 * q] - E[3 * p] * E[3 * q + 2],
              E[3 * p] * E[3 * q + 1] - E[3 * p + 1] * E[3 * q]]
    S = [0.0] * 9
    for j in range(3):
        S[j] = b[1] * E[6 + j] - b[2] * E[3 + j]
        S[3 + j] = b[2] * E[j] - b[0] * E[6 + j]
        S[6 + j] = b[0] * E[3 + j] - b[1] * E[j]
    pose = [ddiv(C[i] - S[i], bb) for i in range(9)] + [ddiv(C[i] + S[i], bb) for i in range(9)] + [ddiv(b[i], nb) for i in range(3)]
    return pose if all(finite(v) for v in pose) else None


def triangulate(R, t, minus, fx1, fy1, fx2, fy2):
    x1, y1, x2, y2 = float(fx1), float(fy1), float(fx2), float(fy2)
    a = [(R[3 * i] * x1 + R[3 * i + 1] * y1) + R[3 * i + 2] for i in range(3)]
    t0, t1, t2 = (-t[0], -t[1], -t[2]) if minus else (t[0], t[1], t[2])
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    bb = (x2 * x2 + y2 * y2) + 1.0
    ab = (a[0] * x2 + a[1] * y2) + a[2]
    at = (a[0] * t0 + a[1] * t1) + a[2] * t2
    bt = (x2 * t0 + y2 * t1) + t2
    det = aa * bb - ab * ab
    if det == 0.0 or not finite(det):
        return None
    return ddiv(ab * bt - at * bb, det), ddiv(aa * bt - ab * at, det)


def config_test(pose, k, x1, y1, x2, y2, dist):
    """-> (passes, d1)"""
    d = triangulate(pose[9:18] if k & 1 else pose[0:9], pose[18:21], k >= 2, x1, y1, x2, y2)
    if d is None:
        return False, 0.0
    return d[0] > 0.0 and d[0] < dist and d[1] > 0.0 and d[1] < dist, d[0]


def choose_config(g):
    if g[0] >= g[1] and g[0] >= g[2] and g[0] >= g[3]:
        return 0
    if g[1] >= g[0] and g[1] >= g[2] and g[1] >= g[3]:
        return 1
    if g[2] >= g[0] and g[2] >= g[1] and g[2] >= g[3]:
        return 2
    return 3


def apply32(m, p):
    with np.errstate(all="ignore"):
        return [((m[4 * r] * p[0] + m[4 * r + 1] * p[1]) + m[4 * r + 2] * p[2]) + m[4 * r + 3] for r in range(3)]


def invert32(m):
    out = [f32(0)] * 12
    with np.errstate(all="ignore"):
        for r in range(3):
            abc = (m[r] * m[3] + m[4 + r] * m[7]) + m[8 + r] * m[11]
            out[4 * r], out[4 * r + 1], out[4 * r + 2], out[4 * r + 3] = m[r], m[4 + r], m[8 + r], -abc
    return out


def compose32(a, b):
    out = [f32(0)] * 12
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(4):
                p = (a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c]) + a[4 * r + 2] * b[8 + c]
                out[4 * r + c] = p + a[4 * r + 3] if c == 3 else p
    return out


def camera_transform(pose, k, local):
    R = pose[9:18] if k & 1 else pose[0:9]
    rt = []
    for i in range(3):
        rt += [f32(R[3 * i]), f32(R[3 * i + 1]), f32(R[3 * i + 2]), f32(-pose[18 + i] if k >= 2 else pose[18 + i])]
    return compose32(compose32(local, invert32(rt)), invert32(local))


def order_key(v):
    b = int(np.float32(v).view(np.uint32))
    if (b & 0x7FFFFFFF) > 0x7F800000:
        return 0xFFFFFFFF
    return (~b) & 0xFFFFFFFF if b & 0x80000000 else b | 0x80000000


def key_value(k):
    if k == 0xFFFFFFFF:
        return f32(np.nan)
    return np.uint32(k & 0x7FFFFFFF if k & 0x80000000 else (~k) & 0xFFFFFFFF).view(np.float32)


def scaled_error(p, g, s):
    with np.errstate(all="ignore"):
        dx, dy, dz = p[0] * s - g[0], p[1] * s - g[1], p[2] * s - g[2]
        return (dx * dx + dy * dy) + dz * dz


def norm3(x, y, z):
    with np.errstate(all="ignore"):
        return np.sqrt((x * x + y * y) + z * z)


def threshold2(thr, fx, fy):
    t = float(thr) / ((float(f32(fx)) + float(f32(fy))) / 2.0)
    return f32(t * t)


def unique_rows(ids):
    seen = {}
    for r, i in enumerate(ids):
        c = seen.get(int(i), (0, 0))
        seen[int(i)] = (c[0] + 1, r)
    return {i: r for i, (n, r) in seen.items() if n == 1}


def guess_is_null(g):
    g = np.asarray(g, np.float32).reshape(12)
    return bool(np.all(g == 0) or np.any(np.isnan(g)))


def join(from_ids, from_points, to_ids, to_points, camera, from_points3=None):
    """-> the pairs' ids ascending and the planes [7 x m] float32 (normalised x, y, x', y' and the from 3-D point, zeros without)"""
    fx, fy, cx, cy = [f32(v) for v in camera]
    fr, to = unique_rows(from_ids), unique_rows(to_ids)
    ids = sorted(i for i in to if i >= 0 and i in fr)
    fp, tp = np.asarray(from_points, np.float32).reshape(-1, 2), np.asarray(to_points, np.float32).reshape(-1, 2)
    rf, rt = [fr[i] for i in ids], [to[i] for i in ids]
    X = np.zeros((7, len(ids)), np.float32)
    if ids:
        with np.errstate(all="ignore"):
            X[0], X[1] = (fp[rf, 0] - cx) / fx, (fp[rf, 1] - cy) / fy
            X[2], X[3] = (tp[rt, 0] - cx) / fx, (tp[rt, 1] - cy) / fy
        if from_points3 is not None:
            X[4:7] = np.asarray(from_points3, np.float32).reshape(-1, 3)[rf].T
    return ids, X


def candidates(X, seed, iterations, thr2, on_candidate=None):
    """the RANSAC of steps 3 and 4 -> (best key or 0, per-hypothesis trace); on_candidate(c, E) sees every valid candidate's fp64 matrix"""
    m = X.shape[1]
    ws = [0.0] * 256
    best, trace = 0, []
    for h in range(iterations):
        idx = draw5(seed, h, m)
        if idx is None:
            trace.append("draw")
            continue
        t = []
        n = solve(ws, X[0][idx], X[1][idx], X[2][idx], X[3][idx], t)
        valid = []
        for r in range(n):
            E = make_model(ws, r)
            if E is None:
                continue
            valid.append(r)
            if on_candidate is not None:
                on_candidate(ROOTS * h + r, E)
            count = int(np.count_nonzero(count_inliers([f32(v) for v in E], X, thr2)))
            key = (count << 32) | ((~(ROOTS * h + r)) & 0xFFFFFFFF)
            if count > 0 and key > best:
                best = key
        trace.append(t[0] + ("" if len(valid) == n else "/valid%d" % len(valid)))
    return best, trace


def model(from_ids, from_points, to_ids, to_points, camera, from_points3=None, local_transform=None, guess=None, min_inliers=20, iterations=1000,
          reproj_threshold=2.0, variance_median_ratio=4, max_variance=0.1, distance_threshold=50.0, seed=0):
    """one pair -> dict(transform [12] float32, status, n_matches, variance (float), matches, inliers (lists of ids), points3 [n x 3] float32,
    trace dict(hypotheses, winner, counts, config, scale_branch, n_usable))"""
    nf, nt = len(from_ids), len(to_ids)
    out = dict(transform=np.zeros(12, np.float32), status=ST_FEW_FEATURES, variance=1.0, matches=[], inliers=[], points3=np.zeros((0, 3), np.float32),
               trace=dict(hypotheses=[], winner=None, counts=None, config=None, scale_branch=None, n_usable=0))
    if nf < min_inliers or nt < min_inliers:
        return out
    ids, X = join(from_ids, from_points, to_ids, to_points, camera, from_points3)
    out["matches"] = ids
    m = len(ids)
    out["status"] = ST_FEW_PAIRS
    if m < MIN_PAIRS:
        return out
    thr2 = threshold2(reproj_threshold, camera[0], camera[1])
    best, out["trace"]["hypotheses"] = candidates(X, seed, iterations, thr2)
    out["status"] = ST_NO_MODEL
    if best == 0:
        return out
    c = (~best) & 0xFFFFFFFF
    h, r = c // ROOTS, c % ROOTS
    out["trace"]["winner"] = (h, r, best >> 32)
    ws = [0.0] * 256
    idx = draw5(seed, h, m)
    solve(ws, X[0][idx], X[1][idx], X[2][idx], X[3][idx])
    E = make_model(ws, r)
    pose = decompose(E)
    if pose is None:
        return out
    mask = count_inliers([f32(v) for v in E], X, thr2)
    dist = float(distance_threshold)
    tests = [[config_test(pose, k, X[0][i], X[1][i], X[2][i], X[3][i], dist) if mask[i] else (False, 0.0) for i in range(m)] for k in range(4)]
    counts = [sum(1 for t in tests[k] if t[0]) for k in range(4)]
    cfg = choose_config(counts)
    out["trace"]["counts"], out["trace"]["config"] = counts, cfg
    local = [f32(v) for v in (IDENTITY if local_transform is None else np.asarray(local_transform, np.float32).reshape(12))]
    rows = [i for i in range(m) if tests[cfg][i][0]]
    pts = []
    for i in rows:
        d1 = tests[cfg][i][1]
        pts.append(apply32(local, [f32(d1 * float(X[0][i])), f32(d1 * float(X[1][i])), f32(d1)]))
    T = camera_transform(pose, cfg, local)
    has_guess = guess is not None and not guess_is_null(guess)
    scale, variance = f32(1.0), f32(1.0)
    branch = "none"
    with np.errstate(all="ignore"):
        if has_guess:
            g = np.asarray(guess, np.float32).reshape(12)
            scale = norm3(g[3], g[7], g[11]) / norm3(T[3], T[7], T[11])
            branch = "guess"
        if from_points3 is not None:
            G = [[X[4][i], X[5][i], X[6][i]] for i in rows]
            usable = [j for j in range(len(rows)) if all(np.isfinite(pts[j])) and all(np.isfinite(G[j])) and any(v != 0 for v in pts[j]) and any(v != 0 for v in G[j])]
            n = len(usable)
            out["trace"]["n_usable"] = n
            if n > 0:
                rank = min(n >> variance_median_ratio, n - 1)
                P = np.array([pts[j] for j in usable], np.float32)
                Q = np.array([G[j] for j in usable], np.float32)
                for cnd in range(1 if has_guess else n):
                    s = scale if has_guess else Q[cnd][0] / P[cnd][0]
                    e = scaled_error(P.T, Q.T, s)
                    keys = sorted(order_key(v) for v in e)
                    var = f32(2.1981 * float(key_value(keys[rank])))
                    if has_guess or cnd == 0 or var < variance:
                        variance, scale = var, s
                branch = "guess+points" if has_guess else "points"
            elif not has_guess:
                branch = "points/none usable"
        if scale != f32(1.0):
            T[3], T[7], T[11] = T[3] * scale, T[7] * scale, T[11] * scale
            pts = [[v * scale for v in p] if all(np.isfinite(p)) else p for p in pts]
    out["trace"]["scale_branch"] = branch
    out["inliers"] = [ids[i] for i in rows]
    out["points3"] = np.array(pts, np.float32).reshape(-1, 3)
    out["variance"] = float(variance)
    out["status"] = ST_FEW_INLIERS if len(rows) < min_inliers else (ST_OK if float(variance) <= float(f32(max_variance)) else ST_HIGH_VARIANCE)
    if out["status"] == ST_OK:
        out["transform"] = np.array(T, np.float32)
    return out


# ---- the float64 yardstick: the same draws and the same scoring, the solver by numpy.linalg.svd and numpy.roots

def yardstick_models(x1, y1, x2, y2):
    """Nister's five-point solution in float64 with library linear algebra -> the list of 3 x 3 matrices of one sample"""
    A = np.array([[xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, 1.0] for x, y, xp, yp in zip(x1, y1, x2, y2)], np.float64)
    N = np.linalg.svd(A)[2][5:9]                                       # the null space, any basis
    import itertools
    exps = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0), (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2),
            (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
    lin = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]

    def mul(p, q):
        o = {}
        for (a, u), (b, v) in itertools.product(p.items(), q.items()):
            k = (a[0] + b[0], a[1] + b[1], a[2] + b[2])
            o[k] = o.get(k, 0.0) + u * v
        return o

    def add(p, q, s=1.0):
        o = dict(p)
        for k, v in q.items():
            o[k] = o.get(k, 0.0) + s * v
        return o

    E = [[{lin[k]: N[k][3 * i + j] for k in range(4)} for j in range(3)] for i in range(3)]
    det = add(add(mul(add(mul(E[1][1], E[2][2]), mul(E[1][2], E[2][1]), -1.0), E[0][0]),
                  mul(add(mul(E[1][0], E[2][2]), mul(E[1][2], E[2][0]), -1.0), E[0][1]), -1.0),
              mul(add(mul(E[1][0], E[2][1]), mul(E[1][1], E[2][0]), -1.0), E[0][2]))
    EEt = [[{} for _ in range(3)] for _ in range(3)]
    for i in range(3):
        for k in range(3):
            for n in range(3):
                EEt[i][k] = add(EEt[i][k], mul(E[i][n], E[k][n]))
    tr = add(add(EEt[0][0], EEt[1][1]), EEt[2][2])
    rows = [det]
    for i in range(3):
        for j in range(3):
            p = {}
            for k in range(3):
                p = add(p, mul(add(EEt[i][k], tr, -0.5) if k == i else EEt[i][k], E[k][j]))
            rows.append(p)
    M = np.array([[p.get(e, 0.0) for e in exps] for p in rows], np.float64)
    try:
        Rm = np.linalg.solve(M[:, :10], M[:, 10:])
    except np.linalg.LinAlgError:
        return []
    P = np.polynomial.polynomial

    def brow(a, b):
        za = lambda c: P.polymul([0.0, 1.0], c)
        x = P.polysub(Rm[a][0:3][::-1], za(Rm[b][0:3][::-1]))
        y = P.polysub(Rm[a][3:6][::-1], za(Rm[b][3:6][::-1]))
        c = P.polysub(Rm[a][6:10][::-1], za(Rm[b][6:10][::-1]))
        return x, y, c

    Bm = [brow(4, 5), brow(6, 7), brow(8, 9)]
    mnr = lambda a, b, c, d: P.polysub(P.polymul(a, d), P.polymul(b, c))
    poly = P.polyadd(P.polysub(P.polymul(Bm[0][0], mnr(Bm[1][1], Bm[1][2], Bm[2][1], Bm[2][2])),
                               P.polymul(Bm[0][1], mnr(Bm[1][0], Bm[1][2], Bm[2][0], Bm[2][2]))),
                     P.polymul(Bm[0][2], mnr(Bm[1][0], Bm[1][1], Bm[2][0], Bm[2][1])))
    out = []
    for z in np.roots(poly[::-1]):
        if abs(z.imag) > 1e-9 * max(1.0, abs(z.real)):
            continue
        z = z.real
        Bz = np.array([[P.polyval(z, c) for c in row] for row in Bm])
        v = np.linalg.svd(Bz)[2][2]
        if v[2] == 0:
            continue
        x, y = v[0] / v[2], v[1] / v[2]
        out.append((x * N[0] + y * N[1] + z * N[2] + N[3]).reshape(3, 3))
    return out


def yardstick(X, seed, iterations, thr2, dtypes=(np.float64,)):
    """the best essential matrix over the same draws, the solver in float64, the scoring in each of dtypes -> per dtype (E [3 x 3] or None,
    inlier mask); the first of the highest count wins"""
    m = X.shape[1]
    best = [[0, None, np.zeros(m, bool)] for _ in dtypes]
    Xd = [X[:4].astype(dt) for dt in dtypes]
    for h in range(iterations):
        idx = draw5(seed, h, m)
        if idx is None:
            continue
        for E in yardstick_models(X[0][idx].astype(np.float64), X[1][idx].astype(np.float64), X[2][idx].astype(np.float64), X[3][idx].astype(np.float64)):
            for b, dt, x in zip(best, dtypes, Xd):
                with np.errstate(all="ignore"):
                    mask = sampson(E.reshape(9).astype(dt), x[0], x[1], x[2], x[3]) <= dt(thr2)
                n = int(np.count_nonzero(mask))
                if n > b[0]:
                    b[0], b[1], b[2] = n, E, mask
    return [(b[1], b[2]) for b in best]


def yardstick_pose(E, X, mask, dist=50.0):
    """cv::recoverPose in float64 with numpy.linalg.svd -> (R, t, mask) of the configuration with most points in front"""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])
    best = None
    for R, t in ((U @ W @ Vt, U[:, 2]), (U @ W.T @ Vt, U[:, 2]), (U @ W @ Vt, -U[:, 2]), (U @ W.T @ Vt, -U[:, 2])):
        good = np.zeros(X.shape[1], bool)
        for i in np.nonzero(mask)[0]:
            a, b = R @ np.array([X[0][i], X[1][i], 1.0], np.float64), np.array([X[2][i], X[3][i], 1.0], np.float64)
            sol = np.linalg.lstsq(np.stack([a, -b], 1), -t, rcond=None)[0]
            good[i] = 0 < sol[0] < dist and 0 < sol[1] < dist
        if best is None or np.count_nonzero(good) > np.count_nonzero(best[2]):
            best = (R, t, good)
    return best


def yardstick_scale(R, t, good, X, ratio=4):
    """the scale block of util3d_features.cpp:304-357 in float64 for the yardstick's pose: one candidate per correspondence, s = g.x / p.x, the
    error list's element at size >> ratio, the smallest wins -> the scale (the baseline, t being a unit vector)"""
    rows = np.nonzero(good)[0]
    P = []
    for i in rows:
        a, b = R @ np.array([X[0][i], X[1][i], 1.0], np.float64), np.array([X[2][i], X[3][i], 1.0], np.float64)
        d1 = np.linalg.lstsq(np.stack([a, -b], 1), -t, rcond=None)[0][0]
        P.append(d1 * np.array([X[0][i], X[1][i], 1.0], np.float64))
    P, G = np.array(P), X[4:7, rows].T.astype(np.float64)
    best = None
    for i in range(len(rows)):
        s = G[i, 0] / P[i, 0]
        e = np.sort(((s * P - G) ** 2).sum(1))
        var = 2.1981 * e[min(len(rows) >> ratio, len(rows) - 1)]
        if best is None or var < best[0]:
            best = (var, s)
    return best[1]
