"""The rule of lcd_verify_epipolar (include/lcd.h) in NumPy, operation for operation: np.float32 arrays and scalars (every NumPy operation rounds
once, nothing is fused).  Vectorised over hypotheses and correspondences, which changes no rounding: every element sees the same operations in
the same order.  Beside it `yardstick`: the same samples, error and winner rule with different linear algebra -- the null space by
numpy.linalg.svd and the roots by numpy.roots -- in float64 (or, to measure the yardstick's own sensitivity to precision, float32)."""
import numpy as np

from motion_3d_model import F, M32, MAX_ROWS, Refused, bits, mix, lane_sum  # noqa: F401

BISECT = 26
MAX_DRAWS = 32
MIN_PAIRS = 8
OK, FEW_PAIRS, NO_MODEL, FEW_INLIERS = 0, 1, 2, 3
SQRT2 = F(1.41421356)
ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")
TINY = np.finfo(np.float32).tiny                                           # the smallest normal float32


def correspondences(from_ids, from_points, to_ids, to_points):
    """step 1 -> (ids [m] int32 ascending, X [m x 4] = u, v, u', v')"""
    from_ids = np.asarray(from_ids, np.int32).reshape(-1)
    to_ids = np.asarray(to_ids, np.int32).reshape(-1)
    P = np.asarray(from_points, np.float32).reshape(-1, 2)
    Q = np.asarray(to_points, np.float32).reshape(-1, 2)

    def unique_rows(ids):
        vals, first, counts = np.unique(ids, return_index=True, return_counts=True)
        return {int(v): int(r) for v, r, c in zip(vals, first, counts) if c == 1}

    f, t = unique_rows(from_ids), unique_rows(to_ids)
    ids = [i for i in sorted(t) if i >= 0 and i in f]
    X = np.zeros((len(ids), 4), np.float32)
    for k, i in enumerate(ids):
        X[k, :2] = P[f[i]]
        X[k, 2:] = Q[t[i]]
    return np.array(ids, np.int32), X


def subnormal(*arrays):
    """whether any value is a nonzero subnormal float32"""
    return any(bool(((a != 0) & (np.abs(a) < TINY)).any()) for a in map(np.asarray, arrays))


def normalisation(P, info=None):
    """step 2 for one image, P [m x 2] -> (ok, s, tx, ty); info (a list): whether a distance square was subnormal is appended"""
    m = F(P.shape[0])
    with np.errstate(**ERR):
        sums = lane_sum(P)
        cx, cy = sums[0] / m, sums[1] / m
        dx, dy = P[:, 0] - cx, P[:, 1] - cy
        xx, yy = dx * dx, dy * dy
        dd = xx + yy
        if info is not None:
            info.append(subnormal(xx, yy, dd))
        dist = np.sqrt(dd)
        d = lane_sum(dist) / m
        if not (d > F(0)) or not np.isfinite(d):
            return False, F(0), F(0), F(0)
        s = SQRT2 / d
        return True, s, -(s * cx), -(s * cy)


def draw7(seed, h, m):
    base = (mix((seed + h) & M32) * 8) & M32
    got = []
    for k in range(MAX_DRAWS):
        d = mix((base + k) & M32) % m
        if d in got:
            continue
        got.append(d)
        if len(got) == 7:
            return got
    return None


def null_space(A):
    """A [H x 7 x 9] (changed in place) -> ok [H], F1 [H x 9], F2 [H x 9]"""
    H = A.shape[0]
    idx = np.arange(H)
    perm = np.tile(np.arange(9), (H, 1))
    ok = np.ones(H, bool)
    for k in range(7):
        mag = np.abs(A[:, k:, k:]).reshape(H, -1)
        mag = np.where(np.isnan(mag), F(-1), mag)
        flat = np.argmax(mag, axis=1)                # the first of the largest: the lowest row, then the lowest column
        pr, pc = k + flat // (9 - k), k + flat % (9 - k)
        tmp = A[idx, k, :].copy()
        A[idx, k, :] = A[idx, pr, :]
        A[idx, pr, :] = tmp
        tmp = A[idx, :, k].copy()
        A[idx, :, k] = A[idx, :, pc]
        A[idx, :, pc] = tmp
        tmp = perm[idx, k].copy()
        perm[idx, k] = perm[idx, pc]
        perm[idx, pc] = tmp
        piv = A[:, k, k].copy()
        ok &= (piv != F(0)) & np.isfinite(piv)
        A[:, k, k + 1:] = A[:, k, k + 1:] / piv[:, None]
        A[:, k, k] = F(1)
        f = A[:, :, k].copy()
        new = A[:, :, k + 1:] - f[:, :, None] * A[:, k, None, k + 1:]
        rows = np.arange(7) != k
        A[:, rows, k + 1:] = new[:, rows]
        A[:, rows, k] = F(0)
    one, zero = np.ones((H, 1), np.float32), np.zeros((H, 1), np.float32)
    v1 = np.concatenate([-A[:, :, 7], one, zero], axis=1)
    v2 = np.concatenate([-A[:, :, 8], zero, one], axis=1)
    F1, F2 = np.zeros((H, 9), np.float32), np.zeros((H, 9), np.float32)
    F1[idx[:, None], perm] = v1
    F2[idx[:, None], perm] = v2
    return ok, F1, F2


def det3(M):
    m0 = M[..., 4] * M[..., 8] - M[..., 5] * M[..., 7]
    m1 = M[..., 3] * M[..., 8] - M[..., 5] * M[..., 6]
    m2 = M[..., 3] * M[..., 7] - M[..., 4] * M[..., 6]
    return (M[..., 0] * m0 - M[..., 1] * m1) + M[..., 2] * m2


def cubic_of(F1, F2):
    """-> ok [H], c [H x 4] (c0 .. c3)"""
    half = F1.dtype.type(0.5)
    d0, dp, dm, d3 = det3(F2), det3(F1 + F2), det3(F2 - F1), det3(F1)
    c = np.stack([d0, half * (dp - dm) - d3, half * (dp + dm) - d0, d3], axis=1)
    return (c[:, 3] != 0) & np.isfinite(c).all(axis=1), c


def poly3(c, x):
    return ((c[:, 3] * x + c[:, 2]) * x + c[:, 1]) * x + c[:, 0]


def bisect(c, lo, hi):
    """-> has [H], root [H]"""
    plo, phi = poly3(c, lo), poly3(c, hi)
    neg_lo = plo < F(0)
    has = neg_lo != (phi < F(0))
    a, b = lo.copy(), hi.copy()
    for _ in range(BISECT):
        mid = F(0.5) * (a + b)
        left = (poly3(c, mid) < F(0)) == neg_lo
        a, b = np.where(left, mid, a), np.where(left, b, mid)
    return has, F(0.5) * (a + b)


def cubic_roots(c, info=None):
    """-> ok [H], n [H], roots [H x 3] (the first n are the roots found, in the brackets' order); info (a dict) receives per hypothesis
    `clamped` (two real roots of the derivative and k1 or k2 is not the root itself but +-B) and `disc_nonpos` (disc <= 0, or NaN)"""
    c3 = c[:, 3]
    q = np.abs(c[:, :3] / c3[:, None])
    m01 = np.where(q[:, 0] > q[:, 1], q[:, 0], q[:, 1])
    mx = np.where(m01 > q[:, 2], m01, q[:, 2])
    B = F(1) + mx
    nB = -B
    ok = np.isfinite(B)
    a, b = F(3) * c3, F(2) * c[:, 2]
    disc = b * b - F(4) * (a * c[:, 1])
    two = disc > F(0)
    sq = np.sqrt(np.where(two, disc, F(0)))
    den = F(2) * a
    r1, r2 = (-b - sq) / den, (-b + sq) / den
    lo, hi = np.where(r1 < r2, r1, r2), np.where(r1 < r2, r2, r1)
    lo1, hi1 = np.where(lo < nB, nB, lo), np.where(hi < nB, nB, hi)
    k1, k2 = np.where(lo1 > B, B, lo1), np.where(hi1 > B, B, hi1)
    k1, k2 = np.where(k1 == k1, k1, B), np.where(k2 == k2, k2, B)
    if info is not None:
        info.update(clamped=two & ((k1 != lo) | (k2 != hi)), disc_nonpos=~two)
    k1, k2 = np.where(two, k1, B), np.where(two, k2, B)
    H = c.shape[0]
    n = np.zeros(H, np.int64)
    roots = np.zeros((H, 3), np.float32)
    for lo_, hi_ in ((nB, k1), (k1, k2), (k2, B)):
        has, x = bisect(c, lo_, hi_)
        rows = np.nonzero(has)[0]
        roots[rows, n[rows]] = x[rows]
        n[rows] += 1
    return ok, np.where(ok, n, 0), roots


def denormalise(Fn, nf, nt):
    """Fn [.. x 9]; nf, nt = (s, tx, ty) -> F [.. x 9] = T'^T (F^ T)"""
    s, tx, ty = nf
    G = np.empty_like(Fn)
    for r in range(3):
        G[..., 3 * r] = Fn[..., 3 * r] * s
        G[..., 3 * r + 1] = Fn[..., 3 * r + 1] * s
        G[..., 3 * r + 2] = (Fn[..., 3 * r] * tx + Fn[..., 3 * r + 1] * ty) + Fn[..., 3 * r + 2]
    s, tx, ty = nt
    out = np.empty_like(Fn)
    for c in range(3):
        out[..., c] = s * G[..., c]
        out[..., 3 + c] = s * G[..., 3 + c]
        out[..., 6 + c] = (tx * G[..., c] + ty * G[..., 3 + c]) + G[..., 6 + c]
    return out


def line_parts(f, u, v, pu, pv):
    """f: nine [C x 1] entries in the order the line is built from; points [1 x m] -> (dd, n), the error's numerator and denominator"""
    lx = (f[0] * u + f[1] * v) + f[2]
    ly = (f[3] * u + f[4] * v) + f[5]
    lz = (f[6] * u + f[7] * v) + f[8]
    d = (pu * lx + pv * ly) + lz
    return d * d, lx * lx + ly * ly


def line_error(f, u, v, pu, pv):
    dd, n = line_parts(f, u, v, pu, pv)
    return dd / n


def transposed(f):
    return [f[0], f[3], f[6], f[1], f[4], f[7], f[2], f[5], f[8]]


def inliers_of(models, X, thr2):
    """models [C x 9], X [m x 4] -> [C x m] bool"""
    f = [models[:, k, None] for k in range(9)]
    u, v, up, vp = (X[None, :, k] for k in range(4))
    with np.errstate(**ERR):
        e1 = line_error(f, u, v, up, vp)
        e2 = line_error(transposed(f), up, vp, u, v)
        return (e1 <= thr2) & (e2 <= thr2)


def line_subnormal(model, X):
    """whether dd or n of either line error of one model [9] is a nonzero subnormal for some correspondence"""
    f = [model[None, k, None] for k in range(9)]
    u, v, up, vp = (X[None, :, k] for k in range(4))
    with np.errstate(**ERR):
        return subnormal(*line_parts(f, u, v, up, vp), *line_parts(transposed(f), up, vp, u, v))


def lead_of(Fm):
    """the largest-magnitude entry, the lowest index on ties"""
    return Fm[int(np.argmax(np.abs(Fm)))]


def unit_matrix(Fm):
    total = F(0)
    for k in range(9):
        total = total + Fm[k] * Fm[k]
    lead = lead_of(Fm)
    n = np.sqrt(total)
    return (Fm / (-n if lead < F(0) else n)).astype(np.float32)


def samples(seed, iterations, m):
    """-> valid [H], idx [H x 7]"""
    valid = np.zeros(iterations, bool)
    idx = np.zeros((iterations, 7), np.int64)
    for h in range(iterations):
        d = draw7(seed, h, m)
        if d is not None:
            valid[h], idx[h] = True, d
    return valid, idx


def candidates(X, seed, iterations, nf, nt, trace=None):
    """step 3 -> valid [3 H], models [3 H x 9]"""
    m = X.shape[0]
    drawn, idx = samples(seed, iterations, m)
    with np.errstate(**ERR):
        x, y = nf[0] * X[:, 0] + nf[1], nf[0] * X[:, 1] + nf[2]
        xp, yp = nt[0] * X[:, 2] + nt[1], nt[0] * X[:, 3] + nt[2]
        x, y, xp, yp = x[idx], y[idx], xp[idx], yp[idx]                   # [H x 7]
        A = np.stack([xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, np.ones_like(x)], axis=2).astype(np.float32)
        pivots, F1, F2 = null_space(A)
        cubic, c = cubic_of(F1, F2)
        info = {}
        bounded, n, roots = cubic_roots(c, info)
        ok = drawn & pivots & cubic & bounded
        Fn = roots[:, :, None] * F1[:, None, :] + F2[:, None, :]          # [H x 3 x 9]
        models = denormalise(Fn, nf, nt)
    valid = ok[:, None] & (np.arange(3)[None, :] < n[:, None])
    if trace is not None:
        trace.update(not_drawn=int((~drawn).sum()), no_pivot=int((drawn & ~pivots).sum()), c3_zero=int((drawn & pivots & (c[:, 3] == 0)).sum()),
                     bad_cubic=int((drawn & pivots & ~cubic).sum()), one_root=int((ok & (n == 1)).sum()), three_roots=int((ok & (n == 3)).sum()),
                     per_hypothesis=dict(n_roots=np.where(ok, n, 0), **info))
    return valid.reshape(-1), models.reshape(-1, 9)


def best_candidate(valid, models, X, thr2, chunk=1 << 21, trace=None):
    """step 5 -> (count, candidate) of the winner; count 0: none; trace receives `tied`, every valid candidate that reaches the count, ascending"""
    counts = np.zeros(valid.shape[0], np.int64)
    step = max(chunk // max(X.shape[0], 1), 1)
    for c0 in range(0, valid.shape[0], step):
        counts[c0:c0 + step] = inliers_of(models[c0:c0 + step], X, thr2).sum(axis=1)
    counts = np.where(valid, counts, 0)
    best = int(np.argmax(counts)) if counts.size else 0
    if trace is not None:
        trace.update(tied=[int(c) for c in np.nonzero(valid & (counts == counts[best]) & (counts > 0))[0]] if counts.size else [])
    return (int(counts[best]) if counts.size else 0), best


def check_args(n_from, n_to, match_count_min, iterations, ransac_threshold):
    thr = F(ransac_threshold)
    with np.errstate(**ERR):
        thr2 = thr * thr
    if n_from > MAX_ROWS or n_to > MAX_ROWS or iterations > 65535:
        raise Refused("unsupported")
    if iterations < 1 or match_count_min < 1 or not np.isfinite(ransac_threshold) or not (thr > 0) or not np.isfinite(thr) or not (thr2 > 0) or \
            not np.isfinite(thr2):
        raise Refused("invalid")
    return thr2


def verify(from_ids, from_points, to_ids, to_points, match_count_min=8, iterations=1000, ransac_threshold=3.0, seed=0, trace=None):
    """the whole rule for one pair -> dict(fundamental [9], status, matches, inliers)"""
    thr2 = check_args(np.asarray(from_ids).size, np.asarray(to_ids).size, match_count_min, iterations, ransac_threshold)
    ids, X = correspondences(from_ids, from_points, to_ids, to_points)
    m = ids.shape[0]
    out = dict(fundamental=np.zeros(9, np.float32), status=FEW_PAIRS, matches=ids, inliers=np.zeros(0, np.int32))
    if m < match_count_min or m < MIN_PAIRS:
        return out
    out["status"] = NO_MODEL
    squares = []
    okf, *nf = normalisation(X[:, :2], squares)
    okt, *nt = normalisation(X[:, 2:], squares)
    if not (okf and okt):
        return out
    if trace is not None:
        trace.update(subnormal=dict(distance=any(squares), thr2=subnormal(thr2), line=False))
    valid, models = candidates(X, seed, iterations, nf, nt, trace)
    count, best = best_candidate(valid, models, X, thr2, trace=trace)
    per = trace.pop("per_hypothesis") if trace is not None else None
    if count == 0:
        return out
    inl = inliers_of(models[best:best + 1], X, thr2)[0]
    out["inliers"] = ids[inl]
    with np.errstate(**ERR):
        out["fundamental"] = unit_matrix(models[best])
    out["status"] = OK if count >= match_count_min else FEW_INLIERS
    if trace is not None:
        trace.update(best=best, count=count, root=best % 3, n_roots=int(per["n_roots"][best // 3]), lead_negative=bool(lead_of(models[best]) < F(0)),
                     clamped=dict(clamped=bool(per["clamped"][best // 3]), disc_nonpos=bool(per["disc_nonpos"][best // 3])))
        trace["subnormal"]["line"] = line_subnormal(models[best], X)
    return out


# ---- the yardstick: the same samples, error and winner rule; the linear algebra by numpy.linalg.svd and numpy.roots

def yardstick(from_ids, from_points, to_ids, to_points, match_count_min=8, iterations=1000, ransac_threshold=3.0, seed=0, dtype=np.float64):
    """-> dict(status, matches, inliers) in `dtype` arithmetic"""
    T = np.dtype(dtype).type
    ids, X32 = correspondences(from_ids, from_points, to_ids, to_points)
    m = ids.shape[0]
    out = dict(status=FEW_PAIRS, matches=ids, inliers=np.zeros(0, np.int32))
    if m < match_count_min or m < MIN_PAIRS:
        return out
    out["status"] = NO_MODEL
    X = X32.astype(dtype)

    def hartley(P):
        c = P.mean(axis=0, dtype=dtype)
        d = np.sqrt(((P - c) ** 2).sum(axis=1)).mean(dtype=dtype)
        s = T(np.sqrt(2.0)) / d
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]], dtype)

    with np.errstate(**ERR):
        Tf, Tt = hartley(X[:, :2]), hartley(X[:, 2:])
        if not (np.isfinite(Tf).all() and np.isfinite(Tt).all()):
            return out
        ones = np.ones((m, 1), dtype)
        pf, pt = np.concatenate([X[:, :2], ones], 1), np.concatenate([X[:, 2:], ones], 1)
        qf, qt = pf @ Tf.T, pt @ Tt.T
        drawn, idx = samples(seed, iterations, m)
        x, y, xp, yp = qf[idx, 0], qf[idx, 1], qt[idx, 0], qt[idx, 1]
        A = np.stack([xp * x, xp * y, xp, yp * x, yp * y, yp, x, y, np.ones_like(x)], axis=2).astype(dtype)
        A[~np.isfinite(A).all(axis=(1, 2))] = 0
        Vt = np.linalg.svd(A, full_matrices=True)[2]
        F1, F2 = Vt[:, 7, :], Vt[:, 8, :]
        _, c = cubic_of(F1, F2)
        tol = T(1e-8 if dtype == np.float64 else 1e-4)
        models = np.zeros((iterations, 3, 9), dtype)
        valid = np.zeros((iterations, 3), bool)
        for h in range(iterations):
            if not drawn[h] or c[h, 3] == 0 or not np.isfinite(c[h]).all():
                continue
            r = np.roots(c[h, ::-1])
            real = np.sort(r.real[np.abs(r.imag) <= tol * np.maximum(1, np.abs(r.real))]).astype(dtype)
            for k, xr in enumerate(real[:3]):
                Fn = (xr * F1[h] + F2[h]).reshape(3, 3)
                models[h, k] = (Tt.T @ Fn @ Tf).reshape(9)
                valid[h, k] = True
        thr = T(np.float32(ransac_threshold))
        count, best = best_candidate(valid.reshape(-1), models.reshape(-1, 9), X, thr * thr)
        if count == 0:
            return out
        inl = inliers_of(models.reshape(-1, 9)[best:best + 1], X, thr * thr)[0]
    out["inliers"] = ids[inl]
    out["status"] = OK if count >= match_count_min else FEW_INLIERS
    return out
