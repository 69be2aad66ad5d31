"""The rule of lcd_register_icp (include/lcd.h) in NumPy, brute force, operation for operation: np.float32 arrays and scalars where the rule is
fp32 (every NumPy operation rounds once, nothing is fused), np.float64 where it says fp64.  Vectorised over rows, which changes no rounding:
every element sees the same operations in the same order.  Also icp64, an independent float64 ICP with the same loop, which the fp32 rule is
measured against and which is not part of it."""
import numpy as np

from motion_3d_model import F, D, MAX_ROWS, Refused, bits, horn_fit, invert, lane_sum  # noqa: F401
from motion_pnp_model import compose, IDENTITY

OK, EMPTY, NOT_CONVERGED, BELOW_RATIO = 0, 1, 2, 3
STOP_NONE, STOP_ITERATIONS, STOP_TRANSFORM, STOP_MSE, STOP_FEW_CORRESPONDENCES = 0, 1, 2, 3, 4
SEARCH_AUTO, SEARCH_BRUTE, SEARCH_GRID = 0, 1, 2
VARIANCE_FACTOR = D(2.1981)
MSE_EPS = F(1e-12)
FLT_MAX = np.finfo(np.float32).max
INF = F(np.inf)


def apply(T, P):
    """T(p) for the rows of P [n x 3] -> [n x 3]"""
    T = np.asarray(T, np.float32)
    with np.errstate(all="ignore"):
        cols = [((T[4 * r] * P[:, 0] + T[4 * r + 1] * P[:, 1]) + T[4 * r + 2] * P[:, 2]) + T[4 * r + 3] for r in range(3)]
    return np.stack(cols, axis=1).astype(np.float32).reshape(-1, 3)


def nearest(P, part_p, C, part_c, chunk=512):
    """step 2 for every row of P in C -> (row [n] int32, -1: none; d2 [n] f32, +inf with none).  Rows that take no part neither ask nor answer."""
    n = P.shape[0]
    row = np.full(n, -1, np.int32)
    best = np.full(n, INF, np.float32)
    if n == 0 or C.shape[0] == 0:
        return row, best
    with np.errstate(all="ignore"):
        for s in range(0, n, chunk):
            p = P[s:s + chunk]
            dx, dy, dz = p[:, None, 0] - C[None, :, 0], p[:, None, 1] - C[None, :, 1], p[:, None, 2] - C[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(np.isnan(d2) | ~part_c[None, :], INF, d2).astype(np.float32)
            j = np.argmin(d2, axis=1)                                  # the first of the smallest: the lowest row
            d = d2[np.arange(p.shape[0]), j]
            found = (d < INF) & part_p[s:s + chunk]
            row[s:s + chunk] = np.where(found, j, -1)
            best[s:s + chunk] = np.where(found, d, INF)
    return row, best


def row_sum(E, has):
    """SUM over the row index: lane (row mod 256) adds the rows that `has` holds for, the others are skipped (adding +0 to a partial that
    began as +0 changes no bit of it, which is what the padding here does)"""
    E = np.asarray(E, np.float32)
    shape = has.shape + (1,) * (E.ndim - 1)
    return lane_sum(np.where(has.reshape(shape), E, F(0)).astype(np.float32))


def fit_2d(cp, cq, S):
    with np.errstate(all="ignore"):
        A = S[0] + S[4]
        B = S[1] - S[3]
        n = np.sqrt(A * A + B * B)
        if n != F(0) and np.isfinite(n):
            c, s = A / n, B / n
        else:
            c, s = F(1), F(0)
        rx = c * cp[0] - s * cp[1]
        ry = s * cp[0] + c * cp[1]
        return np.array([c, -s, 0, cq[0] - rx, s, c, 0, cq[1] - ry, 0, 0, 1, 0], np.float32)


def fit(P, Q, has, c, force_3dof):
    """step 4 over the rows that `has` holds for: P [n x 3] the current cloud, Q [n x 3] each row's correspondent (anything where there is none)"""
    with np.errstate(all="ignore"):
        cp = row_sum(P, has) / F(c)
        cq = row_sum(Q, has) / F(c)
        dp, dq = P - cp, Q - cq
        S = np.stack([row_sum(dp[:, a] * dq[:, b], has) for a in range(3) for b in range(3)])
    return fit_2d(cp, cq, S) if force_3dof else horn_fit(cp, cq, S)


def stop_of(T, iterations, max_iterations, eps2, mse, mse_prev):
    if iterations >= max_iterations:
        return STOP_ITERATIONS
    with np.errstate(all="ignore"):
        cosine = F(0.5) * (((T[0] + T[5]) + T[10]) - F(1))
        t2 = (T[3] * T[3] + T[7] * T[7]) + T[11] * T[11]
        if cosine >= F(1) - eps2 and t2 <= eps2:
            return STOP_TRANSFORM
        if np.abs(mse - mse_prev) < MSE_EPS:
            return STOP_MSE
    return STOP_NONE


def check_args(P, Q, guess, max_iterations, max_laser_scans, search, max_correspondence_distance, epsilon, correspondence_ratio, device_entry):
    thr = D(max_correspondence_distance)
    if P.shape[0] > MAX_ROWS or Q.shape[0] > MAX_ROWS:
        raise Refused("unsupported")
    with np.errstate(all="ignore"):
        if (max_iterations < 1 or max_laser_scans < 0 or search not in (SEARCH_AUTO, SEARCH_BRUTE, SEARCH_GRID) or not np.isfinite(thr) or not thr > 0 or
                not np.isfinite(thr * thr) or not np.isfinite(epsilon) or not epsilon >= 0 or not 0 <= correspondence_ratio <= 1 or
                not np.isfinite(guess).all()):
            raise Refused("invalid")
    if not device_entry and not (np.isfinite(P).all() and np.isfinite(Q).all()):
        raise Refused("invalid")


def register(from_xyz, to_xyz, guess=None, max_iterations=30, force_3dof=False, max_laser_scans=0, search=SEARCH_AUTO, max_correspondence_distance=0.1,
             epsilon=0.0, correspondence_ratio=0.1, device_entry=False):
    """one pair -> dict(transform, icp_transform, correction [12] f32, status, stop, iterations, n_correspondences, ratio f32, variance f64,
    match [n_from] int32, and for the tests: counts (c of every iteration), mses, models (T_k), from_is_target, kept_d2)"""
    P0 = np.ascontiguousarray(from_xyz, np.float32).reshape(-1, 3)
    T0 = np.ascontiguousarray(to_xyz, np.float32).reshape(-1, 3)
    guess = np.asarray(IDENTITY if guess is None else guess, np.float32).reshape(12)
    epsilon, ratio_min = F(epsilon), F(correspondence_ratio)
    check_args(P0, T0, guess, max_iterations, max_laser_scans, search, max_correspondence_distance, epsilon, ratio_min, device_entry)
    thr2 = D(max_correspondence_distance) * D(max_correspondence_distance)
    zeros = np.zeros(12, np.float32)
    r = dict(transform=zeros.copy(), icp_transform=zeros.copy(), correction=zeros.copy(), status=OK, stop=STOP_NONE, iterations=0, n_correspondences=0,
             ratio=F(0), variance=D(1.0), match=np.full(P0.shape[0], -1, np.int32), counts=[], mses=[], models=[], from_is_target=None,
             kept_d2=np.zeros(0, np.float32))
    part_f, part_t = np.isfinite(P0).all(axis=1), np.isfinite(T0).all(axis=1)
    nf, nt = int(part_f.sum()), int(part_t.sum())
    if nf == 0 or nt == 0:
        r["status"] = EMPTY
        return r
    Q = apply(guess, T0)
    P = P0.copy()
    Fm = IDENTITY.copy()
    with np.errstate(all="ignore"):
        eps2 = epsilon * epsilon
    mse_prev = F(FLT_MAX)
    while True:
        row, d2 = nearest(P, part_f, Q, part_t)
        has = (row >= 0) & (d2.astype(np.float64) <= thr2)
        c = int(has.sum())
        r["counts"].append(c)
        if c < 3:
            r["status"], r["stop"] = NOT_CONVERGED, STOP_FEW_CORRESPONDENCES
            return r
        with np.errstate(all="ignore"):
            mse = row_sum(d2, has) / F(c)
        T = fit(P, Q[np.maximum(row, 0)], has, c, force_3dof)
        P = np.where(part_f[:, None], apply(T, P), P).astype(np.float32)
        Fm = compose(T, Fm)
        r["iterations"] += 1
        r["mses"].append(mse)
        r["models"].append(T)
        stop = stop_of(T, r["iterations"], max_iterations, eps2, mse, mse_prev)
        if stop != STOP_NONE:
            break
        mse_prev = mse
    r["stop"] = stop
    A = np.where(part_f[:, None], apply(Fm, P0), P0).astype(np.float32)
    row_a, d2_a = nearest(A, part_f, Q, part_t)
    row_q, d2_q = nearest(Q, part_t, A, part_f)
    from_is_target = nf > nt
    r["from_is_target"] = from_is_target
    if from_is_target:
        src_row, src_d2, tgt_row = row_q, d2_q, row_a
    else:
        src_row, src_d2, tgt_row = row_a, d2_a, row_q
    idx = np.arange(src_row.shape[0])
    keep = (src_row >= 0) & (src_d2.astype(np.float64) <= thr2)
    keep &= tgt_row[np.maximum(src_row, 0)] == idx
    n = int(keep.sum())
    if from_is_target:
        r["match"][src_row[keep]] = idx[keep]
    else:
        r["match"][keep] = src_row[keep]
    r["n_correspondences"] = n
    r["kept_d2"] = src_d2[keep]
    if n >= 3:
        s = np.sort(bits(src_d2[keep]))
        r["variance"] = VARIANCE_FACTOR * D(s[n >> 1:][:1].view(np.float32)[0])
    r["ratio"] = F(n) / F(max_laser_scans if max_laser_scans > 0 else max(nf, nt))
    X = compose(invert(Fm), guess)
    r["icp_transform"] = Fm
    r["correction"] = compose(invert(guess), X)
    if r["ratio"] <= ratio_min:
        r["status"] = BELOW_RATIO
        return r
    r["transform"] = X
    return r


# ---- what the rule is measured against: the same loop in float64, written independently

def _kabsch(P, Q, flat):
    cp, cq = P.mean(axis=0), Q.mean(axis=0)
    H = (P - cp).T @ (Q - cq)
    if flat:
        a = np.arctan2(H[0, 1] - H[1, 0], H[0, 0] + H[1, 1])
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        t = cq - R @ cp
        t[2] = 0.0
        return R, t
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, cq - R @ cp


def icp64(from_xyz, to_xyz, guess=None, max_iterations=30, force_3dof=False, max_correspondence_distance=0.1, epsilon=0.0):
    """float64 point-to-point ICP: scipy's kd-tree where scipy is installed, brute force otherwise -> (out_transform as 3 x 4, iterations)"""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    P0 = np.asarray(from_xyz, np.float64).reshape(-1, 3)
    G = np.vstack([np.asarray(IDENTITY if guess is None else guess, np.float64).reshape(3, 4), [0, 0, 0, 1]])
    Q = np.asarray(to_xyz, np.float64).reshape(-1, 3) @ G[:3, :3].T + G[:3, 3]
    tree = cKDTree(Q) if cKDTree else None
    Fm, P, prev, it = np.eye(4), P0.copy(), np.finfo(np.float32).max, 0
    while True:
        if tree is not None:
            d, j = tree.query(P)
        else:
            dd = ((P[:, None, :] - Q[None, :, :]) ** 2).sum(axis=2)
            j = dd.argmin(axis=1)
            d = np.sqrt(dd[np.arange(len(P)), j])
        has = d <= max_correspondence_distance
        if has.sum() < 3:
            return None, it
        mse = (d[has] ** 2).mean()
        R, t = _kabsch(P[has], Q[j[has]], force_3dof)
        P = P @ R.T + t
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        Fm = T @ Fm
        it += 1
        if it >= max_iterations or (0.5 * (np.trace(R) - 1) >= 1 - epsilon ** 2 and t @ t <= epsilon ** 2) or abs(mse - prev) < 1e-12:
            break
        prev = mse
    return (np.linalg.inv(Fm) @ G)[:3], it
