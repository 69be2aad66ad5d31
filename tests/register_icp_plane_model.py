"""The rule of lcd_register_icp_plane (include/lcd.h) in NumPy, brute-force search, operation for operation: np.float32 where the rule is
fp32 (every NumPy operation rounds once, nothing is fused), np.float64 where it says fp64.  Vectorised over rows, which changes no rounding.
Also icp_plane64, an independent point-to-plane ICP (scipy's kd-tree, numpy.linalg.solve, PCL's Rz Ry Rx, uncentred sums) that runs in
float64 and in float32; the rule is measured against it and it is not part of the rule."""
import numpy as np

from motion_3d_model import F, D, Refused, bits, invert, _rotate
from motion_pnp_model import compose, gn_solve, IDENTITY
from register_icp_model import (OK, EMPTY, NOT_CONVERGED, BELOW_RATIO, STOP_NONE, STOP_ITERATIONS, STOP_TRANSFORM, STOP_MSE,  # noqa: F401
                                STOP_FEW_CORRESPONDENCES, SEARCH_AUTO, SEARCH_BRUTE, SEARCH_GRID, VARIANCE_FACTOR, FLT_MAX, apply, nearest, row_sum,
                                fit, stop_of, check_args)

LOW_COMPLEXITY = 4
STOP_SINGULAR = 5
SWEEPS = 5
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def rotate(T, N):
    """R n for the rows of N [n x 3]"""
    T = np.asarray(T, np.float32)
    with np.errstate(all="ignore"):
        cols = [(T[4 * r] * N[:, 0] + T[4 * r + 1] * N[:, 1]) + T[4 * r + 2] * N[:, 2] for r in range(3)]
    return np.stack(cols, axis=1).astype(np.float32).reshape(-1, 3)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pca(N, fin, sweeps=SWEEPS):
    """step 2 over the rotated normals N [n x 3] and the rows whose given normal is finite -> dict(complexity, values [3], vectors [9], has)"""
    oi = int(fin.sum())
    out = dict(complexity=F(0), values=np.zeros(3, np.float32), vectors=np.zeros(9, np.float32), has=False, oi=oi)
    if oi <= 1:
        return out
    with np.errstate(all="ignore"):
        rows, zeros = F(2 * oi), F(oi)
        mean = row_sum(N, fin) / rows
        d = (N - mean).astype(np.float32)
        cov = {}
        for a, b in PAIRS:
            C = row_sum(d[:, a] * d[:, b], fin)
            cov[(a, b)] = (C + zeros * (mean[a] * mean[b])) / rows
        A = [[F(0) for _ in range(4)] for _ in range(4)]
        V = [[F(1) if r == c else F(0) for c in range(4)] for r in range(4)]
        for (a, b), v in cov.items():
            A[a][b] = A[b][a] = F(v)
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                _rotate(A, V, p, q)
        vals = [F(A[k][k]) for k in range(3)]
        vecs = [[F(V[r][k]) for r in range(3)] for k in range(3)]
        for i, j in ((0, 1), (1, 2), (0, 1)):
            if vals[j] > vals[i]:
                vals[i], vals[j] = vals[j], vals[i]
                vecs[i], vecs[j] = vecs[j], vecs[i]
        out.update(complexity=F(vals[2] * F(3)), values=np.array(vals, np.float32), vectors=np.array(vecs, np.float32).reshape(9), has=True)
    return out


def quat_rot(q0, q1, q2, q3):
    n = np.sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
    w, x, y, z = q0 / n, q1 / n, q2 / n, q3 / n
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return [[F(1) - F(2) * (yy + zz), F(2) * (xy - wz), F(2) * (xz + wy)],
            [F(2) * (xy + wz), F(1) - F(2) * (xx + zz), F(2) * (yz - wx)],
            [F(2) * (xz - wy), F(2) * (yz + wx), F(1) - F(2) * (xx + yy)]]


def plane_terms(P, Q, N):
    """the 27 products of every row: P the current cloud, Q each row's correspondent, N its rotated normal -> [n x 27]"""
    with np.errstate(all="ignore"):
        s, d = P, Q
        a = [s[:, 1] * N[:, 2] - s[:, 2] * N[:, 1], s[:, 2] * N[:, 0] - s[:, 0] * N[:, 2], s[:, 0] * N[:, 1] - s[:, 1] * N[:, 0], N[:, 0], N[:, 1], N[:, 2]]
        b = dot3(N, d) - dot3(N, s)
        cols = [a[i] * a[j] for i in range(6) for j in range(i, 6)] + [a[i] * b for i in range(6)]
    return np.stack(cols, axis=1).astype(np.float32)


def plane_fit(S):
    """-> T [12] or None (singular)"""
    x = gn_solve(S)
    if x is None:
        return None
    with np.errstate(all="ignore"):
        a, b, c = F(0.5) * x[0], F(0.5) * x[1], F(0.5) * x[2]
        ab, ac, bc = a * b, a * c, b * c
        R = quat_rot(F(1) + ab * c, a - bc, b + ac, c - ab)
        T = np.zeros(12, np.float32)
        for r in range(3):
            T[4 * r:4 * r + 3] = R[r]
            T[4 * r + 3] = x[3 + r]
    return T


def fit_plane(P, Q, N, has):
    return plane_fit(row_sum(plane_terms(P, Q, N), has))


def to_3dof(Fm):
    with np.errstate(all="ignore"):
        n = np.sqrt(Fm[0] * Fm[0] + Fm[4] * Fm[4])
        c, s = (Fm[0] / n, Fm[4] / n) if n != F(0) and np.isfinite(n) else (F(1), F(0))
    return np.array([c, -s, 0, Fm[3], s, c, 0, Fm[7], 0, 0, 1, 0], np.float32)


def unit(V):
    with np.errstate(all="ignore"):
        s = dot3(V, V)
        r = np.sqrt(s)
        return np.where((s == F(0))[:, None], V, V / r[:, None]).astype(np.float32)


def gate_dots(V1, V2):
    """the cosines of step 5's gate for the rows of V1 and V2, float32"""
    with np.errstate(all="ignore"):
        return dot3(unit(V1), unit(V2)).astype(np.float32)


def limit_translation(Fm, guess, vectors, has_vectors, second_too):
    with np.errstate(all="ignore"):
        Ginv = invert(guess)
        C = compose(Ginv, compose(invert(Fm), guess))
        v = C[[3, 7, 11]]
        vp = np.zeros(3, np.float32)
        if has_vectors:
            n1, n2 = vectors[:3], vectors[3:6]
            a, b = dot3(v, n1), dot3(v, n2)
            vp = (n1 * a + n2 * b if second_too else n1 * a).astype(np.float32)
        C = C.copy()
        C[[3, 7, 11]] = vp
        return compose(compose(guess, invert(C)), Ginv)


def check_plane_args(min_complexity, low_complexity_strategy, normal_gate, min_normal_cos):
    if not 0 <= min_complexity <= 1 or low_complexity_strategy not in (0, 1, 2) or (normal_gate and not np.isfinite(min_normal_cos)):
        raise Refused("invalid")


def register(from_xyz, from_normals, to_xyz, to_normals, guess=None, max_iterations=30, force_3dof=False, max_laser_scans=0, search=SEARCH_AUTO,
             max_correspondence_distance=0.1, epsilon=0.0, correspondence_ratio=0.1, min_complexity=0.02, low_complexity_strategy=1, normal_gate=False,
             min_normal_cos=0.0, device_entry=False, sweeps=SWEEPS, source_is_to=None):
    """one pair -> dict of the call's outputs (transform, icp_transform, correction, status, stop, iterations, n_correspondences, ratio, variance,
    match, branch, complexity, complexity_values, complexity_vectors, second_eigenvalue) and, for the tests: pca_from, pca_to, counts,
    from_is_target (step 5's decision, None where step 5 is not reached), reciprocal_d2 (the reciprocal correspondences' d2 in source-row
    order), reciprocal_rows (their source rows), reciprocal_pass, reciprocal_dots.  source_is_to is no part of the rule: a bool forces step 5's
    source side, so that a test can show what the other decision would have given"""
    P0 = np.ascontiguousarray(from_xyz, np.float32).reshape(-1, 3)
    T0 = np.ascontiguousarray(to_xyz, np.float32).reshape(-1, 3)
    N0 = np.ascontiguousarray(from_normals, np.float32).reshape(-1, 3)
    NT = np.ascontiguousarray(to_normals, np.float32).reshape(-1, 3)
    guess = np.asarray(IDENTITY if guess is None else guess, np.float32).reshape(12)
    epsilon, ratio_min, min_complexity = F(epsilon), F(correspondence_ratio), F(min_complexity)
    check_args(P0, T0, guess, max_iterations, max_laser_scans, search, max_correspondence_distance, epsilon, ratio_min, device_entry)
    check_plane_args(min_complexity, low_complexity_strategy, normal_gate, min_normal_cos)
    thr2 = D(max_correspondence_distance) * D(max_correspondence_distance)
    zeros = np.zeros(12, np.float32)
    r = dict(transform=zeros.copy(), icp_transform=zeros.copy(), correction=zeros.copy(), status=OK, stop=STOP_NONE, iterations=0, n_correspondences=0,
             ratio=F(0), variance=D(1.0), match=np.full(P0.shape[0], -1, np.int32), branch=0, second_eigenvalue=F(1), counts=[],
             reciprocal_d2=np.zeros(0, np.float32), reciprocal_pass=np.zeros(0, bool), reciprocal_dots=np.zeros(0, np.float32),
             reciprocal_rows=np.zeros(0, np.int64), from_is_target=None)
    fin_f, fin_t = np.isfinite(N0).all(axis=1), np.isfinite(NT).all(axis=1)
    NQ = rotate(guess, NT)
    pf, pt = pca(N0, fin_f, sweeps), pca(NQ, fin_t, sweeps)
    r["pca_from"], r["pca_to"] = pf, pt
    less = pf if pf["complexity"] < pt["complexity"] else pt
    r["complexity"], r["complexity_values"], r["complexity_vectors"] = less["complexity"], less["values"], less["vectors"]
    has_vectors = False
    if r["complexity"] < min_complexity:
        if r["complexity"] > F(0):
            has_vectors = True
            r["second_eigenvalue"] = pf["values"][1] if pf["values"][1] < pt["values"][1] else pt["values"][1]
        if low_complexity_strategy == 0:
            r["status"] = LOW_COMPLEXITY
            return r
        r["branch"] = 1
    rows_f, rows_t = np.isfinite(P0).all(axis=1), np.isfinite(T0).all(axis=1)
    part_f, part_t = (rows_f & fin_f, rows_t & fin_t) if r["branch"] == 0 else (rows_f, rows_t)
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
        j = np.maximum(row, 0)
        T = fit(P, Q[j], has, c, force_3dof) if r["branch"] == 1 else fit_plane(P, Q[j], NQ[j], has)
        if T is None:
            r["status"], r["stop"] = NOT_CONVERGED, STOP_SINGULAR
            return r
        P = np.where(part_f[:, None], apply(T, P), P).astype(np.float32)
        Fm = compose(T, Fm)
        r["iterations"] += 1
        stop = stop_of(T, r["iterations"], max_iterations, eps2, mse, mse_prev)
        if stop != STOP_NONE:
            break
        mse_prev = mse
    r["stop"] = stop
    if r["branch"] == 1 and low_complexity_strategy == 1:
        Fm = limit_translation(Fm, guess, r["complexity_vectors"], has_vectors, bool(r["second_eigenvalue"] >= min_complexity))
    A = np.where(part_f[:, None], apply(Fm, P0), P0).astype(np.float32)
    NA = rotate(Fm, N0)
    if r["branch"] == 0 and force_3dof:
        Fm = to_3dof(Fm)
    row_a, d2_a = nearest(A, part_f, Q, part_t)
    row_q, d2_q = nearest(Q, part_t, A, part_f)
    from_is_target = nf > nt if source_is_to is None else bool(source_is_to)
    r["from_is_target"] = from_is_target
    if from_is_target:
        src_row, src_d2, tgt_row, n_src, n_tgt = row_q, d2_q, row_a, NQ, NA
    else:
        src_row, src_d2, tgt_row, n_src, n_tgt = row_a, d2_a, row_q, NA, NQ
    idx = np.arange(src_row.shape[0])
    keep = (src_row >= 0) & (src_d2.astype(np.float64) <= thr2)
    keep &= tgt_row[np.maximum(src_row, 0)] == idx
    kept = idx[keep]                                                   # ascending source rows
    r["reciprocal_rows"] = kept
    if r["branch"] == 0:
        dots = gate_dots(n_tgt[src_row[kept]], n_src[kept])
        ok = dots.astype(np.float64) > D(min_normal_cos) if normal_gate else np.ones(kept.shape[0], bool)
        r["reciprocal_d2"], r["reciprocal_pass"], r["reciprocal_dots"] = src_d2[kept], ok, dots
        n = int(ok.sum())
        if n >= 1:
            s = np.sort(bits(src_d2[kept][:n]))
            r["variance"] = VARIANCE_FACTOR * D(s[n >> 1:][:1].view(np.float32)[0])
        listed = kept[ok]
    else:
        n = kept.shape[0]
        if n >= 3:
            s = np.sort(bits(src_d2[kept]))
            r["variance"] = VARIANCE_FACTOR * D(s[n >> 1:][:1].view(np.float32)[0])
        listed = kept
    if from_is_target:
        r["match"][src_row[listed]] = listed
    else:
        r["match"][listed] = src_row[listed]
    r["n_correspondences"] = n
    r["ratio"] = F(n) / F(max_laser_scans if max_laser_scans > 0 else max(int(rows_f.sum()), int(rows_t.sum())))
    X = compose(invert(Fm), guess)
    r["icp_transform"] = Fm
    r["correction"] = compose(invert(guess), X)
    if r["ratio"] <= ratio_min:
        r["status"] = BELOW_RATIO
        return r
    r["transform"] = X
    return r


# ---- what the rule is measured against: point-to-plane ICP as PCL writes it, in float64 or float32, written independently

def icp_plane64(from_xyz, to_xyz, to_normals, guess=None, max_iterations=30, max_correspondence_distance=0.1, epsilon=0.0, dtype=np.float64):
    """-> (out_transform as 3 x 4 in dtype, iterations), None when it cannot go on.  The search is scipy's kd-tree over the dtype's points."""
    from scipy.spatial import cKDTree
    dt = np.dtype(dtype).type
    G = np.vstack([np.asarray(IDENTITY if guess is None else guess, dt).reshape(3, 4), [0, 0, 0, 1]]).astype(dt)
    P = np.asarray(from_xyz, dt).reshape(-1, 3)
    Q = (np.asarray(to_xyz, dt).reshape(-1, 3) @ G[:3, :3].T + G[:3, 3]).astype(dt)
    N = (np.asarray(to_normals, dt).reshape(-1, 3) @ G[:3, :3].T).astype(dt)
    tree = cKDTree(Q)
    Fm, prev, it = np.eye(4, dtype=dt), dt(np.finfo(np.float32).max), 0
    while True:
        d, j = tree.query(P)
        has = d <= max_correspondence_distance
        if has.sum() < 6:
            return None, it
        s, q, n = P[has], Q[j[has]], N[j[has]]
        mse = dt(((s - q) ** 2).sum(axis=1).mean())
        A = np.hstack([np.cross(s, n), n]).astype(dt)
        b = ((n * q).sum(axis=1) - (n * s).sum(axis=1)).astype(dt)
        x = np.linalg.solve((A.T @ A).astype(dt), (A.T @ b).astype(dt)).astype(dt)
        ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
        T = np.eye(4, dtype=dt)
        T[:3, :3] = [[cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca], [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca], [-sb, cb * sa, cb * ca]]
        T[:3, 3] = x[3:]
        P = (P @ T[:3, :3].T + T[:3, 3]).astype(dt)
        Fm = (T @ Fm).astype(dt)
        it += 1
        t = T[:3, 3]
        if it >= max_iterations or (0.5 * (np.trace(T[:3, :3]) - 1) >= 1 - epsilon ** 2 and t @ t <= epsilon ** 2) or abs(mse - prev) < 1e-12:
            break
        prev = mse
    Finv = np.eye(4, dtype=dt)
    Finv[:3, :3], Finv[:3, 3] = Fm[:3, :3].T, -Fm[:3, :3].T @ Fm[:3, 3]
    return (Finv @ G)[:3].astype(dt), it
