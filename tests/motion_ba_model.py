"""The rule of lcd_refine_motion_ba (include/lcd.h) in NumPy, operation for operation: np.float32 arrays and scalars where the rule is fp32 (every
NumPy operation rounds once, nothing is fused), np.float64 where it says fp64.  Vectorised over the points, which changes no rounding: every
element sees the same operations in the same order.  The quaternion, the pose update, the 6 x 6 LDL^T and the frames are those of
lcd_estimate_motion_pnp's model, the 256-lane sum that of lcd_estimate_motion_3d's.

ba64 at the end is the accuracy yardstick: the same objective, stages and outlier rule with different linear algebra."""
import numpy as np

from motion_3d_model import F, D, LANES, MAX_ROWS, lane_sum, invert
from motion_pnp_model import IDENTITY, compose, quat_of_model, model_of_pose, gn_solve, pose_update, pose_of_model

SUMS, STAGE1, TRIALS = 27, 5, 10
OK, NO_INPUT, BAD_INLIER, DIVERGED, BELOW_MIN_INLIERS, MEAN_DISTANCE_REJECTED, DISTRIBUTION_REJECTED = range(7)
LINEAR_EPSILON, ANGULAR_EPSILON = D(0.00000001), D(0.00000003)
CHI2_LIMIT, GAIN_EPSILON, THIRD = D(1000000000000.0), D(1e-3), D(1.0) / D(3.0)
LAMBDA_SCALE = F(1e-5)
F_FROM, F_FROM_STEREO, F_TO_STEREO, F_FROM_OUT, F_TO_OUT, F_OUTLIER, F_TO_FINITE = 1, 2, 4, 8, 16, 32, 64
DIAG6 = (0, 6, 11, 15, 18, 20)
DEFAULT_CAMERA = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5)


def lane_sum64(E):
    """SUM64: lane_sum's order in fp64"""
    E = np.asarray(E, np.float64)
    n = E.shape[0]
    rows = max((n + LANES - 1) // LANES, 1)
    pad = np.zeros((rows * LANES,) + E.shape[1:], np.float64)
    pad[:n] = E
    part = np.zeros((LANES,) + E.shape[1:], np.float64)
    for r in range(rows):
        part = part + pad[r * LANES:(r + 1) * LANES]
    s = LANES // 2
    while s >= 1:
        part = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


class View:
    def __init__(self, cam, baseline):
        self.fx, self.fy, self.cx, self.cy = F(cam["fx"]), F(cam["fy"]), F(cam["cx"]), F(cam["cy"])
        self.baseline = D(baseline)
        self.b = F(self.baseline)
        self.width, self.height = int(cam.get("image_width", 0)), int(cam.get("image_height", 0))
        loc = cam.get("local_transform")
        self.local = None if loc is None else np.asarray(loc, np.float32).reshape(12)
        self.inv_local = invert(self.local if self.local is not None else IDENTITY)


class Frame:
    pass


def prior_information(variance, floor):
    v = floor if D(variance) <= floor else D(variance)
    return F(D(1.0) / v)


def apply_z(m, P):
    with np.errstate(all="ignore"):
        return ((m[8] * P[:, 0] + m[9] * P[:, 1]) + m[10] * P[:, 2]) + m[11]


def observe(view, points, UV):
    """-> (obs [n x 3], depth [n], stereo [n]); points None: no depth"""
    n = UV.shape[0]
    depth = np.zeros(n, np.float32) if points is None else apply_z(view.inv_local, points).astype(np.float32)
    with np.errstate(all="ignore"):
        stereo = np.isfinite(depth) & (depth > F(0)) & bool(view.baseline > 0)
        disparity = ((view.baseline * D(view.fx)) / depth.astype(np.float64)).astype(np.float32)
        third = np.where(stereo, UV[:, 0] - disparity, F(0)).astype(np.float32)
    return np.stack([UV[:, 0], UV[:, 1], third], axis=1).astype(np.float32), depth, stereo


def edge(m, k, stereo, P, obs, info):
    """-> (chi2 [n], geometry dict)"""
    with np.errstate(all="ignore"):
        px, py, pz = P[:, 0], P[:, 1], P[:, 2]
        Mx = (m[0] * px + m[1] * py) + m[2] * pz
        My = (m[4] * px + m[5] * py) + m[6] * pz
        Mz = (m[8] * px + m[9] * py) + m[10] * pz
        X, Y, Z = Mx + m[3], My + m[7], Mz + m[11]
        iz = F(1) / Z
        x, y = X * iz, Y * iz
        a, c = k.fx * iz, k.fy * iz
        ax, cy = a * x, c * y
        r0 = obs[:, 0] - (k.fx * x + k.cx)
        r1 = obs[:, 1] - (k.fy * y + k.cy)
        s = r0 * r0 + r1 * r1
        xb = (X - k.b) * iz
        r2 = np.where(stereo, obs[:, 2] - (k.fx * xb + k.cx), F(0)).astype(np.float32)
        axb = np.where(stereo, a * xb, F(0)).astype(np.float32)
        s = np.where(stereo, s + r2 * r2, s).astype(np.float32)
        chi2 = info * s
    return chi2, dict(Mx=Mx, My=My, Mz=Mz, a=a, c=c, ax=ax, cy=cy, axb=axb, r=[r0, r1, r2])


def huber_weight(chi2, f):
    with np.errstate(all="ignore"):
        plain = (not f.delta > 0) | (chi2 <= f.delta2)
        return np.where(plain, F(1), f.delta / np.sqrt(chi2)).astype(np.float32)


def huber_cost(chi2, f):
    with np.errstate(all="ignore"):
        plain = (not f.delta > 0) | (chi2 <= f.delta2)
        return np.where(plain, chi2, f.two_delta * np.sqrt(chi2) - f.delta2).astype(np.float32)


def from_active(flags):
    return (flags & (F_FROM | F_FROM_OUT)) == F_FROM


def to_active(flags):
    return (flags & F_TO_OUT) == 0


def point_cost(f, m2, st):
    """-> (cost [n] fp64, chi_from, chi_to)"""
    fa, ta = from_active(st.flags), to_active(st.flags)
    cost = np.zeros(st.n, np.float64)
    chi_f, _ = edge(f.M1, f.v1, (st.flags & F_FROM_STEREO) != 0, st.P, st.OF, f.info)
    chi_t, _ = edge(m2, f.v2, (st.flags & F_TO_STEREO) != 0, st.P, st.OT, f.info)
    with np.errstate(all="ignore"):
        cost = np.where(fa, cost + huber_cost(chi_f, f).astype(np.float64), cost)
        cost = np.where(ta, cost + huber_cost(chi_t, f).astype(np.float64), cost)
    return cost, np.where(fa, chi_f, F(0)).astype(np.float32), np.where(ta, chi_t, F(0)).astype(np.float32)


class Blocks:
    def __init__(self, n):
        self.Hpp, self.bp, self.Hcp = np.zeros((n, 6), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 18), np.float32)
        self.Hcc, self.bc = np.zeros((n, 21), np.float32), np.zeros((n, 6), np.float32)


def rows_dot(A, B, stereo):
    with np.errstate(all="ignore"):
        s = A[0] * B[0] + A[1] * B[1]
        return np.where(stereo, s + A[2] * B[2], s).astype(np.float32)


def edge_blocks(m, g, stereo, W, moving, B, active):
    def add(col, s):
        with np.errstate(all="ignore"):
            col[:] = np.where(active, col + W * s, col)
    with np.errstate(all="ignore"):
        Jp = [[g["a"] * m[j] - g["ax"] * m[8 + j], g["c"] * m[4 + j] - g["cy"] * m[8 + j], g["a"] * m[j] - g["axb"] * m[8 + j]] for j in range(3)]
        o = 0
        for i in range(3):
            for j in range(i, 3):
                add(B.Hpp[:, o], rows_dot(Jp[i], Jp[j], stereo))
                o += 1
        for i in range(3):
            add(B.bp[:, i], rows_dot(Jp[i], g["r"], stereo))
        if not moving:
            return
        a, c, ax, cy, axb, Mx, My, Mz = g["a"], g["c"], g["ax"], g["cy"], g["axb"], g["Mx"], g["My"], g["Mz"]
        zero = np.zeros_like(a)
        aMz = a * Mz
        Jc = [[-(ax * My), -(c * Mz + cy * My), -(axb * My)], [aMz + ax * Mx, cy * Mx, aMz + axb * Mx], [-(a * My), c * Mx, -(a * My)],
              [a, zero, a], [zero, c, zero], [-ax, -cy, -axb]]
        for i in range(6):
            for j in range(3):
                add(B.Hcp[:, 3 * i + j], rows_dot(Jc[i], Jp[j], stereo))
        o = 0
        for i in range(6):
            for j in range(i, 6):
                add(B.Hcc[:, o], rows_dot(Jc[i], Jc[j], stereo))
                o += 1
        for i in range(6):
            add(B.bc[:, i], rows_dot(Jc[i], g["r"], stereo))


def point_blocks(f, m2, st):
    """-> (Blocks, active [n])"""
    B = Blocks(st.n)
    fa, ta = from_active(st.flags), to_active(st.flags)
    for act, m, k, bit, obs, moving in ((fa, f.M1, f.v1, F_FROM_STEREO, st.OF, False), (ta, m2, f.v2, F_TO_STEREO, st.OT, True)):
        stereo = (st.flags & bit) != 0
        chi2, g = edge(m, k, stereo, st.P, obs, f.info)
        with np.errstate(all="ignore"):
            W = f.info * huber_weight(chi2, f)
        edge_blocks(m, g, stereo, W, moving, B, act)
    return B, fa | ta


def sym3(i, j):
    return j if i == 0 else i if j == 0 else i + j + 1


def inv3(H, lam):
    with np.errstate(all="ignore"):
        a, b, c, d, e, f = H[:, 0] + lam, H[:, 1], H[:, 2], H[:, 3] + lam, H[:, 4], H[:, 5] + lam
        c00, c01, c02, c11, c12, c22 = d * f - e * e, c * e - b * f, b * e - c * d, a * f - c * c, b * c - a * e, a * d - b * b
        det = (a * c00 + b * c01) + c * c02
        return [c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det]


def point_terms(B, lam, active):
    """-> [n x 27]; zeros where the point is not active"""
    inv = inv3(B.Hpp, lam)
    n = B.Hpp.shape[0]
    out = np.zeros((n, SUMS), np.float32)
    with np.errstate(all="ignore"):
        Y = [[(B.Hcp[:, 3 * i] * inv[sym3(0, a)] + B.Hcp[:, 3 * i + 1] * inv[sym3(1, a)]) + B.Hcp[:, 3 * i + 2] * inv[sym3(2, a)] for a in range(3)]
             for i in range(6)]
        o = 0
        for i in range(6):
            for j in range(i, 6):
                out[:, o] = B.Hcc[:, o] - ((Y[i][0] * B.Hcp[:, 3 * j] + Y[i][1] * B.Hcp[:, 3 * j + 1]) + Y[i][2] * B.Hcp[:, 3 * j + 2])
                o += 1
        for i in range(6):
            out[:, 21 + i] = B.bc[:, i] - ((Y[i][0] * B.bp[:, 0] + Y[i][1] * B.bp[:, 1]) + Y[i][2] * B.bp[:, 2])
    out[~active] = F(0)
    return out


def point_step(B, lam, dc):
    """-> (dp [n x 3], scale [n] fp64)"""
    inv = inv3(B.Hpp, lam)
    n = B.Hpp.shape[0]
    with np.errstate(all="ignore"):
        v = []
        for a in range(3):
            s = B.Hcp[:, a] * dc[0]
            for i in range(1, 6):
                s = s + B.Hcp[:, 3 * i + a] * dc[i]
            v.append(B.bp[:, a] - s)
        dp = np.stack([(inv[sym3(a, 0)] * v[0] + inv[sym3(a, 1)] * v[1]) + inv[sym3(a, 2)] * v[2] for a in range(3)], axis=1).astype(np.float32)
        scale = np.zeros(n, np.float64)
        for a in range(3):
            d = dp[:, a].astype(np.float64)
            scale = scale + d * (D(lam) * d + B.bp[:, a].astype(np.float64))
        for i in range(6):
            scale = scale + D(dc[i]) * B.bc[:, i].astype(np.float64)
    return dp, scale


def prior_error(model, C0):
    """-> (e [6], q [4] of E normalised with w >= 0, R t0 [3])"""
    with np.errstate(all="ignore"):
        E = compose(model, C0)
        q = quat_of_model(E)
        n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        sn = -n if q[0] < 0 else n
        q = (q / sn).astype(np.float32)
        e = np.array([E[3], E[7], E[11], F(2) * q[1], F(2) * q[2], F(2) * q[3]], np.float32)
        rt = np.array([(model[4 * r] * C0[3] + model[4 * r + 1] * C0[7]) + model[4 * r + 2] * C0[11] for r in range(3)], np.float32)
    return e, q, rt


def prior_cost(f, e):
    with np.errstate(all="ignore"):
        st = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        sr = (e[3] * e[3] + e[4] * e[4]) + e[5] * e[5]
        return D(f.inf_lin * st + f.inf_ang * sr)


def prior_system(f, model, C0):
    """-> P [27]"""
    e, q, rt = prior_error(model, C0)
    z, one = F(0), F(1)
    J = [[z, rt[2], -rt[1], one, z, z], [-rt[2], z, rt[0], z, one, z], [rt[1], -rt[0], z, z, z, one],
         [q[0], q[3], -q[2], z, z, z], [-q[3], q[0], q[1], z, z, z], [q[2], -q[1], q[0], z, z, z]]
    inf = [f.inf_lin] * 3 + [f.inf_ang] * 3
    P = np.zeros(SUMS, np.float32)
    with np.errstate(all="ignore"):
        o = 0
        for i in range(6):
            for j in range(i, 6):
                acc = F(0)
                for k in range(6):
                    acc = acc + inf[k] * (J[k][i] * J[k][j])
                P[o] = acc
                o += 1
        for i in range(6):
            acc = F(0)
            for k in range(6):
                acc = acc - inf[k] * (J[k][i] * e[k])
            P[21 + i] = acc
    return P


def camera_step(sums, P, lam, q, t):
    """-> (q, t, dc, scale0) or None"""
    with np.errstate(all="ignore"):
        S = (sums + P).astype(np.float32)
        for o in DIAG6:
            S[o] = S[o] + lam
        dc = gn_solve(S)
        if dc is None:
            return None
        q2, t2 = pose_update(q, t, dc)
        scale = D(0)
        for i in range(6):
            scale = scale + D(dc[i]) * (D(lam) * D(dc[i]) + D(P[21 + i]))
    return q2, t2, dc, scale


def small_eigenvalue(a, b, c):
    with np.errstate(all="ignore"):
        half, d = F(0.5) * (a + c), F(0.5) * (a - c)
        return half - np.sqrt(d * d + b * b)


def normalised(u, c, size):
    with np.errstate(all="ignore"):
        return ((u.astype(np.float64) - D(c)) / D(size)).astype(np.float32)


class State:
    pass


def unique_rows(ids):
    rows, seen = {}, {}
    for r, i in enumerate(ids.tolist()):
        seen[i] = seen.get(i, 0) + 1
        rows[i] = r
    return {i: r for i, r in rows.items() if seen[i] == 1}


def check_args(n_from, n_to, camera_from, camera_to, baselines, prior_variance, min_inliers, iterations, pixel_variance, robust_delta,
               max_inliers_mean_distance, min_inliers_distribution):
    """False: what the call refuses"""
    with np.errstate(all="ignore"):
        info, delta = F(D(1.0) / D(pixel_variance)) if pixel_variance != 0 else F(np.inf), F(robust_delta)
        ok = n_from <= MAX_ROWS and n_to <= MAX_ROWS and 0 <= iterations <= 65535 and min_inliers >= 0
        ok = ok and np.isfinite(pixel_variance) and pixel_variance > 0 and np.isfinite(info) and info > 0
        ok = ok and np.isfinite(robust_delta) and robust_delta >= 0 and np.isfinite(delta * delta)
        ok = ok and all(np.isfinite(v) and v >= 0 for v in (max_inliers_mean_distance, min_inliers_distribution))
        ok = ok and all(np.isfinite(b) for b in baselines)
        ok = ok and all(np.isfinite(F(c[k])) and F(c[k]) != 0 for c in (camera_from, camera_to) for k in ("fx", "fy"))
        ok = ok and (prior_variance is None or all(np.isfinite(v) and v >= 0 for v in prior_variance))
    return bool(ok)


def refine(from_ids, from_xyz, to_ids, to_points, inliers, transform, from_points=None, to_xyz=None, prior_variance=None, camera_from=DEFAULT_CAMERA,
           camera_to=DEFAULT_CAMERA, baselines=(0.075, 0.075), n_inliers=None, min_inliers=20, iterations=20, pixel_variance=1.0, robust_delta=8.0,
           max_inliers_mean_distance=0.0, min_inliers_distribution=0.0, trace=None):
    """-> the dict of vwdictionary.motion_ba_cpu, or None where the call is refused.  trace (a list, if given) receives what happened:
    ("trial", stage, iteration, trial, "accepted" | "rejected" | "unsolved"), ("stage_end", stage, iterations run, F),
    ("chi2", stage, from chi2 [n], to chi2 [n]) and ("flagged", stage, [(point, "from" | "to")]) behind a stage, then ("state", stage, flags [n], points [n x 3], initial points [n x 3]), ("edges", from stereo flags, to stereo flags, from present)"""
    from_ids, to_ids = np.asarray(from_ids, np.int32).reshape(-1), np.asarray(to_ids, np.int32).reshape(-1)
    from_xyz, to_points = np.asarray(from_xyz, np.float32).reshape(-1, 3), np.asarray(to_points, np.float32).reshape(-1, 2)
    if not check_args(from_ids.shape[0], to_ids.shape[0], camera_from, camera_to, baselines, prior_variance, min_inliers, iterations, pixel_variance,
                      robust_delta, max_inliers_mean_distance, min_inliers_distribution):
        return None
    fp = None if from_points is None else np.asarray(from_points, np.float32).reshape(-1, 2)
    tx = None if to_xyz is None else np.asarray(to_xyz, np.float32).reshape(-1, 3)
    inliers = np.asarray(inliers, np.int32).reshape(-1)
    T0 = np.asarray(transform, np.float32).reshape(12)
    n_to = to_ids.shape[0]
    n = inliers.shape[0] if n_inliers is None else int(n_inliers)
    inliers = np.concatenate([inliers, np.zeros(max(n_to - inliers.shape[0], 0), np.int32)])      # the pair's to-region: zeros behind the ids
    n_c = min(max(n, 0), n_to)
    out = dict(transform=np.zeros(12, np.float32), status=OK, n_outliers=0, lm_accepted=0, chi2_before=D(0), chi2_after=D(0),
               inliers_mean_distance=F(0), inliers_distribution=F(0), inliers=inliers[:n_c].copy())

    def passed(status):
        out["status"] = status
        return out
    if not T0.any() or n == 0:
        return passed(NO_INPUT)
    if n < 0 or n > n_to:
        return passed(BAD_INLIER)
    rows_f, rows_t = unique_rows(from_ids), unique_rows(to_ids)
    ids = inliers[:n].tolist()
    if any(i not in rows_f or i not in rows_t for i in ids):
        return passed(BAD_INLIER)
    rf, rt = np.array([rows_f[i] for i in ids], np.int64), np.array([rows_t[i] for i in ids], np.int64)
    P0 = from_xyz[rf]
    if not np.isfinite(P0).all():
        return passed(BAD_INLIER)

    f = Frame()
    f.v1, f.v2 = View(camera_from, baselines[0]), View(camera_to, baselines[1])
    f.M1 = f.v1.inv_local
    f.info, f.delta = F(D(1.0) / D(pixel_variance)), F(robust_delta)
    f.delta2, f.two_delta = f.delta * f.delta, F(2) * f.delta
    f.inf_lin = F(1) if prior_variance is None else prior_information(prior_variance[0], LINEAR_EPSILON)
    f.inf_ang = F(1) if prior_variance is None else prior_information(prior_variance[1], ANGULAR_EPSILON)

    st = State()
    st.n, st.P0, st.P = n, P0.copy(), P0.copy()
    st.flags = np.zeros(n, np.uint32)
    st.OF = np.zeros((n, 3), np.float32)
    if fp is not None:
        st.OF, _, stereo = observe(f.v1, P0, fp[rf])
        st.flags |= np.uint32(F_FROM) | np.where(stereo, np.uint32(F_FROM_STEREO), np.uint32(0))
    st.OT, depth_to, stereo = observe(f.v2, None if tx is None else tx[rt], to_points[rt])
    st.flags |= np.where(stereo, np.uint32(F_TO_STEREO), np.uint32(0))
    if tx is not None:
        st.flags |= np.where(np.isfinite(tx[rt]).all(axis=1), np.uint32(F_TO_FINITE), np.uint32(0))
    if trace is not None:
        trace.append(("edges", (st.flags & F_FROM_STEREO) != 0, (st.flags & F_TO_STEREO) != 0, fp is not None))

    C0 = compose(T0, f.v2.local) if f.v2.local is not None else T0.copy()
    m0 = invert(C0)
    q = quat_of_model(m0)
    t = np.array([m0[3], m0[7], m0[11]], np.float32)
    cur, q = model_of_pose(q, t)

    def cost_under(model):
        c, _, _ = point_cost(f, model, st)
        e, _, _ = prior_error(model, C0)
        return lane_sum64(c) + prior_cost(f, e)

    status = OK
    if iterations > 0:
        stages = 2 if f.delta > 0 else 1
        Fc = cost_under(cur)
        out["chi2_before"] = Fc
        diverged = False
        for s in range(stages):
            iters = STAGE1 if s == 0 and stages == 2 else iterations
            if s > 0:
                Fc = cost_under(cur)
            B, active = point_blocks(f, cur, st)
            P = prior_system(f, cur, C0)
            with np.errstate(all="ignore"):
                top = F(0)
                diag = B.Hpp[active][:, [0, 3, 5]]
                if diag.size:
                    for v in diag.reshape(-1):                         # (a NaN never replaces: v > top is false)
                        top = v if v > top else top
                for o in DIAG6:
                    v = lane_sum(B.Hcc[:, o]) + P[o]
                    top = v if v > top else top
                lam, nu = LAMBDA_SCALE * top, F(2)
            done = 0
            for it in range(iters):
                accepted = False
                for trial in range(TRIALS):
                    B, active = point_blocks(f, cur, st)
                    sums = lane_sum(point_terms(B, lam, active))
                    step = camera_step(sums, prior_system(f, cur, C0), lam, q, t)
                    what = "unsolved"
                    if step is not None:
                        q2, t2, dc, scale0 = step
                        moved, q2 = model_of_pose(q2, t2)
                        dp, sc = point_step(B, lam, dc)
                        saved = st.P.copy()
                        with np.errstate(all="ignore"):
                            st.P = np.where(active[:, None], st.P + dp, st.P).astype(np.float32)
                            scale = lane_sum64(np.where(active, sc, D(0))) + scale0
                            Fn = cost_under(moved)
                            rho = (Fc - Fn) / (scale + GAIN_EPSILON)
                        if rho > 0 and np.isfinite(Fn):
                            cur, q, t, Fc = moved, q2, t2, Fn
                            with np.errstate(all="ignore"):
                                tt = D(2.0) * rho - D(1.0)
                                alpha = D(1.0) - (tt * tt) * tt
                                lam = F(D(lam) * (THIRD if alpha < THIRD else alpha))
                            nu = F(2)
                            accepted = True
                            out["lm_accepted"] += 1
                            what = "accepted"
                        else:
                            st.P = saved
                            what = "rejected"
                    if trace is not None:
                        trace.append(("trial", s, it, trial, what))
                    if accepted:
                        break
                    with np.errstate(all="ignore"):
                        lam = lam * nu
                        nu = nu * F(2)
                if not accepted:
                    break
                done += 1
            out["chi2_after"] = Fc
            if trace is not None:
                trace.append(("stage_end", s, done, Fc))
            if np.isnan(Fc) or (s > 0 and (Fc > CHI2_LIMIT or not np.isfinite(Fc))):
                diverged = True
                break
            if stages == 2:
                _, cf, ct = point_cost(f, cur, st)
                with np.errstate(all="ignore"):
                    out_f = from_active(st.flags) & (cf > f.delta)
                    out_t = to_active(st.flags) & (ct > f.delta)
                hit = out_f | out_t
                st.flags = (st.flags | np.where(out_f, np.uint32(F_FROM_OUT), np.uint32(0)) | np.where(out_t, np.uint32(F_TO_OUT), np.uint32(0)) |
                            np.where(hit, np.uint32(F_OUTLIER), np.uint32(0))).astype(np.uint32)
                st.P = np.where(hit[:, None], st.P0, st.P).astype(np.float32)
                if trace is not None:
                    trace.append(("chi2", s, cf, ct))
                    trace.append(("flagged", s, [(int(i), "from") for i in np.flatnonzero(out_f)] + [(int(i), "to") for i in np.flatnonzero(out_t)]))
                    trace.append(("state", s, st.flags.copy(), st.P.copy(), st.P0.copy()))
        if diverged or Fc > CHI2_LIMIT:
            out["inliers"] = inliers[:n].copy()
            return passed(DIVERGED)
    kept = np.flatnonzero((st.flags & F_OUTLIER) == 0)
    out["inliers"] = inliers[:n][kept].copy()
    out["n_outliers"] = n - kept.shape[0]
    if kept.shape[0] < min_inliers:
        return passed(BELOW_MIN_INLIERS)
    if kept.shape[0] > 0 and max_inliers_mean_distance > 0 and tx is not None:
        d = depth_to[kept][(st.flags[kept] & F_TO_FINITE) != 0]
        if d.shape[0]:
            acc = F(0)
            with np.errstate(all="ignore"):
                for v in d:
                    acc = acc + v
                mean = acc / F(d.shape[0])
            out["inliers_mean_distance"] = mean
            if mean > F(max_inliers_mean_distance):
                return passed(MEAN_DISTANCE_REJECTED)
    v2 = f.v2
    valid = v2.fx > 0 and v2.fy > 0 and v2.cx > 0 and v2.cy > 0 and v2.width > 0 and v2.height > 0
    if kept.shape[0] > 0 and min_inliers_distribution > 0 and valid:
        x, y = normalised(st.OT[kept, 0], v2.cx, v2.width), normalised(st.OT[kept, 1], v2.cy, v2.height)
        nn = F(kept.shape[0])
        with np.errstate(all="ignore"):
            mx, my = lane_sum(x) / nn, lane_sum(y) / nn
            dx, dy = x - mx, y - my
            a, b, c = lane_sum(dx * dx) / nn, lane_sum(dx * dy) / nn, lane_sum(dy * dy) / nn
            out["inliers_distribution"] = F(small_eigenvalue(a, b, c))
        if out["inliers_distribution"] < F(min_inliers_distribution):
            return passed(DISTRIBUTION_REJECTED)
    out["transform"] = pose_of_model(cur, f.v2.local) if iterations > 0 else T0.copy()
    return out


# ---- the yardstick

HALVINGS = 12

def _rotation_of(w, dt):
    """exp([w]x) by Rodrigues in dtype dt"""
    th = np.sqrt((w * w).sum())
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dt)
    if th < 1e-12:
        return np.eye(3, dtype=dt) + K
    return np.eye(3, dtype=dt) + (np.sin(th) / th).astype(dt) * K + ((1 - np.cos(th)) / (th * th)).astype(dt) * (K @ K)


def _quat_of(R):
    """the unit quaternion (w >= 0) of a rotation matrix, any dtype"""
    dt = R.dtype.type
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    w = np.sqrt(max(dt(1) + tr, dt(0))) / dt(2)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], R.dtype) / (dt(4) * w)
    q = np.concatenate([[w], v]).astype(R.dtype)
    return q / np.sqrt((q * q).sum())


def ba64(from_ids, from_xyz, to_ids, to_points, inliers, transform, from_points=None, to_xyz=None, prior_variance=None, camera_from=DEFAULT_CAMERA,
         camera_to=DEFAULT_CAMERA, baselines=(0.075, 0.075), pixel_variance=1.0, robust_delta=8.0, dtype=np.float64, max_steps=25, tol=1e-12):
    """The same objective, stages and outlier rule as refine(), with different linear algebra: the full dense Jacobian over pose and points,
    numpy.linalg.lstsq on the re-weighted residuals, a rotation-vector update, no Schur complement, no damping.  A step is halved until it lowers
    the robust objective (undamped Gauss-Newton alone leaves the basin on some pairs); a stage ends when the relative step is below tol, when
    no halving lowers the objective any more in dtype, or after max_steps.  -> dict(transform [12] in dtype, outliers: the set of inlier
    indices, steps)"""
    dt = np.dtype(dtype).type
    ids = np.asarray(inliers, np.int32).reshape(-1).tolist()
    rows_f, rows_t = unique_rows(np.asarray(from_ids, np.int32)), unique_rows(np.asarray(to_ids, np.int32))
    rf, rt = np.array([rows_f[i] for i in ids]), np.array([rows_t[i] for i in ids])
    n = len(ids)
    P0 = np.asarray(from_xyz, np.float32)[rf].astype(dtype)
    views = [View(camera_from, baselines[0]), View(camera_to, baselines[1])]
    mat = lambda m: (np.asarray(m, np.float32).reshape(3, 4)[:, :3].astype(dtype), np.asarray(m, np.float32).reshape(3, 4)[:, 3].astype(dtype))
    R1, t1 = mat(views[0].inv_local)
    T0 = np.asarray(transform, np.float32).reshape(12)
    C0 = compose(T0, views[1].local) if views[1].local is not None else T0
    Rc, tc = mat(C0)
    R2, t2 = Rc.T.copy(), -(Rc.T @ tc)
    # the observations exactly as the rule builds them (fp32 inputs), then in dtype
    obs, stereo, present = [], [], []
    if from_points is not None:
        o, _, s = observe(views[0], np.asarray(from_xyz, np.float32)[rf], np.asarray(from_points, np.float32).reshape(-1, 2)[rf])
        obs.append(o.astype(dtype)); stereo.append(s); present.append(np.ones(n, bool))
    else:
        obs.append(np.zeros((n, 3), dtype)); stereo.append(np.zeros(n, bool)); present.append(np.zeros(n, bool))
    o, _, s = observe(views[1], None if to_xyz is None else np.asarray(to_xyz, np.float32).reshape(-1, 3)[rt], np.asarray(to_points, np.float32).reshape(-1, 2)[rt])
    obs.append(o.astype(dtype)); stereo.append(s); present.append(np.ones(n, bool))
    K = [(dt(v.fx), dt(v.fy), dt(v.cx), dt(v.cy), dt(v.b)) for v in views]
    info, delta = dt(F(D(1.0) / D(pixel_variance))), dt(F(robust_delta))
    inf = np.array([1.0] * 6 if prior_variance is None else [prior_information(prior_variance[0], LINEAR_EPSILON)] * 3 +
                   [prior_information(prior_variance[1], ANGULAR_EPSILON)] * 3, dtype)
    active = [present[0].copy(), present[1].copy()]
    outlier = np.zeros(n, bool)
    P = P0.copy()

    def project(c, R, t, Pw):
        fx, fy, cx, cy, b = K[c]
        Xc = Pw @ R.T + t
        iz = dt(1) / Xc[:, 2]
        pred = np.stack([fx * Xc[:, 0] * iz + cx, fy * Xc[:, 1] * iz + cy, fx * (Xc[:, 0] - b) * iz + cx], axis=1)
        r = obs[c] - pred
        r[:, 2] = np.where(stereo[c], r[:, 2], dt(0))
        # d pred / d Xc, [n x 3 x 3]
        G = np.zeros((n, 3, 3), dtype)
        G[:, 0, 0] = fx * iz; G[:, 0, 2] = -fx * Xc[:, 0] * iz * iz
        G[:, 1, 1] = fy * iz; G[:, 1, 2] = -fy * Xc[:, 1] * iz * iz
        G[:, 2, 0] = fx * iz; G[:, 2, 2] = -fx * (Xc[:, 0] - b) * iz * iz
        G[:, 2, :] = np.where(stereo[c][:, None], G[:, 2, :], dt(0))
        return r, G, Xc

    def prior(R, t):
        E_R, E_t = R @ Rc, R @ tc + t
        q = _quat_of(E_R)
        e = np.concatenate([E_t, dt(2) * q[1:]]).astype(dtype)
        rt0 = R @ tc
        skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype)
        J = np.zeros((6, 6), dtype)
        J[:3, :3] = -skew(rt0); J[:3, 3:] = np.eye(3, dtype=dtype)
        J[3:, :3] = q[0] * np.eye(3, dtype=dtype) - skew(q[1:])
        return e, J

    def chi2s(R, t, Pw):
        out = []
        for c, (Rm, tm) in enumerate(((R1, t1), (R, t))):
            r, _, _ = project(c, Rm, tm, Pw)
            out.append(info * (r * r).sum(axis=1))
        return out

    def objective(R, t, Pw):
        total = dt(0)
        with np.errstate(all="ignore"):
            for c, chi in enumerate(chi2s(R, t, Pw)):
                cost = np.where((delta > 0) & (chi > delta * delta), dt(2) * delta * np.sqrt(chi) - delta * delta, chi)
                total = total + cost[active[c]].sum(dtype=dtype)
            e, _ = prior(R, t)
            return total + (inf * e * e).sum(dtype=dtype)

    def system(R, t, Pw):
        """the re-weighted residuals and their dense Jacobian over (w, dt, every point)"""
        blocks, rhs = [], []
        for c, (Rm, tm) in enumerate(((R1, t1), (R, t))):
            r, G, Xc = project(c, Rm, tm, Pw)
            chi = info * (r * r).sum(axis=1)
            with np.errstate(all="ignore"):
                w = np.where((delta > 0) & (chi > delta * delta), delta / np.sqrt(chi), dt(1))
            sw = np.sqrt(info * w)
            Jp = G @ Rm                                                 # [n x 3 x 3]
            for k in range(3):
                sel = np.flatnonzero(active[c] & (stereo[c] if k == 2 else True))
                A = np.zeros((sel.shape[0], 6 + 3 * n), dtype)
                A[np.arange(sel.shape[0])[:, None], 6 + 3 * sel[:, None] + np.arange(3)] = Jp[sel, k] * sw[sel, None]
                if c == 1:
                    A[:, :3] = np.cross(Xc[sel] - tm, G[sel, k]) * sw[sel, None]
                    A[:, 3:6] = G[sel, k] * sw[sel, None]
                blocks.append(A); rhs.append(r[sel, k] * sw[sel])
        e, Jpr = prior(R, t)
        A = np.zeros((6, 6 + 3 * n), dtype)
        A[:, :6] = Jpr * np.sqrt(inf)[:, None]
        blocks.append(A); rhs.append(-e * np.sqrt(inf))
        return np.concatenate(blocks).astype(dtype), np.concatenate(rhs).astype(dtype)

    steps = []
    stages = 2 if delta > 0 else 1
    for s in range(stages):
        cost = objective(R2, t2, P)
        for step in range(max_steps):
            A, b = system(R2, t2, P)
            used = np.concatenate([np.ones(6, bool), np.repeat(active[0] | active[1], 3)])
            x = np.zeros(6 + 3 * n, dtype)
            x[used] = np.linalg.lstsq(A[:, used], b, rcond=None)[0]
            moved = None
            for halving in range(HALVINGS):                             # the safeguard: the longest of x, x / 2, x / 4, .. that lowers the objective
                Rn = (_rotation_of(x[:3], dt) @ R2).astype(dtype)
                tn, Pn = (t2 + x[3:6]).astype(dtype), (P + x[6:].reshape(n, 3)).astype(dtype)
                cn = objective(Rn, tn, Pn)
                if cn < cost:
                    moved = (Rn, tn, Pn, cn)
                    break
                x = (x * dt(0.5)).astype(dtype)
            if moved is None:                                           # no step lowers the objective any more in this precision
                break
            R2, t2, P, cost = moved
            size = np.sqrt((x * x).sum()) / (np.sqrt((P * P).sum()) + np.sqrt((t2 * t2).sum()) + 1)
            if size < tol:
                break
        steps.append(step + 1)
        if delta > 0:
            cf, ct = chi2s(R2, t2, P)
            of, ot = active[0] & (cf > delta), active[1] & (ct > delta)
            active[0] &= ~of; active[1] &= ~ot
            hit = of | ot
            outlier |= hit
            P[hit] = P0[hit]
    # the camera's pose, then t x inverse(local)
    U, _, Vt = np.linalg.svd(R2.astype(np.float64))
    Rn = (U @ Vt).astype(dtype)
    Cw = np.concatenate([Rn.T, (-(Rn.T @ t2))[:, None]], axis=1)
    if views[1].local is not None:
        L = np.asarray(views[1].local, np.float32).reshape(3, 4).astype(dtype)
        Li = np.concatenate([L[:, :3].T, (-(L[:, :3].T @ L[:, 3]))[:, None]], axis=1)
        Cw = np.concatenate([Cw[:, :3] @ Li[:, :3], (Cw[:, :3] @ Li[:, 3] + Cw[:, 3])[:, None]], axis=1)
    return dict(transform=Cw.reshape(12), outliers=set(np.flatnonzero(outlier).tolist()), steps=steps)
