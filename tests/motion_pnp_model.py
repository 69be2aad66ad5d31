"""The rule of lcd_estimate_motion_pnp (include/lcd.h) in NumPy, operation for operation: np.float32 arrays and scalars where the rule is fp32
(every NumPy operation rounds once, nothing is fused), np.float64 where it says fp64.  Vectorised over hypotheses and correspondences, which
changes no rounding: every element sees the same operations in the same order.  The three-point rigid fit, the 256-lane sum and the mix are
those of lcd_estimate_motion_3d's model."""
import numpy as np

from motion_3d_model import F, D, M32, MAX_DRAWS, MAX_ROWS, Refused, bits, mix, lane_sum, fit3, invert  # noqa: F401

STEPS = 8
BISECT = 26
SUMS = 27
OK, FEW_CORRESPONDENCES, NO_MODEL, BELOW_MIN_INLIERS, VARIANCE_REJECTED = 0, 1, 2, 3, 4
VARIANCE_FACTOR = D(2.1981)
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


class Camera:
    def __init__(self, fx=525.0, fy=525.0, cx=319.5, cy=239.5, image_width=0, image_height=0, local_transform=None):
        self.fx, self.fy, self.cx, self.cy = F(fx), F(fy), F(cx), F(cy)
        self.width, self.height = int(image_width), int(image_height)
        self.local = None if local_transform is None else np.asarray(local_transform, np.float32).reshape(12)

    def as_dict(self):
        d = dict(fx=float(self.fx), fy=float(self.fy), cx=float(self.cx), cy=float(self.cy), image_width=self.width, image_height=self.height)
        if self.local is not None:
            d["local_transform"] = self.local
        return d


def compose(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    out = np.zeros(12, np.float32)
    for r in range(3):
        for c in range(4):
            v = (a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c]) + a[4 * r + 2] * b[8 + c]
            out[4 * r + c] = v + a[4 * r + 3] if c == 3 else v
    return out


def model_of_guess(guess, local):
    g = np.asarray(guess, np.float32).reshape(12)
    return invert(compose(g, local) if local is not None else g)


def pose_of_model(model, local):
    return invert(compose(local, model) if local is not None else model)


def draw4(seed, h, m):
    """hypothesis h's four distinct indices among m, or None"""
    base = (mix((seed + h) & M32) * 4) & M32
    got = []
    for k in range(MAX_DRAWS):
        d = mix((base + k) & M32) % m
        if d in got:
            continue
        got.append(d)
        if len(got) == 4:
            return got
    return None


def correspondences(from_ids, from_xyz, to_ids, to_points, to_xyz=None):
    """steps 1 and 2 -> (matches [m] int32 ascending, P [m x 3], UV [m x 2], T [m x 3] or None)"""
    from_ids = np.asarray(from_ids, np.int32).reshape(-1)
    to_ids = np.asarray(to_ids, np.int32).reshape(-1)
    P = np.asarray(from_xyz, np.float32).reshape(-1, 3)
    UV = np.asarray(to_points, np.float32).reshape(-1, 2)
    T = None if to_xyz is None else np.asarray(to_xyz, np.float32).reshape(-1, 3)

    def unique_rows(ids):
        vals, first, counts = np.unique(ids, return_index=True, return_counts=True)
        return {int(v): int(r) for v, r, c in zip(vals, first, counts) if c == 1}

    f, t = unique_rows(from_ids), unique_rows(to_ids)
    ids, rows_f, rows_t = [], [], []
    for i in sorted(t):
        if i not in f or not np.isfinite(P[f[i]]).all():
            continue
        ids.append(i)
        rows_f.append(f[i])
        rows_t.append(t[i])
    return (np.array(ids, np.int32), P[rows_f].reshape(-1, 3).copy(), UV[rows_t].reshape(-1, 2).copy(),
            None if T is None else T[rows_t].reshape(-1, 3).copy())


def apply(model, P):
    """model [..., 12] on P [m x 3] -> X, Y, Z [..., m]"""
    m = np.asarray(model, np.float32)[..., None]
    px, py, pz = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        return [((m[..., 4 * r, :] * px + m[..., 4 * r + 1, :] * py) + m[..., 4 * r + 2, :] * pz) + m[..., 4 * r + 3, :] for r in range(3)]


def reproj_sq(model, cam, P, UV):
    """-> (e2 [..., m], front [..., m])"""
    X, Y, Z = apply(model, P)
    with np.errstate(all="ignore"):
        front = Z > F(0)
        pu = cam.fx * (X / Z) + cam.cx
        pv = cam.fy * (Y / Z) + cam.cy
        du, dv = UV[:, 0] - pu, UV[:, 1] - pv
        return du * du + dv * dv, front


def reproj_error(model, cam, P, UV):
    e2, front = reproj_sq(model, cam, P, UV)
    with np.errstate(all="ignore"):
        return np.sqrt(e2), front


def inliers_of(e, front, thr):
    with np.errstate(all="ignore"):
        return front & (e <= thr)


# ---- the minimal solver, vectorised over hypotheses

def poly4(c, x):
    return (((c[4] * x + c[3]) * x + c[2]) * x + c[1]) * x + c[0]


def clamp01(x):
    return np.where(~(x > F(0)), F(0), np.where(x > F(1), F(1), x)).astype(np.float32)


def bisect(c, lo, hi):
    """-> (found, root); root = hi where not found"""
    with np.errstate(all="ignore"):
        plo, phi = poly4(c, lo), poly4(c, hi)
        neg_lo = plo < F(0)
        found = neg_lo != (phi < F(0))
        a, b = lo.copy(), hi.copy()
        for _ in range(BISECT):
            mid = F(0.5) * (a + b)
            pm = poly4(c, mid)
            left = (pm < F(0)) == neg_lo
            a = np.where(left, mid, a).astype(np.float32)
            b = np.where(left, b, mid).astype(np.float32)
        root = F(0.5) * (a + b)
        return found, np.where(found, root, hi).astype(np.float32)


def breakpoints(c):
    with np.errstate(all="ignore"):
        a2, a1, a0 = F(12) * c[4], F(6) * c[3], F(2) * c[2]
        disc = a1 * a1 - F(4) * (a2 * a0)
        sq = np.sqrt(disc)
        den = F(2) * a2
        na1 = -a1
        r1, r2 = (na1 - sq) / den, (na1 + sq) / den
        c1, c2 = clamp01(r1), clamp01(r2)
        qa = np.where(c1 < c2, c1, c2).astype(np.float32)
        qb = np.where(c1 < c2, c2, c1).astype(np.float32)
        d = [c[1], F(2) * c[2], F(3) * c[3], F(4) * c[4], np.zeros_like(c[0])]
        zero, one = np.zeros_like(qa), np.ones_like(qa)
        _, k1 = bisect(d, zero, qa)
        _, k2 = bisect(d, qa, qb)
        _, k3 = bisect(d, qb, one)
        return k1, k2, k3


def bearing(cam, UV):
    """UV [..., 2] -> b [..., 3]"""
    with np.errstate(all="ignore"):
        x = (UV[..., 0] - cam.cx) / cam.fx
        y = (UV[..., 1] - cam.cy) / cam.fy
        n = np.sqrt((x * x + y * y) + F(1))
        return np.stack([x / n, y / n, F(1) / n], axis=-1).astype(np.float32)


def p3p(P, B, P4, UV4, cam, sweeps=5):
    """P, B [3 x H x 3], P4 [H x 3], UV4 [H x 2] -> (valid [H], models [H x 12], solutions: a list of (mask, depths [H x 3], error))"""
    P, B = np.asarray(P, np.float32), np.asarray(B, np.float32)
    H = P.shape[1]
    with np.errstate(all="ignore"):
        e1, e2, e3 = P[1] - P[0], P[2] - P[0], P[2] - P[1]
        cr0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cr1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cr2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area2 = (cr0 * cr0 + cr1 * cr1) + cr2 * cr2
        triangle = area2 > F(0)

        def norm2(e):
            return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]

        def dot(a, b):
            return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]

        c2, b2, a2 = norm2(e1), norm2(e2), norm2(e3)
        cg, cb, ca = dot(B[0], B[1]), dot(B[0], B[2]), dot(B[1], B[2])
        K, L = (a2 - c2) / b2, c2 / b2
        n0, n1, n2 = K + F(1), -(F(2) * (K * cb)), K - F(1)
        d0, d1 = F(2) * cg, -(F(2) * ca)
        w1 = -(F(2) * cb)
        n00, n01, n02, n11, n12, n22 = n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2
        NN = [n00, F(2) * n01, F(2) * n02 + n11, F(2) * n12, n22]
        DD = [d0 * d0, F(2) * (d0 * d1), d1 * d1]
        zero = np.zeros_like(K)
        ND = [n0 * d0, n0 * d1 + n1 * d0, n1 * d1 + n2 * d0, n2 * d1, zero]
        E = [DD[0], DD[1] + w1 * DD[0], (DD[2] + w1 * DD[1]) + DD[0], w1 * DD[2] + DD[1], DD[2]]
        Qc = []
        for k in range(5):
            s = NN[k] + DD[k] if k < 3 else NN[k]
            Qc.append((s - d0 * ND[k]) - L * E[k])
        Qc = [np.asarray(q, np.float32) for q in Qc]
        has = np.zeros(H, bool)
        best_e = np.zeros(H, np.float32)
        best = np.zeros((H, 12), np.float32)
        solutions = []
        for rev in (False, True):
            c = Qc[::-1] if rev else Qc
            k1, k2, k3 = breakpoints(c)
            ends = [np.zeros(H, np.float32), k1, k2, k3, np.ones(H, np.float32)]
            for seg in range(4):
                found, x = bisect(c, ends[seg], ends[seg + 1])
                v = F(1) / x if rev else x
                Nv = ((n2 * v + n1) * v) + n0
                Dv = d1 * v + d0
                u = Nv / Dv
                Wv = ((v + w1) * v) + F(1)
                s1 = np.sqrt(b2 / Wv)
                s2, s3 = u * s1, v * s1
                ok = found & triangle & np.isfinite(s1) & np.isfinite(s2) & np.isfinite(s3) & (s1 > F(0)) & (s2 > F(0)) & (s3 > F(0))
                Q = np.stack([s1[:, None] * B[0], s2[:, None] * B[1], s3[:, None] * B[2]]).astype(np.float32)
                models = fit3(P, Q, sweeps)
                X, Y, Z = (((models[:, 4 * r] * P4[:, 0] + models[:, 4 * r + 1] * P4[:, 1]) + models[:, 4 * r + 2] * P4[:, 2]) + models[:, 4 * r + 3]
                           for r in range(3))
                pu, pv = cam.fx * (X / Z) + cam.cx, cam.fy * (Y / Z) + cam.cy
                du, dv = UV4[:, 0] - pu, UV4[:, 1] - pv
                e = np.sqrt(du * du + dv * dv)
                ok = ok & (Z > F(0)) & np.isfinite(e)
                solutions.append((ok, np.stack([s1, s2, s3], axis=-1), e, models))
                take = ok & (~has | (e < best_e))
                best[take] = models[take]
                best_e = np.where(take, e, best_e).astype(np.float32)
                has = has | take
        return has, best, solutions


# ---- the fit of an ordered set

def quat_of_model(m, record=None):
    """record (a dict, if given): "picks" receives the case taken"""
    m = np.asarray(m, np.float32)
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]
    with np.errstate(all="ignore"):
        tr = (r00 + r11) + r22
        b1, b2, b3 = (r00 - r11) - r22, (r11 - r00) - r22, (r22 - r00) - r11
        c = [F(1) + tr, F(1) + b1, F(1) + b2, F(1) + b3]
        pick, top = 0, c[0]
        for k in (1, 2, 3):
            if c[k] > top:
                pick, top = k, c[k]
        if record is not None:
            record["picks"].append(pick)
        r = np.sqrt(top)
        big, f = F(0.5) * r, F(0.5) / r
        fm21, fm02, fm10 = (r21 - r12) * f, (r02 - r20) * f, (r10 - r01) * f
        fp01, fp02, fp12 = (r01 + r10) * f, (r02 + r20) * f, (r12 + r21) * f
    return np.array([[big, fm21, fm02, fm10], [fm21, big, fp01, fp02], [fm02, fp01, big, fp12], [fm10, fp02, fp12, big]][pick], np.float32)


def model_of_pose(q, t):
    """-> (model [12], the normalised q)"""
    with np.errstate(all="ignore"):
        q0, q1, q2, q3 = (F(v) for v in q)
        n = np.sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
        w, x, y, z = q0 / n, q1 / n, q2 / n, q3 / n
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        R = [[F(1) - F(2) * (yy + zz), F(2) * (xy - wz), F(2) * (xz + wy)],
             [F(2) * (xy + wz), F(1) - F(2) * (xx + zz), F(2) * (yz - wx)],
             [F(2) * (xz - wy), F(2) * (yz + wx), F(1) - F(2) * (xx + yy)]]
    out = np.zeros(12, np.float32)
    for r in range(3):
        out[4 * r:4 * r + 3] = R[r]
        out[4 * r + 3] = t[r]
    return out, np.array([w, x, y, z], np.float32)


def gn_terms(model, cam, P, UV):
    """-> [n x 27]"""
    m = np.asarray(model, np.float32)
    px, py, pz = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        Mx = (m[0] * px + m[1] * py) + m[2] * pz
        My = (m[4] * px + m[5] * py) + m[6] * pz
        Mz = (m[8] * px + m[9] * py) + m[10] * pz
        X, Y, Z = Mx + m[3], My + m[7], Mz + m[11]
        iz = F(1) / Z
        x, y = X * iz, Y * iz
        a, c = cam.fx * iz, cam.fy * iz
        ax, cy = a * x, c * y
        ru = UV[:, 0] - (cam.fx * x + cam.cx)
        rv = UV[:, 1] - (cam.fy * y + cam.cy)
        zero = np.zeros_like(a)
        Ju = [-(ax * My), a * Mz + ax * Mx, -(a * My), a, zero, -ax]
        Jv = [-(c * Mz + cy * My), cy * Mx, c * Mx, zero, c, -cy]
        cols = [Ju[i] * Ju[j] + Jv[i] * Jv[j] for i in range(6) for j in range(i, 6)]
        cols += [Ju[i] * ru + Jv[i] * rv for i in range(6)]
        out = np.stack(cols, axis=-1).astype(np.float32)
        out[~(Z > F(0))] = F(0)
    return out


def gn_solve(S):
    """-> delta [6] or None"""
    S = np.asarray(S, np.float32)
    A = np.zeros((6, 6), np.float32)
    o = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = S[o]
            o += 1
    Lm = np.zeros((6, 6), np.float32)
    d = np.zeros(6, np.float32)
    w = np.zeros(6, np.float32)
    with np.errstate(all="ignore"):
        for j in range(6):
            acc = A[j, j]
            for k in range(j):
                w[k] = Lm[j, k] * d[k]
                acc = acc - Lm[j, k] * w[k]
            if not (acc > 0 and np.isfinite(acc)):
                return None
            d[j] = acc
            for i in range(j + 1, 6):
                a = A[i, j]
                for k in range(j):
                    a = a - Lm[i, k] * w[k]
                Lm[i, j] = a / acc
        z = np.zeros(6, np.float32)
        for i in range(6):
            a = S[21 + i]
            for k in range(i):
                a = a - Lm[i, k] * z[k]
            z[i] = a
        x = np.zeros(6, np.float32)
        for i in range(5, -1, -1):
            a = z[i] / d[i]
            for k in range(i + 1, 6):
                a = a - Lm[k, i] * x[k]
            x[i] = a
    return x if np.isfinite(x).all() else None


def pose_update(q, t, delta):
    hx, hy, hz = F(0.5) * delta[0], F(0.5) * delta[1], F(0.5) * delta[2]
    w, x, y, z = (F(v) for v in q)
    with np.errstate(all="ignore"):
        q2 = np.array([((w - hx * x) - hy * y) - hz * z,
                       ((x + hx * w) + hy * z) - hz * y,
                       ((y - hx * z) + hy * w) + hz * x,
                       ((z + hx * y) - hy * x) + hz * w], np.float32)
        t2 = np.array([t[0] + delta[3], t[1] + delta[4], t[2] + delta[5]], np.float32)
    return q2, t2


def fit_set(model, cam, P, UV, steps=STEPS, record=None):
    """the fit of an ordered set (P, UV [n x ...]) from `model`; record (a dict, if given): "picks" receives the fit's Shepperd case and
    "refused" the number of its steps that gn_solve refused"""
    if P.shape[0] < 4:
        return model
    q = quat_of_model(model, record)
    t = np.array([model[3], model[7], model[11]], np.float32)
    for _ in range(steps):
        cur, q = model_of_pose(q, t)
        S = lane_sum(gn_terms(cur, cam, P, UV))
        delta = gn_solve(S)
        if delta is not None:
            q, t = pose_update(q, t, delta)
        elif record is not None:
            record["refused"].append(1)
    return model_of_pose(q, t)[0]


def refined_threshold(e, thr0):
    e = np.asarray(e, np.float32)
    n = len(e)
    with np.errstate(all="ignore"):
        buf = F(0)
        for v in e:
            buf = buf + v
        mean = buf / F(n)
        total = F(0)
        for v in e:
            dv = v - mean
            total = total + dv * dv
        variance = total / F(n - 1)
        s3 = F(3) * np.sqrt(variance)
    return s3 if s3 < thr0 else thr0


def order_key(v):
    b = bits(v).astype(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def cov_terms(pose, model, cam, P, UV, T):
    """-> (d2 [n], cosine [n]) of the inliers P, UV, T (T None without to_xyz)"""
    n = P.shape[0]
    with np.errstate(all="ignore"):
        X, Y, Z = apply(model, P)
        ccx = cam.cx if cam.cx > 0 else F(cam.width // 2) - F(0.5)
        ccy = cam.cy if cam.cy > 0 else F(cam.height // 2) - F(0.5)
        rx, ry = (UV[:, 0] - ccx) / cam.fx, (UV[:, 1] - ccy) / cam.fy
        s = Z.astype(np.float64) * D(1.1)
        ray = np.stack([(rx.astype(np.float64) * s), (ry.astype(np.float64) * s), D(1.0) * s], axis=-1).astype(np.float32)
        N = np.stack(apply(invert(model), ray), axis=-1)
        if T is not None:
            fin = np.isfinite(T).all(axis=1)
            NT = np.stack(apply(pose, T), axis=-1)
            N = np.where(fin[:, None], NT, N).astype(np.float32)
        dx, dy, dz = P[:, 0] - N[:, 0], P[:, 1] - N[:, 1], P[:, 2] - N[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        dot = (P[:, 0] * N[:, 0] + P[:, 1] * N[:, 1]) + P[:, 2] * N[:, 2]
        pp = (P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2]
        qq = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        den = np.sqrt(pp) * np.sqrt(qq)
        c = dot / den
        cosine = np.where(~(den > F(0)) | np.isnan(c), F(1), np.where(c > F(1), F(1), np.where(c < F(-1), F(-1), c))).astype(np.float32)
    assert d2.shape == (n,)
    return d2.astype(np.float32), cosine


def ranked(values, rank):
    """the element of rank `rank` in the order of the keys"""
    v = np.asarray(values, np.float32)
    return v[np.argsort(order_key(v), kind="stable")[rank]]


class _Backend:
    def __init__(self, P, UV, T, cam, model0, seed, iterations, steps):
        self.P, self.UV, self.T, self.cam, self.m = P, UV, T, cam, P.shape[0]
        self.model0, self.seed, self.iterations, self.steps = model0, seed, iterations, steps
        self.cur = np.zeros(12, np.float32)
        self.prev, self.next, self.last_e = [], [], np.zeros(0, np.float32)
        self.counts = None
        self.record = dict(picks=[], refused=[], first_differing=[])

    def ransac(self, thr):
        """-> the best candidate or None; counts [iterations + 1]"""
        draws = [draw4(self.seed, h, self.m) for h in range(self.iterations)]
        hs = [h for h, d in enumerate(draws) if d is not None]
        models = np.zeros((self.iterations + 1, 12), np.float32)
        valid = np.zeros(self.iterations + 1, bool)
        models[0], valid[0] = self.model0, True
        if hs:
            idx = np.array([draws[h] for h in hs]).T                   # [4 x H]
            has, best, _ = p3p(self.P[idx[:3]], bearing(self.cam, self.UV[idx[:3]]), self.P[idx[3]], self.UV[idx[3]], self.cam)
            cand = np.array(hs) + 1
            models[cand], valid[cand] = best, has
        self.counts = np.zeros(self.iterations + 1, np.int64)
        step = max(1, (1 << 21) // max(self.m, 1))
        for c0 in range(0, self.iterations + 1, step):
            e, front = reproj_error(models[c0:c0 + step], self.cam, self.P, self.UV)
            self.counts[c0:c0 + step] = inliers_of(e, front, thr).sum(axis=1)
        self.counts[~valid] = 0
        best = int(np.argmax(self.counts))                             # the first of the largest: the lowest candidate
        if self.counts[best] == 0:
            return None
        self.cur = models[best].copy()
        return best

    def fit_prev(self):
        self.cur = fit_set(self.cur, self.cam, self.P[self.prev], self.UV[self.prev], self.steps, self.record)

    def select(self, thr):
        e, front = reproj_error(self.cur, self.cam, self.P, self.UV)
        inside = inliers_of(e, front, thr)
        self.next = np.nonzero(inside)[0].tolist()
        self.last_e = e[inside]
        return len(self.next)

    def swap_sets(self):
        self.prev, self.next = self.next, self.prev


def refine(b, thr0, refine_iterations, min_count, trace):
    """util3d_motion_estimation.cpp:880-984; trace receives one word per pass"""
    error_threshold = thr0
    it = 0
    inlier_changed = False
    sizes = []
    while True:                                                        # do {
        b.fit_prev()
        sizes.append(len(b.prev))
        found = b.select(error_threshold)
        if found < min_count:
            trace.append("few")
            it += 1
            if it >= refine_iterations:
                break
            # continue: to the condition
        else:
            error_threshold = refined_threshold(b.last_e, thr0)
            inlier_changed = False
            b.swap_sets()
            if len(b.next) != len(b.prev):
                if len(sizes) >= min_count and sizes[-1] == sizes[-3] and sizes[-2] == sizes[-4]:
                    trace.append("oscillating")
                    break
                trace.append("size_changed")
                inlier_changed = True
            elif b.prev != b.next:
                b.record["first_differing"].append(next(i for i, (p, n) in enumerate(zip(b.prev, b.next)) if p != n))
                trace.append("members_changed")
                inlier_changed = True
            else:
                trace.append("converged")
        if not inlier_changed:                                         # } while (inlier_changed && ++it < refine_iterations)
            break
        it += 1
        if not it < refine_iterations:
            break


def check_args(n_from, n_to, min_inliers, reproj_error, iterations, refine_iterations, variance_median_ratio, max_variance):
    if n_from > MAX_ROWS or n_to > MAX_ROWS or iterations > 65535:
        raise Refused("unsupported")
    thr0 = F(reproj_error) if np.isfinite(reproj_error) else F(0)
    with np.errstate(all="ignore"):
        sq = F(D(thr0) * D(thr0))
    if (iterations < 1 or min_inliers < 1 or refine_iterations < 0 or variance_median_ratio <= 1 or not np.isfinite(reproj_error) or
            not reproj_error > 0 or not thr0 > 0 or not np.isfinite(sq) or not max_variance >= 0 or not np.isfinite(F(max_variance))):
        raise Refused("invalid")


def estimate(from_ids, from_xyz, to_ids, to_points, to_xyz=None, camera=None, guess=None, min_inliers=20, iterations=100, reproj_error=2.0,
             refine_iterations=1, variance_median_ratio=4, max_variance=0.0, seed=0, steps=STEPS):
    """one pair -> dict(transform [12] f32, status, matches, inliers (ids), variance_lin f64, angle_cos f64, variance_kind, inlier_index, model,
    trace, best, counts, picks (the Shepperd case of every fit), refused (the Gauss-Newton steps that gn_solve refused, over all fits),
    first_differing (per members_changed pass, the first position at which the two index sets differ))"""
    cam = camera if camera is not None else Camera()
    check_args(np.asarray(from_ids).size, np.asarray(to_ids).size, min_inliers, reproj_error, iterations, refine_iterations, variance_median_ratio,
               max_variance)
    matches, P, UV, T = correspondences(from_ids, from_xyz, to_ids, to_points, to_xyz)
    m = len(matches)
    r = dict(transform=np.zeros(12, np.float32), status=OK, matches=matches, inliers=np.zeros(0, np.int32), variance_lin=D(1.0), angle_cos=D(1.0),
             variance_kind=0, inlier_index=[], model=None, trace=[], best=None, counts=None, P=P, UV=UV, T=T, picks=[], refused=[], first_differing=[])
    if m < min_inliers or m < 4:
        r["status"] = FEW_CORRESPONDENCES
        return r
    thr0 = F(reproj_error)
    thr_ransac = F(D(thr0) * D(thr0))
    model0 = model_of_guess(IDENTITY if guess is None else guess, cam.local)
    b = _Backend(P, UV, T, cam, model0, seed & M32, iterations, steps)
    b.record = {k: r[k] for k in b.record}
    r["best"] = b.ransac(thr_ransac)
    r["counts"] = b.counts
    if r["best"] is None:
        r["status"] = NO_MODEL
        return r
    b.select(thr_ransac)
    b.swap_sets()
    b.next = []
    min_count = max(4, min_inliers)
    if len(b.prev) >= min_count and refine_iterations > 0:
        refine(b, thr0, refine_iterations, min_count, r["trace"])
        b.swap_sets()
    r["model"] = b.cur
    n = len(b.prev)
    r["inlier_index"] = list(b.prev)
    r["inliers"] = matches[b.prev] if n else np.zeros(0, np.int32)
    if n < min_inliers:
        r["status"] = BELOW_MIN_INLIERS
        return r
    pose = pose_of_model(b.cur, cam.local)
    kind = 1 if (to_xyz is not None or cam.width != 0 or cam.height != 0) else 2
    Pi, UVi = P[b.prev], UV[b.prev]
    if kind == 1:
        d2, cosine = cov_terms(pose, b.cur, cam, Pi, UVi, None if T is None else T[b.prev])
        k = n // variance_median_ratio
        lin = VARIANCE_FACTOR * D(ranked(d2, k))
        ang = D(ranked(cosine, n - 1 - k))
        r["d2"], r["cosines"] = d2, cosine
        if max_variance > 0 and lin > D(F(max_variance)):
            r["status"] = VARIANCE_REJECTED
            return r
    else:
        e2, _ = reproj_sq(b.cur, cam, Pi, UVi)
        with np.errstate(all="ignore"):
            err = F(0)
            for v in e2:
                err = err + v
            lin, ang = D(np.sqrt(err / F(n))), D(1.0)
    r["variance_kind"], r["variance_lin"], r["angle_cos"] = kind, lin, ang
    r["transform"] = pose
    return r


# ---- float64 yardsticks: what the fp32 rule is measured against, not part of it

def p3p_start(P, UV, cam):
    """the hypothesis of the correspondences 0, 1, 2 with 3 as the fourth -> model [12] or None"""
    idx = np.array([[0], [1], [2], [3]])
    has, best, _ = p3p(P[idx[:3]], bearing(cam, UV[idx[:3]]), P[idx[3]], UV[idx[3]], cam)
    return best[0] if has[0] else None


def lsq64(P, UV, cam, R0, t0):
    """scipy.optimize.least_squares in float64 on the pixel error from (R0, t0) -> (R, t)"""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation
    P, UV = np.asarray(P, np.float64), np.asarray(UV, np.float64)
    fx, fy, cx, cy = (float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))

    def residual(x):
        C = P @ Rotation.from_rotvec(x[:3]).as_matrix().T + x[3:]
        return np.concatenate([fx * C[:, 0] / C[:, 2] + cx - UV[:, 0], fy * C[:, 1] / C[:, 2] + cy - UV[:, 1]])

    x0 = np.concatenate([Rotation.from_matrix(R0).as_rotvec(), t0])
    s = least_squares(residual, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return Rotation.from_rotvec(s.x[:3]).as_matrix(), s.x[3:]


def fit_deviation(sets, cam, steps=STEPS):
    """over the sets of motion_pnp_inputs.fit_sets, noise-free and noisy: the worst |entry| difference between the rule's fit from the P3P start
    and the float64 least squares, for rotation and translation; and the worst reprojection error of the held-out noise-free points under the
    noise-free hypothesis -> (rotation, translation, p3p pixels, fits compared)"""
    worst_r = worst_t = worst_p = 0.0
    n = 0
    for s in sets:
        start = p3p_start(s["P"], s["UV0"], cam)
        if start is None:
            continue
        e, front = reproj_error(start, cam, s["P"][4:], s["UV0"][4:])
        assert front.all()
        worst_p = max(worst_p, float(e.max()))
        for uv in (s["UV0"], s["UV1"]):
            m = fit_set(start, cam, s["P"], uv, steps).reshape(3, 4).astype(np.float64)
            R, t = lsq64(s["P"], uv, cam, s["R"], s["t"])
            worst_r, worst_t = max(worst_r, np.abs(m[:, :3] - R).max()), max(worst_t, np.abs(m[:, 3] - t).max())
            n += 1
    return worst_r, worst_t, worst_p, n
