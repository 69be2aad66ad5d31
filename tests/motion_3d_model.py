"""The rule of lcd_estimate_motion_3d (include/lcd.h) in NumPy, operation for operation: np.float32 arrays and scalars where the rule is fp32
(every NumPy operation rounds once, nothing is fused), np.float64 where it says fp64.  Vectorised over hypotheses and correspondences, which
changes no rounding: every element sees the same operations in the same order."""
import numpy as np

F = np.float32
D = np.float64
M32 = 0xFFFFFFFF
LANES = 256
MAX_DRAWS = 16
SWEEPS = 5
MAX_ROWS = 8192
OK, FEW_CORRESPONDENCES, NO_MODEL, FEW_INLIERS, BELOW_MIN_INLIERS = 0, 1, 2, 3, 4
VARIANCE_FACTOR = D(2.1981)
PLANES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


class Refused(Exception):
    pass


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw3(seed, h, m):
    """hypothesis h's three distinct indices among m, or None"""
    base = (mix((seed + h) & M32) * 3) & M32
    got = []
    for k in range(MAX_DRAWS):
        d = mix((base + k) & M32) % m
        if d in got:
            continue
        got.append(d)
        if len(got) == 3:
            return got
    return None


def correspondences(from_ids, from_xyz, to_ids, to_xyz):
    """steps 1 and 2 -> (matches [m] int32 ascending, P [m x 3], Q [m x 3])"""
    from_ids = np.asarray(from_ids, np.int32).reshape(-1)
    to_ids = np.asarray(to_ids, np.int32).reshape(-1)
    P = np.asarray(from_xyz, np.float32).reshape(-1, 3)
    Q = np.asarray(to_xyz, np.float32).reshape(-1, 3)

    def unique_rows(ids):
        vals, first, counts = np.unique(ids, return_index=True, return_counts=True)
        return {int(v): int(r) for v, r, c in zip(vals, first, counts) if c == 1}

    f, t = unique_rows(from_ids), unique_rows(to_ids)
    ids, rows_f, rows_t = [], [], []
    for i in sorted(f):
        if i not in t:
            continue
        p, q = P[f[i]], Q[t[i]]
        if not (np.isfinite(p).all() and np.isfinite(q).all()):
            continue
        if not ((p != 0).any() and (q != 0).any()):
            continue
        ids.append(i)
        rows_f.append(f[i])
        rows_t.append(t[i])
    return np.array(ids, np.int32), P[rows_f].reshape(-1, 3).copy(), Q[rows_t].reshape(-1, 3).copy()


def lane_sum(E):
    """SUM over axis 0 in the rule's order: lane l adds E[l], E[l + 256], .. onto +0, then the halving tree"""
    E = np.asarray(E, np.float32)
    n = E.shape[0]
    rows = max((n + LANES - 1) // LANES, 1)
    pad = np.zeros((rows * LANES,) + E.shape[1:], np.float32)
    pad[:n] = E
    part = np.zeros((LANES,) + E.shape[1:], np.float32)
    for r in range(rows):
        part = part + pad[r * LANES:(r + 1) * LANES]
    s = LANES // 2
    while s >= 1:
        part = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def sum3(e0, e1, e2):
    a, b, c = F(0) + e0, F(0) + e1, F(0) + e2
    return (a + c) + b


def _rotate(A, V, p, q):
    apq = A[p][q]
    go = apq != F(0)
    diff = A[q][q] - A[p][p]
    den = F(2) * apq
    theta = diff / den
    mag = np.abs(theta)
    th2 = theta * theta
    root = np.sqrt(th2 + F(1))
    total = mag + root
    sgn = np.where(theta < F(0), F(-1), F(1)).astype(np.float32)
    t = sgn / total
    croot = np.sqrt(t * t + F(1))
    c = F(1) / croot
    s = t * c
    tapq = t * apq
    new = {}
    new[(p, p)] = A[p][p] - tapq
    new[(q, q)] = A[q][q] + tapq
    new[(p, q)] = new[(q, p)] = np.zeros_like(apq)
    for r in range(4):
        if r in (p, q):
            continue
        arp, arq = A[r][p], A[r][q]
        np_ = c * arp - s * arq
        nq_ = s * arp + c * arq
        new[(r, p)] = new[(p, r)] = np_
        new[(r, q)] = new[(q, r)] = nq_
    for (r, c_), v in new.items():
        A[r][c_] = np.where(go, v, A[r][c_]).astype(np.float32)
    for r in range(4):
        vrp, vrq = V[r][p], V[r][q]
        a = c * vrp - s * vrq
        b = s * vrp + c * vrq
        V[r][p] = np.where(go, a, vrp).astype(np.float32)
        V[r][q] = np.where(go, b, vrq).astype(np.float32)


def horn_fit(cp, cq, S, sweeps=SWEEPS):
    """cp, cq [..., 3], S [..., 9] -> model [..., 12] (row-major 3 x 4: R p + t ~ q)"""
    cp, cq, S = (np.asarray(x, np.float32) for x in (cp, cq, S))
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (S[..., k] for k in range(9))
    with np.errstate(all="ignore"):
        A = [[None] * 4 for _ in range(4)]
        A[0][0] = (Sxx + Syy) + Szz
        A[0][1] = Syz - Szy
        A[0][2] = Szx - Sxz
        A[0][3] = Sxy - Syx
        A[1][1] = (Sxx - Syy) - Szz
        A[1][2] = Sxy + Syx
        A[1][3] = Szx + Sxz
        A[2][2] = (Syy - Sxx) - Szz
        A[2][3] = Syz + Szy
        A[3][3] = (Szz - Sxx) - Syy
        for r in range(4):
            for c in range(r):
                A[r][c] = A[c][r]
        one, zero = np.ones_like(Sxx), np.zeros_like(Sxx)
        V = [[one if r == c else zero for c in range(4)] for r in range(4)]
        for _ in range(sweeps):
            for p, q in PLANES:
                _rotate(A, V, p, q)
        top = A[0][0]
        quat = [V[r][0] for r in range(4)]
        for k in (1, 2, 3):
            better = A[k][k] > top
            top = np.where(better, A[k][k], top)
            quat = [np.where(better, V[r][k], quat[r]) for r in range(4)]
        q0, q1, q2, q3 = quat
        n2 = ((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3
        n = np.sqrt(n2)
        w, x, y, z = q0 / n, q1 / n, q2 / n, q3 / n
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        R = [[F(1) - F(2) * (yy + zz), F(2) * (xy - wz), F(2) * (xz + wy)],
             [F(2) * (xy + wz), F(1) - F(2) * (xx + zz), F(2) * (yz - wx)],
             [F(2) * (xz - wy), F(2) * (yz + wx), F(1) - F(2) * (xx + yy)]]
        out = np.zeros(S.shape[:-1] + (12,), np.float32)
        for r in range(3):
            rot = (R[r][0] * cp[..., 0] + R[r][1] * cp[..., 1]) + R[r][2] * cp[..., 2]
            for c in range(3):
                out[..., 4 * r + c] = R[r][c]
            out[..., 4 * r + 3] = cq[..., r] - rot
    return out


def fit3(P, Q, sweeps=SWEEPS):
    """P, Q [3, ..., 3]: three correspondences in draw order (axis 0), vectorised over the middle axes -> model [..., 12]"""
    P, Q = np.asarray(P, np.float32), np.asarray(Q, np.float32)
    with np.errstate(all="ignore"):
        cp = sum3(P[0], P[1], P[2]) / F(3)
        cq = sum3(Q[0], Q[1], Q[2]) / F(3)
        dp, dq = P - cp, Q - cq
        S = np.stack([sum3(dp[0][..., a] * dq[0][..., b], dp[1][..., a] * dq[1][..., b], dp[2][..., a] * dq[2][..., b])
                      for a in range(3) for b in range(3)], axis=-1)
    return horn_fit(cp, cq, S, sweeps)


def fit_set(P, Q, sweeps=SWEEPS):
    """the fit of an ordered set of n correspondences, P, Q [n x 3]"""
    P, Q = np.asarray(P, np.float32), np.asarray(Q, np.float32)
    n = F(P.shape[0])
    with np.errstate(all="ignore"):
        cp = lane_sum(P) / n
        cq = lane_sum(Q) / n
        dp, dq = P - cp, Q - cq
        S = np.stack([lane_sum(dp[:, a] * dq[:, b]) for a in range(3) for b in range(3)], axis=-1)
    return horn_fit(cp, cq, S, sweeps)


def dist2(model, P, Q):
    """model [..., 12] against P, Q [m x 3] -> d2 [..., m]"""
    m = np.asarray(model, np.float32)[..., None]
    px, py, pz = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        d = []
        for r in range(3):
            v = ((m[..., 4 * r, :] * px + m[..., 4 * r + 1, :] * py) + m[..., 4 * r + 2, :] * pz) + m[..., 4 * r + 3, :]
            d.append(v - Q[:, r])
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def invert(model):
    m = np.asarray(model, np.float32)
    out = np.zeros(12, np.float32)
    for r in range(3):
        abc = (m[r] * m[3] + m[4 + r] * m[7]) + m[8 + r] * m[11]
        out[4 * r], out[4 * r + 1], out[4 * r + 2] = m[r], m[4 + r], m[8 + r]
        out[4 * r + 3] = -abc
    return out


def variance_of(d2):
    """computeVariance: 2.1981 x the element of rank size >> 1"""
    s = np.sort(bits(d2))
    return VARIANCE_FACTOR * D(s[len(s) >> 1:][:1].view(np.float32)[0])


def threshold_of(inlier_distance, variance):
    sigma = D(3.0) * np.sqrt(D(variance))
    return sigma if sigma < inlier_distance else inlier_distance


class _Backend:
    def __init__(self, P, Q, seed, iterations, thr2, sweeps):
        self.P, self.Q, self.m = P, Q, P.shape[0]
        self.seed, self.iterations, self.thr2, self.sweeps = seed, iterations, thr2, sweeps
        self.cur = np.zeros(12, np.float32)
        self.prev, self.next, self.last_d2 = [], [], np.zeros(0, np.float32)
        self.counts = None

    def ransac(self):
        draws = [draw3(self.seed, h, self.m) for h in range(self.iterations)]
        hs = [h for h, d in enumerate(draws) if d is not None]
        self.counts = np.zeros(self.iterations, np.int64)
        if not hs:
            return None
        idx = np.array([draws[h] for h in hs]).T                     # [3 x H]
        models = fit3(self.P[idx], self.Q[idx], self.sweeps)           # [H x 12]
        step = max(1, (1 << 21) // max(self.m, 1))
        for c0 in range(0, len(hs), step):
            d2 = dist2(models[c0:c0 + step], self.P, self.Q)
            self.counts[hs[c0:c0 + step]] = (d2.astype(np.float64) < self.thr2).sum(axis=1)
        best = int(np.argmax(self.counts))                             # the first of the largest: the lowest h
        if self.counts[best] == 0:
            return None
        self.cur = models[hs.index(best)]
        return best

    def fit_prev(self):
        if len(self.prev) >= 3:
            self.cur = fit_set(self.P[self.prev], self.Q[self.prev], self.sweeps)

    def select(self, thr2):
        d2 = dist2(self.cur, self.P, self.Q)
        inside = d2.astype(np.float64) < thr2
        self.next = np.nonzero(inside)[0].tolist()
        self.last_d2 = d2[inside]
        return len(self.next)

    def swap_sets(self):
        self.prev, self.next = self.next, self.prev


def refine(b, inlier_distance, refine_iterations, trace, first_differing=None):
    """util3d_registration.cpp:115-196; trace receives one word per pass, first_differing (a list, if given) the first index at which the two
    compared sets differ, once per pass that says members_changed"""
    error_threshold = D(inlier_distance)
    it = 0
    inlier_changed = False
    sizes = []
    while True:                                                        # do {
        b.fit_prev()
        sizes.append(len(b.prev))
        found = b.select(error_threshold * error_threshold)
        if found == 0:
            trace.append("empty")
            it += 1
            if it >= refine_iterations:
                break
            # continue: to the condition
        else:
            variance = variance_of(b.last_d2)
            error_threshold = threshold_of(D(inlier_distance), variance)
            inlier_changed = False
            b.swap_sets()
            if len(b.next) != len(b.prev):
                if len(sizes) >= 4 and sizes[-1] == sizes[-3] and sizes[-2] == sizes[-4]:
                    trace.append("oscillating")
                    break
                trace.append("size_changed")
                inlier_changed = True
            elif b.prev != b.next:
                trace.append("members_changed")
                if first_differing is not None:
                    first_differing.append(next(i for i, (p, n) in enumerate(zip(b.prev, b.next)) if p != n))
                inlier_changed = True
            else:
                trace.append("converged")
        if not inlier_changed:                                         # } while (inlier_changed && ++it < refine_iterations)
            break
        it += 1
        if not it < refine_iterations:
            break


def check_args(n_from, n_to, min_inliers, inlier_distance, iterations, refine_iterations):
    if n_from > MAX_ROWS or n_to > MAX_ROWS or iterations > 65535:
        raise Refused("unsupported")
    if iterations < 1 or min_inliers < 1 or refine_iterations < 0 or not np.isfinite(inlier_distance) or not inlier_distance > 0:
        raise Refused("invalid")


def estimate(from_ids, from_xyz, to_ids, to_xyz, min_inliers=20, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=0, sweeps=SWEEPS):
    """one pair -> dict(transform [12] f32, status, matches, inliers (ids), variance f64, inlier_index, model, trace, best, counts, last_d2 (the
    d2 of the last selection, what the variance is the median of), first_differing (see refine))"""
    matches, P, Q = correspondences(from_ids, from_xyz, to_ids, to_xyz)
    check_args(np.asarray(from_ids).size, np.asarray(to_ids).size, min_inliers, inlier_distance, iterations, refine_iterations)
    m = len(matches)
    thr = D(inlier_distance)
    r = dict(transform=np.zeros(12, np.float32), status=OK, matches=matches, inliers=np.zeros(0, np.int32), variance=D(1.0),
             inlier_index=[], model=None, trace=[], best=None, counts=None, P=P, Q=Q, last_d2=np.zeros(0, np.float32), first_differing=[])
    if m < min_inliers or m < 3:
        r["status"] = FEW_CORRESPONDENCES
        return r
    b = _Backend(P, Q, seed & M32, iterations, thr * thr, sweeps)
    r["best"] = b.ransac()
    r["counts"] = b.counts
    if r["best"] is None:
        r["status"] = NO_MODEL
        return r
    b.select(thr * thr)
    b.swap_sets()
    b.next = []
    if refine_iterations > 0:
        refine(b, thr, refine_iterations, r["trace"], r["first_differing"])
        b.swap_sets()
    r["model"] = b.cur
    r["last_d2"] = b.last_d2
    n = len(b.prev)
    if n < 3:
        r["status"] = FEW_INLIERS
        return r
    r["inlier_index"] = list(b.prev)
    r["inliers"] = matches[b.prev]
    r["variance"] = variance_of(b.last_d2)
    if n < min_inliers:
        r["status"] = BELOW_MIN_INLIERS
        return r
    r["transform"] = invert(b.cur)
    return r


def kabsch64(P, Q):
    """float64 SVD fit (R, t) of P onto Q: what the fp32 rule is measured against, not part of it"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    cp, cq = P.mean(axis=0), Q.mean(axis=0)
    H = (P - cp).T @ (Q - cq)
    U, s, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, cq - R @ cp, s
