"""The rule of lcd_filter_scans (include/lcd.h) in NumPy, operation for operation: np.float32 arrays where the rule is fp32 (every NumPy
operation rounds once, nothing is fused).  Vectorised over rows, which changes no rounding; every sum is taken in the rule's order.
Also pipeline64, an independent filter (numpy.lexsort voxel grid, scipy's kd-tree, numpy.linalg.eigh) that runs in float64 and in float32;
the rule is measured against it and it is not part of the rule."""
import numpy as np

from motion_3d_model import F, bits, _rotate  # noqa: F401
from register_icp_plane_model import SWEEPS

OK, EMPTY, GRID_TOO_LARGE, TOO_MANY_ROWS, NO_ROOM = 0, 1, 2, 3, 4
INVALID, UNSUPPORTED = 1, 5
MAX_K, MAX_SAMPLED, MAX_NORMAL_ROWS = 32, 16384, 8192
NAN_BITS = np.uint32(0x7FC00000)
INT32_MAX = 2147483647


class Refused(Exception):
    def __init__(self, code):
        super().__init__("refused with %d" % code)
        self.code = code


def dist2(P, Q):
    """[a x 3], [b x 3] -> [a x b], the ICP's distance"""
    d = [(P[:, None, a] - Q[None, :, a]).astype(np.float32) for a in range(3)]
    return ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(np.float32)


def stays(X, is_2d, range_min, range_max):
    """step 1's test for the rows of X"""
    with np.errstate(all="ignore"):
        keep = np.isfinite(X).all(axis=1)
        lo, hi = F(range_min), F(range_max)
        if lo > 0 or hi > 0:
            r = X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]
            if not is_2d:
                r = r + X[:, 2] * X[:, 2]
            keep &= np.isfinite(r)
            if lo > 0:
                keep &= ~(r < lo * lo)
            if hi > 0:
                keep &= ~(r > hi * hi)
    return keep


def voxel_grid(X, voxel_size):
    """step 2 -> (centroids [v x 3] in ascending voxel index, or None: LCD_SCAN_GRID_TOO_LARGE)"""
    with np.errstate(all="ignore"):
        inv = F(1) / F(voxel_size)
        f = np.floor((X * inv).astype(np.float32))
    if not ((f >= F(-2147483648.0)) & (f < F(2147483648.0))).all():
        return None
    cells = f.astype(np.int64)
    lo, hi = cells.min(axis=0), cells.max(axis=0)
    d = [int(hi[a] - lo[a] + 1) for a in range(3)]
    if max(d) > INT32_MAX or d[0] * d[1] > INT32_MAX or d[0] * d[1] * d[2] > INT32_MAX:
        return None
    idx = (cells[:, 0] - lo[0]) + (cells[:, 1] - lo[1]) * d[0] + (cells[:, 2] - lo[2]) * (d[0] * d[1])
    order = np.argsort(idx, kind="stable")                               # ascending index, ascending row inside a voxel
    sidx = idx[order]
    head = np.ones(len(order), bool)
    head[1:] = sidx[1:] != sidx[:-1]
    starts = np.flatnonzero(head)
    counts = np.diff(np.append(starts, len(order)))
    voxel = np.cumsum(head) - 1
    rank = np.arange(len(order)) - starts[voxel]
    S = np.zeros((len(starts), 3), np.float32)
    short = counts <= 64
    for r in range(int(counts[short].max()) if short.any() else 0):      # the r-th row of every short run at once
        sel = (rank == r) & short[voxel]
        S[voxel[sel]] = S[voxel[sel]] + X[order[sel]]
    for v in np.flatnonzero(~short):                                     # a long run: a running sum from +0
        rows = X[order[starts[v]:starts[v] + counts[v]]]
        S[v] = np.cumsum(np.vstack([np.zeros((1, 3), np.float32), rows]), axis=0, dtype=np.float32)[-1]
    return (S / counts.astype(np.float32)[:, None]).astype(np.float32)


def _acc(P, Q, S, SS, mask=None):
    """one neighbour Q[i] of every row P[i] into the sums"""
    with np.errstate(all="ignore"):
        u = (Q - P).astype(np.float32)
        nS = S + u
        prods = np.stack([u[:, 0] * u[:, 0], u[:, 0] * u[:, 1], u[:, 0] * u[:, 2], u[:, 1] * u[:, 1], u[:, 1] * u[:, 2], u[:, 2] * u[:, 2]], axis=1)
        nSS = SS + prods
    if mask is None:
        return nS.astype(np.float32), nSS.astype(np.float32)
    return np.where(mask[:, None], nS, S).astype(np.float32), np.where(mask[:, None], nSS, SS).astype(np.float32)


def points_away(vp, P, N):
    with np.errstate(all="ignore"):
        v = (np.asarray(vp, np.float32)[None, :] - P).astype(np.float32)
        return ((v[:, 0] * N[:, 0] + v[:, 1] * N[:, 1]) + v[:, 2] * N[:, 2]) < F(0)


def normals_of(P, S, SS, n, viewpoint, sweeps=SWEEPS):
    """the normal of every row out of its sums; n [rows] neighbours each"""
    rows = P.shape[0]
    out = np.full((rows, 3), NAN_BITS.view(np.float32), np.float32)
    if rows == 0:
        return out
    with np.errstate(all="ignore"):
        fn = n.astype(np.float32)
        m = (S / fn[:, None]).astype(np.float32)
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        A = [[np.zeros(rows, np.float32) for _ in range(4)] for _ in range(4)]
        V = [[np.full(rows, 1 if r == c else 0, np.float32) for c in range(4)] for r in range(4)]
        for k, (a, b) in enumerate(pairs):
            cov = (SS[:, k] / fn - m[:, a] * m[:, b]).astype(np.float32)
            A[a][b] = cov
            A[b][a] = cov.copy()
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                _rotate(A, V, p, q)
        best = A[0][0]
        e = np.stack([V[0][0], V[1][0], V[2][0]], axis=1)
        for k in (1, 2):
            lt = A[k][k] < best
            best = np.where(lt, A[k][k], best)
            e = np.where(lt[:, None], np.stack([V[0][k], V[1][k], V[2][k]], axis=1), e)
        e = e.astype(np.float32)
        flip = points_away(viewpoint, P, e)
        e = np.where(flip[:, None], -e, e).astype(np.float32)
    has = n >= 3
    out[has] = e[has]
    return out


def neighbours_k(C, k, chunk=512):
    """K mode: [rows x min(k, rows)] neighbour rows in ascending key"""
    c = C.shape[0]
    n = min(k, c)
    out = np.zeros((c, n), np.int64)
    row = np.arange(c, dtype=np.uint64)
    for a in range(0, c, chunk):
        with np.errstate(all="ignore"):
            keys = (dist2(C[a:a + chunk], C).view(np.uint32).astype(np.uint64) << np.uint64(32)) | row[None, :]
        part = np.partition(keys, n - 1, axis=1)[:, :n]
        part.sort(axis=1)
        out[a:a + chunk] = (part & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return out


def estimate_normals(C, normal_k, normal_radius, viewpoint, sweeps=SWEEPS):
    """step 3 over the cloud C -> normals [rows x 3]"""
    c = C.shape[0]
    S, SS = np.zeros((c, 3), np.float32), np.zeros((c, 6), np.float32)
    if normal_k > 0:
        nb = neighbours_k(C, normal_k)
        for s in range(nb.shape[1]):
            S, SS = _acc(C, C[nb[:, s]], S, SS)
        n = np.full(c, nb.shape[1], np.int64)
    else:
        with np.errstate(all="ignore"):
            r2 = F(normal_radius) * F(normal_radius)
            inside = dist2(C, C) <= r2
        for j in range(c):
            S, SS = _acc(C, np.broadcast_to(C[j], C.shape), S, SS, inside[:, j])
        n = inside.sum(axis=1)
    return normals_of(C, S, SS, n, viewpoint, sweeps)


def ground_up(up, P, N):
    with np.errstate(all="ignore"):
        flip = points_away((0.0, 0.0, 10.0), P, N) | ((N[:, 2] < -F(up)) & (P[:, 2] < F(10)))
        return np.where(flip[:, None], -N, N).astype(np.float32)


def filter_scan(xyz, capacity=None, downsampling_step=1, is_2d=False, normal_k=0, range_min=0.0, range_max=0.0, voxel_size=0.0, normal_radius=0.0,
                ground_normals_up=0.0, viewpoint=(0.0, 0.0, 0.0), device_entry=False, sweeps=SWEEPS):
    """one scan [n x 3] into a region of `capacity` rows (default n) -> dict(xyz, normals [capacity x 3] (None without normals), count, status,
    stage_counts [3]); raises Refused(code)"""
    X = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = X.shape[0]
    cap = n if capacity is None else int(capacity)
    floats = [range_min, range_max, voxel_size, normal_radius, ground_normals_up] + list(viewpoint)
    if not np.isfinite(np.asarray(floats, np.float32)).all() or F(voxel_size) < 0 or F(normal_radius) < 0 or F(ground_normals_up) < 0:
        raise Refused(INVALID)
    if normal_k < 0 or normal_k > MAX_K or (normal_k > 0 and F(normal_radius) > 0):
        raise Refused(INVALID)
    normals = normal_k > 0 or F(normal_radius) > 0
    if normals and is_2d:
        raise Refused(UNSUPPORTED)
    step = 1 if downsampling_step <= 1 or n <= downsampling_step else int(downsampling_step)
    m = n // step
    if m > MAX_SAMPLED:
        raise Refused(UNSUPPORTED)
    if not device_entry and not np.isfinite(X).all():
        raise Refused(INVALID)
    nan = NAN_BITS.view(np.float32)
    out = dict(xyz=np.full((cap, 3), nan, np.float32), normals=np.full((cap, 3), nan, np.float32) if normals else None, count=0, status=OK,
               stage_counts=np.zeros(3, np.int32))
    C = X[np.arange(m) * step]
    C = C[stays(C, is_2d, range_min, range_max)]
    out["stage_counts"][0] = C.shape[0]
    if C.shape[0] == 0:
        out["status"] = EMPTY
        return out
    if F(voxel_size) > 0:
        C = voxel_grid(C, voxel_size)
        if C is None:
            out["status"] = GRID_TOO_LARGE
            return out
    out["stage_counts"][1] = C.shape[0]
    N = None
    if normals:
        if C.shape[0] > MAX_NORMAL_ROWS:
            out["status"] = TOO_MANY_ROWS
            return out
        N = estimate_normals(C, normal_k, normal_radius, viewpoint, sweeps)
        keep = np.isfinite(N).all(axis=1)
        C, N = C[keep], N[keep]
    if C.shape[0] == 0:
        out["status"] = EMPTY
        return out
    out["stage_counts"][2] = C.shape[0]
    if C.shape[0] > cap:
        out["status"] = NO_ROOM
        return out
    if normals and F(ground_normals_up) > 0:
        N = ground_up(ground_normals_up, C, N)
    out["count"] = C.shape[0]
    out["xyz"][:C.shape[0]] = C
    if normals:
        out["normals"][:C.shape[0]] = N
    return out


def filter_scans(scans, capacities=None, **kw):
    """a batch -> the arrays both entries return: xyz, normals [M x 3] (None without normals), count, status [n], stage_counts [n x 3]"""
    caps = [None] * len(scans) if capacities is None else capacities
    rs = [filter_scan(s, c, **kw) for s, c in zip(scans, caps)]
    normals = rs[0]["normals"] is not None if rs else False
    z = np.zeros((0, 3), np.float32)
    return dict(xyz=np.concatenate([r["xyz"] for r in rs] + [z]), normals=np.concatenate([r["normals"] for r in rs] + [z]) if normals else None,
                count=np.array([r["count"] for r in rs], np.int32), status=np.array([r["status"] for r in rs], np.int32),
                stage_counts=np.array([r["stage_counts"] for r in rs], np.int32).reshape(-1, 3))


def pipeline64(xyz, leaf, k, dtype=np.float64, viewpoint=(0.0, 0.0, 0.0)):
    """an independent voxel grid + K-neighbour normals in `dtype` -> dict(cloud, neighbours (sorted rows), normals, gap): lexsort on the floored
    cells, centroids by np.add.at, scipy's kd-tree, the covariance about the neighbours' mean, numpy.linalg.eigh"""
    from scipy.spatial import cKDTree
    X = np.asarray(xyz, dtype)
    cells = np.floor(X / dtype(leaf)).astype(np.int64)
    order = np.lexsort((cells[:, 0], cells[:, 1], cells[:, 2]))          # x fastest, as the voxel index
    sc = cells[order]
    head = np.ones(len(order), bool)
    head[1:] = (sc[1:] != sc[:-1]).any(axis=1)
    voxel = np.cumsum(head) - 1
    cloud = np.zeros((voxel[-1] + 1, 3), dtype)
    np.add.at(cloud, voxel, X[order])
    cloud = (cloud / np.bincount(voxel).astype(dtype)[:, None]).astype(dtype)
    _, nb = cKDTree(cloud.astype(np.float64)).query(cloud.astype(np.float64), k=k)
    Q = cloud[nb]                                                       # [rows x k x 3]
    d = (Q - Q.mean(axis=1, keepdims=True)).astype(dtype)
    cov = (np.einsum("nka,nkb->nab", d, d) / dtype(k)).astype(dtype)
    w, v = np.linalg.eigh(cov)
    nrm = v[:, :, 0]
    away = (((np.asarray(viewpoint, dtype) - cloud) * nrm).sum(axis=1) < 0)
    nrm = np.where(away[:, None], -nrm, nrm)
    with np.errstate(all="ignore"):
        gap = (w[:, 1] - w[:, 0]) / w[:, 2]
    return dict(cloud=cloud, neighbours=np.sort(nb, axis=1), normals=nrm, gap=gap)
