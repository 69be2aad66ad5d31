"""Inputs of the guided matcher's GPU tests (tests/test_gpu_guided_match*.py), NumPy only, and the property each input is there for, stated
over the MODEL's output (guided_match_model): tests/test_guided_match_inputs.py asserts them without a GPU.

An input that lacks its property is replaced by the next seed (first_seed), never skipped; the number of seeds is capped.
A pair is the tuple (from, to, corners, corner_from_row, to_points)."""
import numpy as np

import guided_match_model as M
from pair_match_inputs import first_seed, fresh, noisy

WIDTH, HEIGHT, RADIUS = 640.0, 480.0, 40.0
KINDS = [("f32", 64), ("f32", 128), ("f32", 256), ("u8", 32), ("u8", 64), ("f32", 96), ("f32", 61), ("u8", 48), ("u8", 5)]
SIZES = [(0, 0, 5), (5, 0, 5), (5, 5, 0), (1, 1, 1), (2, 2, 2), (33, 31, 65), (300, 280, 300), (1100, 1100, 1100)]   # (nf, nc, nt)
GENERAL = [(33, 31, 65), (300, 280, 300), (1100, 1100, 1100)]
WINDOW_COUNTS = [63, 64, 65, 128, 129]                         # the list drain: one short of a full list, full, one over, two lists, two and one
ALL_OUTCOMES = {"empty", "single", "accepted", "rejected", "contested"}


def uniform_points(rng, n):
    return (rng.random((n, 2)) * np.array([WIDTH, HEIGHT])).astype(np.float32)


def general_pair(dtype, dim, nf, nc, nt, seed):
    """Points uniform in 640 x 480.  The corners belong to a random subset of the from-rows in random order (corner_from_row is a
    permutation: not monotone, not covering).  Half of the to-points are noisy copies (sigma 3 px) of corners drawn WITH replacement -- two
    copies of one corner are what the ratio rejects -- with noisy copies of that corner's descriptor; the rest are fresh points with fresh
    descriptors.  From eight corners on: corner 1 sits beside corner 0 with a near copy of its descriptor and to-row 0 is the only copy of
    either (a contested to-row); to-rows 2 and 3 are both copies of corner 2, side by side (two to-rows for one corner); corner 5 and
    to-point 5 lie far outside the image, alone (empty windows at any density), corner 6 and its copy, to-point 4, likewise but together
    (single candidates)."""
    rng = np.random.default_rng(seed)
    frm = fresh(rng, dtype, dim, nf)
    cfr = rng.permutation(nf)[:nc].astype(np.int32)
    corners = uniform_points(rng, nc)
    n_copy = nt // 2 if nc else 0
    planted = nc >= 8 and n_copy >= 6
    src = rng.integers(0, max(nc, 1), n_copy)
    if planted:
        corners[1] = corners[0] + np.float32(1.5)
        frm[cfr[1]] = noisy(rng, frm[cfr[0]][None])[0]
        src[src <= 1] = 3
        corners[5], corners[6] = (-500.0, -500.0), (-1000.0, 1000.0)
        src[src <= 1] = 3
        src[(src == 5) | (src == 6)] = 7
        src[:6] = [0, 4, 2, 2, 6, 3]
    pts = np.concatenate([corners[src] + rng.standard_normal((n_copy, 2)).astype(np.float32) * np.float32(3.0), uniform_points(rng, nt - n_copy)])
    to = np.concatenate([noisy(rng, frm[cfr[src]]) if n_copy else frm[:0], fresh(rng, dtype, dim, nt - n_copy)])
    perm = rng.permutation(nt)
    if planted:
        pts[3] = pts[2] + np.float32(1.0)
        pts[5] = (2000.0, 2000.0)
        perm = np.concatenate([np.arange(6), 6 + rng.permutation(nt - 6)])      # to-rows 0 .. 5 stay where they are
    return (np.ascontiguousarray(frm), np.ascontiguousarray(to[perm]), np.ascontiguousarray(corners), cfr,
            np.ascontiguousarray(pts[perm].astype(np.float32)))


def swapped(pair):
    """the pair with the roles of corners and to-rows exchanged: frame-to-projected on it asks what projected-to-frame asks on `pair`"""
    frm, to, corners, cfr, pts = pair
    return to, np.ascontiguousarray(frm[cfr]), pts, np.arange(to.shape[0], dtype=np.int32), corners


def has_every_outcome(oracle, pair, radius=RADIUS):
    """both directions under the ratio rule hold an empty window, a single candidate, an accepted and a rejected comparison and a target
    chosen twice; projected-to-frame really drops a corner by the first-come rule"""
    for direction in (M.P2F, M.F2P):
        res = M.guided_pair(oracle, *pair, radius, 0.8, M.RATIO, direction)
        if M.outcomes(res, direction) != ALL_OUTCOMES:
            return False
    return True


_general = {}


def general_case(oracle, dtype, dim, nf, nc, nt):
    k = (dtype, dim, nf, nc, nt)
    if k not in _general:
        seed0 = 9000 + 1000 * (dtype == "u8") + 7 * dim + nf + 3 * nt
        if (nf, nc, nt) in GENERAL:
            _general[k] = first_seed(lambda s: general_pair(dtype, dim, nf, nc, nt, s), lambda p: has_every_outcome(oracle, p), seed0)
        else:
            _general[k] = general_pair(dtype, dim, nf, nc, nt, seed0)
    return _general[k]


def window_pair(dtype, dim, direction, seed, counts=WINDOW_COUNTS):
    """one query per entry of `counts`, 130 px apart, with exactly that many targets within 30 px of it and nothing else within 100 px"""
    rng = np.random.default_rng(seed)
    n_many = int(sum(counts))
    centres = np.array([[60.0 + 130.0 * k, 100.0 + 60.0 * (k % 2)] for k in range(len(counts))], np.float32)
    ang, rad = rng.random(n_many) * 2 * np.pi, 30.0 * np.sqrt(rng.random(n_many))
    many = (np.repeat(centres, counts, axis=0) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)).astype(np.float32)
    base = fresh(rng, dtype, dim, len(counts))
    near = noisy(rng, np.repeat(base, counts, axis=0))
    perm = rng.permutation(n_many)
    if direction == M.P2F:                                                # the corners are the queries
        return base, np.ascontiguousarray(near[perm]), centres, np.arange(len(counts), dtype=np.int32), np.ascontiguousarray(many[perm])
    cfr = rng.permutation(n_many).astype(np.int32)                        # the corners are the targets; corner c -> from-row cfr[c]
    frm = np.empty_like(near)
    frm[cfr] = near[perm]
    return np.ascontiguousarray(frm), base, np.ascontiguousarray(many[perm]), cfr, centres


def best_behind_first_drain(oracle, pair, direction):
    """per window of more than 64 candidates: does the nearest candidate lie behind the first 64 in index order (found after a drain)?"""
    res = M.guided_pair(oracle, *pair, RADIUS, 0.8, M.NEAREST, direction)
    q_pts, t_pts = (pair[2], pair[4]) if direction == M.P2F else (pair[4], pair[2])
    W = M.windows(q_pts, t_pts, RADIUS)
    return [bool(np.flatnonzero(W[q]).tolist().index(int(res["match"][q])) >= 64) for q in np.flatnonzero(res["count"] > 64)]


_window = {}


def window_case(oracle, dtype, dim, direction):
    """window_pair whose wide windows have their nearest candidate before the first drain in one and behind it in another"""
    k = (dtype, dim, direction)
    if k not in _window:
        _window[k] = first_seed(lambda s: window_pair(dtype, dim, direction, s), lambda p: len(set(best_behind_first_drain(oracle, p, direction))) == 2,
                                300 + dim)
    return _window[k]


def grid_pair(dtype, dim, seed):
    """integer coordinates, radius 5: around each of three corners (100 px apart) the to-points (3, 4), (4, 3), (5, 0), (0, -5), (-3, -4) lie
    at exactly the radius -- outside -- and (3, 3), (-4, 2), (0, 4) inside"""
    rng = np.random.default_rng(seed)
    centres = np.array([[100, 100], [200, 100], [300, 200]], np.float32)
    offs = np.array([[3, 4], [4, 3], [5, 0], [0, -5], [-3, -4], [3, 3], [-4, 2], [0, 4]], np.float32)
    pts = (centres[:, None, :] + offs[None, :, :]).reshape(-1, 2)
    frm = fresh(rng, dtype, dim, 3)
    to = fresh(rng, dtype, dim, pts.shape[0])
    return frm, to, centres, np.array([2, 0, 1], np.int32), np.ascontiguousarray(pts)


def no_fma_pair(dtype, dim, seed, n=1100):
    """four corners with `n` to-points rounded onto the circle of radius 40 around them: d2 lands within a few units in the last place of
    1600 on either side, where one rounding more or less decides"""
    rng = np.random.default_rng(seed)
    corners = (np.array([[150.3, 120.7], [450.1, 130.9], [160.6, 350.2], [440.8, 340.4]]) + rng.random((4, 2))).astype(np.float32)
    ang = rng.random(n) * 2 * np.pi
    which = rng.integers(0, 4, n)
    pts = (corners[which].astype(np.float64) + 40.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)).astype(np.float32)
    frm = fresh(rng, dtype, dim, 4)
    return frm, noisy(rng, frm[which]), corners, np.arange(4, dtype=np.int32), np.ascontiguousarray(pts)


def fma_matters(pair, radius=RADIUS):
    """number of (corner, to-point) whose membership differs between L2_Simple's arithmetic and a fused evaluation"""
    r2 = np.float32(radius) * np.float32(radius)
    return int(((M.window_d2(pair[2], pair[4]) < r2) != (M.window_d2_fused(pair[2], pair[4]) < r2)).sum())


def no_fma_case(dtype, dim):
    return first_seed(lambda s: no_fma_pair(dtype, dim, s), lambda p: fma_matters(p) > 0, 31 + dim)


def tie_pair(dtype, dim, seed, n_clusters=12):
    """clusters 100 px apart; each holds one corner and four to-points within 6 px of it; the to-rows of a cluster are: two
    identical noisy copies of the corner's descriptor (d1 == d2 > 0), or two exact copies of it (d1 == d2 == 0), plus two fresh rows.
    The twins lie at random to-rows."""
    rng = np.random.default_rng(seed)
    centres = np.array([[60.0 + 100.0 * (k % 6), 80.0 + 120.0 * (k // 6)] for k in range(n_clusters)], np.float32)
    frm = fresh(rng, dtype, dim, n_clusters)
    cfr = rng.permutation(n_clusters).astype(np.int32)
    pts, rows = [], []
    for k in range(n_clusters):
        twin = frm[cfr[k]][None] if k % 2 else noisy(rng, frm[cfr[k]][None])
        pts.append(centres[k] + (rng.random((4, 2)) * 8 - 4).astype(np.float32))
        rows.append(np.concatenate([twin, twin, fresh(rng, dtype, dim, 2)]))
    perm = rng.permutation(4 * n_clusters)
    return frm, np.ascontiguousarray(np.concatenate(rows)[perm]), centres, cfr, np.ascontiguousarray(np.concatenate(pts)[perm].astype(np.float32))


def ties(res):
    """(queries whose two best distances are equal and positive, ... equal and zero)"""
    d = res["dist"]
    both = (res["count"] >= 2) & (d[:, 0].view(np.uint32) == d[:, 1].view(np.uint32))
    return int((both & (d[:, 0] > 0)).sum()), int((both & (d[:, 0] == 0)).sum())


def one_row_pair(dtype, dim, seed, nc=70):
    """every corner within 10 px of to-point 2 and far from the two others: each window holds that row alone, corner 0 keeps it"""
    rng = np.random.default_rng(seed)
    pts = np.array([[50, 50], [600, 400], [320, 240]], np.float32)
    corners = (pts[2] + (rng.random((nc, 2)) * 14 - 7)).astype(np.float32)
    frm = fresh(rng, dtype, dim, nc)
    return frm, fresh(rng, dtype, dim, 3), corners, rng.permutation(nc).astype(np.int32), pts


def nan_pair(oracle, dtype, dim):
    """the (300, 280, 300) general pair with every seventh corner and every fifth to-point NaN in x, y or both"""
    frm, to, corners, cfr, pts = [x.copy() for x in general_case(oracle, dtype, dim, 300, 280, 300)]
    corners[3::7, 0] = np.nan
    corners[5::14, 1] = np.nan
    pts[2::5, 1] = np.nan
    pts[4::10, 0] = np.nan
    return frm, to, corners, cfr, pts


def many_tiny_pairs(dtype, dim, n_pairs, seed):
    """n_pairs pairs with 0..6 from-rows, corners and to-rows in a 120 x 90 image (so that windows are not empty); pair 3 has no corners,
    pair 5 no to-rows, pair 7 nothing"""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(n_pairs):
        nf, nt = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        nc = int(rng.integers(0, nf + 1))
        if p == 3:
            nc = 0
        if p == 5:
            nt = 0
        if p == 7:
            nf = nc = nt = 0
        frm, to, corners, cfr, pts = general_pair(dtype, dim, nf, nc, nt, seed + 1 + p)
        scale = np.float32(120.0 / WIDTH)
        out.append((frm, to, corners * scale, cfr, pts * scale))
    return out


def concat(pairs):
    """-> (from, to, corners, corner_from_row, to_points, from_offsets, to_offsets, corner_offsets)"""
    offs = [np.cumsum([0] + [p[k].shape[0] for p in pairs]).astype(np.int64) for k in (0, 1, 2)]
    return (np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]), np.concatenate([p[2] for p in pairs]).astype(np.float32).reshape(-1, 2),
            np.concatenate([p[3] for p in pairs]).astype(np.int32), np.concatenate([p[4] for p in pairs]).astype(np.float32).reshape(-1, 2),
            offs[0], offs[1], offs[2])


def expected_batch(oracle, pairs, radius, nndr, nn_type, direction):
    """the model over every pair, concatenated as the engine's outputs are"""
    res = [M.guided_pair(oracle, *p, radius, nndr, nn_type, direction) for p in pairs]
    out = dict(count=np.concatenate([r["count"] for r in res]), match=np.concatenate([r["match"] for r in res]),
               dist=np.concatenate([r["dist"] for r in res]).reshape(-1, 2))
    out["owner"] = np.concatenate([r["owner"] for r in res]) if direction == M.P2F else None
    return out


# ---------------------------------------------------------------------------------------------------------------- running the engine
CANARY = -7


def run_host(eng, pairs, radius=RADIUS, nndr=0.8, nn_type=M.RATIO, direction=M.P2F, with_dist=True):
    """the batch through lcd_match_guided -> dict like expected_batch's"""
    count, match, dist, owner = eng.match_guided(*concat(pairs), radius=radius, nndr=nndr, nn_type=nn_type, direction=direction, with_dist=with_dist)
    return dict(count=count, match=match, dist=dist, owner=owner)


def run_dev(eng, pairs, radius=RADIUS, nndr=0.8, nn_type=M.RATIO, direction=M.P2F, with_dist=True):
    """the batch through lcd_match_guided_dev on canary-filled outputs, results read back"""
    import torch
    f, t, c, r, p, fo, to, co = concat(pairs)
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (f, t, c, r, p)]
    nq = c.shape[0] if direction == M.P2F else t.shape[0]
    count = torch.full((nq,), CANARY, dtype=torch.int32, device="cuda")
    match = torch.full((nq,), CANARY, dtype=torch.int32, device="cuda")
    dist = torch.full((nq, 2), float(CANARY), dtype=torch.float32, device="cuda") if with_dist else None
    owner = torch.full((t.shape[0],), CANARY, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.match_guided_dev(*d, fo, to, co, count, match, dist, owner, radius=radius, nndr=nndr, nn_type=nn_type, direction=direction)
    eng.synchronize()
    out = dict(count=count.cpu().numpy(), match=match.cpu().numpy(), dist=dist.cpu().numpy() if with_dist else None, owner=owner.cpu().numpy())
    if direction != M.P2F:
        assert (out["owner"] == CANARY).all()                             # frame-to-projected leaves out_to_owner alone
        out["owner"] = None
    return out


def assert_same(got, exp, what=""):
    """indices, counts and distance BITS"""
    np.testing.assert_array_equal(got["count"], exp["count"], err_msg=what + " count")
    np.testing.assert_array_equal(got["match"], exp["match"], err_msg=what + " match")
    if got["dist"] is not None:
        np.testing.assert_array_equal(np.ascontiguousarray(got["dist"], np.float32).view(np.uint32).reshape(-1, 2),
                                      np.ascontiguousarray(exp["dist"], np.float32).view(np.uint32).reshape(-1, 2), err_msg=what + " dist")
    if exp["owner"] is not None:
        np.testing.assert_array_equal(got["owner"], exp["owner"], err_msg=what + " owner")
    else:
        assert got["owner"] is None
