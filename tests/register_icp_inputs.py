"""Inputs of the lcd_register_icp tests: scans with structure (so that ICP has something to hold on to), small known motions, the hand-made
cases of every branch of the rule, and the batches of the GPU tests.  tests/test_register_icp_inputs.py proves the properties the cases rely
on with tests/register_icp_model.py."""
import numpy as np

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
SIZES = (0, 1, 2, 3, 255, 256, 257, 511, 512, 513)                 # the lane order of SUM, the tile and block edges
KW = dict(max_iterations=30, max_correspondence_distance=0.3, epsilon=0.0, correspondence_ratio=0.1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def motion(rng, flat, angle=0.04, shift=0.08):
    """a small rigid motion as a 3 x 4 in float64"""
    if flat:
        a = rng.uniform(-angle, angle)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        t = np.array([rng.uniform(-shift, shift), rng.uniform(-shift, shift), 0.0])
    else:
        w = rng.uniform(-angle, angle, 3)
        th = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        t = rng.uniform(-shift, shift, 3)
    return np.hstack([R, t[:, None]])


def inverse(T):
    R, t = T[:, :3], T[:, 3]
    return np.hstack([R.T, (-R.T @ t)[:, None]])


def moved(T, P):
    return (np.asarray(P, np.float64) @ T[:, :3].T + T[:, 3]).astype(np.float32)


def room_2d(rng, n):
    """n points of a laser scan (z = 0): an L-shaped room's walls, sampled along the perimeter"""
    corners = np.array([[-4, -3], [5, -3], [5, 1], [1, 1], [1, 4], [-4, 4], [-4, -3]], np.float64)
    seg = np.diff(corners, axis=0)
    length = np.linalg.norm(seg, axis=1)
    s = np.sort(rng.uniform(0, length.sum(), n))
    k = np.minimum(np.searchsorted(np.cumsum(length), s), len(length) - 1)
    along = (s - np.concatenate([[0], np.cumsum(length)])[k]) / length[k]
    xy = corners[k] + seg[k] * along[:, None]
    return np.column_stack([xy, np.zeros(n)])


def room_3d(rng, n):
    """n points of a 3-D cloud: a room's corner (three planes) and a slanted board in it"""
    which = rng.integers(0, 4, n)
    u, v = rng.uniform(0, 4, n), rng.uniform(0, 3, n)
    P = np.zeros((n, 3))
    P[which == 0] = np.column_stack([u, v, np.zeros(n)])[which == 0]
    P[which == 1] = np.column_stack([u, np.zeros(n), v])[which == 1]
    P[which == 2] = np.column_stack([np.zeros(n), u, v])[which == 2]
    P[which == 3] = np.column_stack([1 + 0.5 * u, 1 + 0.3 * v, 0.5 + 0.25 * u + 0.2 * v])[which == 3]
    return P


def pair(n_from, n_to, flat, seed, noise=0.0, guess_off=False, angle=0.04, shift=0.08):
    """a pair whose out_transform should be `truth`: from = the scene, to = inverse(truth)(the scene sampled again), a guess near truth or the identity"""
    rng = np.random.default_rng(seed)
    scene = room_2d if flat else room_3d
    truth = motion(rng, flat, angle, shift)
    frm, to = scene(rng, n_from), scene(rng, n_to)
    if noise:
        sigma = np.array([noise, noise, 0.0 if flat else noise])
        frm, to = frm + rng.normal(0, 1, frm.shape) * sigma, to + rng.normal(0, 1, to.shape) * sigma
    guess = IDENTITY.copy() if not guess_off else np.hstack([truth[:, :3], (truth[:, 3] + np.array([0.02, -0.01, 0.0]))[:, None]]).astype(np.float32).reshape(12)
    return dict(from_xyz=frm.astype(np.float32).reshape(-1, 3), to_xyz=moved(inverse(truth), to).reshape(-1, 3), guess=guess, truth=truth, flat=flat)


def scans(p):
    return p["from_xyz"], p["to_xyz"], p["guess"]


def concatenate(pairs):
    """-> from_xyz, from_offsets, to_xyz, to_offsets, guesses of the batch"""
    fx = np.concatenate([p["from_xyz"] for p in pairs] + [np.zeros((0, 3), np.float32)])
    tx = np.concatenate([p["to_xyz"] for p in pairs] + [np.zeros((0, 3), np.float32)])
    fo = np.concatenate([[0], np.cumsum([p["from_xyz"].shape[0] for p in pairs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([p["to_xyz"].shape[0] for p in pairs])]).astype(np.int64)
    return fx, fo, tx, to, np.stack([p["guess"] for p in pairs]).astype(np.float32)


def raw(frm, to, guess=None, flat=False):
    return dict(from_xyz=np.asarray(frm, np.float32).reshape(-1, 3), to_xyz=np.asarray(to, np.float32).reshape(-1, 3),
                guess=IDENTITY.copy() if guess is None else np.asarray(guess, np.float32).reshape(12), flat=flat)


# ---- the hand-made cases: name -> (pair, keyword arguments beyond force_3dof)

GRID3 = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1]]


def _near(points, d):
    return (np.asarray(points, np.float64) + d).tolist()


def hand_cases():
    c = {}
    # a source row in the middle of two targets (rows 1 and 0 at the same d2: row 0 wins), and a doubled target point (rows 2 and 3)
    c["ties"] = (raw([[0, 0, 0], [5, 0, 0], [5, 5, 0], [0, 5.25, 0]], [[-1, 0, 0], [1, 0, 0], [5, 0.25, 0], [5, 0.25, 0], [5, 5, 0], [0, 5, 0]]),
                 dict(max_iterations=1, max_correspondence_distance=2.0))
    # d2 = 0.25 exactly against thr2 = 0.25: a correspondence; one ulp more: none (then only two are left)
    to3 = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
    c["d2_at_thr2"] = (raw([[0.5, 0, 0], [4, 0.5, 0], [0, 4.5, 0]], to3), dict(max_iterations=1, max_correspondence_distance=0.5))
    above = float(np.nextafter(F(0.5), F(1)))
    c["d2_above_thr2"] = (raw([[above, 0, 0], [4, 0.5, 0], [0, 4.5, 0]], to3), dict(max_iterations=1, max_correspondence_distance=0.5))
    c["two_correspondences"] = (raw([[0.1, 0, 0], [4, 0.1, 0], [9, 9, 9]], to3), dict(max_correspondence_distance=0.5))
    c["three_correspondences"] = (raw([[0.1, 0, 0], [4, 0.1, 0], [0, 4.1, 0], [9, 9, 9]], to3), dict(max_correspondence_distance=0.5))
    # three correspondences that no rigid motion serves: the fit pushes one of them out of reach
    c["falls_below_three"] = (raw([[0.45, 0, 0], [3.55, 0, 0], [0, 4.45, 0]], to3), dict(max_correspondence_distance=0.5))
    c["stop_iterations"] = (pair(300, 300, False, 11), dict(KW, max_iterations=2))
    c["max_iterations_1"] = (pair(300, 300, False, 11), dict(KW, max_iterations=1))
    c["stop_transform"] = (pair(300, 300, False, 11), dict(KW, epsilon=1e-3))
    c["stop_mse"] = (pair(300, 300, True, 12, noise=0.005), dict(KW))
    same = room_3d(np.random.default_rng(5), 200)
    c["identical_clouds"] = (raw(same, same), dict(KW))
    same2 = room_2d(np.random.default_rng(6), 200)
    c["identical_clouds_2d"] = (raw(same2, same2, flat=True), dict(KW))
    # 2-D with every correspondence's source at one point: A = B = 0, a pure translation
    c["a_b_zero"] = (raw([[0.1, 0.1, 0]] * 3 + [[9, 9, 0]], [[0, 0, 0], [4, 0, 0], [0, 4, 0]], flat=True), dict(max_iterations=1, max_correspondence_distance=0.2))
    for name, nf, nt in (("swap_less", 200, 300), ("swap_equal", 250, 250), ("swap_more", 300, 200)):
        c[name] = (pair(nf, nt, True, 21, noise=0.005), dict(KW))
    # five kept correspondences of six rows: the ratio 5 / 10 against 0.5 (refused at equality), against the next float below, and relative
    six = _near(GRID3, 0.01) + [[9, 9, 9]]
    c["ratio_at_equality"] = (raw(six, GRID3), dict(max_correspondence_distance=0.2, max_laser_scans=10, correspondence_ratio=0.5))
    c["ratio_above"] = (raw(six, GRID3), dict(max_correspondence_distance=0.2, max_laser_scans=10, correspondence_ratio=float(np.nextafter(F(0.5), F(0)))))
    c["ratio_relative"] = (raw(six, GRID3), dict(max_correspondence_distance=0.2, max_laser_scans=0, correspondence_ratio=0.5))
    c["guess_far"] = (pair(300, 280, False, 31, guess_off=True), dict(KW))
    c["huge_coordinates"] = (raw([[3e38, 0, 0], [0, 3e38, 0], [1, 1, 1], [2, 2, 2]], [[3e38, 0, 0], [-3e38, 0, 0], [1, 1, 1]]), dict(max_correspondence_distance=1e10))
    return c


def epsilon_pair(model):
    """(epsilon, the float below it, the iteration the larger one stops at): the transform test of step 6 decided by one float.  `model` is
    tests/register_icp_model.py; the pair is stop_mse's, run without an epsilon to see every T_k."""
    p, kw = hand_cases()["stop_mse"]
    r = model.register(*scans(p), **kw)
    k = len(r["models"]) - 2                                           # an iteration before the last: nothing else stops there
    T = r["models"][k]
    t2 = (T[3] * T[3] + T[7] * T[7]) + T[11] * T[11]
    eps = F(np.sqrt(t2))
    while eps * eps < t2:
        eps = np.nextafter(eps, F(1))
    while np.nextafter(eps, F(0)) * np.nextafter(eps, F(0)) >= t2:
        eps = np.nextafter(eps, F(0))
    return float(eps), float(np.nextafter(eps, F(0))), k + 1


# ---- the GPU batches

def size_batch(flat):
    """every size of SIZES on the from-side against a neighbour of it on the to-side, and the other way round: the empty and the tiny pairs
    stand between full ones"""
    out = []
    for k, n in enumerate(SIZES):
        other = SIZES[(k + 5) % len(SIZES)]
        out.append(pair(n, max(other, 3) if n else other, flat, 100 + k, noise=0.004))
        out.append(pair(max(other, 3), n, flat, 200 + k, noise=0.004))
    return out


def with_non_finite(p, rows_from=(255, 256, 511), rows_to=(255, 256, 511)):
    """the pair with the rows given made non-finite (NaN, +inf, -inf in turn, in one coordinate each)"""
    q = dict(p, from_xyz=p["from_xyz"].copy(), to_xyz=p["to_xyz"].copy())
    bad = (np.nan, np.inf, -np.inf)
    for k, r in enumerate(rows_from):
        q["from_xyz"][r, k % 3] = bad[k % 3]
    for k, r in enumerate(rows_to):
        q["to_xyz"][r, (k + 1) % 3] = bad[(k + 1) % 3]
    return q


# ---- where the grid form of the search can go wrong.  GRID_THR = 0.25 makes the cell exact: h = 0.25 x 1.0625 = 0.265625

GRID_THR = 0.25
GRID_KW = dict(max_iterations=3, max_correspondence_distance=GRID_THR, correspondence_ratio=0.0)


def grid_edge_pairs():
    """name -> pair.  Each is searched in the grid form under LCD_ICP_SEARCH_GRID except where the name says what falls back."""
    h, d = 0.265625, GRID_THR
    rng = np.random.default_rng(3)
    out = {}
    one = rng.uniform(0.1 * h, 0.9 * h, (40, 3))
    out["one_cell"] = raw(np.concatenate([one[:25] + rng.normal(0, 0.02, (25, 3)), one[:5] + [3 * h, 0, 0]]), one)
    k = np.arange(-2, 3) * h
    corners = np.array([[x, y, z] for x in k for y in k for z in k])
    corners[corners == 0] = -0.0
    steps = np.array([[d, 0, 0], [-d, 0, 0], [0, d, 0], [0, 0, -d], [0.14, 0.14, 0.14], [-0.14, 0.14, -0.14], [0, 0, 0]]) * 0.99
    out["faces_and_corners"] = raw(np.concatenate([corners[rng.permutation(len(corners))[:12]] + s for s in steps]), corners)
    e = 0.05
    out["diagonal_neighbour"] = raw([[h - e, h - e, h - e], [2 * h - e, h - e, -e], [-h + e, -e, h - e], [0.5 * h, 0.5 * h, 0.5 * h]],
                                    [[0.1 * h, 0.1 * h, 0.1 * h], [h + e, h + e, h + e], [2 * h + e, h + e, -2 * e], [-h - e, e, h + e], [0.5 * h, 0.5 * h, 0.4 * h]])
    # a row on the face between two cells, a target an eighth to either side of it (exact): the same d2 in two cells, the lower row wins
    c = np.array([[1 * h, 0.1, 0.1], [-2 * h, 0.1, 0.1], [0.1, 3 * h, 0.1], [0.1, 0.1, -1 * h]])
    ax = np.array([[1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]) * 0.125
    out["equal_across_cells"] = raw(c, np.concatenate([np.stack([a + b, a - b]) for a, b in zip(c, ax)] + [np.stack([a - b, a + b]) for a, b in zip(c + [0, 5 * h, 0], ax)]))
    out["equal_across_cells"]["from_xyz"] = np.concatenate([out["equal_across_cells"]["from_xyz"], (c + [0, 5 * h, 0]).astype(np.float32)])
    g = np.arange(-3, 4) * d
    flat = np.array([[x, y, 0.0] for x in g for y in g])
    flat[flat == 0] = -0.0
    rows = np.concatenate([flat[rng.permutation(len(flat))[:30]] + [d / 2, 0, 0], flat[:20] + [d / 2, d / 2, 0], flat[5:25] + [0, d / 2, 0], flat[::3]])
    out["flat_nine_cells"] = raw(rows, flat, flat=True)
    out["one_point_off_the_plane"] = raw(rows, np.concatenate([flat, [[0.0, 0.0, d]]]))
    out["flat_swapped"] = raw(flat, rows, flat=True)
    far = 70000 * h
    out["target_beyond_the_range_falls_back"] = raw(one[:20] + 0.01, np.concatenate([one, [[far, 0, 0], [0, -far, 0]]]))
    out["row_beyond_the_range_walks_the_target"] = raw(np.concatenate([one[:20] + 0.01, [[far, 0, 0], [0.1, 0.1, -far], [65534.5 * h, 0, 0]]]), one)
    out["edge_of_the_range"] = raw(np.concatenate([one[:10] + 0.01, [[65534 * h + 0.1, 0.1, 0.1], [-65534.9 * h, 0, 0]]]),
                                   np.concatenate([one, [[65534 * h + 0.05, 0.1, 0.1], [-65534.9 * h + 0.03, 0, 0]]]))
    return out
