"""Inputs of the lcd_register_icp_plane tests: 3-D scans with normals, the hand-made cases of every branch of the rule, and the batches of the
GPU tests.  tests/test_register_icp_plane_inputs.py proves with tests/register_icp_plane_model.py that each case takes its branch."""
import numpy as np

from register_icp_inputs import F, IDENTITY, bits, motion, inverse, moved  # noqa: F401

SIZES = (0, 1, 2, 3, 5, 6, 7, 255, 256, 257, 511, 512, 513)
KW = dict(max_iterations=30, max_correspondence_distance=0.3, epsilon=0.0, correspondence_ratio=0.1, min_complexity=0.02, low_complexity_strategy=1)
BOARD = np.array([-0.5, -2.0 / 3.0, 1.0]) / np.linalg.norm([-0.5, -2.0 / 3.0, 1.0])


def room(rng, n):
    """n points of register_icp_inputs.room_3d's scene -- a room's corner and a slanted board -- and the normals of their surfaces"""
    which = rng.integers(0, 4, n)
    u, v = rng.uniform(0, 4, n), rng.uniform(0, 3, n)
    P, N = np.zeros((n, 3)), np.zeros((n, 3))
    planes = (np.column_stack([u, v, np.zeros(n)]), np.column_stack([u, np.zeros(n), v]), np.column_stack([np.zeros(n), u, v]),
              np.column_stack([1 + 0.5 * u, 1 + 0.3 * v, 0.5 + 0.25 * u + 0.2 * v]))
    normals = ([0, 0, 1.0], [0, 1.0, 0], [1.0, 0, 0], BOARD)
    for k in range(4):
        P[which == k] = planes[k][which == k]
        N[which == k] = normals[k]
    return P, N


def corridor(rng, n, floor=0.0, end=0.0):
    """two long walls facing each other; a share `floor` of the points on the floor and `end` on the end wall"""
    u, v, w = rng.uniform(0, 8, n), rng.uniform(0, 2.5, n), rng.uniform(-1, 1, n)
    side = rng.integers(0, 2, n)
    P = np.column_stack([u, np.where(side == 0, -1.0, 1.0), v])
    N = np.column_stack([np.zeros(n), np.where(side == 0, 1.0, -1.0), np.zeros(n)])
    kind = rng.uniform(0, 1, n)
    on_floor, on_end = kind < floor, (kind >= floor) & (kind < floor + end)
    P[on_floor] = np.column_stack([u, w, np.zeros(n)])[on_floor]
    N[on_floor] = [0, 0, 1.0]
    P[on_end] = np.column_stack([np.full(n, 8.0), w, v])[on_end]
    N[on_end] = [-1.0, 0, 0]
    return P, N


def pair(n_from, n_to, seed, noise=0.0, scene=room, angle=0.04, shift=0.08, guess_off=False, normal_noise=0.0, **scene_kw):
    """from = the scene, to = inverse(truth)(the scene sampled again), the normals in each scan's own frame; out_transform should be truth"""
    rng = np.random.default_rng(seed)
    truth = motion(rng, False, angle, shift)
    (frm, nf), (to, nt) = scene(rng, n_from, **scene_kw), scene(rng, n_to, **scene_kw)
    if noise:
        frm, to = frm + rng.normal(0, noise, frm.shape), to + rng.normal(0, noise, to.shape)
    if normal_noise:
        nf, nt = nf + rng.normal(0, normal_noise, nf.shape), nt + rng.normal(0, normal_noise, nt.shape)
        nf, nt = nf / np.linalg.norm(nf, axis=1, keepdims=True), nt / np.linalg.norm(nt, axis=1, keepdims=True)
    inv = inverse(truth)
    guess = IDENTITY.copy() if not guess_off else np.hstack([truth[:, :3], (truth[:, 3] + np.array([0.02, -0.01, 0.01]))[:, None]]).astype(np.float32).reshape(12)
    return dict(from_xyz=frm.astype(np.float32).reshape(-1, 3), from_normals=nf.astype(np.float32).reshape(-1, 3), to_xyz=moved(inv, to).reshape(-1, 3),
                to_normals=(nt @ inv[:, :3].T).astype(np.float32).reshape(-1, 3), guess=guess, truth=truth)


def raw(frm, nf, to, nt, guess=None):
    a = lambda x: np.array(x, np.float32).reshape(-1, 3)
    return dict(from_xyz=a(frm), from_normals=a(nf), to_xyz=a(to), to_normals=a(nt), guess=IDENTITY.copy() if guess is None else np.asarray(guess, np.float32).reshape(12))


def scans(p):
    return p["from_xyz"], p["from_normals"], p["to_xyz"], p["to_normals"], p["guess"]


def changed(p, **arrays):
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    q.update(arrays)
    return q


def concatenate(pairs):
    """-> from_xyz, from_normals, from_offsets, to_xyz, to_normals, to_offsets, guesses of the batch"""
    z = [np.zeros((0, 3), np.float32)]
    cat = lambda k: np.concatenate([p[k] for p in pairs] + z)
    fo = np.concatenate([[0], np.cumsum([p["from_xyz"].shape[0] for p in pairs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([p["to_xyz"].shape[0] for p in pairs])]).astype(np.int64)
    return cat("from_xyz"), cat("from_normals"), fo, cat("to_xyz"), cat("to_normals"), to, np.stack([p["guess"] for p in pairs]).astype(np.float32)


def with_nan_normals(p, rows_from=(255, 256, 511), rows_to=(255, 256, 511)):
    """the pair with the normals of the rows given made NaN, +inf, -inf in turn, in one component each"""
    q = changed(p)
    bad = (np.nan, np.inf, -np.inf)
    for k, r in enumerate(rows_from):
        q["from_normals"][r, k % 3] = bad[k % 3]
    for k, r in enumerate(rows_to):
        q["to_normals"][r, (k + 1) % 3] = bad[(k + 1) % 3]
    return q


def only_normals(p, n_kept):
    """the pair with all but the first n_kept normals of either side NaN: oi = n_kept"""
    q = changed(p)
    q["from_normals"][n_kept:] = np.nan
    q["to_normals"][n_kept:] = np.nan
    return q


def flipped(p, rows):
    """the pair with the from-normals of `rows` negated: their correspondences fail any gate with a positive cosine; no fit reads a from-normal"""
    q = changed(p)
    q["from_normals"][rows] = -q["from_normals"][rows]
    return q


def hand_cases():
    """name -> (pair, keyword arguments)"""
    c = {}
    base = pair(300, 280, 11, noise=0.004)
    c["plane"] = (base, dict(KW))
    c["plane_guess_far"] = (pair(300, 300, 12, noise=0.004, guess_off=True), dict(KW))
    c["plane_swapped"] = (pair(320, 250, 13, noise=0.004), dict(KW))             # the from-side is the target of step 5
    c["plane_3dof"] = (base, dict(KW, force_3dof=True))
    c["plane_stop_iterations"] = (base, dict(KW, max_iterations=2))
    c["plane_stop_transform"] = (base, dict(KW, epsilon=1e-3))
    c["plane_max_laser_scans"] = (base, dict(KW, max_laser_scans=600))
    c["plane_below_ratio"] = (base, dict(KW, correspondence_ratio=0.99))
    c["plane_noisy_normals"] = (pair(300, 280, 14, noise=0.004, normal_noise=0.05), dict(KW))
    # every normal the same: complexity 0 exactly, no vectors
    flat = pair(300, 280, 15, noise=0.004, scene=corridor)
    flat["from_normals"][:], flat["to_normals"][:] = [0, 1, 0], [0, 1, 0]
    for s in (0, 1, 2):
        c["corridor_exact_strategy_%d" % s] = (flat, dict(KW, low_complexity_strategy=s))
    c["corridor_exact_3dof"] = (flat, dict(KW, force_3dof=True))
    c["parallel_normals_singular"] = (flat, dict(KW, min_complexity=0.0))
    # walls, a little floor and a trace of an end wall: 0 < complexity < 0.02, the second value on either side of min_complexity
    low = pair(400, 380, 16, noise=0.004, scene=corridor, floor=0.12, end=0.004)
    for s in (0, 1, 2):
        c["corridor_strategy_%d" % s] = (low, dict(KW, low_complexity_strategy=s))
    c["corridor_second_below"] = (low, dict(KW, min_complexity=0.5))
    c["corridor_3dof"] = (low, dict(KW, force_3dof=True))
    # the 2 oi quirk: one finite normal a side is no PCA, two are the smallest one
    c["one_normal"] = (only_normals(base, 1), dict(KW))
    c["two_normals"] = (only_normals(base, 2), dict(KW))
    c["no_normal"] = (only_normals(base, 0), dict(KW, low_complexity_strategy=2))
    # the same normals on both sides but for the sign of x: equal complexities, different vectors
    same = changed(base, to_xyz=base["from_xyz"].copy(), to_normals=base["from_normals"] * np.array([-1, 1, 1], np.float32))
    c["equal_complexities"] = (same, dict(KW, min_complexity=1.0, low_complexity_strategy=1))
    # the gate
    cos = float(np.cos(0.78))
    c["gate_on"] = (pair(300, 280, 14, noise=0.004, normal_noise=0.05), dict(KW, normal_gate=True, min_normal_cos=cos))
    c["gate_fails_among_the_first"] = (flipped(base, np.arange(80)), dict(KW, normal_gate=True, min_normal_cos=cos))
    c["gate_fails_swapped"] = (flipped(pair(320, 250, 13, noise=0.004), np.arange(80)), dict(KW, normal_gate=True, min_normal_cos=cos))
    c["gate_count_1"] = (flipped(base, np.arange(300) != 17), dict(KW, normal_gate=True, min_normal_cos=cos, correspondence_ratio=0.0))
    c["gate_count_2"] = (flipped(base, ~np.isin(np.arange(300), [17, 90])), dict(KW, normal_gate=True, min_normal_cos=cos, correspondence_ratio=0.0))
    c["gate_count_0"] = (flipped(base, np.arange(300)), dict(KW, normal_gate=True, min_normal_cos=cos, correspondence_ratio=0.0))
    return c


def complexity_edge(model):
    """(pair, kw, the pair's complexity c): min_complexity = c is branch 0, the next float above it the low-complexity path"""
    p, kw = hand_cases()["corridor_strategy_1"]
    return p, kw, model.register(*scans(p), **kw)["complexity"]


def gate_edge(model):
    """(pair, kw, a cosine d of one of its reciprocal correspondences): min_normal_cos = d fails that correspondence, the float below passes it"""
    p, kw = hand_cases()["gate_on"]
    r = model.register(*scans(p), **kw)
    dots = np.unique(r["reciprocal_dots"])
    return p, kw, dots[len(dots) // 2]


# ---- the GPU batches

def size_batch():
    """every size of SIZES on the from-side against a neighbour of it on the to-side, and the other way round"""
    out = []
    for k, n in enumerate(SIZES):
        other = SIZES[(k + 3) % len(SIZES)]
        out.append(pair(n, max(other, 7) if n else other, 100 + k, noise=0.004))
        out.append(pair(max(other, 7), n, 200 + k, noise=0.004))
    return out
