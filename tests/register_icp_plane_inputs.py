"""Inputs of the lcd_register_icp_plane tests: 3-D scans with normals, the hand-made cases of every branch of the rule, and the batches of the
GPU tests, among them the cases at block, batch and region edges.  tests/test_register_icp_plane_inputs.py proves with
tests/register_icp_plane_model.py that each case takes its branch."""
import numpy as np

from register_icp_inputs import F, IDENTITY, GRID_KW, bits, motion, inverse, moved  # noqa: F401
from register_icp_inputs import grid_edge_pairs as _p2p_grid_edge_pairs

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


# ---- the branches at block, batch and region edges.  Every generator builds its pairs once: the same objects come back on every call, so that
# a cache keyed by the pair serves every test of a module.

EDGE_SIZES = (255, 256, 257, 511, 512, 513, 1025)
GATE_COS = float(np.cos(0.78))
GATE_KW = dict(KW, normal_gate=True, min_normal_cos=GATE_COS)
_built = {}


def _once(name, make):
    if name not in _built:
        _built[name] = make()
    return _built[name]


def swapped(p):
    """the pair with its sides exchanged; the guess has to be the identity, which it stays"""
    assert np.array_equal(p["guess"], IDENTITY)
    return changed(p, from_xyz=p["to_xyz"].copy(), from_normals=p["to_normals"].copy(), to_xyz=p["from_xyz"].copy(), to_normals=p["from_normals"].copy())


def low_complexity_sizes():
    """name -> (pairs, kw).  Corridor pairs -- walls, a little floor and a trace of an end wall -- with a from-side of every EDGE_SIZES against a
    to-side 20 rows smaller, and each of them with its sides exchanged: 0 < complexity < min_complexity, so under strategies 1 and 2 the
    point-to-point loop runs inside the plane kernel and completes.  The same pairs with min_complexity = 0.5 (the second value below it too),
    under strategy 2 and with force_3dof; and one pair of 513 x 493 rows whose normals are all [0, 1, 0]: complexity 0 exactly, no vectors"""
    def make():
        pairs = []
        for n in EDGE_SIZES:
            p = pair(n, n - 20, 300 + n, noise=0.004, scene=corridor, floor=0.12, end=0.01)
            pairs += [p, swapped(p)]
        flat = changed(pairs[10])
        assert (flat["from_xyz"].shape[0], flat["to_xyz"].shape[0]) == (513, 493)
        flat["from_normals"][:], flat["to_normals"][:] = [0, 1, 0], [0, 1, 0]
        return dict(strategy_1=(pairs, dict(KW)), second_below=(pairs, dict(KW, min_complexity=0.5)), strategy_2=(pairs, dict(KW, low_complexity_strategy=2)),
                    force_3dof=(pairs, dict(KW, force_3dof=True)), exact_zero=([flat], dict(KW)))
    return _once("low", make)


def gate_sizes():
    """(pairs, kw): room pairs with noisy normals at the sizes of low_complexity_sizes(), both ways round, the gate on; every fifth from-normal
    is negated, so failing correspondences stand between passing ones in every trip of 256 source rows -- source rows are from-rows where
    nf <= nt, and to-rows, whose from-row carries the negated normal, where nf > nt"""
    def make():
        pairs = []
        for n in EDGE_SIZES:
            p = pair(n, n - 20, 400 + n, noise=0.004, normal_noise=0.05)
            pairs += [flipped(p, np.arange(0, n, 5)), flipped(swapped(p), np.arange(0, n - 20, 5))]
        return pairs, dict(GATE_KW)
    return _once("gate", make)


def swap_turned_by_normals():
    """([300 x 280 with every fourth from-normal NaN, its mirror image], kw): 225 rows take part against 280, so the from-side is step 5's
    source although it has more rows; in the mirror image 280 rows stand against 225 and the to-side is the source although it has more.
    Reciprocity and the gate's cosine are symmetric in the two sides, so neither out_match nor the count depends on which side is the source;
    what does is the variance under the gate once a correspondence fails -- the median is taken over the first `count` reciprocal
    correspondences in the SOURCE's row order.  Hence the gate is on, and the normals of the rows 1, 5, 9, ... of the same side are negated"""
    def make():
        p = pair(300, 280, 11, noise=0.004)
        p["from_normals"][::4] = np.nan
        p["from_normals"][1::4] *= np.float32(-1)
        return [p, swapped(p)], dict(GATE_KW)
    return _once("swap", make)


def _mostly_elsewhere(p, kept):
    """the pair with all but the first `kept` from-rows moved 100 m away: they find nothing, and the ratio falls below 0.1"""
    q = changed(p)
    q["from_xyz"][kept:, 0] += np.float32(100)
    return q


def mixed_batch():
    """{strategy: (pairs, kw)} for the strategies 0 and 1, the same pairs in the same order.  (branch, status) per pair:

        pair                                   strategy 0                strategy 1
        room 513 x 257                         (0, OK)                   (0, OK)
        corridor 400 x 380                     (0, LOW_COMPLEXITY)       (1, OK)
        0 x 7 rows                             (0, LOW_COMPLEXITY)       (1, EMPTY)
        room 300 x 280, 25 rows in reach       (0, BELOW_RATIO)          (0, BELOW_RATIO)
        room 1030 x 700                        (0, OK)                   (0, OK)
        corridor 257 x 237                     (0, LOW_COMPLEXITY)       (1, OK)
        room 256 x 300, 100 m apart            (0, NOT_CONVERGED)        (0, NOT_CONVERGED)
        corridor 300 x 280, 25 rows in reach   (0, LOW_COMPLEXITY)       (1, BELOW_RATIO)
        corridor 512 x 492, 100 m apart        (0, LOW_COMPLEXITY)       (1, NOT_CONVERGED)
        room 255 x 275                         (0, OK)                   (0, OK)

    A side without rows has no normals and the complexity 0: under strategy 0 the empty pair returns early as the corridors do, and EMPTY is not
    reachable there through the host entry (a side of which no row takes part has no finite normal).  The largest pair stands in the middle:
    the stride and the LDS size of every other workgroup are not its own."""
    def make():
        cor = dict(noise=0.004, scene=corridor, floor=0.12, end=0.01)
        apart = lambda p: changed(p, to_xyz=p["to_xyz"] + np.float32(100))
        pairs = [pair(513, 257, 601, noise=0.004), pair(400, 380, 602, **cor), pair(0, 7, 603), _mostly_elsewhere(pair(300, 280, 604, noise=0.004), 25),
                 pair(1030, 700, 605, noise=0.004), pair(257, 237, 606, **cor), apart(pair(256, 300, 607, noise=0.004)),
                 _mostly_elsewhere(pair(300, 280, 608, **cor), 25), apart(pair(512, 492, 609, **cor)), pair(255, 275, 610, noise=0.004)]
        return {0: (pairs, dict(KW, low_complexity_strategy=0)), 1: (pairs, dict(KW, low_complexity_strategy=1))}
    return _once("mixed", make)


MIXED = {0: [(0, 0), (0, 4), (0, 4), (0, 3), (0, 0), (0, 4), (0, 2), (0, 4), (0, 4), (0, 0)],
         1: [(0, 0), (1, 0), (1, 1), (0, 3), (0, 0), (1, 0), (0, 2), (1, 3), (1, 2), (0, 0)]}         # (branch, status) as the docstring lists them


def padded(p, region):
    """the pair as lcd_filter_scans_dev leaves it: each side in the first rows of a region of `region` rows, quiet NaNs behind, in coordinates
    and normals alike"""
    q = changed(p)
    for k in ("from_xyz", "from_normals", "to_xyz", "to_normals"):
        a = np.full((region, 3), np.nan, np.float32)
        a[:p[k].shape[0]] = p[k]
        q[k] = a
    return q


def padded_regions():
    """[(region, padded pairs, the same pairs without the padding, kw)].  Regions of 1 024 rows hold 900 x 880 and 1 023 x 1 000 points: the
    sort is sized by the region, and AUTO, which counts the rows that take part, stays brute.  Regions of 2 048 rows hold 1 100 x 1 080 points
    (AUTO takes the grid form) and 600 x 1 030 (brute towards the from-side, grid towards the to-side)"""
    def make():
        out = []
        for region, sizes, kw in ((1024, ((900, 880), (1023, 1000)), dict(KW)), (2048, ((1100, 1080), (600, 1030)), dict(KW, max_iterations=3))):
            plain = [pair(nf, nt, 700 + nf, noise=0.004) for nf, nt in sizes]
            out.append((region, [padded(p, region) for p in plain], plain, kw))
        return out
    return _once("padded", make)


def spun_normals(n, phase):
    """n unit normals, each a function of its row index alone, no two neighbours alike"""
    i = np.arange(n, dtype=np.float64)
    a, b = 0.7 * i + phase, 0.3 * i
    return np.column_stack([np.cos(a), np.sin(a) * np.cos(b), np.sin(a) * np.sin(b)]).astype(np.float32).reshape(-1, 3)


GRID_EDGE_KW = dict(GRID_KW, min_complexity=0.0, low_complexity_strategy=1)
GRID_EDGE_ONCE_KW = dict(GRID_EDGE_KW, max_iterations=1)                   # the first fit goes straight to the outputs
GRID_CELL = 0.265625                                                       # the cell of register_icp_inputs.GRID_THR, exact


def grid_edge_pairs():
    """name -> register_icp_inputs.grid_edge_pairs()'s 3-D pairs with spun_normals on both sides: the normal fit_plane reads is that of the
    row the search found, so a wrong row changes the sums.  With min_complexity = 0 every pair takes branch 0.  diagonal_neighbour has four
    from-rows, too few for the six unknowns of the plane fit: it stays, as diagonal_neighbour_singular, and diagonal_neighbour is three copies
    of it, eight cells apart along x and along y"""
    def make():
        with_normals = lambda f, t, g=None: raw(f, spun_normals(f.shape[0], 0.4), t, spun_normals(t.shape[0], 1.3), g)
        out = {}
        for name, p in _p2p_grid_edge_pairs().items():
            if not p["flat"]:
                out[name] = with_normals(p["from_xyz"], p["to_xyz"], p["guess"])
        four = out["diagonal_neighbour_singular"] = out["diagonal_neighbour"]
        steps = np.array([[0, 0, 0], [8 * GRID_CELL, 0, 0], [0, 8 * GRID_CELL, 0]], np.float32)
        out["diagonal_neighbour"] = with_normals(np.concatenate([four["from_xyz"] + s for s in steps]), np.concatenate([four["to_xyz"] + s for s in steps]))
        return out
    return _once("grid_edges", make)


def non_finite_coordinates():
    """600 x 600 rows (brute under AUTO) and 1 100 x 1 100 (grid) with rows 255, 256 and 511 of the from-side and 255 and 511 of the to-side not
    finite in a coordinate, and the latter with two more from-rows and seven of every eight to-rows NaN: the region asks for the grid form,
    the rows that take part do not, and the from-side becomes step 5's target -- device entry only"""
    def make():
        out = []
        for n in (600, 1100):
            q = pair(n, n, 800 + n, noise=0.004)
            q["from_xyz"][[255, 256, 511], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
            q["to_xyz"][[255, 511], [1, 2]] = [np.nan, np.inf]
            out.append(q)
        few = changed(out[1])
        few["from_xyz"][[3, 1099], [0, 2]] = np.nan
        few["to_xyz"][np.arange(1100) % 8 != 5, 1] = np.nan
        out.append(few)
        return out
    return _once("non_finite", make)


def rows_8192():
    """(corridor 8192 x 8100, room 8192 x 8000 with noisy normals and every fifth from-normal negated, a 257 x 513 room pair to stand between
    them, kw): max_iterations = 2 and the gate on, which the low-complexity branch does not read"""
    def make():
        low = pair(8192, 8100, 901, noise=0.004, scene=corridor, floor=0.12, end=0.01)
        gate = flipped(pair(8192, 8000, 902, noise=0.003, normal_noise=0.05), np.arange(0, 8192, 5))
        return low, gate, pair(257, 513, 903, noise=0.004), dict(GATE_KW, max_iterations=2)
    return _once("8192", make)


FILTER_KW = dict(voxel_size=0.15, normal_k=8)
FILTER_REGION = 2048


def filter_chain():
    """(pair, the filter's kw, the region size): two room scans of 3 000 and 2 900 points that a voxel grid of FILTER_KW's leaf brings to between
    1 100 and 1 900 points a scan, in regions of 2 048 rows; the ICP over them runs with max_iterations = 3"""
    return _once("chain", lambda: (pair(3000, 2900, 905, noise=0.004), dict(FILTER_KW), FILTER_REGION))
