"""Inputs for lcd_estimate_motion_pnp's tests.  A pair is a dict with from_ids, from_xyz [n x 3], to_ids, to_points [n x 2], to_xyz [n x 3] and
what the generator knows about it (the true model R, t that maps from-points into the to-camera, the inlier flags in ascending-id order).
tests/test_motion_pnp_inputs.py proves without a GPU that each input has the property it exists for."""
import numpy as np

import motion_3d_inputs as T3
import motion_pnp_model as M
from motion_3d_inputs import rotation

BATCH_SIZES = (0, 3, 4, 5, 6, 63, 64, 65, 255, 256, 257, 1100)      # correspondences of the pairs of the mixed batch
ITERATIONS = (1, 255, 256, 257, 300)
REFINE = (0, 1, 5)
FX, FY, CX, CY, WIDTH, HEIGHT = 525.0, 525.0, 319.5, 239.5, 640, 480
CAMERA = dict(fx=FX, fy=FY, cx=CX, cy=CY)
CAMERA_SIZED = dict(fx=FX, fy=FY, cx=CX, cy=CY, image_width=WIDTH, image_height=HEIGHT)
LOCAL = np.array([0, 0, 1, 0.1, -1, 0, 0, 0.02, 0, -1, 0, 0.3], np.float32)      # the optical frame on a robot's base: exact in fp32 but for t


def camera(sized=False, local=False):
    d = dict(CAMERA_SIZED if sized else CAMERA)
    if local:
        d["local_transform"] = LOCAL
    return d


def model_camera(d):
    return M.Camera(d["fx"], d["fy"], d["cx"], d["cy"], d.get("image_width", 0), d.get("image_height", 0), d.get("local_transform"))


def scene(rng, m, noise=0.5, depth=(0.5, 10.0), angle=(0.05, 0.5), shift=0.5, pose=None, cam=None):
    """m points seen by the to-camera inside the image at depths `depth`, the from-points P with R P + t = their camera coordinates; pose: (R, t)
    instead of a drawn one; cam: a camera dict whose fx, fy, cx, cy project instead of CAMERA's"""
    if pose is None:
        R = rotation(rng.normal(size=3), rng.uniform(*angle))
        t = rng.uniform(-shift, shift, 3)
    else:
        R, t = np.asarray(pose[0], np.float64), np.asarray(pose[1], np.float64)
    k = CAMERA if cam is None else cam
    z = rng.uniform(depth[0], depth[1], m)
    u, v = rng.uniform(0, WIDTH - 1, m), rng.uniform(0, HEIGHT - 1, m)
    C = np.stack([(u - k["cx"]) / k["fx"] * z, (v - k["cy"]) / k["fy"] * z, z], axis=1)
    P = (C - t) @ R                                                     # R^T (C - t)
    UV = np.stack([u, v], axis=1) + rng.normal(size=(m, 2)) * noise
    return R, t, P, UV, C


def random_pair(rng, m, outliers=0.4, noise=0.5, decoys=True, **kw):
    """m correspondences (exactly: every shared unique id has a finite from-point), a fraction of them outliers (their keypoint is anywhere in
    the image), inside frames that also hold ids of one side only and -- with decoys -- ids that occur twice in one frame and once in the
    other, which take no part, and a shared id whose from-point is not finite.  to_xyz: the to-camera's own 3-D points with 1 % depth noise, a
    tenth of them NaN.  Rows shuffled."""
    R, t, P, UV, C = scene(rng, m, noise, **kw)
    out = rng.random(m) < outliers
    UV[out] = np.stack([rng.uniform(0, WIDTH - 1, int(out.sum())), rng.uniform(0, HEIGHT - 1, int(out.sum()))], axis=1)
    T = C * (1 + rng.normal(size=(m, 1)) * 0.01)
    T[rng.random(m) < 0.1] = np.nan
    pool = rng.permutation(4 * m + 64)[: m + 24].astype(np.int64) - m // 2          # negative ids too: the rule has no sign test
    ids, extra = pool[:m], pool[m:]
    f_ids, f_xyz, t_ids, t_uv, t_xyz = list(ids), list(P), list(ids), list(UV), list(T)
    point = lambda: rng.uniform(-3, 3, 3)
    pixel = lambda: rng.uniform(0, 400, 2)
    for k in range(9 if decoys else 0):
        e = int(extra[k])
        if k < 3:                                                       # only in from
            f_ids.append(e); f_xyz.append(point())
        elif k < 6:                                                     # only in to
            t_ids.append(e); t_uv.append(pixel()); t_xyz.append(point())
        elif k == 6:                                                    # twice in from, once in to
            f_ids += [e, e]; f_xyz += [point(), point()]
            t_ids.append(e); t_uv.append(pixel()); t_xyz.append(point())
        elif k == 7:                                                    # once in from, twice in to
            f_ids.append(e); f_xyz.append(point())
            t_ids += [e, e]; t_uv += [pixel(), pixel()]; t_xyz += [point(), point()]
        else:                                                           # shared and unique, the from-point not finite
            f_ids.append(e); f_xyz.append(np.array([1.0, np.inf, 2.0]))
            t_ids.append(e); t_uv.append(pixel()); t_xyz.append(point())
    pf, pt = rng.permutation(len(f_ids)), rng.permutation(len(t_ids))
    order = np.argsort(ids)
    return dict(from_ids=np.array(f_ids, np.int32)[pf], from_xyz=np.array(f_xyz, np.float32).reshape(-1, 3)[pf],
                to_ids=np.array(t_ids, np.int32)[pt], to_points=np.array(t_uv, np.float32).reshape(-1, 2)[pt],
                to_xyz=np.array(t_xyz, np.float32).reshape(-1, 3)[pt], m=m, R=R, t=t, inlier=(~out)[order], ids=np.sort(ids).astype(np.int32))


def frames(pair, to_xyz=True):
    """the positional arguments of M.estimate / motion_pnp_cpu"""
    return pair["from_ids"], pair["from_xyz"], pair["to_ids"], pair["to_points"], pair["to_xyz"] if to_xyz else None


def true_model(pair):
    return np.concatenate([pair["R"], pair["t"][:, None]], axis=1).reshape(12).astype(np.float32)


def guess_of(model, local=None):
    """the guess whose model is `model` (up to rounding): guess = inverse(model) x inverse(local)"""
    g = M.invert(model)
    return g if local is None else M.compose(g, M.invert(local))


def mixed_batch(seed=21):
    rng = np.random.default_rng(seed)
    return [random_pair(rng, m) for m in BATCH_SIZES]


def all_outlier_pair(seed=22, m=40):
    """no pose explains more than its own sample: the keypoints are independent of the points"""
    return random_pair(np.random.default_rng(seed), m, outliers=1.1)


def behind_pair(seed=23, m=40):
    """every from-point lies behind the camera of the identity guess, and on one line: every triple is collinear, so no hypothesis is valid
    and the guess is the only candidate"""
    p = random_pair(np.random.default_rng(seed), m, outliers=0.0, decoys=False)
    ids = p["from_ids"]
    p["from_xyz"] = np.stack([0.25 * np.arange(m) - 5.0, np.zeros(m), np.full(m, -3.0)], axis=1).astype(np.float32)[np.argsort(np.argsort(ids))]
    return p


def seed_with_invalid_first(m=4, invalid=1):
    """the first seed whose hypotheses 0 .. invalid - 1 find no four distinct indices among m while hypothesis `invalid` does"""
    seed = 0
    while True:
        if all(M.draw4(seed, h, m) is None for h in range(invalid)) and M.draw4(seed, invalid, m) is not None:
            return seed
        seed += 1


# refinement branches, found by searching seeds with the model: (seed, m, outliers, noise, reproj_error, min_inliers, refine_iterations, the word
# the trace must contain)
REFINE_CASES = {
    "few_first": (57, 15, 0.4, 2.0, 2.0, 8, 10, "few"),
    "size_members_few": (0, 61, 0.4, 1.0, 1.0, 4, 10, "members_changed"),
    "converged": (1, 39, 0.4, 2.0, 4.0, 4, 10, "converged"),
    "step_sensitive": (2011, 30, 0.4, 2.0, 2.0, 4, 12, "members_changed"),         # its inlier lists still change between 6 and 7 Gauss-Newton steps
    "oscillating": (5736, 13, 0.0, 1.0, 2.0, 4, 12, "oscillating"),
    "oscillating_guarded": (5736, 13, 0.0, 1.0, 2.0, 6, 12, "converged"),          # :944: no oscillation test before six recorded sizes
}


SHORT_CASES = ("step_sensitive", "oscillating", "oscillating_guarded")


def refine_case(name):
    seed, m, outliers, noise, reproj, min_inliers, refine, _ = REFINE_CASES[name]
    pair = random_pair(np.random.default_rng(seed), m, outliers=outliers, noise=noise, decoys=False)
    return pair, dict(min_inliers=min_inliers, reproj_error=reproj, iterations=20 if name in SHORT_CASES else 60, refine_iterations=refine, seed=seed)


FIXED_BYTES = (256 * 12 + 256 * 27) * 4
LDS_LIMIT = 2 * (8192 + 8192 // 8) * 8
STAGE_CAP = {True: (LDS_LIMIT - FIXED_BYTES) // 32, False: (LDS_LIMIT - FIXED_BYTES) // 20}   # with / without to_xyz: 3360, 5376


def big_pair(seed=25, m=8000, rows=8192, outliers=0.3):
    """`rows` rows on both sides, m correspondences among them, the rest ids of one side only"""
    rng = np.random.default_rng(seed)
    pair = random_pair(rng, m, outliers=outliers, decoys=False)
    out = dict(pair)
    extra = rows - pair["from_ids"].shape[0]
    perm = rng.permutation(rows)
    out["from_ids"] = np.concatenate([pair["from_ids"], (1 << 20) + np.arange(extra, dtype=np.int32)])[perm].astype(np.int32)
    out["from_xyz"] = np.concatenate([pair["from_xyz"], rng.uniform(-3, 3, (extra, 3)).astype(np.float32)])[perm]
    extra = rows - pair["to_ids"].shape[0]
    perm = rng.permutation(rows)
    out["to_ids"] = np.concatenate([pair["to_ids"], (1 << 21) + np.arange(extra, dtype=np.int32)])[perm].astype(np.int32)
    out["to_points"] = np.concatenate([pair["to_points"], rng.uniform(0, 400, (extra, 2)).astype(np.float32)])[perm]
    out["to_xyz"] = np.concatenate([pair["to_xyz"], rng.uniform(-3, 3, (extra, 3)).astype(np.float32)])[perm]
    return out


def concatenate(pairs, to_xyz=True):
    """-> dict(from_ids, from_xyz, from_offsets, to_ids, to_points, to_offsets, to_xyz) of a batch"""
    fo = np.cumsum([0] + [p["from_ids"].shape[0] for p in pairs]).astype(np.int64)
    to = np.cumsum([0] + [p["to_ids"].shape[0] for p in pairs]).astype(np.int64)
    cat = lambda k, shape, dt: np.concatenate([p[k].reshape(shape) for p in pairs] + [np.zeros((0,) + shape[1:], dt)])
    return dict(from_ids=cat("from_ids", (-1,), np.int32), from_xyz=cat("from_xyz", (-1, 3), np.float32), from_offsets=fo,
                to_ids=cat("to_ids", (-1,), np.int32), to_points=cat("to_points", (-1, 2), np.float32), to_offsets=to,
                to_xyz=cat("to_xyz", (-1, 3), np.float32) if to_xyz else None)


def general_position(UV, C):
    """the first four points can carry a hypothesis: the image triangle of the first three covers more than 5 % of the image, and their
    distances from the camera differ pairwise by more than 10 % (depths in a ratio near 1 put the roots of the P3P quartic next to each other)"""
    a, b = UV[1] - UV[0], UV[2] - UV[0]
    area = 0.5 * abs(a[0] * b[1] - a[1] * b[0])
    d = np.linalg.norm(C[:3], axis=1)
    ratios = [d[i] / d[j] for i in range(3) for j in range(3) if i != j]
    return bool(area > 0.05 * WIDTH * HEIGHT and all(abs(r - 1) > 0.1 for r in ratios))


def fit_sets(n=27, seed=78):
    """dict(P, UV0 noise-free, UV1 with 0.5 px noise, R, t, C) inlier sets in general position for the comparison with a float64 fit: 20 to
    650 points at depths 0.5 to 10 m in a 640 x 480 image"""
    rng = np.random.default_rng(seed)
    sets = []
    while len(sets) < n:
        m = int(rng.integers(20, 651))
        R, t, P, UV, C = scene(rng, m, noise=0.0)
        if not general_position(UV, C):
            continue
        sets.append(dict(P=P.astype(np.float32), UV0=UV.astype(np.float32), UV1=(UV + rng.normal(size=(m, 2)) * 0.5).astype(np.float32), R=R, t=t, C=C))
    return sets


# ---------------------------------------------------------------------------------------------------------------------------------------
# Inputs for the places where the kernel's join, layout, hypothesis chunks, minimal solver, fit and covariance change shape
# (tests/test_gpu_motion_pnp_shapes.py).  What a search found is kept as a constant; tests/test_motion_pnp_inputs.py proves each constant and
# each property again with the model.

INT32_MIN, INT32_MAX = T3.INT32_MIN, T3.INT32_MAX
FLIP_GUESS = np.array([1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0], np.float32)    # half a turn about x: every point in front of a camera is behind this one


def model_of_guess_flip():
    return M.model_of_guess(FLIP_GUESS, None)


def exact_pair(seed, m, **kw):
    """m noise-free correspondences without outliers, decoys or NaN rows of to_xyz"""
    pair = random_pair(np.random.default_rng(seed), m, outliers=0.0, noise=0.0, decoys=False, **kw)
    pair["to_xyz"] = true_points(pair)
    return pair


def true_points(pair):
    """per to-row of a pair whose two frames hold the same unique ids: the point's coordinates in the to-camera under the true pose"""
    P = pair["from_xyz"][np.argsort(pair["from_ids"])][np.argsort(np.argsort(pair["to_ids"]))].astype(np.float64)
    return (P @ pair["R"].T + pair["t"]).astype(np.float32)


def sized_pair(seed, m, n_from, n_to, **kw):
    """random_pair's m correspondences (no decoys) inside frames of exactly n_from and n_to rows: the rest are ids of one side only"""
    rng = np.random.default_rng(seed)
    out = dict(random_pair(rng, m, decoys=False, **kw))
    T3.pad_side(rng, out, "from", 1 << 20, n_from, (("from_xyz", -3, 3),))
    T3.pad_side(rng, out, "to", 1 << 21, n_to, (("to_points", 0, 400), ("to_xyz", -3, 3)))
    return out


# ---- A. the join

JOIN_SIZES = ((0, 50), (50, 0), (1, 8192), (8192, 1), (8192, 60), (60, 8192), (255, 257), (257, 255))


def join_size_pairs(seed=51):
    """one pair per entry of JOIN_SIZES, every row of the smaller side a correspondence (at most 60 of them)"""
    return [sized_pair(seed + k, min(nf, nt, 60), nf, nt, outliers=0.2) for k, (nf, nt) in enumerate(JOIN_SIZES)]


def duplicate_run_pairs(seed=52):
    """Six pairs of T3.RUN_ROWS x T3.RUN_ROWS rows over the same ids on both sides, the id frames of motion_3d_inputs.run_id_frames: runs of 2,
    3 and 5 equal ids from sorted position 0, up to the last one and over the positions 63/64, 255/256 and 511/512, the lengths rotating; pairs
    1, 3, 5 are pairs 0, 2, 4 with the id frames exchanged.  An id that runs in one frame stands once in the other, so it is no correspondence;
    every other id is one."""
    rng = np.random.default_rng(seed)
    pairs = []
    for rot in range(3):
        distinct, ids_a, ids_b, carried_a, carried_b = T3.run_id_frames(rng, rot)
        n = len(distinct)
        R, t, P, UV, C = scene(rng, n)
        running = sorted(int(distinct[j]) for j in carried_a + carried_b)
        for f_sorted, t_sorted in ((ids_a, ids_b), (ids_b, ids_a)):
            cols = []
            for ids, sources in ((f_sorted, ((P, -3, 3),)), (t_sorted, ((UV, 0, 400), (C, -3, 3)))):
                j = np.searchsorted(distinct, ids)
                in_run = np.bincount(j, minlength=n)[j] > 1                 # the rows of a run: values of their own each
                perm = rng.permutation(T3.RUN_ROWS)
                side = [ids[perm].astype(np.int32)]
                for X, low, high in sources:
                    x = X[j].copy()
                    x[in_run] = rng.uniform(low, high, (int(in_run.sum()), X.shape[1]))
                    side.append(np.ascontiguousarray(x[perm], dtype=np.float32))
                cols.append(side)
            pairs.append(dict(from_ids=cols[0][0], from_xyz=cols[0][1], to_ids=cols[1][0], to_points=cols[1][1], to_xyz=cols[1][2], running=running,
                              m=n - len(running), R=R, t=t))
    return pairs


def extreme_id_pairs(seed=53):
    """three pairs of T3.EXTREME_ROWS rows, the id lists of motion_3d_inputs.extreme_id_lists.  0: INT32_MIN and INT32_MAX are unique shared
    ids, both correspondences.  1: INT32_MAX twice in `to`, INT32_MIN twice in `from`: neither is.  2: INT32_MAX twice in `from`, INT32_MIN twice
    in `to`: neither is."""
    rng = np.random.default_rng(seed)
    nf, nt = T3.EXTREME_ROWS
    pairs = []
    for case in range(3):
        f_ids, t_ids = T3.extreme_id_lists(rng, case, nf, nt)
        if case == 1:
            f_ids[-1] = INT32_MIN                                       # in the place of an id of this side only
        if case == 2:
            t_ids[-1] = INT32_MIN
        every = sorted(set(f_ids) | set(t_ids))
        R, t, P, UV, C = scene(rng, len(every))
        at = {i: k for k, i in enumerate(every)}
        jf, jt = [at[i] for i in f_ids], [at[i] for i in t_ids]
        pf, pt = rng.permutation(nf), rng.permutation(nt)
        pairs.append(dict(from_ids=np.array(f_ids, np.int64).astype(np.int32)[pf], from_xyz=P[jf].astype(np.float32)[pf],
                          to_ids=np.array(t_ids, np.int64).astype(np.int32)[pt], to_points=UV[jt].astype(np.float32)[pt],
                          to_xyz=C[jt].astype(np.float32)[pt], R=R, t=t))
    return pairs


PREDICATE_ROWS = 600
# the to-frame's sorted position -> the from-point's coordinate that is not finite, and its value: the rows the compaction drops stand on
# either side of the first block edge and in front of the second
PREDICATE_FROM = {255: (0, np.nan), 256: (1, np.inf), 511: (2, -np.inf)}
PREDICATE_KEYPOINT = {100: (0, np.nan), 300: (1, np.inf), 500: (0, -np.inf)}     # -> the keypoint's coordinate: these stay correspondences


def predicate_pair(seed=54):
    """PREDICATE_ROWS x PREDICATE_ROWS rows, every id shared and unique, no outliers.  The from-points of PREDICATE_FROM are non-finite in one
    coordinate only (no correspondence); the keypoints of PREDICATE_KEYPOINT are (a correspondence that no model holds)."""
    rng = np.random.default_rng(seed)
    n = PREDICATE_ROWS
    ids = np.sort(rng.permutation(6 * n)[:n] - 3 * n).astype(np.int32)
    R, t, P, UV, C = scene(rng, n)
    P, UV = P.astype(np.float32), UV.astype(np.float32)
    for k, (c, v) in PREDICATE_FROM.items():
        P[k, c] = v
    for k, (c, v) in PREDICATE_KEYPOINT.items():
        UV[k, c] = v
    pf, pt = rng.permutation(n), rng.permutation(n)
    return dict(from_ids=ids[pf], from_xyz=np.ascontiguousarray(P[pf]), to_ids=ids[pt], to_points=np.ascontiguousarray(UV[pt]),
                to_xyz=np.ascontiguousarray(C.astype(np.float32)[pt]), ids=ids, R=R, t=t)


KEYPOINT_ROWS = {2: (0, np.nan), 5: (1, np.inf), 8: (0, -np.inf)}      # the correspondence (ascending id) -> the keypoint's coordinate and its value
KEYPOINT_KW = dict(min_inliers=4, reproj_error=2.0, iterations=30, refine_iterations=0, variance_median_ratio=4, max_variance=0.0, seed=0)


def keypoint_pair(seed=100):
    """ten noise-free correspondences, three of them with a keypoint that is not finite: under KEYPOINT_KW's seed most hypotheses draw one
    among their three points or as the fourth, and each of those is invalid"""
    pair = exact_pair(seed, 10)
    for k, (c, v) in KEYPOINT_ROWS.items():
        pair["to_points"][pair["to_ids"] == pair["ids"][k], c] = v
    return pair


def join_pairs():
    return join_size_pairs() + duplicate_run_pairs() + extreme_id_pairs() + [predicate_pair()]


# ---- B. the layout

def layout_pairs(to_xyz, seed=55):
    """a staged pair whose stride (m = 150) is far from its rows (8192 x 200), a pair of five correspondences, and the smallest kind of pair
    that is read from the scratch with a stride that is not its correspondences: STAGE_CAP + 4 of 8192 x 5500 rows without to_xyz,
    STAGE_CAP + 1 of 3500 x 8192 rows with"""
    big = sized_pair(seed + 3, STAGE_CAP[True] + 1, 3500, 8192, outliers=0.3) if to_xyz else sized_pair(seed + 2, STAGE_CAP[False] + 4, 8192, 5500, outliers=0.3)
    return [sized_pair(seed, 150, 8192, 200, outliers=0.2), random_pair(np.random.default_rng(seed + 1), 5, outliers=0.0, decoys=False), big]


# ---- C. the hypothesis chunks

CHUNK_KW = dict(min_inliers=3, reproj_error=2.0, refine_iterations=0, variance_median_ratio=4, max_variance=0.0)
TIE_ITERATIONS = (255, 256, 257, 511, 512, 65534, 65535)              # 65536 candidates are 256 whole chunks; 65535 end in a chunk of 255
TIE_SEED = 7


def tie_pair():
    """40 noise-free correspondences without outliers: nearly every hypothesis holds all of them"""
    return random_pair(np.random.default_rng(5), 40, outliers=0, noise=0, decoys=False)


# Sixteen draws among 40 leave fewer than four distinct values with a probability below 1e-17, so no seed makes a hypothesis of tie_pair()
# invalid; among m = 4 it is 4 % of all hypotheses.  (m, invalid, seed, the pair's seed): seed = seed_with_invalid_first(m, invalid)
TIE_INVALID_FIRST = (4, 2, 1355, 6)


def tie_small_pair():
    m, _, _, pair_seed = TIE_INVALID_FIRST
    return random_pair(np.random.default_rng(pair_seed), m, outliers=0, noise=0, decoys=False)


LATE_ROWS, LATE_INLIERS = 24, 5


def late_winner_pair(seed=56):
    """LATE_ROWS correspondences, LATE_INLIERS of them noise-free under one pose, the keypoints of the others uniform in the image: a hypothesis
    holds all five only when its three points are among them"""
    rng = np.random.default_rng(seed)
    m = LATE_ROWS
    R, t, P, UV, C = scene(rng, m, noise=0.0)
    inlier = np.zeros(m, bool)
    inlier[rng.permutation(m)[:LATE_INLIERS]] = True
    UV[~inlier] = np.stack([rng.uniform(0, WIDTH - 1, m - LATE_INLIERS), rng.uniform(0, HEIGHT - 1, m - LATE_INLIERS)], axis=1)
    ids = np.arange(1, m + 1, dtype=np.int32)
    pf, pt = rng.permutation(m), rng.permutation(m)
    return dict(from_ids=ids[pf], from_xyz=P.astype(np.float32)[pf], to_ids=ids[pt], to_points=UV.astype(np.float32)[pt],
                to_xyz=C.astype(np.float32)[pt], m=m, R=R, t=t, inlier=inlier, ids=ids)


LATE_GAP = 519                                                        # the hypotheses in front of the winner when it is the last of 520


def stream_counts(pair, first, n):
    """the counts of the hypotheses at the stream positions first .. first + n - 1 (draw4 mixes seed + h: position = seed + h)"""
    return M.estimate(*frames(pair), guess=FLIP_GUESS, iterations=n, seed=first, **CHUNK_KW)["counts"][1:]


def find_late_winner(pair, start=0, block=4000):
    """the first stream position >= start + LATE_GAP whose hypothesis holds LATE_INLIERS, which no hypothesis at the LATE_GAP positions in
    front of it equals or exceeds, with a hypothesis that holds something at the 254 positions in front of it: what wins when the winner is
    cut off"""
    first = start
    while True:
        counts = stream_counts(pair, first, block)
        for w in np.nonzero(counts == LATE_INLIERS)[0]:
            if w >= LATE_GAP and counts[w - LATE_GAP:w].max() < LATE_INLIERS and counts[w - 254:w].max() > 0:
                return first + int(w)
        first += block - LATE_GAP


LATE_POSITION = 3265                                                  # find_late_winner(late_winner_pair())
# (the winning candidate c, iterations): the last of chunk 0, the first and second of chunk 1, the last of chunk 1, the first of chunk 2, and
# the very last candidate (c = iterations) of a partial chunk
LATE_CASES = ((255, 600), (256, 600), (257, 600), (511, 600), (512, 600), (520, 520))


def late_kw(c, iterations):
    """candidate c is hypothesis c - 1"""
    return dict(CHUNK_KW, iterations=iterations, seed=(LATE_POSITION - (c - 1)) & M.M32)


# ---- D. the minimal solver on degenerate geometry

SOLVER_KW = dict(min_inliers=4, reproj_error=2.0, iterations=30, refine_iterations=0, variance_median_ratio=4, max_variance=0.0, seed=9)


def _seen(points, ids=None, keypoints=None):
    """a pair whose from-points are `points` in the to-camera's own frame (the true pose is the identity) and whose keypoints are their
    projections by CAMERA, rounded once; keypoints: {index: (u, v)} instead"""
    C = np.asarray(points, np.float64)
    UV = np.stack([FX * C[:, 0] / C[:, 2] + CX, FY * C[:, 1] / C[:, 2] + CY], axis=1)
    for k, uv in (keypoints or {}).items():
        UV[k] = uv
    ids = np.arange(1, len(C) + 1, dtype=np.int32) if ids is None else np.asarray(ids, np.int32)
    return dict(from_ids=ids, from_xyz=C.astype(np.float32), to_ids=ids.copy(), to_points=UV.astype(np.float32), to_xyz=C.astype(np.float32), m=len(C),
                R=np.eye(3), t=np.zeros(3))


SOLVER_RANDOM = (4, 5, 6, 6, 5, 4)
FAR_KEYPOINT_SEED = 82                                                # of 80 .. 89, the first whose winner would be another one if the last solution found were kept


def solver_pairs(seed=57):
    """name -> pair of 4 to 6 correspondences: the degenerate geometries, and SOLVER_RANDOM generic pairs beside them"""
    pairs = {
        "collinear": _seen([[-1, 0, 4], [0, 0, 4], [1, 0, 4], [0.5, 1, 2], [-0.75, -0.5, 3]]),          # rows 0, 1, 2: area2 = 0 exactly
        "coincident": _seen([[0.5, 0.25, 2], [0.5, 0.25, 2], [-1, 0.5, 4], [1, -1, 3], [-0.5, -0.75, 5]]),
        "equidistant": _seen([[1, 0, 4], [-1, 0, 4], [0, 1, 4], [0.5, -0.5, 2], [-1.5, 0.5, 6]]),         # rows 0, 1, 2: |C|^2 = 17
        "principal": _seen([[0, 0, 3], [1, 0.5, 4], [-1, 1, 5], [0.5, -1, 2], [-0.5, -0.25, 6], [1.5, 1, 7]]),   # row 0's keypoint is (cx, cy)
        "plane": _seen([[-1, -1, 4], [1, -0.5, 4], [0.5, 1, 4], [-0.75, 0.5, 4], [0.25, -0.25, 4], [1.5, 1.25, 4]]),
        # row 3 lies on the camera's side of the fronto-parallel triangle of rows 0, 1, 2 and five times its depth away from it: behind the
        # camera under every solution of that triple, so a hypothesis whose fourth point it is has none; its keypoint is anywhere
        "behind": _seen([[-1, -0.5, 4], [1, -0.25, 4], [0.25, 1, 4], [0, 0, -20]], keypoints={3: (100.0, 50.0)}),
        "line": _seen([[-1, 0, 4], [0, 0, 4], [1, 0, 4], [2, 0, 4]]),          # every triple: area2 = 0 exactly, no hypothesis at all
    }
    # a keypoint so far outside any image that the fourth point's error has the same bits under every solution: the first found is kept
    far = exact_pair(FAR_KEYPOINT_SEED, 6)
    far["to_points"][far["to_ids"] == far["ids"][-1]] = np.array([1e18, -1e18], np.float32)
    pairs["far_keypoint"] = far
    rng = np.random.default_rng(seed)
    for k, m in enumerate(SOLVER_RANDOM):
        pairs["random_%d" % k] = random_pair(rng, m, outliers=0, noise=0.2, decoys=False)
    return pairs


def hypotheses(pair, cam, seed, iterations):
    """the minimal solver on every valid draw of a pair -> (h [H], valid [H], solutions as M.p3p returns them)"""
    _, P, UV, _ = M.correspondences(*frames(pair))
    draws = [M.draw4(seed, h, len(P)) for h in range(iterations)]
    hs = [h for h, d in enumerate(draws) if d is not None]
    idx = np.array([draws[h] for h in hs]).T
    has, _, solutions = M.p3p(P[idx[:3]], M.bearing(cam, UV[idx[:3]]), P[idx[3]], UV[idx[3]], cam)
    return np.array(hs), has, solutions


def winning_cells(solutions):
    """per hypothesis the (pass, bracket) cell 0 .. 7 whose solution the solver keeps (the smallest error, the first on ties), -1 for none;
    and the number of valid solutions"""
    ok = np.stack([s[0] for s in solutions])
    e = np.stack([s[2] for s in solutions]).astype(np.float64)
    e[~ok] = np.inf
    return np.where(ok.any(axis=0), np.argmin(e, axis=0), -1), ok.sum(axis=0)


# ---- E. the fit

SHEPPERD_KW = dict(min_inliers=6, reproj_error=2.0, iterations=100, refine_iterations=3, variance_median_ratio=4, max_variance=0.0)
SHEPPERD_SEEDS = {1: (8, 36), 2: (81, 128), 3: (9, 20)}                  # the case every fit takes -> two seeds of shepperd_pair


def shepperd_pair(seed):
    """60 correspondences under a rotation by 3.0 to 3.14: the trace is negative"""
    return random_pair(np.random.default_rng(seed), 60, decoys=False, angle=(3.0, 3.14))


# rotations that are exact in fp32 -> the case Shepperd's rule takes and the pivot it takes it with
EXACT_ROTATIONS = (
    ([[1, 0, 0], [0, -1, 0], [0, 0, -1]], 1, 4.0),
    ([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], 2, 4.0),
    ([[-1, 0, 0], [0, -1, 0], [0, 0, 1]], 3, 4.0),
    ([[0, 1, 0], [1, 0, 0], [0, 0, -1]], 1, 2.0),                       # cases 1 and 2 tie
    ([[0, 0, 1], [1, 0, 0], [0, 1, 0]], 0, 1.0),                        # all four tie
)
EXACT_SHIFT = (0.25, -0.5, 0.125)
EXACT_KW = dict(SHEPPERD_KW, iterations=1, refine_iterations=1)


def exact_rotation_pairs(seed=58):
    return [exact_pair(seed + k, 60, pose=(np.array(R, np.float64), np.array(EXACT_SHIFT))) for k, (R, _, _) in enumerate(EXACT_ROTATIONS)]


# A tie between exact pivots cannot show: the tied cases give the same quaternion.  Half a turn less 0.04 about an axis with two equal
# components has two equal diagonal entries, in fp32 too, so two pivots tie near 2 while the other entries are rounded: (axis, the case the
# rule takes, the case that ties with it).  The case that >= in the place of > would take ends in other transform bits for TIED_SEED.
TIED_ROTATIONS = (((1, 1, 0.3), 1, 2), ((0.3, 1, 1), 2, 3), ((1, 0.3, 1), 1, 3))
TIED_ANGLE, TIED_SEED = 3.1, 90


def tied_rotation_pairs():
    return [exact_pair(TIED_SEED, 60, pose=(rotation(axis, TIED_ANGLE), np.array(EXACT_SHIFT))) for axis, _, _ in TIED_ROTATIONS]


LANE_SIZES = (255, 256, 257, 512, 513)
LANE_KW = dict(SHEPPERD_KW, min_inliers=4, iterations=20, refine_iterations=2, seed=4)


def lane_pair(m):
    """m noise-free correspondences without outliers: every fit's set is all of them"""
    return exact_pair(60 + m, m)


LATE_MEMBERS_KW = dict(min_inliers=4, reproj_error=2.0, iterations=60, refine_iterations=10, variance_median_ratio=4, max_variance=0.0)


LATE_MEMBERS_EXACT, LATE_MEMBERS_NOISY = 300, 200


def late_members_pair(seed):
    """LATE_MEMBERS_EXACT noise-free correspondences under the lowest ids, which every selection holds, and LATE_MEMBERS_NOISY under the
    highest whose keypoints lie 1.95 to 2.05 px beside their projections, on either side of the threshold: what enters or leaves a selection
    does so behind position 300.  (Errors spread evenly below the threshold would shrink the refined threshold, three standard deviations,
    pass by pass until only the exact rows are left; two clusters keep it at reproj_error.)"""
    rng = np.random.default_rng(seed)
    m = LATE_MEMBERS_EXACT + LATE_MEMBERS_NOISY
    R, t, P, UV, C = scene(rng, m, noise=0.0)
    turn, radius = rng.uniform(0, 2 * np.pi, LATE_MEMBERS_NOISY), rng.uniform(1.95, 2.05, LATE_MEMBERS_NOISY)
    UV[LATE_MEMBERS_EXACT:] += np.stack([radius * np.cos(turn), radius * np.sin(turn)], axis=1)
    ids = np.arange(1, m + 1, dtype=np.int32)
    pf, pt = rng.permutation(m), rng.permutation(m)
    return dict(from_ids=ids[pf], from_xyz=P.astype(np.float32)[pf], to_ids=ids[pt], to_points=UV.astype(np.float32)[pt],
                to_xyz=C.astype(np.float32)[pt], m=m, R=R, t=t, ids=ids)


def find_late_members(seeds=range(200)):
    """the seeds whose refinement has a members_changed pass -> [(seed, the first differing index of each)]"""
    found = []
    for s in seeds:
        r = M.estimate(*frames(late_members_pair(s)), seed=s, **LATE_MEMBERS_KW)
        if r["first_differing"]:
            found.append((s, r["first_differing"]))
    return found


LATE_MEMBERS = {3: [306, 305], 4: [329]}                              # of find_late_members(range(5)): seed -> the first differing index per members_changed pass

REFUSED_KW = dict(SHEPPERD_KW, min_inliers=4, iterations=10, refine_iterations=2, seed=1)


def refused_pair(n=6):
    """n copies of one point on the optical axis and its keypoint, the principal point, under n ids: every triple is coincident, the identity
    guess holds all n, and the fit's 6 x 6 system has an exact zero on its diagonal"""
    return _seen([[0, 0, 4]] * n)


# ---- F. the covariance

RATIO_SIZES = (4, 5, 255, 256, 257)
RATIOS = (2, 3, 4, 5, 6, 255, 256, 257, 258, (1 << 31) - 1)           # 2, 3, n and n + 1 of every size, and the largest int


def ratio_pair(n):
    return lane_pair(n) if n in LANE_SIZES else exact_pair(60 + n, n)


def negative_cosine_pair(seed=70):
    """60 noise-free correspondences; to_xyz is the negated true point on 80 % of the rows"""
    pair = exact_pair(seed, 60)
    flip = np.random.default_rng(seed + 1).permutation(60) < 48
    pair["to_xyz"][flip] = -pair["to_xyz"][flip]
    return pair


def nonfinite_to_pair(seed=71):
    """60 noise-free correspondences; every row of to_xyz is NaN, +inf or -inf in one coordinate or NaN in all"""
    pair = exact_pair(seed, 60)
    for k in range(60):
        if k % 4 == 3:
            pair["to_xyz"][k] = np.nan
        else:
            pair["to_xyz"][k, k % 4] = (np.nan, np.inf, -np.inf)[k % 4]
    return pair


ZERO_POSE_SHIFT = (0.25, -0.125, 2.0)


def zero_point_pair(seed=72):
    """40 noise-free correspondences; the from-point of the smallest id is exactly (0, 0, 0): the camera sees it at t"""
    rng = np.random.default_rng(seed)
    t = np.array(ZERO_POSE_SHIFT)
    pair = exact_pair(seed, 40, pose=(rotation(rng.normal(size=3), 0.3), t))
    i = pair["ids"][0]
    pair["from_xyz"][pair["from_ids"] == i] = 0.0
    pair["to_points"][pair["to_ids"] == i] = np.array([FX * t[0] / t[2] + CX, FY * t[1] / t[2] + CY], np.float32)
    pair["to_xyz"][pair["to_ids"] == i] = t.astype(np.float32)
    return pair


def raw_cosine(P, N):
    """dot / (|P| |N|) as the rule rounds it, before its clamps"""
    P, N = np.asarray(P, np.float32), np.asarray(N, np.float32)
    dot = (P[:, 0] * N[:, 0] + P[:, 1] * N[:, 1]) + P[:, 2] * N[:, 2]
    pp = (P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2]
    qq = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
    return dot / (np.sqrt(pp) * np.sqrt(qq))


def clamp_pair(sign, seed=74, n=20):
    """n points seen under the identity, which the identity guess holds and no refinement moves, whose to_xyz is the point itself (sign 1)
    or its negative (sign -1): only points are kept whose product of two rounded lengths is below the rounded dot product, so every raw
    cosine lies beyond +-1 by a unit in the last place"""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-2, 2, 40 * n), rng.uniform(-1.5, 1.5, 40 * n), rng.uniform(1, 8, 40 * n)], axis=1).astype(np.float32)
    P = P[np.abs(raw_cosine(P, np.float32(sign) * P)) > 1][:n]
    assert len(P) == n
    pair = _seen(P)
    pair["to_xyz"] = np.float32(sign) * P
    return pair


# cameras that all differ: a principal point that is not positive in x, y or both with odd and degenerate image sizes, fx != fy, fy < 0
CAMERA_CASES = (dict(fx=525.0, fy=525.0, cx=0.0, cy=0.0, image_width=641, image_height=479),
                dict(fx=525.0, fy=525.0, cx=-3.0, cy=240.0, image_width=640, image_height=481),
                dict(fx=525.0, fy=525.0, cx=320.0, cy=-1.0, image_width=1, image_height=1),
                dict(fx=500.0, fy=540.0, cx=319.5, cy=239.5, image_width=640, image_height=480),
                dict(fx=525.0, fy=-525.0, cx=319.5, cy=239.5, image_width=640, image_height=480))
CAMERA_UNSIZED = dict(fx=525.0, fy=525.0, cx=0.0, cy=239.5)           # with to_xyz: the rows that are NaN take the ray with ccx = -0.5


def camera_pairs(seed=73):
    """one pair of 40 correspondences per camera of CAMERA_CASES, its scene built for that camera"""
    return [random_pair(np.random.default_rng(seed + k), 40, outliers=0.2, decoys=False, cam=cam) for k, cam in enumerate(CAMERA_CASES)]


def camera_unsized_pair(seed=79):
    pair = random_pair(np.random.default_rng(seed), 40, outliers=0.2, decoys=False, cam=CAMERA_UNSIZED)
    pair["to_xyz"][::2] = np.nan
    return pair


def float32_neighbours(x):
    """the largest float32 below the double x and the smallest above it"""
    f = np.float32(x)
    lo = f if np.float64(f) < x else np.nextafter(f, np.float32(-np.inf))
    hi = f if np.float64(f) > x else np.nextafter(f, np.float32(np.inf))
    return float(lo), float(hi)


# ---- the calls: what tests/test_gpu_motion_pnp_shapes.py sends to both entries and tests/test_motion_pnp_model.py to the host mirror

BASE_KW = dict(min_inliers=6, reproj_error=2.0, iterations=300, refine_iterations=5, variance_median_ratio=4, max_variance=0.0, seed=3)
JOIN_KW = dict(BASE_KW, min_inliers=4, iterations=50, refine_iterations=2, seed=1)
LAYOUT_KW = dict(BASE_KW, min_inliers=4, iterations=32, refine_iterations=2, seed=8)
COV_KW = dict(BASE_KW, iterations=40, refine_iterations=2)
CLAMP_KW = dict(COV_KW, min_inliers=4, iterations=1, refine_iterations=0)      # the identity guess wins and stays
_made = {}


def made(name, *args):
    """a generator's result, built once per process: the tests cache the model's results per pair object"""
    if (name,) + args not in _made:
        _made[(name,) + args] = globals()[name](*args)
    return _made[(name,) + args]


def _call(pairs, kw, cam=CAMERA, guesses=None, to_xyz=True):
    return dict(pairs=list(pairs), kw=kw, cam=cam, guesses=None if guesses is None else np.stack(guesses), to_xyz=to_xyz)


def max_variance_bounds():
    """the float32 neighbours of the variance that negative_cosine's pair ends with"""
    pair = made("negative_cosine_pair")
    r = M.estimate(*frames(pair), camera=model_camera(CAMERA), **COV_KW)
    assert r["status"] == M.OK
    return float32_neighbours(r["variance_lin"])


# the sections of shape_calls(): every call is filed under exactly one
SHAPE_SECTIONS = ("join", "keypoints", "layout", "tie", "late", "cut", "solver", "shepperd", "exact_rotations", "lanes", "late_members", "refused", "ratio",
                  "negative_cosine", "nonfinite_to", "zero_point", "clamps", "camera", "max_variance")


def section_calls(section, calls=None):
    calls = shape_calls() if calls is None else calls
    return {name: c for name, c in calls.items() if c["section"] == section}


def shape_calls():
    """name -> dict(section, pairs, kw, cam, guesses, to_xyz), in the order of the sections A .. F"""
    calls = {}

    def add(section, name, call):
        assert section in SHAPE_SECTIONS and name not in calls
        calls[name] = dict(call, section=section)

    for to_xyz in (True, False):
        add("join", "join_%d" % to_xyz, _call(made("join_pairs"), JOIN_KW, to_xyz=to_xyz))
    add("keypoints", "keypoints", _call([made("keypoint_pair")], KEYPOINT_KW, guesses=[FLIP_GUESS]))
    for to_xyz in (True, False):
        pairs = made("layout_pairs", to_xyz)
        add("layout", "layout_%d_forward" % to_xyz, _call(pairs, LAYOUT_KW, to_xyz=to_xyz))
        add("layout", "layout_%d_reverse" % to_xyz, _call(pairs[::-1], LAYOUT_KW, to_xyz=to_xyz))
    tie, small = made("tie_pair"), made("tie_small_pair")
    for it in TIE_ITERATIONS:
        add("tie", "tie_%d" % it, _call([tie], dict(CHUNK_KW, iterations=it, seed=TIE_SEED), guesses=[FLIP_GUESS]))
    add("tie", "tie_guess", _call([tie], dict(CHUNK_KW, iterations=257, seed=TIE_SEED), guesses=[guess_of(true_model(tie))]))
    add("tie", "tie_invalid_first", _call([small], dict(CHUNK_KW, iterations=257, seed=TIE_INVALID_FIRST[2]), guesses=[FLIP_GUESS]))
    late = made("late_winner_pair")
    for c, it in LATE_CASES:
        add("late", "late_%d" % c, _call([late], late_kw(c, it), guesses=[FLIP_GUESS]))
        add("cut", "cut_%d" % c, _call([late], late_kw(c, c - 1), guesses=[FLIP_GUESS]))
    solver = list(made("solver_pairs").values())
    add("solver", "solver", _call(solver, SOLVER_KW, guesses=[FLIP_GUESS] * len(solver)))
    for pick, seeds in sorted(SHEPPERD_SEEDS.items()):
        for s in seeds:
            add("shepperd", "shepperd_%d_%d" % (pick, s), _call([made("shepperd_pair", s)], dict(SHEPPERD_KW, seed=s)))
    exact = made("exact_rotation_pairs")
    for local in (False, True):
        cam = made("camera", True, local)
        add("exact_rotations", "exact_rotations_%d" % local,
            _call(exact, EXACT_KW, cam=cam, guesses=[guess_of(true_model(p), cam.get("local_transform")) for p in exact]))
    tied = made("tied_rotation_pairs")
    add("exact_rotations", "exact_rotations_tied", _call(tied, EXACT_KW, guesses=[guess_of(true_model(p)) for p in tied]))
    add("lanes", "lanes", _call([made("lane_pair", m) for m in LANE_SIZES], LANE_KW))
    for s in sorted(LATE_MEMBERS):
        add("late_members", "late_members_%d" % s, _call([made("late_members_pair", s)], dict(LATE_MEMBERS_KW, seed=s)))
    add("refused", "refused", _call([made("refused_pair")], REFUSED_KW))
    for ratio in RATIOS:
        add("ratio", "ratio_%d" % ratio, _call([made("ratio_pair", n) for n in RATIO_SIZES], dict(LANE_KW, variance_median_ratio=ratio)))
    add("negative_cosine", "negative_cosine", _call([made("negative_cosine_pair")], COV_KW))
    add("nonfinite_to", "nonfinite_to", _call([made("nonfinite_to_pair")], COV_KW))
    add("zero_point", "zero_point", _call([made("zero_point_pair")], COV_KW))
    add("clamps", "clamps", _call([made("clamp_pair", 1), made("clamp_pair", -1)], CLAMP_KW))
    add("camera", "cameras", _call(made("camera_pairs"), COV_KW, cam=list(CAMERA_CASES), to_xyz=False))
    add("camera", "camera_unsized", _call([made("camera_unsized_pair")], COV_KW, cam=CAMERA_UNSIZED))
    below, above = made("max_variance_bounds")
    add("max_variance", "max_variance_below", _call([made("negative_cosine_pair")], dict(COV_KW, max_variance=below)))
    add("max_variance", "max_variance_above", _call([made("negative_cosine_pair")], dict(COV_KW, max_variance=above)))
    return calls
