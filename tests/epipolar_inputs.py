"""Inputs of the lcd_verify_epipolar tests: two-view scenes from one recipe, and hand-made pairs that each take one branch of the rule
(test_epipolar_inputs.py proves that they do).  A pair is a dict(from_ids, from_points, to_ids, to_points[, planted])."""
import numpy as np

FX = FY = 525.0
CX, CY = 319.5, 239.5
WIDTH, HEIGHT = 640, 480
K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]])
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def _rotation(angles):
    ax, ay, az = angles
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return rz @ ry @ rx


def _line_distance(Fm, p, q):
    """the distance of q from the line Fm p, both [n x 2]"""
    ph = np.concatenate([p, np.ones((p.shape[0], 1))], 1)
    line = ph @ Fm.T
    return np.abs((line[:, :2] * q).sum(1) + line[:, 2]) / np.sqrt((line[:, :2] ** 2).sum(1))


def scene(seed, m, outliers=0.4, noise=0.5, planar=False, extra=5, shuffle=True):
    """A 640 x 480 pinhole (fx = fy = 525), 3-D points at depths uniform in 1 .. 8 m (planar: all at 4 m), a rotation of up to +-12 degrees per
    axis, a translation of up to +-0.4 m per axis, `noise` px Gaussian noise on both keypoints, a fraction `outliers` of the to-keypoints
    replaced by positions at least 30 px from the true epipolar line in BOTH images (`planted`: their ids); `extra` unpaired rows per frame."""
    rng = np.random.default_rng(seed)
    R = _rotation(np.deg2rad(rng.uniform(-12, 12, 3)))
    t = rng.uniform(-0.4, 0.4, 3)
    t[np.argmax(np.abs(t))] = np.sign(t[np.argmax(np.abs(t))] or 1.0) * max(np.abs(t).max(), 0.15)    # a baseline worth the name
    p = np.stack([rng.uniform(0, WIDTH, m), rng.uniform(0, HEIGHT, m)], 1)
    z = np.full(m, 4.0) if planar else rng.uniform(1.0, 8.0, m)
    P = np.stack([(p[:, 0] - CX) / FX * z, (p[:, 1] - CY) / FY * z, z], 1)
    Q = P @ R.T + t
    q = np.stack([FX * Q[:, 0] / Q[:, 2] + CX, FY * Q[:, 1] / Q[:, 2] + CY], 1)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Fm = np.linalg.inv(K).T @ tx @ R @ np.linalg.inv(K)                    # q^T Fm p = 0
    pn, qn = p + rng.normal(0, noise, p.shape), q + rng.normal(0, noise, q.shape)
    n_out = int(round(outliers * m))
    planted_rows = []
    for r in rng.permutation(m):                                           # a from-keypoint within 30 px of the epipole cannot be planted: every line passes it
        if len(planted_rows) == n_out:
            break
        cand = np.stack([rng.uniform(0, WIDTH, 64), rng.uniform(0, HEIGHT, 64)], 1)
        far = (_line_distance(Fm, np.repeat(pn[r:r + 1], 64, 0), cand) >= 30.0) & (_line_distance(Fm.T, cand, np.repeat(pn[r:r + 1], 64, 0)) >= 30.0)
        if far.any():
            qn[r] = cand[np.argmax(far)]
            planted_rows.append(int(r))
    assert len(planted_rows) == n_out
    planted_rows = np.array(planted_rows, np.int64)
    ids = rng.choice(100000, m + 2 * extra, replace=False).astype(np.int32)
    from_ids = np.concatenate([ids[:m], ids[m:m + extra]])
    to_ids = np.concatenate([ids[:m], ids[m + extra:]])
    from_points = np.concatenate([pn, rng.uniform(0, HEIGHT, (extra, 2))]).astype(np.float32)
    to_points = np.concatenate([qn, rng.uniform(0, HEIGHT, (extra, 2))]).astype(np.float32)
    if shuffle:
        a, b = rng.permutation(m + extra), rng.permutation(m + extra)
        from_ids, from_points, to_ids, to_points = from_ids[a], from_points[a], to_ids[b], to_points[b]
    return dict(from_ids=from_ids, from_points=from_points, to_ids=to_ids, to_points=to_points, planted=set(int(i) for i in ids[planted_rows]))


def accuracy_scenes():
    """the twelve scenes of the accuracy test: m from 60 to 300"""
    return [scene(1000 + k, int(m)) for k, m in enumerate(np.linspace(60, 300, 12))]


def frames(pair):
    return pair["from_ids"], pair["from_points"], pair["to_ids"], pair["to_points"]


def with_m(m, seed=7):
    """a clean scene with exactly m pairs"""
    return scene(seed, m, outliers=0.0, extra=3)


def id_cases():
    """One pair whose ids are negative, doubled in one frame, doubled in both, INT32_MAX and INT32_MIN beside twelve ordinary ones;
    `expect_matches`: the ids that take part, ascending"""
    s = scene(11, 12, outliers=0.0, extra=0, shuffle=False)
    rng = np.random.default_rng(5)
    extra_from = np.array([-3, -7, 500001, 500001, 500002, 500003, 500003, INT32_MAX, INT32_MIN, 500004], np.int32)
    extra_to = np.array([-3, -7, 500001, 500002, 500002, 500003, 500003, INT32_MAX, INT32_MIN, 500005], np.int32)
    s["from_ids"] = np.concatenate([s["from_ids"], extra_from])
    s["to_ids"] = np.concatenate([s["to_ids"], extra_to])
    s["from_points"] = np.concatenate([s["from_points"], rng.uniform(0, HEIGHT, (extra_from.size, 2)).astype(np.float32)])
    s["to_points"] = np.concatenate([s["to_points"], rng.uniform(0, HEIGHT, (extra_to.size, 2)).astype(np.float32)])
    s["expect_matches"] = sorted(int(i) for i in s["from_ids"][:12]) + [INT32_MAX]
    return s


def all_equal(m=10):
    """every keypoint of the from-frame at one position: d = 0"""
    s = with_m(m)
    s["from_points"] = np.full_like(s["from_points"], 100.0)
    return s


def collinear(m=9):
    """every from-keypoint on the horizontal line through the centroid: the normalised y is exactly 0, three columns of every sample are zero,
    and the seventh pivot is 0"""
    s = scene(13, m, outliers=0.0, extra=0)
    s["from_points"][:, 0] = np.arange(m, dtype=np.float32) * 16.0 + 8.0
    s["from_points"][:, 1] = 64.0
    return s


def c3_zero():
    """Eight pairs, five with the from-keypoint's v at the from-centroid (normalised y = 0) and three with the to-keypoint at the
    to-centroid (normalised x' = y' = 0): the columns x'y and y'y of every sample are exactly zero and no other is, so they stay free,
    F1 and F2 have one entry each, and c3 = det F1 = 0."""
    fu = np.array([40, 90, 170, 260, 330, 120, 200, 310], np.float32)
    fv = np.array([64, 64, 64, 64, 64, 34, 74, 84], np.float32)             # mean 64
    tu = np.array([100, 180, 260, 210, 250, 200, 200, 200], np.float32)      # mean 200
    tv = np.array([80, 170, 110, 60, 80, 100, 100, 100], np.float32)         # mean 100
    ids = np.arange(10, 18, dtype=np.int32)
    return dict(from_ids=ids, from_points=np.stack([fu, fv], 1), to_ids=ids.copy(), to_points=np.stack([tu, tv], 1))


def nan_keypoint(m=40):
    """one to-keypoint of a pair is NaN: it is a pair, the centroid is NaN, and no model comes out"""
    s = with_m(m)
    row = int(np.nonzero(np.isin(s["to_ids"], s["from_ids"]))[0][0])
    s["to_points"][row, 0] = np.nan
    s["nan_id"] = int(s["to_ids"][row])
    return s


def scaled(pair, k):
    """both keypoint arrays times float32(2^k), which is exact while nothing leaves the normal range; the caller scales ransac_threshold alike"""
    f = np.float32(2.0 ** k)
    return dict(pair, from_points=pair["from_points"] * f, to_points=pair["to_points"] * f)


# Found with the model alone (test_epipolar_inputs.py proves each class).  Scenes 0 .. 39 of the census recipe put winners on every root, on
# one and three real roots, in chunks 0 .. 3, on every quarter of a chunk, every scoring wave and both signs of the leading entry; the four
# scenes behind them are the first of 20 000 whose winner is candidate 1024 (421, 2815) or 1025 (6636, 9193), the final chunk of two, and
# the last two (45, 278) join scene 14 in winning with a cubic whose derivative has no two real roots (disc <= 0).
CENSUS_ITERATIONS, CENSUS_SEED = 342, 5
CENSUS_SCENES = tuple(range(40)) + (421, 2815, 6636, 9193, 45, 278)
# With this seed hypothesis 85 fits each of the three clean pairs, so at 86 iterations their ties reach into the second chunk
TIE_SEED, TIE_NOISY_SCENE = 19, 10
# draw7 fails when seed + h = 304 (the first such value for m = 8): hypothesis 3 of 60
DRAW_FAILURE_SEED, DRAW_FAILURE_H, DRAW_FAILURE_ITERATIONS = 301, 3, 60


def census_scene(s):
    return scene(s, 40, outliers=0.6, extra=2)


def census_batch():
    """-> (pairs, iterations, seed) of one call: 1 026 candidates a pair, four chunks of 256 and a last one of two, the winners spread over them"""
    return [census_scene(s) for s in CENSUS_SCENES], CENSUS_ITERATIONS, CENSUS_SEED


def tie_pairs():
    """-> (pairs, seed): three clean pairs on which every sound hypothesis reaches all m inliers, and a noisy one whose best count is reached
    by candidates of different waves of one chunk"""
    return [with_m(8), with_m(9), with_m(12), census_scene(TIE_NOISY_SCENE)], TIE_SEED


def draw_failure():
    """-> (pair, seed, iterations): eight pairs, and hypothesis DRAW_FAILURE_H does not find seven distinct indices within its 32 draws"""
    return with_m(8), DRAW_FAILURE_SEED, DRAW_FAILURE_ITERATIONS


def _paired_row(s, side):
    other = "to" if side == "from" else "from"
    return int(np.nonzero(np.isin(s[side + "_ids"], s[other + "_ids"]))[0][0])


def inf_keypoint(sign, side, m=40):
    """one keypoint coordinate of a pair, in the `side` frame ("from" or "to"), is sign x infinity: it is a pair, and no model comes out"""
    s = with_m(m)
    s[side + "_points"][_paired_row(s, side), 1] = np.float32(sign) * np.float32(np.inf)
    return s


def nan_unpaired(m=40):
    """-> (pair, twin): the rows that pair with nothing hold NaN keypoints in both frames of `pair` and finite ones in `twin`"""
    twin = scene(21, m, outliers=0.3, extra=6)
    s = dict(twin, from_points=twin["from_points"].copy(), to_points=twin["to_points"].copy())
    s["from_points"][~np.isin(s["from_ids"], s["to_ids"])] = np.nan
    s["to_points"][~np.isin(s["to_ids"], s["from_ids"])] = np.nan
    return s, twin


def batch(pairs):
    """pairs concatenated -> (from_ids, from_points, from_offsets, to_ids, to_points, to_offsets)"""
    fo = np.concatenate([[0], np.cumsum([p["from_ids"].shape[0] for p in pairs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([p["to_ids"].shape[0] for p in pairs])]).astype(np.int64)
    cat = lambda k, shape, dt: np.concatenate([np.asarray(p[k], dt).reshape(shape) for p in pairs]) if pairs else np.zeros(shape, dt).reshape(shape)[:0]
    return (cat("from_ids", (-1,), np.int32), cat("from_points", (-1, 2), np.float32), fo, cat("to_ids", (-1,), np.int32),
            cat("to_points", (-1, 2), np.float32), to)


def empty_frame(n, seed=3):
    """a frame of n rows that pairs with nothing"""
    rng = np.random.default_rng(seed)
    return (900000 + np.arange(n)).astype(np.int32), rng.uniform(0, HEIGHT, (n, 2)).astype(np.float32)
