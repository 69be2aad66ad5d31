"""Inputs for lcd_estimate_motion_3d's tests.  A frame is (word ids [n] int32, points [n x 3] float32); a pair is a dict with from_ids, from_xyz,
to_ids, to_xyz and what the generator knows about it.  tests/test_motion_3d_inputs.py proves without a GPU that each input has the property
it exists for."""
import numpy as np

import motion_3d_model as M

BATCH_SIZES = (0, 2, 3, 5, 6, 63, 64, 65, 255, 256, 257, 1100)     # correspondences of the pairs of the mixed batch
ITERATIONS = (1, 255, 256, 257, 300)
REFINE = (0, 1, 5)
SIGMA_FLOOR = 0.5                                                   # second-smallest singular value of the inliers' cross-covariance, per inlier


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def random_pair(rng, m, outliers=0.4, noise=0.01, extent=3.0, decoys=True):
    """m correspondences (exactly: every shared unique id has finite non-zero points), a fraction of them outliers, inside frames that also
    hold ids of one side only and -- with decoys -- ids that occur twice in one frame and once in the other, which take no part.  Rows shuffled."""
    R = rotation(rng.normal(size=3), rng.uniform(0.2, 1.2))
    t = rng.uniform(-1, 1, 3)
    P = rng.uniform(-extent, extent, (m, 3))
    Q = P @ R.T + t + rng.normal(size=(m, 3)) * noise
    out = rng.random(m) < outliers
    Q[out] = rng.uniform(-extent, extent, (int(out.sum()), 3))
    pool = rng.permutation(4 * m + 64)[: m + 24].astype(np.int64) - m // 2          # negative ids too: the rule has no sign test
    ids = pool[:m]
    extra = pool[m:]
    f_ids, f_xyz, t_ids, t_xyz = list(ids), list(P), list(ids), list(Q)
    point = lambda: rng.uniform(-extent, extent, 3)
    n_extra = 8 if decoys else 0
    for k in range(n_extra):
        e = int(extra[k])
        if k < 3:                                                       # only in from
            f_ids.append(e); f_xyz.append(point())
        elif k < 6:                                                     # only in to
            t_ids.append(e); t_xyz.append(point())
        elif k == 6:                                                    # twice in from, once in to
            f_ids += [e, e]; f_xyz += [point(), point()]
            t_ids.append(e); t_xyz.append(point())
        else:                                                           # once in from, twice in to
            f_ids.append(e); f_xyz.append(point())
            t_ids += [e, e]; t_xyz += [point(), point()]
    pf, pt = rng.permutation(len(f_ids)), rng.permutation(len(t_ids))
    return dict(from_ids=np.array(f_ids, np.int32)[pf], from_xyz=np.array(f_xyz, np.float32).reshape(-1, 3)[pf],
                to_ids=np.array(t_ids, np.int32)[pt], to_xyz=np.array(t_xyz, np.float32).reshape(-1, 3)[pt],
                m=m, R=R, t=t, inlier=~out, ids=np.sort(ids).astype(np.int32))


def frames(pair):
    return pair["from_ids"], pair["from_xyz"], pair["to_ids"], pair["to_xyz"]


def mixed_batch(seed=11):
    rng = np.random.default_rng(seed)
    return [random_pair(rng, m) for m in BATCH_SIZES]


def all_outlier_pair(seed=12, m=40):
    """no rigid motion explains more than its own sample: both sides are independent noise"""
    rng = np.random.default_rng(seed)
    return random_pair(rng, m, outliers=1.1)


def exact_pair(m, seed=13):
    """to = from, small integers: every valid hypothesis is the identity exactly and holds all m correspondences -- a tie among all of them"""
    rng = np.random.default_rng(seed)
    P = rng.integers(-8, 9, (m, 3)).astype(np.float32)
    P[np.all(P == 0, axis=1)] = 1.0
    ids = np.arange(1, m + 1, dtype=np.int32)
    return dict(from_ids=ids, from_xyz=P, to_ids=ids.copy(), to_xyz=P.copy(), m=m)


def seed_with_invalid_first(m=3, invalid=1):
    """the first seed whose hypotheses 0 .. invalid - 1 find no three distinct indices among m while hypothesis `invalid` does"""
    seed = 0
    while True:
        if all(M.draw3(seed, h, m) is None for h in range(invalid)) and M.draw3(seed, invalid, m) is not None:
            return seed
        seed += 1


OVERFLOW_DISTANCE = 1.0e15


def overflow_refit_pair(n=64, seed=14):
    """to = from turned by a quarter about z (exact in fp32) at a scale where the sums of three products are finite and the sums of n are not:
    under OVERFLOW_DISTANCE every hypothesis holds all n correspondences, the fit of all n overflows to a model of NaNs, and the selection
    behind it is empty -- on the refinement's first pass"""
    rng = np.random.default_rng(seed)
    s = np.float32(4.4e18)
    P = (rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(0.5, 1.0, (n, 3)) * s).astype(np.float32)
    Q = np.stack([-P[:, 1], P[:, 0], P[:, 2]], axis=1).astype(np.float32)
    ids = np.arange(1, n + 1, dtype=np.int32)
    return dict(from_ids=ids, from_xyz=P, to_ids=ids.copy(), to_xyz=Q, m=n)


# refinement branches, found by searching seeds with the model: (seed, m, outliers, noise, inlier_distance, refine_iterations, the word the
# trace must contain)
REFINE_CASES = {
    "converged": (1, 34, 0.4, 0.04, 0.2, 10, "converged"),
    "size_changed": (2, 52, 0.2, 0.02, 0.05, 10, "size_changed"),
    "members_changed": (26, 53, 0.2, 0.04, 0.1, 10, "members_changed"),
    "oscillating": (39, 58, 0.4, 0.04, 0.05, 10, "oscillating"),
}


def refine_case(name):
    seed, m, outliers, noise, dist, refine, _ = REFINE_CASES[name]
    pair = random_pair(np.random.default_rng(seed), m, outliers=outliers, noise=noise, decoys=False)
    return pair, dict(min_inliers=4, inlier_distance=dist, iterations=60, refine_iterations=refine, seed=seed)


def well_conditioned(P, Q):
    """at least six points, and the second-smallest singular value of their cross-covariance above SIGMA_FLOOR per point"""
    if len(P) < 6:
        return False
    s = M.kabsch64(P, Q)[2]
    return bool(np.sort(s)[1] / len(P) > SIGMA_FLOOR)


STAGE_CAP = (2 * (8192 + 8192 // 8) * 8 - (256 * 12 + 256 * 9) * 4) // 24   # correspondences the kernel stages in LDS at most: 5248


def big_pair(seed=15, m=8000, rows=8192):
    """`rows` rows on both sides, m correspondences among them (more than STAGE_CAP: read from the scratch), the rest ids of one side only"""
    rng = np.random.default_rng(seed)
    pair = random_pair(rng, m, outliers=0.3, decoys=False)
    out = dict(pair)
    for side, base in (("from", 1 << 20), ("to", 1 << 21)):
        extra = rows - pair[side + "_ids"].shape[0]
        ids = np.concatenate([pair[side + "_ids"], base + np.arange(extra, dtype=np.int32)])
        xyz = np.concatenate([pair[side + "_xyz"], rng.uniform(-3, 3, (extra, 3)).astype(np.float32)])
        perm = rng.permutation(rows)
        out[side + "_ids"], out[side + "_xyz"] = ids[perm].astype(np.int32), xyz[perm]
    return out


def concatenate(pairs):
    """-> from_ids, from_xyz, from_offsets, to_ids, to_xyz, to_offsets of a batch"""
    fo = np.cumsum([0] + [p["from_ids"].shape[0] for p in pairs]).astype(np.int64)
    to = np.cumsum([0] + [p["to_ids"].shape[0] for p in pairs]).astype(np.int64)
    cat = lambda k, shape, dt: np.concatenate([p[k].reshape(shape) for p in pairs] + [np.zeros((0,) + shape[1:], dt)])
    return (cat("from_ids", (-1,), np.int32), cat("from_xyz", (-1, 3), np.float32), fo, cat("to_ids", (-1,), np.int32), cat("to_xyz", (-1, 3), np.float32), to)


def fit_sets(n_random=20, seed=77):
    """(P, Q) inlier sets for the comparison with a float64 fit: the inliers the model finds in the mixed batch and in n_random pairs of
    30 .. 400 correspondences, those that are well conditioned"""
    rng = np.random.default_rng(seed)
    pairs = [p for p in mixed_batch() if p["m"] >= 6] + [random_pair(rng, int(rng.integers(30, 400))) for _ in range(n_random)]
    sets = []
    for k, p in enumerate(pairs):
        r = M.estimate(*frames(p), min_inliers=6, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=k)
        if r["status"] != M.OK:
            continue
        P, Q = r["P"][r["inlier_index"]], r["Q"][r["inlier_index"]]
        if well_conditioned(P, Q):
            sets.append((P, Q))
    return sets


# ---------------------------------------------------------------------------------------------------------------------------------------
# Inputs for the places where the kernel's join, staging and hypothesis chunks change shape (tests/test_gpu_motion_3d_shapes.py).  What a
# search found is kept as a constant; tests/test_motion_3d_inputs.py proves each constant and each property again with the model.

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
QUARTER = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])           # a quarter turn about z: exact in fp32 on small integers


def sort_length(n):
    """the keys the kernel sorts for a side of n rows: the power of two >= n, at least 2"""
    p = 2
    while p < n:
        p <<= 1
    return p


def pad_side(rng, pair, side, base, rows, columns):
    """one frame of `pair` grown to exactly `rows` rows in place: the new rows carry the ids base, base + 1, .. (of this side only) and, per
    (key, low, high) of `columns`, values uniform in [low, high); then the frame's rows are shuffled"""
    extra = rows - pair[side + "_ids"].shape[0]
    assert extra >= 0
    ids = np.concatenate([pair[side + "_ids"], base + np.arange(extra, dtype=np.int32)])
    grown = [np.concatenate([pair[key], rng.uniform(low, high, (extra, pair[key].shape[1])).astype(np.float32)]) for key, low, high in columns]
    perm = rng.permutation(rows)
    pair[side + "_ids"] = ids[perm].astype(np.int32)
    for (key, _, _), a in zip(columns, grown):
        pair[key] = np.ascontiguousarray(a[perm])


def sized_pair(seed, m, n_from, n_to, **kw):
    """random_pair's m correspondences (no decoys) inside frames of exactly n_from and n_to rows: the rest are ids of one side only"""
    rng = np.random.default_rng(seed)
    pair = random_pair(rng, m, decoys=False, **kw)
    out = dict(pair)
    pad_side(rng, out, "from", 1 << 20, n_from, (("from_xyz", -3, 3),))
    pad_side(rng, out, "to", 1 << 21, n_to, (("to_xyz", -3, 3),))
    return out


ASYMMETRIC_SIZES = ((1, 300), (300, 1), (3, 2049), (2049, 3), (65, 8192), (8192, 65), (0, 50), (50, 0))
ASYMMETRIC_DISJOINT = (40, 70)


def asymmetric_pairs(seed=31):
    """one pair per entry of ASYMMETRIC_SIZES, every row of the smaller side a correspondence (at most 60 of them), and a last pair of
    ASYMMETRIC_DISJOINT rows whose ids are disjoint"""
    pairs = [sized_pair(seed + k, min(nf, nt, 60), nf, nt, outliers=0.2) for k, (nf, nt) in enumerate(ASYMMETRIC_SIZES)]
    pairs.append(sized_pair(seed + len(pairs), 0, *ASYMMETRIC_DISJOINT))
    return pairs


RUN_ROWS = 600
RUN_BOUNDARIES = (63, 255, 511)                                      # a run straddles b when it covers the sorted positions b and b + 1
RUN_LENGTHS = (2, 3, 5)


def _run_frame(distinct, runs, other_runs):
    """distinct: the frame's ids, ascending.  runs: {sorted position of a run's first row: length}.  -> the frame's ids in sorted order with the
    runs laid where they are asked for, and the indices into `distinct` that carry them; none of them is in other_runs"""
    counts = np.ones(len(distinct), np.int64)
    at, j, carried = 0, 0, []
    while j < len(distinct):
        if at in runs:
            assert j not in other_runs, "a run of the other frame stands here"
            counts[j] = runs[at]
            carried.append(j)
        at += int(counts[j])
        j += 1
    assert at == RUN_ROWS and len(carried) == len(runs), (at, carried)
    return np.repeat(distinct, counts), carried


def run_id_frames(rng, rot):
    """the ids of two frames of RUN_ROWS rows over the same distinct ids, in sorted order.  Frame A holds a run from sorted position 0 and a
    run over each of RUN_BOUNDARIES that ends just behind it, frame B a run over each boundary that starts just in front of it (another
    length there) and a run up to its last position; `rot` rotates the lengths through RUN_LENGTHS.  An id that runs in one frame stands
    once in the other.  -> (distinct, ids_a, ids_b, the indices into distinct that run in A, those that run in B)"""
    L = [RUN_LENGTHS[(rot + k) % 3] for k in range(3)]
    edge = L[0]                                                        # the length of the run at either end
    n_distinct = RUN_ROWS - (edge - 1) - sum(l - 1 for l in RUN_LENGTHS)
    distinct = np.sort(rng.permutation(20000)[:n_distinct].astype(np.int64) - 10000)
    runs_a = {0: edge}
    runs_b = {RUN_ROWS - edge: edge}
    for k, b in enumerate(RUN_BOUNDARIES):
        runs_a[b + 2 - L[k]] = L[k]
        runs_b[b] = L[(k + 1) % 3]
    ids_a, carried_a = _run_frame(distinct, runs_a, ())
    ids_b, carried_b = _run_frame(distinct, runs_b, set(carried_a))
    return distinct, ids_a, ids_b, carried_a, carried_b


def duplicate_run_pairs(seed=32):
    """Six pairs of RUN_ROWS x RUN_ROWS rows over the same ids on both sides.  In each, one frame holds a run from sorted position 0 and a
    run over each of RUN_BOUNDARIES, the other a run that ends at its last sorted position and a run over each boundary; the run lengths
    rotate through RUN_LENGTHS from pair to pair, and pairs 3 .. 5 are pairs 0 .. 2 with the frames exchanged.  An id that runs in one frame
    stands once in the other, so it is no correspondence; every other id is one."""
    rng = np.random.default_rng(seed)
    pairs = []
    for rot in range(3):
        distinct, ids_a, ids_b, carried_a, carried_b = run_id_frames(rng, rot)
        n_distinct = len(distinct)
        R, t = rotation(rng.normal(size=3), rng.uniform(0.2, 1.2)), rng.uniform(-1, 1, 3)
        P = rng.uniform(-3, 3, (n_distinct, 3))
        Q = P @ R.T + t + rng.normal(size=(n_distinct, 3)) * 0.01
        frames_ab = []
        for ids, X in ((ids_a, P), (ids_b, Q)):
            j = np.searchsorted(distinct, ids)
            xyz = X[j]
            in_run = np.bincount(j)[j] > 1                              # the rows of a run: a point of their own each
            xyz[in_run] = rng.uniform(-3, 3, (int(in_run.sum()), 3))
            perm = rng.permutation(RUN_ROWS)
            frames_ab.append((ids[perm].astype(np.int32), np.ascontiguousarray(xyz[perm], dtype=np.float32)))
        running = sorted(int(distinct[j]) for j in carried_a + carried_b)
        pairs.append(dict(from_ids=frames_ab[0][0], from_xyz=frames_ab[0][1], to_ids=frames_ab[1][0], to_xyz=frames_ab[1][1], running=running))
    for p in list(pairs):
        pairs.append(dict(from_ids=p["to_ids"], from_xyz=p["to_xyz"], to_ids=p["from_ids"], to_xyz=p["from_xyz"], running=p["running"]))
    return pairs


def runs_of(ids):
    """{sorted position of the first row: length} of every run of equal ids in the ascending signed order"""
    s = np.sort(np.asarray(ids, np.int64))
    starts = np.nonzero(np.concatenate([[True], s[1:] != s[:-1]]))[0]
    lengths = np.diff(np.concatenate([starts, [len(s)]]))
    return {int(a): int(l) for a, l in zip(starts, lengths) if l > 1}


EXTREME_IDS = (INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX)
EXTREME_ROWS = (13, 70)                                               # no power of two: INT32_MAX's key stands next to the all-ones padding keys


def extreme_id_lists(rng, case, nf, nt):
    """the ids of a from-frame of nf rows and a to-frame of nt: EXTREME_IDS and five ordinary ids on both sides and ids of one side only.
    case 0: INT32_MIN + 1 is in `from` only.  1: INT32_MAX twice in `to`.  2: INT32_MAX twice in `from`."""
    common = [int(v) for v in rng.permutation(4000)[:5] - 2000 + 5000 * (rng.random(5) < 0.5)]
    f_ids = list(EXTREME_IDS) + common
    t_ids = [i for i in EXTREME_IDS if not (case == 0 and i == INT32_MIN + 1)] + common
    if case == 1:
        t_ids.append(INT32_MAX)
    if case == 2:
        f_ids.append(INT32_MAX)
    f_ids += [int(v) for v in 100000 + np.arange(nf - len(f_ids))]
    t_ids += [int(v) for v in 200000 + np.arange(nt - len(t_ids))]
    return f_ids, t_ids


def extreme_id_pairs(seed=33):
    """three pairs of EXTREME_ROWS rows.  0: INT32_MIN, -1, 0, 1 and INT32_MAX are correspondences, INT32_MIN + 1 is in `from` only.
    1: as 0 with INT32_MIN + 1 a correspondence too and INT32_MAX twice in `to`.  2: as 1 with INT32_MAX twice in `from` and once in `to`."""
    rng = np.random.default_rng(seed)
    nf, nt = EXTREME_ROWS
    pairs = []
    for case in range(3):
        f_ids, t_ids = extreme_id_lists(rng, case, nf, nt)
        P = {i: rng.uniform(-3, 3, 3) for i in set(f_ids) | set(t_ids)}
        R, t = rotation(rng.normal(size=3), 0.7), rng.uniform(-1, 1, 3)
        f_xyz = np.array([P[i] for i in f_ids], np.float32)
        t_xyz = np.array([R @ P[i] + t for i in t_ids], np.float32)
        pf, pt = rng.permutation(nf), rng.permutation(nt)
        pairs.append(dict(from_ids=np.array(f_ids, np.int64).astype(np.int32)[pf], from_xyz=f_xyz[pf], to_ids=np.array(t_ids, np.int64).astype(np.int32)[pt], to_xyz=t_xyz[pt]))
    return pairs


PREDICATE_ROWS = 700


def predicate_causes():
    """(side, what) of the 22 ways one correspondence is dropped: NaN, +inf, -inf in each of the six coordinates; the all-zero and the
    all-minus-zero point on each side"""
    causes = [(c, v) for v in (np.nan, np.inf, -np.inf) for c in range(6)]
    return causes + [("from", 0.0), ("from", -0.0), ("to", 0.0), ("to", -0.0)]


def predicate_pair(seed=34):
    """PREDICATE_ROWS x PREDICATE_ROWS rows, every id shared and unique.  In ascending id, every third correspondence (0, 3, 6, ..) is dropped
    by exactly one of predicate_causes(), in turn; of the others every fifth has one coordinate of one point set to zero, which drops nothing."""
    rng = np.random.default_rng(seed)
    n = PREDICATE_ROWS
    ids = np.sort(rng.permutation(6 * n)[:n] - 3 * n).astype(np.int32)
    R, t = rotation(rng.normal(size=3), 0.5), rng.uniform(-1, 1, 3)
    P = rng.uniform(0.5, 3, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    X = np.concatenate([P, P @ R.T + t], axis=1).astype(np.float32)    # [n x 6]: from x, y, z, to x, y, z
    causes = predicate_causes()
    dropped, zeroed = np.zeros(n, bool), np.zeros(n, bool)
    for k in range(n):
        if k % 3 == 0:
            side, v = causes[(k // 3) % len(causes)]
            if side == "from":
                X[k, :3] = v
            elif side == "to":
                X[k, 3:] = v
            else:
                X[k, side] = v
            dropped[k] = True
        elif k % 5 == 0:
            X[k, (k // 5) % 6] = 0.0 if k % 2 else -0.0
            zeroed[k] = True
    pf, pt = rng.permutation(n), rng.permutation(n)
    return dict(from_ids=ids[pf], from_xyz=np.ascontiguousarray(X[pf, :3]), to_ids=ids[pt], to_xyz=np.ascontiguousarray(X[pt, 3:]),
                ids=ids, dropped=dropped, zeroed=zeroed)


SWITCH_ROWS = (5400, 5300)


def stage_switch_pairs(seed=35):
    """two pairs of SWITCH_ROWS rows from the same rows: STAGE_CAP correspondences, the last the kernel stages in LDS, and -- one id of `to`
    alone replaced by an id of `from` alone -- STAGE_CAP + 1, the first it reads from the scratch"""
    at = sized_pair(seed, STAGE_CAP, *SWITCH_ROWS, outliers=0.3)
    above = dict(at, to_ids=at["to_ids"].copy())
    only_from = np.setdiff1d(at["from_ids"], at["to_ids"])
    only_to = np.setdiff1d(at["to_ids"], at["from_ids"])
    above["to_ids"][np.nonzero(above["to_ids"] == only_to[0])[0][0]] = only_from[0]
    return at, above


def stride_pairs(seed=36):
    """a staged pair whose stride (m = 150) is far from its rows (8192 x 200), a pair of five correspondences, and a pair read from the scratch
    (m = 5260 of 8192 x 5300 rows: stride n_from, n_to < n_from)"""
    return [sized_pair(seed, 150, 8192, 200, outliers=0.2), random_pair(np.random.default_rng(seed + 1), 5, outliers=0.0),
            sized_pair(seed + 2, 5260, 8192, 5300, outliers=0.3)]


TIE_ITERATIONS = (512, 513, 600, 65535)                               # whole chunks, one hypothesis more, a partial chunk, the entry's maximum
TIE_SEED = 5


# exact_pair(m) under a seed whose first hypotheses find no three distinct indices: the tie's winner is not hypothesis 0.  Sixteen draws
# among m = 40 leave fewer than three distinct values with a probability below 1e-19, so no seed does that to exact_pair(40); among m = 3
# it is 0.5 % of all hypotheses, which also puts invalid hypotheses into every chunk.  (m, invalid, seed): seed = seed_with_invalid_first(m, invalid)
TIE_INVALID_FIRST = (3, 2, 32127)


def tie_pairs():
    """exact_pair(40), and exact_pair of TIE_INVALID_FIRST's m"""
    return exact_pair(40), exact_pair(TIE_INVALID_FIRST[0])


def planted_pair(seed, k, noise_rows, noise=0.0):
    """k correspondences related by a quarter turn about z and an integer shift (exact in fp32; plus `noise`), among noise_rows correspondences
    whose two points are independent.  Ids 1 .. k + noise_rows in a random order over the rows; `planted` says which ids move together."""
    rng = np.random.default_rng(seed)
    m = k + noise_rows
    P = rng.integers(-8, 9, (m, 3)).astype(np.float64)
    P[np.all(P == 0, axis=1)] = 1.0
    Q = P @ QUARTER.T + np.array([2.0, -1.0, 3.0]) + rng.normal(size=(m, 3)) * noise
    planted = np.zeros(m, bool)
    planted[rng.permutation(m)[:k]] = True
    Q[~planted] = rng.uniform(-9, 9, (m - k, 3))
    ids = np.arange(1, m + 1, dtype=np.int32)
    pf, pt = rng.permutation(m), rng.permutation(m)
    return dict(from_ids=ids[pf], from_xyz=P[pf].astype(np.float32), to_ids=ids[pt], to_xyz=Q[pt].astype(np.float32), m=m, planted=planted)


LATE_KW = dict(min_inliers=3, inlier_distance=0.05, refine_iterations=0)
LATE_GAP = 599


def late_winner_pair():
    """40 correspondences, five of them related by an exact rigid motion: a hypothesis holds all five only when it draws three of them"""
    return planted_pair(37, 5, 35)


def stream_counts(pair, first, n):
    """the counts of the hypotheses at the stream positions first .. first + n - 1 (draw3 hashes seed + h: position = seed + h)"""
    return M.estimate(*frames(pair), iterations=n, seed=first, **LATE_KW)["counts"]


def find_late_winner(pair, start=0, block=4000):
    """the first stream position >= start + LATE_GAP whose hypothesis holds five, which no hypothesis at the LATE_GAP positions in front of
    it equals or exceeds, and which has a hypothesis that holds something (fewer) at the 255 positions in front of it: what wins when the
    winner is cut off"""
    first = start
    while True:
        counts = stream_counts(pair, first, block)
        for w in np.nonzero(counts == 5)[0]:
            if w >= LATE_GAP and counts[w - LATE_GAP:w].max() < 5 and counts[w - 255:w].max() > 0:
                return first + int(w)
        first += block - LATE_GAP


LATE_POSITION = 6738                                                  # find_late_winner(late_winner_pair())
# (winner's hypothesis index h, iterations): the last of chunk 0, the first of chunk 1, the last of chunk 1, the last of a partial chunk 2,
# the only hypothesis of a partial chunk 1
LATE_CASES = ((255, 600), (256, 600), (511, 600), (599, 600), (256, 257))
CUT_OFF = (255, 511, 599)                                             # iterations = h: the winner is the first hypothesis that is not evaluated


def late_kw(h, iterations):
    return dict(LATE_KW, iterations=iterations, seed=(LATE_POSITION - h) & M.M32)


LATE_MEMBERS_KW = dict(min_inliers=4, inlier_distance=0.1, iterations=60, refine_iterations=10)


def late_members_pair(seed):
    return random_pair(np.random.default_rng(seed), 420, outliers=0.2, noise=0.04, decoys=False)


def find_late_members(seeds=range(200)):
    """the seeds whose refinement says members_changed for two sets that are equal at every index below 256 -> [(seed, first differing index)]"""
    found = []
    for s in seeds:
        r = M.estimate(*frames(late_members_pair(s)), seed=s, **LATE_MEMBERS_KW)
        if r["first_differing"] and min(r["first_differing"]) >= 256:  # every members_changed pass differs late
            found.append((s, r["first_differing"]))
    return found


# find_late_members(): of the first 200 seeds, those that qualify -> the first differing index of their (one) members_changed pass
LATE_MEMBERS = {154: 275, 197: 284}


def offset_pair(m, seed, offsets):
    """exact_pair(m) with offsets[k] added to the `to` point of the k-th correspondence in the order: the three that hypothesis 0 of `seed`
    draws, then the others ascending.  The first three offsets are zero, so hypothesis 0 is the identity exactly, and with every offset inside
    the inlier distance it holds all m and wins: the last selection's d2 are |offset|^2, exactly where the arithmetic is"""
    offsets = np.asarray(offsets, np.float32).reshape(m, 3)
    drawn = M.draw3(seed, 0, m)
    assert drawn is not None and not offsets[:3].any()
    order = list(drawn) + [i for i in range(m) if i not in drawn]
    pair = exact_pair(m)
    pair["to_xyz"][order] = pair["to_xyz"][order] + offsets
    return pair


def _offsets(groups):
    return np.concatenate([np.tile(np.array(v, np.float32), (n, 1)) for n, v in groups])


B19 = 2.0 ** -19
SELECT_KW = dict(min_inliers=3, refine_iterations=0)
# radix select: name -> (pair, keyword arguments); the property each has is proved from the model's last_d2 in tests/test_motion_3d_inputs.py
SELECT_SIZES = {"size_3": 3, "size_4": 4, "size_255": 255, "size_256": 256, "size_257": 257}


def select_cases():
    cases = {}
    for k in (3, 4):                                                    # (a)
        cases["size_%d" % k] = (planted_pair(40 + k, k, 3, noise=0.003), dict(SELECT_KW, inlier_distance=0.05, iterations=60, seed=1))
    for k in (255, 256, 257):                                           # (b)
        cases["size_%d" % k] = (planted_pair(40 + k, k, 20, noise=0.002), dict(SELECT_KW, inlier_distance=0.1, iterations=20, seed=2))
    cases["all_zero"] = (exact_pair(300), dict(SELECT_KW, inlier_distance=0.1, iterations=20, seed=3))                       # (c)
    # (d) 25 at 0, 60 at 0.25^2, 16 at 0.5^2: the median is 0.0625 and so are more than half
    cases["majority_is_median"] = (offset_pair(101, 4, _offsets([(25, (0, 0, 0)), (60, (0.25, 0, 0)), (16, (0, 0.5, 0))])),
                                   dict(SELECT_KW, inlier_distance=1.0, iterations=20, seed=4))
    cases["even_middle_differs"] = (planted_pair(50, 100, 20, noise=0.01), dict(SELECT_KW, inlier_distance=0.2, iterations=20, seed=5))   # (e)
    # (f) 2^-4 + (j 2^-19)^2 for j = 0, 45, 64, 78, 90 is 2^-4 plus 0, 1, 2, 3, 4 units of its last place: ranks 19, 20, 21 of 40 carry 1, 2, 3
    low_byte = [(10, (0, 0, 0)), (5, (0.125, 0, 0)), (4, (0.25, 0, 0)), (1, (0.25, 45 * B19, 0)), (1, (0.25, 64 * B19, 0)), (1, (0.25, 78 * B19, 0)),
                (4, (0.25, 90 * B19, 0)), (14, (0.375, 0, 0))]
    cases["low_byte"] = (offset_pair(40, 6, _offsets(low_byte)), dict(SELECT_KW, inlier_distance=1.0, iterations=20, seed=6))
    return cases


SCRATCH_TABLE_SEED = 154                                              # of LATE_MEMBERS
SCRATCH_TABLE_EXACT = 5000


def scratch_table_pair():
    """late_members_pair(SCRATCH_TABLE_SEED) and SCRATCH_TABLE_EXACT exact correspondences of the same motion: more than STAGE_CAP, so the
    selection, the refinement and the median run with the coordinates in global memory"""
    base = late_members_pair(SCRATCH_TABLE_SEED)
    rng = np.random.default_rng(38)
    n = SCRATCH_TABLE_EXACT
    P = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    Q = (P.astype(np.float64) @ base["R"].T + base["t"]).astype(np.float32)
    ids = (10000 + np.arange(n)).astype(np.int32)
    out = dict(base)
    for side, X in (("from", P), ("to", Q)):
        perm = rng.permutation(base["m"] + n)
        out[side + "_ids"] = np.concatenate([base[side + "_ids"], ids])[perm]
        out[side + "_xyz"] = np.ascontiguousarray(np.concatenate([base[side + "_xyz"], X])[perm])
    out["m"] = base["m"] + n
    return out


def scratch_table_kws():
    """case 10's arguments; and, found by trying seeds and distances, arguments without refinement under which the last selection has an even
    size and two different middle elements"""
    return [dict(LATE_MEMBERS_KW, seed=SCRATCH_TABLE_SEED), dict(LATE_MEMBERS_KW, seed=14, refine_iterations=0, inlier_distance=0.12)]


WRAPPER_KW = dict(min_inliers=50, inliers_distance=0.1, iterations=100, refine_iterations=5, seed=7)


def wrapper_pairs():
    """for the C++ wrapper under WRAPPER_KW: too few correspondences (2), below min_inliers (63 correspondences, about 38 inliers), accepted
    (255), and a pair of frames with runs of repeated ids (accepted)"""
    batch = mixed_batch()
    return [batch[1], batch[5], batch[8], duplicate_run_pairs()[2]]
