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
