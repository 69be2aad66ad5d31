"""Inputs for lcd_estimate_motion_pnp's tests.  A pair is a dict with from_ids, from_xyz [n x 3], to_ids, to_points [n x 2], to_xyz [n x 3] and
what the generator knows about it (the true model R, t that maps from-points into the to-camera, the inlier flags in ascending-id order).
tests/test_motion_pnp_inputs.py proves without a GPU that each input has the property it exists for."""
import numpy as np

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


def scene(rng, m, noise=0.5, depth=(0.5, 10.0), angle=(0.05, 0.5), shift=0.5):
    """m points seen by the to-camera inside the image at depths `depth`, the from-points P with R P + t = their camera coordinates"""
    R = rotation(rng.normal(size=3), rng.uniform(*angle))
    t = rng.uniform(-shift, shift, 3)
    z = rng.uniform(depth[0], depth[1], m)
    u, v = rng.uniform(0, WIDTH - 1, m), rng.uniform(0, HEIGHT - 1, m)
    C = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], axis=1)
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
