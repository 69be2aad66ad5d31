"""Inputs for lcd_refine_motion_ba's tests, built on motion_pnp_inputs.scene.  A pair is a dict with the frames (from_ids, from_xyz, from_points,
to_ids, to_points, to_xyz), the PnP's result (inliers, transform) and what the generator knows about it (the planted outliers as indices into
`inliers`, the true transform).  args(pair, ...) gives the keyword arguments of motion_ba_model.refine / vwdictionary.motion_ba_cpu.
tests/test_motion_ba_inputs.py proves without a GPU that each hand-made case takes the branch it exists for."""
import numpy as np

import motion_ba_model as M
import motion_pnp_inputs as PI
from motion_3d_inputs import rotation
from motion_pnp_model import compose, invert

FX, FY, CX, CY, WIDTH, HEIGHT = PI.FX, PI.FY, PI.CX, PI.CY, PI.WIDTH, PI.HEIGHT
BASELINE = 0.075
COUNTS = (1, 3, 4, 63, 64, 65, 255, 256, 257, 1100)                      # inliers of the pairs both entries are compared on
FIXED_BYTES = 256 * 27 * 4
LDS_LIMIT = PI.LDS_LIMIT
STAGE_CAP = (LDS_LIMIT - FIXED_BYTES) // (17 * 4)                       # 1761 points' state fits the LDS carve


def rigid(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], axis=1).reshape(12).astype(np.float32)


def pair(rng, m, outliers=0, extra=8, local=False, noise=0.5, depth_noise=0.01, start=(0.01, 0.02), outlier_px=(10.0, 40.0), nan_to=0.1, rows=None, depth=(1.5, 10.0)):
    """m inliers of a PnP between two views of one scene in section 4m's ranges: 0.5 px keypoint noise, 1 cm depth noise, a PnP-like start
    (the true transform turned by start[0] rad and moved by start[1] m); `outliers` of them have their to-keypoint moved by outlier_px; the
    frames hold `extra` more rows each (rows: pad both to this many), shuffled; a fraction nan_to of the to-points is NaN."""
    R, t, P, UV, C = PI.scene(rng, m, noise, depth=depth, angle=(0.02, 0.2), shift=0.3)
    uv_from = np.stack([FX * P[:, 0] / P[:, 2] + CX, FY * P[:, 1] / P[:, 2] + CY], axis=1) + rng.normal(size=(m, 2)) * noise
    planted = np.sort(rng.choice(m, outliers, replace=False)) if outliers else np.zeros(0, np.int64)
    for i in planted:
        a = rng.uniform(0, 2 * np.pi)
        UV[i] += rng.uniform(*outlier_px) * np.array([np.cos(a), np.sin(a)])
    Pn = P * (1 + rng.normal(size=(m, 1)) * depth_noise / np.maximum(P[:, 2:3], 1e-3))
    Cn = C * (1 + rng.normal(size=(m, 1)) * depth_noise / C[:, 2:3])
    Cn[rng.random(m) < nan_to] = np.nan
    true = invert(rigid(R, t))                                           # the to-camera's pose in the from-camera
    dR = rotation(rng.normal(size=3), start[0])
    guess = compose(rigid(dR, rng.normal(size=3) * start[1] / np.sqrt(3)), true)
    n_extra = extra if rows is None else rows - m
    ids = (rng.permutation(4 * (m + n_extra) + 64)[: m + 2 * n_extra] - m // 2).astype(np.int32)
    shared, only_f, only_t = ids[:m], ids[m:m + n_extra], ids[m + n_extra:]
    point, pixel = lambda k: rng.uniform(-3, 3, (k, 3)) + [0, 0, 5], lambda k: rng.uniform(0, 400, (k, 2))
    f_ids, f_xyz, f_uv = np.concatenate([shared, only_f]), np.concatenate([Pn, point(n_extra)]), np.concatenate([uv_from, pixel(n_extra)])
    t_ids, t_uv, t_xyz = np.concatenate([shared, only_t]), np.concatenate([UV, pixel(n_extra)]), np.concatenate([Cn, point(n_extra)])
    if local:                                                           # both cameras on the robot's base: points and transform in the base frame
        L = PI.LOCAL.astype(np.float64).reshape(3, 4)
        f_xyz, t_xyz = f_xyz @ L[:, :3].T + L[:, 3], t_xyz @ L[:, :3].T + L[:, 3]
        true, guess = (compose(compose(PI.LOCAL, x), invert(PI.LOCAL)) for x in (true, guess))
    pf, pt = rng.permutation(f_ids.shape[0]), rng.permutation(t_ids.shape[0])
    order = rng.permutation(m)
    where = {int(i): k for k, i in enumerate(order)}
    return dict(from_ids=f_ids[pf].astype(np.int32), from_xyz=f_xyz[pf].astype(np.float32), from_points=f_uv[pf].astype(np.float32),
                to_ids=t_ids[pt].astype(np.int32), to_points=t_uv[pt].astype(np.float32), to_xyz=t_xyz[pt].astype(np.float32),
                inliers=shared[order].astype(np.int32), transform=guess.astype(np.float32), true=true, local=local,
                planted=sorted(where[int(i)] for i in planted), m=m)


def camera(sized=True, local=False):
    return PI.camera(sized, local)


def args(p, from_points=True, to_xyz=True, **kw):
    """(positional, keyword) arguments of M.refine / motion_ba_cpu for a pair"""
    k = dict(from_points=p["from_points"] if from_points else None, to_xyz=p["to_xyz"] if to_xyz else None, camera_from=camera(True, p["local"]),
             camera_to=camera(True, p["local"]), baselines=(BASELINE, BASELINE), min_inliers=1)
    k.update(kw)
    return (p["from_ids"], p["from_xyz"], p["to_ids"], p["to_points"], p["inliers"], p["transform"]), k


def seeded(seed, m, **kw):
    return pair(np.random.default_rng(seed), m, **kw)


def count_pairs(seed=300):
    """one pair per entry of COUNTS, a tenth of the larger ones' inliers planted outliers"""
    rng = np.random.default_rng(seed)
    return [pair(rng, m, outliers=m // 10, local=(k % 3 == 1)) for k, m in enumerate(COUNTS)]


ACCURACY_SIZES = (60, 64, 70, 76, 84, 92, 100, 112, 128, 160, 220, 300)
ACCURACY_PRIOR = (1e-4, 4e-4)


def accuracy_pairs(seed=900):
    """Twelve pairs in section 4m's ranges for the comparison with the yardstick: 60 to 300 inliers, 0.5 px keypoint noise, 1 cm depth noise, a
    PnP-like start, every third pair behind a local transform.  The outliers are planted where no residual can lie near the threshold: 30 to
    60 px off (the floor is 10 px), on points whose to-edge is stereo (every to-point finite: a mono to-edge lets the point absorb part of an
    offset along the epipolar line), and few (max(2, m / 40)): many large outliers pull the pose until a near point passes delta."""
    rng = np.random.default_rng(seed)
    return [pair(rng, m, outliers=max(2, m // 40), local=(k % 3 == 1), outlier_px=(30.0, 60.0), nan_to=0.0) for k, m in enumerate(ACCURACY_SIZES)]


# ---- hand-made cases, one branch each (test_motion_ba_inputs.py proves them)

def mixed_edges_pair(seed=310, m=40):
    """every to-point NaN or at depth <= 0 on half of the rows: those points have a stereo from-edge and a mono to-edge"""
    p = seeded(seed, m, nan_to=0.5)
    return p


def to_only_pair(seed=602):
    """eight to-keypoints 5 .. 60 px off, each flagged through both of its edges; another point is flagged after stage 1 through its to-edge
    alone: it is reset and its from-edge stays in the second stage (the seed was searched for; the test proves it)"""
    return pair(np.random.default_rng(seed), 40, outliers=8, outlier_px=(5.0, 60.0))


def late_outlier_pair(seed=616):
    """as to_only_pair; one point passes the test behind stage 1 and is flagged behind stage 2, when the large outliers no longer pull the pose"""
    return pair(np.random.default_rng(seed), 40, outliers=8, outlier_px=(5.0, 60.0))


def between_thresholds_pair(seed=313, m=60):
    """one to-keypoint 12 px off: the chi2 of its edges lies between delta = 8 and delta^2 = 64; the reference's `> delta` flags it"""
    return seeded(seed, m, outliers=1, outlier_px=(12.0, 12.0), noise=0.1)


def nan_pair(seed=314, m=30):
    """a NaN to-keypoint among the inliers: the cost is NaN from the start"""
    p = seeded(seed, m)
    row = int(np.flatnonzero(p["to_ids"] == p["inliers"][3])[0])
    p["to_points"][row, 0] = np.nan
    return p


def huge_pair(seed=315, m=30):
    """a to-keypoint 1e7 px away and no robust kernel: the cost stays above 1e12"""
    p = seeded(seed, m)
    row = int(np.flatnonzero(p["to_ids"] == p["inliers"][3])[0])
    p["to_points"][row, 0] = 1e7
    return p


def narrow_pair(seed=316, m=900):
    """only the inliers whose to-keypoint lies within 20 px of the image's middle column: the smaller eigenvalue of their distribution is
    (40 / 640)^2 / 12 ~ 3e-4"""
    p = seeded(seed, m)
    row = {int(i): r for r, i in enumerate(p["to_ids"].tolist())}
    keep = [k for k, i in enumerate(p["inliers"].tolist()) if abs(p["to_points"][row[i], 0] - 320.0) < 20.0]
    p["inliers"] = p["inliers"][keep]
    p["m"] = len(keep)
    return p


def status_batch(seed=320):
    """(pairs, per-pair keyword overrides, the expected statuses): every status in one launch"""
    ok = seeded(seed, 70, outliers=5)
    no_transform = seeded(seed + 1, 20)
    no_transform["transform"] = np.zeros(12, np.float32)
    no_inliers = seeded(seed + 2, 20)
    no_inliers["n_inliers"] = 0
    bad = seeded(seed + 3, 20)
    bad["inliers"] = bad["inliers"].copy()
    bad["inliers"][7] = bad["to_ids"].max() + 5                          # occurs in neither frame
    twice = seeded(seed + 4, 20)
    twice["to_ids"] = twice["to_ids"].copy()
    other = int(np.flatnonzero(twice["to_ids"] != twice["inliers"][2])[0])
    twice["to_ids"][other] = twice["inliers"][2]                        # occurs twice in the to-frame
    few = seeded(seed + 5, 24, outliers=6)
    far = seeded(seed + 6, 50, depth=(8.0, 10.0))
    pairs = [ok, no_transform, no_inliers, bad, twice, nan_pair(), few, far, narrow_pair()]
    expect = [M.OK, M.NO_INPUT, M.NO_INPUT, M.BAD_INLIER, M.BAD_INLIER, M.DIVERGED, M.BELOW_MIN_INLIERS, M.MEAN_DISTANCE_REJECTED, M.DISTRIBUTION_REJECTED]
    return pairs, expect


STATUS_KW = dict(min_inliers=20, max_inliers_mean_distance=7.5, min_inliers_distribution=0.01)


def concatenate(pairs, from_points=True, to_xyz=True):
    """the arrays of Engine.refine_motion_ba for the pairs: every pair's inliers at the front of its to-region"""
    cat = lambda k, dt: np.concatenate([p[k] for p in pairs]).astype(dt)
    fo = np.cumsum([0] + [p["from_ids"].shape[0] for p in pairs]).astype(np.int64)
    to = np.cumsum([0] + [p["to_ids"].shape[0] for p in pairs]).astype(np.int64)
    inl = np.zeros(int(to[-1]), np.int32)
    for p, o in zip(pairs, to[:-1]):
        inl[o:o + p["inliers"].shape[0]] = p["inliers"]
    n_in = np.array([p.get("n_inliers", p["inliers"].shape[0]) for p in pairs], np.int32)
    tr = np.stack([p["transform"] for p in pairs]).astype(np.float32)
    return dict(from_ids=cat("from_ids", np.int32), from_xyz=cat("from_xyz", np.float32), from_offsets=fo, to_ids=cat("to_ids", np.int32),
                to_points=cat("to_points", np.float32), to_offsets=to, inliers=inl, n_inliers=n_in, transforms=tr,
                from_points=cat("from_points", np.float32) if from_points else None, to_xyz=cat("to_xyz", np.float32) if to_xyz else None,
                cameras_from=[camera(True, p["local"]) for p in pairs], cameras_to=[camera(True, p["local"]) for p in pairs])
