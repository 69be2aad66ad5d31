"""Inputs for lcd_refine_motion_ba's tests, built on motion_pnp_inputs.scene.  A pair is a dict with the frames (from_ids, from_xyz, from_points,
to_ids, to_points, to_xyz), the PnP's result (inliers, transform) and what the generator knows about it (the planted outliers as indices into
`inliers`, the true transform).  args(pair, ...) gives the keyword arguments of motion_ba_model.refine / vwdictionary.motion_ba_cpu.
tests/test_motion_ba_inputs.py proves without a GPU that each hand-made case takes the branch it exists for."""
import numpy as np

import motion_ba_model as M
import motion_3d_inputs as T3
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


def cameras_of(p):
    """(from, to): a pair's own cameras when it carries them, else the one sized camera behind its `local`"""
    return p.get("camera_from", camera(True, p["local"])), p.get("camera_to", camera(True, p["local"]))


def args(p, from_points=True, to_xyz=True, **kw):
    """(positional, keyword) arguments of M.refine / motion_ba_cpu for a pair"""
    cf, ct = cameras_of(p)
    k = dict(from_points=p["from_points"] if from_points else None, to_xyz=p["to_xyz"] if to_xyz else None, camera_from=cf, camera_to=ct,
             baselines=(BASELINE, BASELINE), min_inliers=1)
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
                cameras_from=[cameras_of(p)[0] for p in pairs], cameras_to=[cameras_of(p)[1] for p in pairs])


# ---------------------------------------------------------------------------------------------------------------------------------------
# Inputs for the places where the kernel's two sides, its join, its staged state, its per-pair arguments and its gates change shape
# (tests/test_gpu_motion_ba_shapes.py).  tests/test_motion_ba_inputs.py proves each one with the model's trace.

INT32_MIN, INT32_MAX = T3.INT32_MIN, T3.INT32_MAX
# two cameras that share nothing: fx != fy on both sides, every intrinsic and the image size differ between the sides
CAMERA_FROM = dict(fx=500.0, fy=540.0, cx=310.5, cy=250.25, image_width=640, image_height=512)
CAMERA_TO = dict(fx=610.0, fy=585.0, cx=335.25, cy=228.5, image_width=672, image_height=464)
TWO_BASELINES = (0.12, 0.075)
LOCAL_SIDES = ("to", "from", None)


def rescaled(uv, cam):
    """keypoints of the generator's camera (FX, FY, CX, CY) as cam sees the same rays: (uv - c) f' / f + c', in float64, then cast"""
    uv = np.asarray(uv, np.float64)
    return ((uv - [CX, CY]) * [cam["fx"] / FX, cam["fy"] / FY] + [cam["cx"], cam["cy"]]).astype(np.float32)


def two_camera_pair(seed, m, local_side, camera_from=CAMERA_FROM, camera_to=CAMERA_TO, **kw):
    """pair(...) seen by two different cameras: the keypoints are re-expressed per side, PI.LOCAL stands on the side local_side names ("from",
    "to", "both" or None): that side's 3-D points are in its base frame, and the start and the true transform are T L^-1 ("to"), L T
    ("from"), L T L^-1 ("both").  The pair carries its own camera_from and camera_to."""
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    p = pair(rng, m, local=False, **kw)
    L = PI.LOCAL.astype(np.float64).reshape(3, 4)
    based = lambda xyz: (xyz.astype(np.float64) @ L[:, :3].T + L[:, 3]).astype(np.float32)
    cf, ct = dict(camera_from), dict(camera_to)
    p["from_points"], p["to_points"] = rescaled(p["from_points"], cf), rescaled(p["to_points"], ct)
    if local_side in ("from", "both"):
        cf["local_transform"] = PI.LOCAL
        p["from_xyz"] = based(p["from_xyz"])
        p["transform"], p["true"] = (compose(PI.LOCAL, x) for x in (p["transform"], p["true"]))
    if local_side in ("to", "both"):
        ct["local_transform"] = PI.LOCAL
        p["to_xyz"] = based(p["to_xyz"])
        p["transform"], p["true"] = (compose(x, invert(PI.LOCAL)) for x in (p["transform"], p["true"]))
    p["transform"] = p["transform"].astype(np.float32)
    p.update(camera_from=cf, camera_to=ct, local_side=local_side)
    return p


def two_camera_batch(seed=700):
    """one pair per side of the local transform (to, from, none) and one with it on both sides, 30 to 70 inliers, a tenth planted outliers"""
    rng = np.random.default_rng(seed)
    return [two_camera_pair(rng, m, side, outliers=m // 10) for m, side in zip((50, 70, 30, 64), LOCAL_SIDES + ("both",))]


TWO_CAMERA_SIZES = ACCURACY_SIZES


def two_camera_accuracy_pairs(seed=950):
    """accuracy_pairs()'s recipe and sizes on two-camera pairs: twelve pairs of 60 to 300 inliers, the local transform on the to side, the from side, on
    none, in turn; outliers 30 to 60 px off on stereo to-edges"""
    rng = np.random.default_rng(seed)
    return [two_camera_pair(rng, m, LOCAL_SIDES[k % 3], outliers=max(2, m // 40), outlier_px=(30.0, 60.0), nan_to=0.0) for k, m in enumerate(TWO_CAMERA_SIZES)]


def id_pair(seed, f_ids, t_ids, inliers, **kw):
    """a pair whose frames hold exactly the ids f_ids and t_ids, rows shuffled, with one scene point of pair(...) behind every distinct id (the
    rows of an id that stands twice in a frame are copies); inliers: the id list as it is given, whether the frames hold its ids or not"""
    rng = np.random.default_rng(seed)
    every = sorted(set(f_ids) | set(t_ids))
    base = pair(rng, max(len(every), 1), extra=0, nan_to=0.0, **kw)
    F, T = np.argsort(base["from_ids"]), np.argsort(base["to_ids"])     # both frames hold the same ids: position j is one point on both sides
    at = {i: j for j, i in enumerate(every)}
    jf, jt = np.array([at[i] for i in f_ids], np.int64), np.array([at[i] for i in t_ids], np.int64)
    pf, pt = rng.permutation(len(f_ids)), rng.permutation(len(t_ids))
    ids = lambda v: np.array(v, np.int64).astype(np.int32)
    return dict(from_ids=ids(f_ids)[pf], from_xyz=base["from_xyz"][F][jf][pf], from_points=base["from_points"][F][jf][pf], to_ids=ids(t_ids)[pt],
                to_points=base["to_points"][T][jt][pt], to_xyz=base["to_xyz"][T][jt][pt], inliers=ids(inliers), transform=base["transform"],
                true=base["true"], local=False, planted=[], m=len(inliers))


def extreme_id_pairs(seed=720):
    """name -> (pair, status): frames of T3.EXTREME_ROWS rows over T3.EXTREME_IDS (motion_3d_inputs.extreme_id_lists), INT32_MAX's key next to
    the all-ones padding keys, and the small frames.  The OK pairs have INT32_MIN, -1, 0, 1 and INT32_MAX among their inliers, INT32_MAX
    the largest key of both frames; every other pair has exactly one reason to be LCD_BA_BAD_INLIER (or, with no inliers, NO_INPUT)."""
    rng = np.random.default_rng(seed)
    nf, nt = T3.EXTREME_ROWS
    out = {}
    lists = {case: T3.extreme_id_lists(rng, case, nf, nt) for case in range(3)}
    shared = lambda f, t: [i for i in f if i in set(t)]

    def add(name, status, f, t, inliers, **more):
        p = id_pair(seed + 1 + len(out), f, t, inliers)
        p.update(more)
        out[name] = (p, status)
        return p
    f0, t0 = lists[0]
    add("ok", M.OK, f0, t0, shared(f0, t0))                             # INT32_MIN + 1 is in `from` only and no inlier
    six = t0[:-1] + [INT32_MIN + 1]
    add("ok_six", M.OK, f0, six, shared(f0, six))                      # all six extreme ids
    without = lambda ids, i: [j for j in ids if j != i]
    add("above_every_key", M.BAD_INLIER, without(f0, INT32_MAX), without(t0, INT32_MAX), shared(f0, t0))    # lo >= n in both frames
    add("below_every_key", M.BAD_INLIER, without(f0, INT32_MIN), without(t0, INT32_MIN), shared(f0, t0))
    f1, t1 = lists[1]
    add("max_twice_in_to", M.BAD_INLIER, f1, t1, shared(f1, without(t1, INT32_MIN + 1)))
    f2, t2 = lists[2]
    add("max_twice_in_from", M.BAD_INLIER, f2, t2, shared(without(f2, INT32_MIN + 1), t2)[:-1])     # (shared() lists the doubled id twice)
    add("in_to_only", M.BAD_INLIER, f0, t0, shared(f0, t0)[:4] + [t0[-1]])
    add("in_from_only", M.BAD_INLIER, f0, t0, shared(f0, t0)[:4] + [INT32_MIN + 1])
    add("twice_in_from", M.BAD_INLIER, f0[:-1] + [f0[7]], t0, shared(f0, t0))                       # an ordinary shared id
    p = add("from_point_not_finite", M.BAD_INLIER, f0, t0, shared(f0, t0))
    p["from_xyz"][p["from_ids"] == 1, 1] = np.inf
    add("count_negative", M.BAD_INLIER, f0, t0, shared(f0, t0), n_inliers=-1)
    add("count_above_rows", M.BAD_INLIER, f0, t0, shared(f0, t0) + t0[-(nt - len(shared(f0, t0))):], n_inliers=nt + 1)
    add("rows_0_from", M.BAD_INLIER, [], t0[:5], t0[:3])
    add("rows_0_to_none", M.NO_INPUT, f0[:5], [], [], n_inliers=0)
    add("rows_0_to_one", M.BAD_INLIER, f0[:5], [], [], n_inliers=1)
    add("rows_1", M.OK, [INT32_MAX], [INT32_MAX], [INT32_MAX])
    add("rows_1_70", M.OK, [INT32_MAX], t0, [INT32_MAX])
    add("rows_2", M.OK, [INT32_MAX, INT32_MIN], [INT32_MIN, INT32_MAX], [INT32_MIN, INT32_MAX])
    add("rows_2_missing", M.BAD_INLIER, [7, INT32_MIN], [INT32_MIN, 7], [INT32_MIN, INT32_MAX])    # p2 = 2: no padding key to match
    return out


TO_EDGE_ROWS = (2, 11, 29)                                              # indices into the inliers
TO_EDGE_KINDS = ("nan", "inf", "zero", "negative")


def to_edge_pair(kind, seed=730, m=40):
    """a pair of m inliers whose to-points are all finite but for TO_EDGE_ROWS: one coordinate (x, y, z in turn) NaN or +inf, or the depth
    exactly 0, or negative.  Each of those to-edges is mono."""
    p = seeded(seed + TO_EDGE_KINDS.index(kind), m, nan_to=0.0)
    for c, i in enumerate(TO_EDGE_ROWS):
        row = int(np.flatnonzero(p["to_ids"] == p["inliers"][i])[0])
        if kind in ("nan", "inf"):
            p["to_xyz"][row, c % 3] = np.nan if kind == "nan" else np.inf
        else:
            p["to_xyz"][row, 2] = 0.0 if kind == "zero" else -p["to_xyz"][row, 2]
    return p


def no_finite_to_pair(seed=735, m=40):
    """every inlier's to-point has one coordinate that is not finite (NaN, +inf, -inf in x, y, z in turn): no survivor counts for the mean distance"""
    p = seeded(seed, m, nan_to=0.0)
    for i in range(m):
        row = int(np.flatnonzero(p["to_ids"] == p["inliers"][i])[0])
        p["to_xyz"][row, i % 3] = (np.nan, np.inf, -np.inf)[(i // 3) % 3]
    return p


# to-cameras that are not valid for reprojection, in the style of PI.CAMERA_CASES: each fails one condition of the distribution gate only
GATE_CAMERAS = (dict(CAMERA_TO, cx=0.0), dict(CAMERA_TO, cy=-1.0), dict(CAMERA_TO, image_width=0), dict(CAMERA_TO, image_height=0))
GATES_KW = dict(max_inliers_mean_distance=7.5, min_inliers_distribution=0.01)


def gate_camera_pairs(seed=740):
    """one narrow pair (narrow_pair's selection: a valid camera would reject its distribution) per camera of GATE_CAMERAS"""
    pairs = []
    for k, cam in enumerate(GATE_CAMERAS):
        p = two_camera_pair(seed + k, 600, (None, "to")[k % 2], camera_to=cam)
        pairs.append(narrowed(p, cam["cx"], 20.0 * cam["fx"] / FX))
    return pairs


def narrowed(p, centre, half):
    """p with only the inliers whose to-keypoint lies within `half` px of the column `centre`"""
    row = {int(i): r for r, i in enumerate(p["to_ids"].tolist())}
    keep = [k for k, i in enumerate(p["inliers"].tolist()) if abs(p["to_points"][row[i], 0] - centre) < half]
    p["inliers"] = p["inliers"][keep]
    p["m"] = len(keep)
    return p


def far_narrow_pair(seed=745, m=900):
    """far (depths 8 to 10 m) and narrow: either gate alone rejects it, so the first one, the mean distance, does"""
    return narrowed(seeded(seed, m, depth=(8.0, 10.0)), 320.0, 20.0)


PRIOR_FLOORS = ((0.0, 0.0), (1e-8, 3e-8))                               # at and below LINEAR_EPSILON / ANGULAR_EPSILON: both informations are the floor's


def per_pair_kw(pairs, period=None):
    """dict(prior=[n x 2], baselines=[n x 2]): row k differs from every other row (of the same period, if given: row k = row k % period);
    every third row's prior variances are PRIOR_FLOORS', in turn"""
    n = len(pairs)
    k = np.arange(n) % (period or max(n, 1))
    prior = np.stack([1e-4 * (1 + k), 4e-4 * (1 + 0.5 * k)], axis=1)
    for j in range(n):
        if k[j] % 3 == 0:
            prior[j] = PRIOR_FLOORS[(k[j] // 3) % 2]
    baselines = np.stack([0.05 + 0.01 * k, 0.2 - 0.01 * k], axis=1)
    return dict(prior=prior, baselines=baselines)


MANY_SIZES = (3, 4, 9, 17, 33, 40, 64, 65)
MANY_PAIRS, MANY_PERIOD = 320, 9                                        # more pairs than an MI355X has compute units (256)


def many_pairs(seed=750):
    """eight distinct pairs of 3 to 65 inliers, every other one a two-camera pair"""
    rng = np.random.default_rng(seed)
    return [two_camera_pair(rng, m, LOCAL_SIDES[k % 3], outliers=m // 10) if k % 2 else pair(rng, m, outliers=m // 10, local=(k % 4 == 0))
            for k, m in enumerate(MANY_SIZES)]


def staging_pairs(seed=760):
    """[STAGE_CAP + 1 inliers in 1800 rows, 40 inliers, STAGE_CAP + 1 inliers in 1790 rows]: two pairs whose state is read from the scratch at
    strides that are not their inlier counts, the second one's behind the first's, and a staged pair between them"""
    n = STAGE_CAP + 1
    return [seeded(seed, n, outliers=n // 20, rows=1800), seeded(seed + 1, 40, outliers=4), seeded(seed + 2, n, outliers=n // 20, rows=1790)]


def wide_pair(seed=770):
    """8192 rows a side and 100 inliers: the state is staged in LDS over the carve that held 2 x 8192 keys"""
    return seeded(seed, 100, outliers=10, rows=8192)


def nine_row_pair(seed=771):
    return seeded(seed, 5, rows=9)


_made = {}


def made(name, *args):
    """a generator's result, built once per process: the GPU tests cache the model's results per pair object"""
    if (name,) + args not in _made:
        _made[(name,) + args] = globals()[name](*args)
    return _made[(name,) + args]
