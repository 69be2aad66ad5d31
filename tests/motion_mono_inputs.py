"""Inputs of the lcd_estimate_motion_mono tests: synthetic two-view scenes in the style of tests/epipolar_inputs.py (640 x 480, f = 525), and the
constants of the scenes whose winners were found with the model alone (tests/motion_mono_model.py)."""
import numpy as np

CAMERA = (525.0, 525.0, 319.5, 239.5)
CAMERA_DICT = dict(fx=CAMERA[0], fy=CAMERA[1], cx=CAMERA[2], cy=CAMERA[3])
LOCAL = np.array([0, 0, 1, 0.1, -1, 0, 0, 0.0, 0, -1, 0, 0.3], np.float32)   # the optical rotation of a forward-looking camera, and a lever arm


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def scene(seed, m=40, outliers=0.0, noise=0.0, max_rot_deg=12.0, max_baseline=0.4, extra=5, pure_rotation=False, shuffle=True):
    """m correspondences of a rigid scene (depths 1 .. 8 m) seen from two poses, x2 ~ R x1 + t; a share of planted outliers (the to keypoint
    drawn anew); `extra` rows per frame without a partner and one repeated id per frame, which the join drops.  -> dict(from_ids,
    from_points, from_points3 (the true points, from-camera frame), to_ids, to_points, R, t, outlier_ids)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = CAMERA
    R = rotation(*(np.deg2rad(max_rot_deg) * rng.uniform(-1, 1, 3)))
    t = np.zeros(3) if pure_rotation else max_baseline * rng.uniform(-1, 1, 3)
    P = np.zeros((0, 3))
    while P.shape[0] < m:
        u, v, z = rng.uniform(20, 620, 4 * m), rng.uniform(20, 460, 4 * m), rng.uniform(1.0, 8.0, 4 * m)
        X = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
        Y = X @ R.T + t
        ok = (Y[:, 2] > 0.5)
        u2, v2 = fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy
        ok &= (u2 > 0) & (u2 < 640) & (v2 > 0) & (v2 < 480)
        P = np.concatenate([P, X[ok]])[:m]
    Y = P @ R.T + t
    p1 = np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], 1) + noise * rng.standard_normal((m, 2))
    p2 = np.stack([fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy], 1) + noise * rng.standard_normal((m, 2))
    ids = rng.choice(np.arange(1, 20 * m + 100), m, replace=False).astype(np.int32)
    n_out = int(round(outliers * m))
    bad = rng.choice(m, n_out, replace=False)
    # a planted outlier lies at least 30 px from the true epipolar line in both images
    Kinv = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]])
    F = Kinv.T @ (np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R) @ Kinv
    for i in bad:
        for _ in range(1000):
            q = np.array([rng.uniform(0, 640), rng.uniform(0, 480), 1.0])
            l2, l1 = F @ np.array([p1[i, 0], p1[i, 1], 1.0]), F.T @ q
            d2 = abs(q @ l2) / max(np.hypot(l2[0], l2[1]), 1e-300)
            d1 = abs(np.array([p1[i, 0], p1[i, 1], 1.0]) @ l1) / max(np.hypot(l1[0], l1[1]), 1e-300)
            if pure_rotation or (d1 >= 30 and d2 >= 30):
                break
        p2[i] = q[:2]
    # rows without a partner, a repeated id and a negative id that both frames hold
    far = 100000
    fi = np.concatenate([ids, far + np.arange(extra), [ids[0], -7]]).astype(np.int32) if extra else ids.copy()
    ti = np.concatenate([ids, 2 * far + np.arange(extra), [ids[1], -7]]).astype(np.int32) if extra else ids.copy()
    ne = fi.shape[0] - m
    fp = np.concatenate([p1, rng.uniform(0, 480, (ne, 2))]).astype(np.float32)
    tp = np.concatenate([p2, rng.uniform(0, 480, (ne, 2))]).astype(np.float32)
    f3 = np.concatenate([P, rng.uniform(1, 8, (ne, 3))]).astype(np.float32)
    if shuffle:
        a, b = rng.permutation(fi.shape[0]), rng.permutation(ti.shape[0])
        fi, fp, f3, ti, tp = fi[a], fp[a], f3[a], ti[b], tp[b]
    dropped = {int(ids[0]), int(ids[1])} if extra else set()
    return dict(from_ids=fi, from_points=fp, from_points3=f3, to_ids=ti, to_points=tp, R=R, t=t,
                outlier_ids=sorted(int(i) for i in ids[bad] if int(i) not in dropped))


def batch(scenes):
    """concatenate scenes -> (from_ids, from_points, from_points3, from_offsets, to_ids, to_points, to_offsets)"""
    fo = np.concatenate([[0], np.cumsum([s["from_ids"].shape[0] for s in scenes])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([s["to_ids"].shape[0] for s in scenes])]).astype(np.int64)
    cat = lambda k, w, dt: np.concatenate([np.asarray(s[k], dt).reshape(-1, w) for s in scenes]) if scenes else np.zeros((0, w), dt)
    return (cat("from_ids", 1, np.int32).reshape(-1), cat("from_points", 2, np.float32), cat("from_points3", 3, np.float32), fo,
            cat("to_ids", 1, np.int32).reshape(-1), cat("to_points", 2, np.float32), to)


# ---- scenes whose winners were found with the model alone (a search over seeds 3000 .. 4499 of scene(seed, rows, **kw) with iterations = 8,
# min_inliers = 8 and the call's seed = the scene's).  Each row: (seed, rows, kw, what the model's trace must show).
SEARCH_KW = dict(iterations=8, min_inliers=8)
FOUND = [
    (3000, 12, dict(noise=0.8, outliers=0.15), dict(roots=("roots2", "roots4", "roots6"), winner_r=5, config=2)),
    (3010, 22, dict(noise=0.4, outliers=0.15), dict(roots=("roots0",))),            # no real root: an invalid hypothesis
    (3081, 33, dict(noise=0.8, outliers=0.15), dict(roots=("roots8",))),
    (3089, 41, dict(noise=0.0, outliers=0.0), dict(roots=("roots10",))),
    (3001, 13, dict(noise=0.8, outliers=0.15), dict(winner_r=0, config=3)),
    (3007, 19, dict(noise=0.0, outliers=0.0), dict(winner_r=1)),
    (3004, 16, dict(noise=0.0, outliers=0.3), dict(winner_r=2, tie=[3, 3, 0, 0], config=0)),   # counts 1 and 2 tie: the first >= takes (R1, t)
    (3002, 14, dict(noise=0.8, outliers=0.15), dict(winner_r=3, config=0)),
    (3005, 17, dict(noise=0.0, outliers=0.3), dict(winner_r=4, config=1)),
    (4083, 15, dict(noise=0.4, outliers=0.3), dict(winner_r=6)),
    (3478, 40, dict(noise=0.4, outliers=0.15), dict(winner_r=7)),
    (3211, 13, dict(noise=0.8, outliers=0.3), dict(winner_r=9)),
    (3167, 29, dict(noise=0.8, outliers=0.3), dict(tie=[1, 3, 0, 3], config=1)),     # counts 2 and 4 tie: the second >= takes (R2, t)
    (3230, 32, dict(noise=0.8, outliers=0.3), dict(tie=[4, 0, 4, 0], config=0)),     # counts 1 and 3 tie
]
# Classes the search did not find, and which no test therefore holds the device to:
#   - a winner that is its hypothesis' root 8 (roots 0 .. 7 and 9 win above; ten real roots occur);
#   - a tie of the counts (1, 4), (2, 3), (3, 4) or of three or four positive counts (the all-zero tie is test_parallel_rays_give_no_point's);
#   - a hypothesis invalid by its null space's pivot, its polynomial's leading coefficient, its bound or its draws (the constraint matrix'
#     zero pivot is met by the identity motion; zero real roots above);
#   - a candidate whose root leaves an x, y or entry that is not finite, other than under the scaled cameras;
#   - a triangulation whose determinant is exactly 0 under a valid model.


def found_scene(k):
    seed, rows, kw, _ = FOUND[k]
    return scene(seed, rows, **kw)


# ---- the twelve accuracy scenes: 640 x 480, f = 525, depths 1 .. 8 m, up to +-12 degrees and +-0.4 m per axis, 0.5 px noise, m from 60 to 300,
# 40 % planted outliers at least 30 px from the true epipolar line in both images
def accuracy_scenes():
    return [scene(500 + k, 60 + (240 * k) // 11 + 2, outliers=0.4, noise=0.5) for k in range(12)]


# ---- powers of two
def scaled(p, k):
    """the scene with every keypoint coordinate and the camera's fx, fy, cx, cy times 2^k (the caller scales the threshold alike): the
    normalised coordinates, and so every result, keep their bits"""
    f = np.float32(2.0 ** k)
    return dict(p, from_points=p["from_points"] * f, to_points=p["to_points"] * f, camera=tuple(float(np.float32(c) * f) for c in p.get("camera", CAMERA)))


def telephoto(seed, k, m=60):
    """A camera of f = 525 x 2^k that moves forward and rolls, so that the scene stays in the 640 x 480 image whatever f is: the geometry is
    a true essential geometry whose normalised coordinates are of the order 2^-k.  The threshold scales with them by itself (it is divided
    by (fx + fy) / 2).  With k = 10 and k = 20 the model's fp64 workspace spans 9e-16 .. 9e21 and 8e-28 .. 1.3e40 and the pair passes
    through the decomposition, the triangulation and the scale; from k = 30 on the float32 keypoints no longer resolve the motion."""
    rng = np.random.default_rng(seed)
    f = 525.0 * 2.0 ** k
    cx, cy = CAMERA[2], CAMERA[3]
    a = np.deg2rad(5.0 * rng.uniform(-1, 1))
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    t = np.array([0, 0, 0.3 * rng.uniform(0.5, 1)])
    u, v, z = rng.uniform(40, 600, m), rng.uniform(40, 440, m), rng.uniform(2, 8, m)
    X = np.stack([(u - cx) / f * z, (v - cy) / f * z, z], 1)
    Y = X @ R.T + t
    p1 = np.stack([f * X[:, 0] / X[:, 2] + cx, f * X[:, 1] / X[:, 2] + cy], 1)
    p2 = np.stack([f * Y[:, 0] / Y[:, 2] + cx, f * Y[:, 1] / Y[:, 2] + cy], 1)
    ids = np.arange(1, m + 1, dtype=np.int32)
    return dict(from_ids=ids, from_points=p1.astype(np.float32), from_points3=X.astype(np.float32), to_ids=ids.copy(), to_points=p2.astype(np.float32),
                camera=(f, f, cx, cy), R=R, t=t)
