"""motion_mono_cpu (rtabmap_amd/host/MotionMono.cpp, the engine's arithmetic compiled for the host) against the Python model of the rule, bit for
bit -- ints and float bits -- on every generator of the GPU tests; the model against the planted truth; the stand-alone sanitizer driver's
count of clean cases; and the rule's accuracy against an independent float64 yardstick.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import motion_mono_inputs as I
import motion_mono_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZER_CASES = 102                                                      # tools/sanitize_motion_mono.cpp prints "ok 102"
KW = dict(min_inliers=8, iterations=20, reproj_threshold=2.0, variance_median_ratio=4, max_variance=0.1, distance_threshold=50.0, seed=5)
GUESS = np.array([1, 0, 0, 0.3, 0, 1, 0, -0.2, 0, 0, 1, 0.6], np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64).tobytes()


def both(p, camera=I.CAMERA, use3=False, local=None, guess=None, **kw):
    from rtabmap_amd import vwdictionary as V
    kw = dict(KW, **kw)
    f3 = p["from_points3"] if use3 else None
    want = M.model(p["from_ids"], p["from_points"], p["to_ids"], p["to_points"], camera, from_points3=f3, local_transform=local, guess=guess, **kw)
    got = V.motion_mono_cpu(p["from_ids"], p["from_points"], p["to_ids"], p["to_points"], camera, from_points3=f3, local_transform=local, guess=guess, **kw)
    assert got is not None
    assert got["status"] == want["status"], (got["status"], want["status"])
    assert got["matches"].tolist() == want["matches"] and got["inliers"].tolist() == want["inliers"]
    assert bits(got["transform"]) == bits(want["transform"]), (got["transform"], want["transform"])
    assert bits(np.array([got["variance"]])) == bits(np.array([want["variance"]])), (got["variance"], want["variance"])
    assert bits(got["points3"]) == bits(want["points3"])
    return want


def with_m(m, seed=None, **kw):
    return I.scene(1000 + m if seed is None else seed, m + 2, **kw)


def clean():
    return with_m(60, seed=77)


def filled(v):
    p = clean()
    return dict(p, from_points3=np.full_like(p["from_points3"], v))


def broken(v):
    p = clean()
    fp, tp = p["from_points"].copy(), p["to_points"].copy()
    fp[7, 0], tp[11, 1] = v, v
    return dict(p, from_points=fp, to_points=tp)


CASES = [("m%d" % m, lambda m=m: with_m(m, outliers=0.2, noise=0.3), {}) for m in (8, 9, 63, 64, 65, 257)]
CASES += [("iterations%d" % n, lambda: with_m(64, outliers=0.2, noise=0.3), dict(iterations=n)) for n in (1, 25, 26, 31, 32, 33, 52, 64, 65)]
CASES += [("few_features", lambda: with_m(20), dict(min_inliers=40)), ("rotation", lambda: with_m(40, seed=4, pure_rotation=True), {}),
          ("identity", lambda: dict(clean(), to_ids=clean()["from_ids"], to_points=clean()["from_points"]), {}),
          ("guess", clean, dict(guess=GUESS, max_variance=100.0)), ("points", clean, dict(use3=True, max_variance=100.0)),
          ("both", clean, dict(use3=True, guess=GUESS, max_variance=100.0)), ("local", clean, dict(use3=True, local=I.LOCAL, max_variance=100.0)),
          ("zero_guess", clean, dict(guess=np.zeros(12, np.float32))), ("nan_guess", clean, dict(guess=np.full(12, np.nan, np.float32))),
          ("large", lambda: I.scene(10, 3000, extra=0, outliers=0.3, noise=0.3), dict(iterations=6, use3=True, guess=GUESS, max_variance=100.0))]
CASES += [("points3_%s" % v, lambda v=v: filled(v), dict(use3=True)) for v in (np.nan, np.inf, 0.0)]
CASES += [("keypoint_%s" % v, lambda v=v: broken(v), dict(use3=True, iterations=40, max_variance=100.0)) for v in (np.nan, np.inf, -np.inf)]
CASES += [("ratio%d_%s" % (r, "guess" if g else "points"), clean, dict(use3=True, variance_median_ratio=r, max_variance=100.0, guess=GUESS if g else None))
          for r in (0, 1, 4, 6, 31) for g in (0, 1)]
CASES += [("camera2^%d" % k, clean, dict(use3=True, max_variance=1e30, camera=(I.CAMERA[0] * 2.0 ** k, I.CAMERA[1] * 2.0 ** k, I.CAMERA[2], I.CAMERA[3])))
          for k in (20, -20, 60, -60)]
CASES += [("telephoto2^%d" % k, lambda k=k: I.telephoto(5, k), dict(use3=True, max_variance=1e30, camera=I.telephoto(5, k)["camera"])) for k in (10, 20, 30)]
CASES += [("pixels2^%d" % k, lambda k=k: I.scaled(clean(), k), dict(use3=True, max_variance=1e30, reproj_threshold=2.0 * 2.0 ** k,
                                                                  camera=I.scaled(clean(), k)["camera"])) for k in (-20, 40)]
CASES += [("found%d" % k, lambda k=k: I.found_scene(k), dict(I.SEARCH_KW, seed=I.FOUND[k][0])) for k in range(len(I.FOUND))]


@pytest.mark.parametrize("name,make,kw", CASES, ids=[c[0] for c in CASES])
def test_the_mirror_equals_the_model(name, make, kw):
    both(make(), **kw)


def test_the_found_scenes_show_what_they_were_found_for():
    for k, (seed, rows, kw, show) in enumerate(I.FOUND):
        p = I.found_scene(k)
        t = M.model(p["from_ids"], p["from_points"], p["to_ids"], p["to_points"], I.CAMERA, seed=seed, **I.SEARCH_KW)["trace"]
        for r in show.get("roots", ()):
            assert r in t["hypotheses"], (k, r, t["hypotheses"])
        if "winner_r" in show:
            assert t["winner"][1] == show["winner_r"], (k, t["winner"])
        if "tie" in show:
            assert t["counts"] == show["tie"], (k, t["counts"])
        if "config" in show:
            assert t["config"] == show["config"], (k, t["config"])


def test_the_model_recovers_a_planted_motion_and_its_scale():
    p = clean()
    r = both(p, use3=True, max_variance=1.0)
    assert r["status"] == M.ST_OK and len(r["inliers"]) == 60
    T = r["transform"].reshape(3, 4).astype(np.float64)
    assert np.abs(T[:, :3] - p["R"].T).max() < 1e-5
    assert np.abs(T[:, 3] - (-p["R"].T @ p["t"])).max() < 1e-4          # cameraTransform = inverse([R | t]), scaled by words3
    ids = M.join(p["from_ids"], p["from_points"], p["to_ids"], p["to_points"], I.CAMERA, p["from_points3"])
    truth = {i: ids[1][4:7, k] for k, i in enumerate(ids[0])}
    assert max(np.abs(r["points3"][k] - truth[i]).max() for k, i in enumerate(r["inliers"])) < 1e-3


def test_the_gates_at_equality():
    p = clean()
    r = both(p, use3=True, max_variance=100.0)
    n, var = len(r["inliers"]), np.float32(r["variance"])
    below = float(np.nextafter(var, np.float32(0)))
    assert both(p, use3=True, min_inliers=n, max_variance=float(var))["status"] == M.ST_OK
    assert both(p, use3=True, min_inliers=n + 1, max_variance=float(var))["status"] == M.ST_FEW_INLIERS
    assert both(p, use3=True, min_inliers=n, max_variance=below)["status"] == M.ST_HIGH_VARIANCE


def test_refusals_row_by_row():
    from rtabmap_amd import vwdictionary as V
    p = with_m(20)
    nan = float("nan")
    for kw in (dict(iterations=0), dict(iterations=65536), dict(min_inliers=0), dict(reproj_threshold=0.0), dict(reproj_threshold=nan),
               dict(reproj_threshold=float("inf")), dict(reproj_threshold=1e-30), dict(distance_threshold=0.0), dict(distance_threshold=nan),
               dict(variance_median_ratio=-1), dict(variance_median_ratio=32), dict(max_variance=-1.0), dict(max_variance=nan),
               dict(camera=(0.0, 525.0, 320.0, 240.0)), dict(camera=(525.0, nan, 320.0, 240.0)), dict(camera=(525.0, 525.0, float("inf"), 240.0))):
        k = dict(KW, **kw)
        cam = k.pop("camera", I.CAMERA)
        assert V.motion_mono_cpu(p["from_ids"], p["from_points"], p["to_ids"], p["to_points"], cam, **k) is None, kw
    wide = np.arange(8193, dtype=np.int32)
    assert V.motion_mono_cpu(wide, np.zeros((8193, 2), np.float32), p["to_ids"], p["to_points"], I.CAMERA, **KW) is None


def test_the_sanitizer_driver_runs_clean(tmp_path):
    """tools/sanitize_motion_mono.cpp as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU"""
    cxx = shutil.which("g++")
    exe = str(tmp_path / "motion_mono_asan")
    host = os.path.join(ROOT, "rtabmap_amd", "host")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + host,
           os.path.join(ROOT, "tools", "sanitize_motion_mono.cpp"), os.path.join(host, "MotionMono.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert ran.returncode == 0, ran.stdout
    assert ran.stdout.strip().splitlines()[-1] == "ok %d" % SANITIZER_CASES, ran.stdout


def _angle(a, b):
    return float(np.degrees(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0))))


def _rotation_angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0))))


def test_the_rule_is_as_accurate_as_the_yardstick():
    """Twelve scenes of one recipe (motion_mono_inputs.accuracy_scenes: 640 x 480, f = 525, depths 1 .. 8 m, up to +-12 degrees and +-0.4 m per
    axis, 0.5 px noise, m from 60 to 300, 40 % planted outliers at least 30 px from the true epipolar line in both images), threshold 2 px,
    1000 samples, from_points3 at the true depths.  The yardstick solves the same samples in float64 with numpy.linalg.svd and numpy.roots and
    is scored in float64 and in float32.  Per figure (rotation error and translation-direction error against the planted motion in degrees,
    inlier count, scale over the planted baseline) the rule may be worse than the yardstick's float64 value of the same scene by the largest
    float32-against-float64 difference of the yardstick plus twice the standard deviation of the yardstick's figure over the twelve scenes.
    No planted outlier is among the rule's inliers in any scene.  The bound is computed here from the yardstick alone; DESIGN.md 4t records
    the values measured."""
    from rtabmap_amd import vwdictionary as V
    fig = dict(rule=[], y64=[], y32=[])
    for k, s in enumerate(I.accuracy_scenes()):
        r = V.motion_mono_cpu(s["from_ids"], s["from_points"], s["to_ids"], s["to_points"], I.CAMERA, from_points3=s["from_points3"], min_inliers=20,
                              iterations=1000, max_variance=1e30, seed=k)
        assert r["status"] == M.ST_OK
        assert not set(r["inliers"].tolist()) & set(s["outlier_ids"]), k
        Rt, tt = s["R"].T, -s["R"].T @ s["t"]                              # cameraTransform = inverse([R | t])
        T = r["transform"].reshape(3, 4).astype(np.float64)
        fig["rule"].append((_rotation_angle(T[:, :3], Rt), _angle(T[:, 3], tt), len(r["inliers"]) / len(r["matches"]),
                            np.linalg.norm(T[:, 3]) / np.linalg.norm(tt)))
        ids, X = M.join(s["from_ids"], s["from_points"], s["to_ids"], s["to_points"], I.CAMERA, s["from_points3"])
        thr2 = M.threshold2(2.0, I.CAMERA[0], I.CAMERA[1])
        for name, (E, mask) in zip(("y64", "y32"), M.yardstick(X, k, 1000, thr2, (np.float64, np.float32))):
            R, t, good = M.yardstick_pose(E, X, mask)
            fig[name].append((_rotation_angle(R.T, Rt), _angle(-R.T @ t, tt), np.count_nonzero(good) / len(ids),
                              M.yardstick_scale(R, t, good, X) / np.linalg.norm(tt)))
    rule, y64, y32 = (np.array(fig[k]) for k in ("rule", "y64", "y32"))
    floor = np.abs(y32 - y64).max(0)
    margin = 2.0 * y64.std(0)
    print("yardstick float64 (rotation deg, direction deg, inlier share, scale ratio), per scene:\n", y64)
    print("rule:\n", rule)
    print("float32-against-float64 floor", floor, "margin (2 sigma)", margin, "largest rule - yardstick", np.abs(rule - y64).max(0))
    for c, what in enumerate(("rotation", "direction")):
        assert (rule[:, c] <= y64[:, c] + floor[c] + margin[c]).all(), what
    assert (rule[:, 2] >= y64[:, 2] - floor[2] - margin[2]).all(), "inlier share"
    assert (np.abs(rule[:, 3] - 1.0) <= np.abs(y64[:, 3] - 1.0) + floor[3] + margin[3]).all(), "scale"
