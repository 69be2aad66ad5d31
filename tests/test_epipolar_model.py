"""epipolar_cpu (rtabmap_amd/host/EpipolarGeometryHip.cpp, the engine's arithmetic compiled for the host) against the NumPy model of the rule,
bit for bit -- ints and float bits -- on the hand-made pairs and on the refusals row by row; the stand-alone sanitizer driver's count of clean
cases; and the rule's accuracy against an independent yardstick.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import epipolar_inputs as I
import epipolar_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZER_CASES = 83                                                       # tools/sanitize_epipolar.cpp prints "ok 83"
# Measured on I.accuracy_scenes(): the largest difference between the yardstick's own float32 and float64 inlier counts
RECORDED_D = 1


def both(pair, **kw):
    from rtabmap_amd import vwdictionary as V
    try:
        want = M.verify(*I.frames(pair), **kw)
    except M.Refused:
        want = None
    got = V.epipolar_cpu(*I.frames(pair), **kw)
    assert (want is None) == (got is None)
    if want is not None:
        assert got["status"] == want["status"]
        assert np.array_equal(got["matches"], want["matches"]) and np.array_equal(got["inliers"], want["inliers"])
        assert np.array_equal(M.bits(got["fundamental"]), M.bits(want["fundamental"])), (got["fundamental"], want["fundamental"])
    return want


CASES = [("ids", I.id_cases, {}), ("m7", lambda: I.with_m(7), {}), ("m8", lambda: I.with_m(8), {}), ("m9", lambda: I.with_m(9), {}),
         ("below_min", lambda: I.with_m(11), dict(match_count_min=12)), ("equal", I.all_equal, {}), ("collinear", I.collinear, {}),
         ("c3_zero", I.c3_zero, {}), ("nan", I.nan_keypoint, {}), ("planar", lambda: I.scene(4, 120, planar=True), {}),
         ("outliers", lambda: I.scene(1, 120), dict(iterations=200)), ("all_outliers", lambda: I.scene(5, 40, outliers=1.0), dict(match_count_min=30)),
         ("large", lambda: I.scene(6, 1100, extra=40), dict(iterations=20)), ("thr", lambda: I.scene(8, 90), dict(ransac_threshold=0.75, seed=0xFFFFFFF0))]
# the generators of the shape tests (test_gpu_epipolar_shapes.py): the model is right where squares go subnormal or overflow before the device is asked
SCALES = (-74, -70, -66, -64, -62, -20, 20, 55, 60, 62)
CASES += [("scale%+d" % k, lambda k=k: I.scaled(I.scene(3, 100), k), dict(ransac_threshold=3.0 * 2.0 ** k, seed=5)) for k in SCALES]
CASES += [("scale%+d_m8" % k, lambda k=k: I.scaled(I.with_m(8), k), dict(ransac_threshold=3.0 * 2.0 ** k, seed=5)) for k in SCALES]
CASES += [("census%d" % k, lambda k=k: I.census_batch()[0][k], dict(iterations=I.CENSUS_ITERATIONS, seed=I.CENSUS_SEED)) for k in (0, 1, 40, 41, 42, 43)]
CASES += [("tie%d_%d" % (k, it), lambda k=k: I.tie_pairs()[0][k], dict(iterations=it, seed=I.TIE_SEED)) for k in range(4) for it in (86, 300)]
CASES += [("draw_failure", lambda: I.draw_failure()[0], dict(seed=I.DRAW_FAILURE_SEED, iterations=I.DRAW_FAILURE_ITERATIONS))]
CASES += [("inf%+d_%s" % (sign, side), lambda sign=sign, side=side: I.inf_keypoint(sign, side), {}) for sign in (1, -1) for side in ("from", "to")]
CASES += [("nan_unpaired", lambda: I.nan_unpaired()[0], {}), ("nan_unpaired_twin", lambda: I.nan_unpaired()[1], {})]


@pytest.mark.parametrize("name,make,kw", CASES, ids=[c[0] for c in CASES])
def test_the_mirror_equals_the_model(name, make, kw):
    kw = dict(kw)
    kw.setdefault("iterations", 60)
    both(make(), **kw)


def test_every_status_is_met_and_the_count_decides():
    p = I.scene(3, 100)
    n = both(p, iterations=60)["inliers"].shape[0]
    assert both(p, iterations=60, match_count_min=n)["status"] == M.OK
    assert both(p, iterations=60, match_count_min=n + 1)["status"] == M.FEW_INLIERS
    assert both(I.with_m(7), iterations=60)["status"] == M.FEW_PAIRS
    assert both(I.all_equal(), iterations=60)["status"] == M.NO_MODEL


def test_refusals_row_by_row():
    p = I.with_m(10)
    for kw in (dict(iterations=0), dict(iterations=65536), dict(ransac_threshold=0.0), dict(ransac_threshold=-1.0), dict(ransac_threshold=float("nan")),
               dict(ransac_threshold=float("inf")), dict(ransac_threshold=1e-30), dict(ransac_threshold=1e30), dict(match_count_min=0)):
        assert both(p, **kw) is None, kw
    big = dict(from_ids=np.arange(8193, dtype=np.int32), from_points=np.zeros((8193, 2), np.float32), to_ids=p["to_ids"], to_points=p["to_points"])
    assert both(big) is None                                               # epipolar_cpu's own refusal: the wrapper passes the rows on
    assert both(dict(big, from_ids=p["from_ids"], from_points=p["from_points"], to_ids=big["from_ids"], to_points=big["from_points"])) is None
    assert both(p, iterations=1) is not None                               # the ends that are accepted
    assert both(p, iterations=65535) is not None
    assert both(p, iterations=3, ransac_threshold=1e-18) is not None


def test_the_sanitizer_driver_runs_clean(tmp_path):
    """tools/sanitize_epipolar.cpp as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU"""
    cxx = shutil.which("g++")
    exe = str(tmp_path / "epipolar_asan")
    host = os.path.join(ROOT, "rtabmap_amd", "host")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + host,
           os.path.join(ROOT, "tools", "sanitize_epipolar.cpp"), os.path.join(host, "EpipolarGeometryHip.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert ran.returncode == 0, ran.stdout
    assert ran.stdout.strip().splitlines()[-1] == "ok %d" % SANITIZER_CASES


def test_the_rule_is_as_accurate_as_the_yardstick():
    """Twelve scenes of one recipe (epipolar_inputs.scene: 640 x 480, fx = fy = 525, depths 1 .. 8 m, up to +-12 degrees and +-0.4 m per axis,
    0.5 px noise, m from 60 to 300, 40 % planted outliers at least 30 px from the true epipolar line in both images), thr = 3, 1000 samples.
    On every scene: the rule's decision is the yardstick's float64 decision; no planted outlier is among the rule's inliers; the rule's
    inlier count is at least the yardstick's float64 count minus d, d the largest difference between the yardstick's OWN float32 and float64
    counts over the twelve scenes and at least 1.  Measured: the yardstick's two counts are equal on every scene (so d = 1),
    and the rule's count equals the yardstick's float64 count on every scene."""
    from rtabmap_amd import vwdictionary as V
    scenes = I.accuracy_scenes()
    ms = [M.correspondences(*I.frames(s))[0].shape[0] for s in scenes]
    assert len(scenes) == 12 and min(ms) == 60 and max(ms) == 300
    rows, d = [], 1
    for s in scenes:
        y64, y32 = M.yardstick(*I.frames(s), dtype=np.float64), M.yardstick(*I.frames(s), dtype=np.float32)
        r = V.epipolar_cpu(*I.frames(s))
        d = max(d, abs(int(y64["inliers"].shape[0]) - int(y32["inliers"].shape[0])))
        rows.append((s, y64, r))
        print("m %3d planted %3d  yardstick64 %3d yardstick32 %3d rule %3d  status %d / %d" %
              (y64["matches"].shape[0], len(s["planted"]), y64["inliers"].shape[0], y32["inliers"].shape[0], r["inliers"].shape[0], y64["status"], r["status"]))
    assert d <= RECORDED_D
    for s, y64, r in rows:
        assert r["status"] == y64["status"] == M.OK
        assert not (s["planted"] & set(r["inliers"].tolist()))
        assert r["inliers"].shape[0] >= y64["inliers"].shape[0] - d
