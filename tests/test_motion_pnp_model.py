"""tests/motion_pnp_model.py on hand-made cases with hand-computed values, every branch of the refinement loop reached by a constructed input,
all three covariance branches, the host mirror (rtabmap_amd/host/Motion2D.cpp, through c_shim.cpp) against the model bit for bit, and the fp32
fit and minimal solver against float64 yardsticks.  No GPU."""
import numpy as np
import pytest

import motion_pnp_inputs as I
import motion_pnp_model as M

F = np.float32
KW = dict(min_inliers=4, reproj_error=2.0, iterations=60, refine_iterations=5, variance_median_ratio=4, max_variance=0.0, seed=3)
# Measured on I.fit_sets() (27 sets of 28 .. 601 points in general position, depths 0.5 .. 10 m, 640 x 480, noise-free and with 0.5 px noise,
# tools/motion_pnp_steps.py): the largest difference between an entry of the rule's 8-step fit from the P3P start and of
# scipy.optimize.least_squares in float64 was 3.787e-8 for the rotation and 1.392e-7 for the translation; the worst reprojection of a
# held-out noise-free point under a noise-free hypothesis was 0.8379 px.  The bounds are four times that.
ROTATION_BOUND, TRANSLATION_BOUND, P3P_BOUND = 4 * 3.787e-8, 4 * 1.392e-7, 4 * 0.8379
EXACT = dict(fx=512.0, fy=512.0, cx=0.0, cy=0.0)                         # with depths that are powers of two the projection is exact


def mirror(pair, cam=I.CAMERA, guess=None, to_xyz=True, **kw):
    from rtabmap_amd import vwdictionary as V
    return V.motion_pnp_cpu(*I.frames(pair, to_xyz), camera=(cam["fx"], cam["fy"], cam["cx"], cam["cy"]),
                            image_size=(cam.get("image_width", 0), cam.get("image_height", 0)), local_transform=cam.get("local_transform"), guess=guess, **kw)


def assert_same(got, want):
    assert int(got["status"]) == want["status"] and int(got["variance_kind"]) == want["variance_kind"]
    np.testing.assert_array_equal(M.bits(got["transform"]), M.bits(want["transform"]))
    for name in ("variance_lin", "angle_cos"):
        assert np.float64(got[name]).view(np.uint64) == np.float64(want[name]).view(np.uint64), name
    assert list(got["matches"]) == list(want["matches"]) and list(got["inliers"]) == list(want["inliers"])


def both(pair, cam=I.CAMERA, guess=None, to_xyz=True, **kw):
    want = M.estimate(*I.frames(pair, to_xyz), camera=I.model_camera(cam), guess=guess, **kw)
    assert_same(mirror(pair, cam, guess, to_xyz, **kw), want)
    return want


def frame_pair(f_ids, f_xyz, t_ids, t_uv, t_xyz=None):
    n = len(t_ids)
    return dict(from_ids=np.array(f_ids, np.int32), from_xyz=np.array(f_xyz, np.float32).reshape(-1, 3), to_ids=np.array(t_ids, np.int32),
                to_points=np.array(t_uv, np.float32).reshape(-1, 2), to_xyz=np.full((n, 3), np.nan, np.float32) if t_xyz is None else np.array(t_xyz, np.float32).reshape(-1, 3))


def exact_pair(n, shift=None):
    """n points at depth 4 seen by the EXACT camera under the identity: u = 128 x, v = 128 y, every error 0 exactly; shift: {index: du}"""
    xs = [(k % 5) - 2.0 for k in range(n)]
    ys = [((k * 3) % 7) - 3.0 + 0.5 * (k // 7) for k in range(n)]
    P = np.array([[x, y, 4.0] for x, y in zip(xs, ys)], np.float32)
    UV = np.array([[128.0 * x, 128.0 * y] for x, y in zip(xs, ys)], np.float32)
    for k, du in (shift or {}).items():
        UV[k, 0] += du
    ids = np.arange(1, n + 1, dtype=np.int32)
    return dict(from_ids=ids, from_xyz=P, to_ids=ids.copy(), to_points=UV, to_xyz=P.copy(), m=n)


def test_unique_ids_the_finite_from_point_and_the_untested_keypoint():
    """7 twice in from and once in to, 9 once in from and twice in to, a NaN and an infinity in a from-point: none takes part; a zero from-point
    and a NaN keypoint do (no zero test, the to-keypoint is not tested); ascending id, negative ids first"""
    nan, inf = float("nan"), float("inf")
    pair = frame_pair([5, 7, 7, 9, 11, 13, -3, 2, 21], [[1, 0, 4], [1, 1, 1], [2, 2, 2], [3, 3, 3], [nan, 1, 1], [0, 0, 0], [0, 2, 4], [0, 0, 4], [1, inf, 1]],
                      [7, 5, 9, 9, 11, 13, 2, -3, 99, 21], [[1, 1], [128, 0], [3, 3], [4, 4], [1, 1], [nan, 5], [0, 0], [0, 256], [5, 5], [1, 1]])
    ids, P, UV, T = M.correspondences(*I.frames(pair))
    assert ids.tolist() == [-3, 2, 5, 13]
    np.testing.assert_array_equal(P, np.array([[0, 2, 4], [0, 0, 4], [1, 0, 4], [0, 0, 0]], np.float32))
    np.testing.assert_array_equal(UV[:3], np.array([[0, 256], [0, 0], [128, 0]], np.float32))
    r = both(pair, cam=EXACT, **dict(KW, min_inliers=3, iterations=4, refine_iterations=0))
    assert r["status"] == M.OK and r["best"] == 0 and r["inliers"].tolist() == [-3, 2, 5]        # the identity guess explains the three exactly
    np.testing.assert_array_equal(r["transform"], M.IDENTITY)
    r = both(pair, cam=EXACT, **dict(KW, min_inliers=5, iterations=4, refine_iterations=0))
    assert r["status"] == M.FEW_CORRESPONDENCES and r["matches"].tolist() == [-3, 2, 5, 13] and len(r["inliers"]) == 0
    assert not r["transform"].any() and r["variance_lin"] == 1.0 and r["angle_cos"] == 1.0 and r["variance_kind"] == 0


def test_three_four_and_min_inliers():
    for min_inliers in (1, 3):                                          # fewer than four correspondences solve nothing, whatever min_inliers says
        assert both(exact_pair(3), cam=EXACT, **dict(KW, min_inliers=min_inliers))["status"] == M.FEW_CORRESPONDENCES
    r = both(exact_pair(4), cam=EXACT, **dict(KW, min_inliers=1, refine_iterations=0))
    assert r["status"] == M.OK and len(r["inliers"]) == 4
    nine = exact_pair(9)
    assert both(nine, cam=EXACT, **dict(KW, min_inliers=10))["status"] == M.FEW_CORRESPONDENCES       # m = min_inliers - 1
    assert both(nine, cam=EXACT, **dict(KW, min_inliers=9, refine_iterations=0))["status"] == M.OK     # m = min_inliers
    far = exact_pair(9, shift={k: 100.0 for k in range(4)})            # five inliers of nine under min_inliers = 6: the gate of :147
    r = both(far, cam=EXACT, **dict(KW, min_inliers=6, iterations=1, refine_iterations=0))
    assert r["status"] == M.BELOW_MIN_INLIERS and len(r["inliers"]) == 5 and not r["transform"].any() and r["variance_kind"] == 0


def test_the_ransac_threshold_is_squared_and_the_refinement_threshold_is_not():
    """an error of exactly 3 px under reproj_error = 2: 3 <= float(2 x 2) makes it a RANSAC inlier, 3 > 2 keeps it out of the refinement's
    selection (solvepnp.cpp:253 against util3d_motion_estimation.cpp:832)"""
    pair = exact_pair(12, shift={5: 3.0})
    cam = I.model_camera(EXACT)
    e, front = M.reproj_error(M.IDENTITY, cam, pair["from_xyz"], pair["to_points"])
    assert e.tolist() == [0.0] * 5 + [3.0] + [0.0] * 6 and front.all()
    assert M.inliers_of(e, front, F(4)).sum() == 12 and M.inliers_of(e, front, F(2)).sum() == 11
    r = both(pair, cam=EXACT, **dict(KW, iterations=1, refine_iterations=0))
    assert r["best"] == 0 and r["counts"][0] == 12 and len(r["inliers"]) == 12
    r = both(pair, cam=EXACT, **dict(KW, iterations=1, refine_iterations=1))
    assert r["trace"] == ["size_changed"] and len(r["inliers"]) == 12  # eleven were selected; the final swap (:981) returns the set that was fitted
    r = both(pair, cam=EXACT, **dict(KW, iterations=1, refine_iterations=2))
    assert r["trace"][0] == "size_changed" and 6 not in r["inliers"].tolist() and len(r["inliers"]) == 11


def test_candidate_zero_wins_a_tie_a_collinear_triple_and_a_seed_without_four_indices():
    pair = exact_pair(12)
    r = both(pair, cam=EXACT, **dict(KW, iterations=40, refine_iterations=0))
    assert r["best"] == 0 and (r["counts"] == 12).sum() > 1            # hypotheses reach all twelve too: the lowest candidate wins
    line = exact_pair(8)
    line["from_xyz"] = np.array([[k - 3.0, 0.0, 4.0] for k in range(8)], np.float32)
    line["to_points"] = np.array([[128.0 * (k - 3.0) + 1000.0, 0.0] for k in range(8)], np.float32)
    r = both(line, cam=EXACT, **dict(KW, iterations=30, refine_iterations=0))
    assert r["status"] == M.NO_MODEL and not r["counts"].any()         # every triple is collinear: no hypothesis, and the guess explains nothing
    idx = np.array([[0], [1], [2], [3]])
    has, _, _ = M.p3p(line["from_xyz"][idx[:3]], M.bearing(I.model_camera(EXACT), line["to_points"][idx[:3]]), line["from_xyz"][idx[3]], line["to_points"][idx[3]],
                      I.model_camera(EXACT))
    assert not has[0]
    seed = I.seed_with_invalid_first(4, 1)
    assert M.draw4(seed, 0, 4) is None and sorted(M.draw4(seed, 1, 4)) == [0, 1, 2, 3]
    four = exact_pair(4, shift={0: 50.0, 1: -50.0, 2: 50.0, 3: -50.0})     # the guess explains nothing either
    assert both(four, cam=EXACT, **dict(KW, min_inliers=4, iterations=1, refine_iterations=0, seed=seed))["status"] == M.NO_MODEL


def test_the_summation_order_shows():
    """the 27 sums of a fit over 1100 members in the rule's 256-lane order differ in their bits from a serial sum"""
    pair = I.mixed_batch()[-1]
    _, P, UV, _ = M.correspondences(*I.frames(pair))
    terms = M.gn_terms(I.true_model(pair), I.model_camera(I.CAMERA), P, UV)
    serial = np.zeros(M.SUMS, np.float32)
    for row in terms:
        serial = serial + row
    assert (M.bits(M.lane_sum(terms)) != M.bits(serial)).any()
    both(pair, **KW)


@pytest.mark.parametrize("name", sorted(I.REFINE_CASES))
def test_refinement_branches(name):
    pair, kw = I.refine_case(name)
    kw = dict(KW, **kw)
    r = both(pair, **kw)
    assert I.REFINE_CASES[name][7] in r["trace"], r["trace"]
    for refine in I.REFINE:                                             # 0 / 1 / 5 passes
        r = both(pair, **dict(kw, refine_iterations=refine))
        assert len(r["trace"]) <= refine
    if name == "few_first":
        assert r["trace"] == ["few"]                                    # below minInliersCount on the first pass: counted, and the loop's condition ends it
    if name == "oscillating":
        guarded = M.estimate(*I.frames(pair), **dict(KW, **I.refine_case("oscillating_guarded")[1]))
        full = M.estimate(*I.frames(pair), **kw)
        assert full["trace"][-1] == "oscillating" and len(guarded["trace"]) > len(full["trace"])     # :944 holds the test back until six sizes


def test_covariance_branches_the_cosine_rank_and_the_rejection():
    pair = I.mixed_batch()[8]
    sized, local = I.camera(True), I.camera(False, local=True)
    with_points = both(pair, cam=local, to_xyz=True, **KW)              # kind 1: the to-frame's points, the ray where they are NaN
    rays = both(pair, cam=sized, to_xyz=False, **KW)                    # kind 1: rays only
    rms = both(pair, cam=I.CAMERA, to_xyz=False, **KW)                  # kind 2
    assert (with_points["variance_kind"], rays["variance_kind"], rms["variance_kind"]) == (1, 1, 2)
    assert rms["angle_cos"] == 1.0 and 0.0 < rms["variance_lin"] < 2.0
    for r in (with_points, rays):
        n = len(r["inliers"])
        k = n // 4
        angles = np.sort(np.arccos(r["cosines"].astype(np.float64)))
        assert np.arccos(r["angle_cos"]) == angles[k]                   # the cosine of rank n - 1 - k is the angle of rank k
        assert r["variance_lin"] == 2.1981 * float(np.sort(r["d2"])[k])
    # the ray is 1.1 x the depth along the keypoint's ray: every distance is about a tenth of the depth, squared
    assert 0.005 < rays["variance_lin"] / 2.1981 < 1.5
    low = float(F(rays["variance_lin"] * 0.5))
    rej = both(pair, cam=sized, to_xyz=False, **dict(KW, max_variance=low))
    assert rej["status"] == M.VARIANCE_REJECTED and not rej["transform"].any() and rej["variance_kind"] == 0 and rej["variance_lin"] == 1.0
    assert len(rej["inliers"]) == len(rays["inliers"])
    assert both(pair, cam=sized, to_xyz=False, **dict(KW, max_variance=float(F(rays["variance_lin"] * 2))))["status"] == M.OK
    assert both(pair, cam=I.CAMERA, to_xyz=False, **dict(KW, max_variance=1e-9))["status"] == M.OK      # the RMS branch has no rejection


@pytest.mark.parametrize("refine", I.REFINE)
@pytest.mark.parametrize("iterations", (1, 300))
def test_mirror_equals_model_on_the_generators(iterations, refine):
    for k, pair in enumerate(I.mixed_batch()):
        cam = I.camera(sized=k % 3 == 0, local=k % 2 == 1)
        guess = I.guess_of(I.true_model(pair), cam.get("local_transform")) if k % 4 == 3 else None
        both(pair, cam=cam, guess=guess, to_xyz=k % 3 != 1, **dict(KW, iterations=iterations, refine_iterations=refine, seed=k))
    both(I.all_outlier_pair(), **dict(KW, min_inliers=10, iterations=iterations, refine_iterations=refine))
    assert both(I.behind_pair(), **dict(KW, iterations=iterations, refine_iterations=refine))["status"] == M.NO_MODEL


def test_refused_arguments():
    pair = exact_pair(6)
    for bad in (dict(iterations=0), dict(iterations=65536), dict(reproj_error=0.0), dict(reproj_error=float("nan")), dict(reproj_error=1e30),
                dict(refine_iterations=-1), dict(min_inliers=0), dict(variance_median_ratio=1), dict(max_variance=-1.0)):
        assert mirror(pair, **dict(KW, **bad)) is None
        with pytest.raises(M.Refused):
            M.estimate(*I.frames(pair), **dict(KW, **bad))


def test_the_fit_and_the_minimal_solver_against_float64():
    """a check that the rule estimates what it should, not a parity claim"""
    sets = I.fit_sets()
    rotation, translation, pixels, n = M.fit_deviation(sets, I.model_camera(I.CAMERA))
    print("fit against float64 least squares over %d fits: rotation %.3e, translation %.3e; P3P held-out reprojection %.3e px" % (n, rotation, translation, pixels))
    assert n == 2 * len(sets) == 54
    assert rotation <= ROTATION_BOUND and translation <= TRANSLATION_BOUND and pixels <= P3P_BOUND


@pytest.mark.parametrize("section", I.SHAPE_SECTIONS)
def test_mirror_equals_model_on_the_shape_inputs(section):
    """every call of tests/test_gpu_motion_pnp_shapes.py, pair by pair: a disagreement between the two CPU implementations shows here"""
    calls = I.section_calls(section)
    assert calls
    for name, call in calls.items():
        cams = [call["cam"]] * len(call["pairs"]) if isinstance(call["cam"], dict) else call["cam"]
        for k, pair in enumerate(call["pairs"]):
            both(pair, cam=cams[k], guess=None if call["guesses"] is None else call["guesses"][k], to_xyz=call["to_xyz"], **call["kw"])
