"""GPU tests of lcd_estimate_motion_pnp and lcd_estimate_motion_pnp_dev (rtabmap_amd/csrc/motion_pnp.hip) where the kernel's own parts change
shape: the join (two sorts of different lengths, runs of duplicates over the block boundaries, the extreme ids, the finite test inside the
compaction, keypoints that are not finite), the scratch layout with a stride that is not the correspondences, the hypothesis chunks (ties and
a unique winner across them, a winner beyond the iterations, 65536 candidates), the minimal solver on degenerate geometry, Shepperd's four
cases and their ties, the lane partials of the fit, two index sets that differ behind the first 256, a refused Gauss-Newton step, and the
covariance (the rank at k = 0 and k = n / 2, negative ordered keys, the clamps, cameras whose principal point is not positive).
The reference is tests/motion_pnp_model.py; every comparison is exact, as in tests/test_gpu_motion_pnp.py, whose helpers these tests use.
The calls are tests/motion_pnp_inputs.py's shape_calls(); tests/test_motion_pnp_inputs.py proves without a GPU that each input has the
property it is here for, and tests/test_motion_pnp_model.py that the host mirror agrees with the model on each."""
import numpy as np
import pytest

import motion_pnp_inputs as I
import motion_pnp_model as M
from test_gpu_motion_pnp import check_both, model_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import rtabmap_amd
    e = rtabmap_amd.Engine("f32", 64)
    yield e
    assert e.vocab_count() == (0, 0) and e.sig_count() == (0, 0)
    e.close()


@pytest.fixture(scope="module")
def calls():
    return I.shape_calls()


def run(eng, calls, name):
    """both entries against the model on one call -> the model's results as the call lays them out"""
    c = calls[name]
    return check_both(eng, c["pairs"], name, cam=c["cam"], guesses=c["guesses"], to_xyz=c["to_xyz"], **c["kw"])


def model(calls, name, k=0):
    """the model's own record of pair k of a call (cached by check_both)"""
    c = calls[name]
    cam = c["cam"] if isinstance(c["cam"], dict) else c["cam"][k]
    return model_of(c["pairs"][k], cam, None if c["guesses"] is None else c["guesses"][k], c["to_xyz"], **c["kw"])


@pytest.mark.parametrize("to_xyz", (1, 0))
def test_the_join_in_one_batch(eng, calls, to_xyz):
    """A in ONE call: sides of 0 .. 8192 rows against 0 .. 8192, runs of 2, 3 and 5 equal ids over the sorted positions 63/64, 255/256, 511/512
    and at both ends in either frame, INT32_MIN and INT32_MAX unique and doubled, from-points that are not finite in one coordinate on the
    to-positions 255, 256 and 511, and three keypoints that are not finite"""
    want = run(eng, calls, "join_%d" % to_xyz)
    n = want["n_matches"].tolist()
    assert n[:8] == [min(nf, nt, 60) for nf, nt in I.JOIN_SIZES]
    assert all(580 < v < 590 for v in n[8:14]) and n[14:17] == [10, 9, 9] and n[17] == I.PREDICATE_ROWS - 3
    assert want["status"].tolist() == [M.FEW_CORRESPONDENCES] * 4 + [M.OK] * 14
    assert want["n_inliers"][17] == n[17] - 3                           # the keypoints that are not finite are matches and never inliers
    first = int(np.cumsum([0] + [p["to_ids"].shape[0] for p in calls["join_1"]["pairs"]])[14])       # the first extreme pair's region
    assert want["matches"][first] == I.INT32_MIN and want["matches"][first + 9] == I.INT32_MAX


def test_hypotheses_that_draw_a_keypoint_that_is_not_finite(eng, calls):
    """A: ten correspondences, three with a NaN, +inf or -inf keypoint, the guess turned away: 28 of 30 hypotheses draw one of them among
    their three points or as the fourth and are invalid, one of the two others wins with the seven finite ones"""
    want = run(eng, calls, "keypoints")
    r = model(calls, "keypoints")
    assert want["status"][0] == M.OK and want["n_matches"][0] == 10 and want["n_inliers"][0] == 7
    assert (r["counts"] > 0).sum() == 2 and r["counts"][r["best"]] == 7


@pytest.mark.parametrize("to_xyz", (0, 1))
def test_a_stride_that_is_not_the_correspondences_in_either_layout(eng, calls, to_xyz):
    """B: m = 150 of 8192 x 200 rows (staged, stride m), five correspondences, and a pair just above the staged limit whose to-frame has more
    rows than correspondences (scratch, stride n_to), in one call and again in the reverse order: both calls equal the model's results of
    the same three pairs, so a pair's outputs do not depend on where it stands"""
    big = I.STAGE_CAP[bool(to_xyz)] + (1 if to_xyz else 4)
    want = run(eng, calls, "layout_%d_forward" % to_xyz)
    assert want["n_matches"].tolist() == [150, 5, big] and want["status"].tolist() == [M.OK] * 3
    back = run(eng, calls, "layout_%d_reverse" % to_xyz)              # the same model results (cached per pair), in the other order
    assert back["n_matches"].tolist() == [big, 5, 150]


@pytest.mark.parametrize("iterations", I.TIE_ITERATIONS)
def test_a_tie_across_chunks_goes_to_the_lowest_candidate(eng, calls, iterations):
    """C: nearly every hypothesis of every chunk holds all 40 correspondences and the guess holds none: candidate 1 wins; 65536 candidates
    are 256 whole chunks, 65535 end in a chunk of 255"""
    want = run(eng, calls, "tie_%d" % iterations)
    r = model(calls, "tie_%d" % iterations)
    assert r["best"] == 1 and r["counts"][0] == 0 and (r["counts"] == 40).sum() > 0.9 * iterations and want["n_inliers"][0] == 40


def test_a_tie_with_the_guess_and_behind_invalid_hypotheses(eng, calls):
    """C: the true pose as the guess ties with the hypotheses and wins as candidate 0; under a seed whose hypotheses 0 and 1 find no four
    distinct indices among four, candidate 3 wins"""
    run(eng, calls, "tie_guess")
    assert model(calls, "tie_guess")["best"] == 0
    want = run(eng, calls, "tie_invalid_first")
    assert model(calls, "tie_invalid_first")["best"] == 3 and want["n_inliers"][0] == 4


@pytest.mark.parametrize("c,iterations", I.LATE_CASES)
def test_a_unique_winner_late_in_the_chunks(eng, calls, c, iterations):
    """C: the only candidate that holds all five is the last of a chunk, the first or second of the next, or the very last one"""
    want = run(eng, calls, "late_%d" % c)
    assert model(calls, "late_%d" % c)["best"] == c and want["n_inliers"][0] == I.LATE_INLIERS and want["status"][0] == M.OK


@pytest.mark.parametrize("c", [c for c, _ in I.LATE_CASES])
def test_a_hypothesis_beyond_the_iterations_never_wins(eng, calls, c):
    """C: iterations = c - 1: the winner would be the next candidate"""
    want = run(eng, calls, "cut_%d" % c)
    r = model(calls, "cut_%d" % c)
    assert r["best"] < c and 0 < want["n_inliers"][0] < I.LATE_INLIERS and want["status"][0] == M.OK


def test_the_minimal_solver_on_degenerate_geometry(eng, calls):
    """D: pairs of 4 to 6 correspondences, each its own workgroup: a collinear triple, coincident points, three points at one distance, a
    keypoint at the principal point, a fronto-parallel plane, a fourth point behind the camera, a line"""
    want = run(eng, calls, "solver")
    names = list(I.solver_pairs())
    assert want["status"][names.index("line")] == M.NO_MODEL and want["status"][names.index("behind")] == M.BELOW_MIN_INLIERS
    assert (want["status"] == M.OK).sum() == len(names) - 2


@pytest.mark.parametrize("pick", sorted(I.SHEPPERD_SEEDS))
def test_shepperd_cases_of_a_negative_trace(eng, calls, pick):
    """E: rotations by 3.0 to 3.14 whose fits all take case 1, 2 or 3"""
    for s in I.SHEPPERD_SEEDS[pick]:
        name = "shepperd_%d_%d" % (pick, s)
        want = run(eng, calls, name)
        assert want["status"][0] == M.OK and set(model(calls, name)["picks"]) == {pick}


@pytest.mark.parametrize("local", (0, 1))
def test_shepperd_pivots_that_are_exact_and_tie(eng, calls, local):
    """E: the guess as the winner under rotations that are exact in fp32: the three half turns (cases 1, 2, 3 with a pivot of 4), a rotation
    whose cases 1 and 2 tie at 2, and one whose four cases tie at 1"""
    name = "exact_rotations_%d" % local
    want = run(eng, calls, name)
    assert (want["status"] == M.OK).all() and (want["n_inliers"] == 60).all()
    assert [model(calls, name, k)["picks"] for k in range(5)] == [[pick] for _, pick, _ in I.EXACT_ROTATIONS]


def test_shepperd_pivots_that_tie_between_rounded_entries(eng, calls):
    """E: rotations with two equal diagonal entries: two pivots tie near 2, the lower case is taken, and the other one would end in other bits"""
    want = run(eng, calls, "exact_rotations_tied")
    assert (want["status"] == M.OK).all() and (want["n_inliers"] == 60).all()
    assert [model(calls, "exact_rotations_tied", k)["picks"] for k in range(3)] == [[pick] for _, pick, _ in I.TIED_ROTATIONS]


def test_lane_partials_of_the_fit(eng, calls):
    """E: fits over 255, 256, 257, 512 and 513 members: 0/1, 1, 1/2, 2, 2/3 per lane"""
    want = run(eng, calls, "lanes")
    assert want["n_inliers"].tolist() == list(I.LANE_SIZES) and (want["status"] == M.OK).all()


@pytest.mark.parametrize("seed", sorted(I.LATE_MEMBERS))
def test_two_index_sets_that_differ_only_behind_the_first_256(eng, calls, seed):
    """E: two successive selections of equal size that first differ behind position 300"""
    want = run(eng, calls, "late_members_%d" % seed)
    assert model(calls, "late_members_%d" % seed)["first_differing"] == I.LATE_MEMBERS[seed] and want["n_inliers"][0] > 256


def test_a_fit_whose_every_step_is_refused(eng, calls):
    """E: six copies of one point and keypoint: gn_solve refuses each Gauss-Newton step and the pose stays the guess's"""
    want = run(eng, calls, "refused")
    assert want["status"][0] == M.OK and want["n_inliers"][0] == 6 and len(model(calls, "refused")["refused"]) == M.STEPS
    np.testing.assert_array_equal(want["transform"][0], M.IDENTITY)


@pytest.mark.parametrize("ratio", I.RATIOS)
def test_the_rank_of_the_covariance(eng, calls, ratio):
    """F: selections of 4, 5, 255, 256 and 257 inliers under variance_median_ratio = 2, 3, n, n + 1 and 2^31 - 1: k = n / 2, 1 and 0"""
    want = run(eng, calls, "ratio_%d" % ratio)
    assert want["n_inliers"].tolist() == list(I.RATIO_SIZES) and (want["variance_kind"] == 1).all()


def test_negative_keys_the_ray_for_every_inlier_and_a_zero_point(eng, calls):
    """F: a ranked cosine below zero, to_xyz without one finite row, a from-point of (0, 0, 0), and cosines that the clamps bring back"""
    want = run(eng, calls, "negative_cosine")
    assert want["angle_cos"][0] < 0 and want["status"][0] == M.OK
    want = run(eng, calls, "nonfinite_to")
    assert want["variance_kind"][0] == 1 and want["status"][0] == M.OK
    want = run(eng, calls, "zero_point")
    assert want["status"][0] == M.OK and want["n_inliers"][0] == 40
    want = run(eng, calls, "clamps")                       # raw cosines a unit in the last place beyond 1 and -1
    assert want["angle_cos"].tolist() == [1.0, -1.0] and (want["status"] == M.OK).all()


def test_cameras_that_all_differ_in_one_batch(eng, calls):
    """F: cx, cy not positive with odd and 1 x 1 images, fx != fy, fy < 0, sized and without to_xyz; and cx = 0 unsized beside NaN rows"""
    want = run(eng, calls, "cameras")
    assert (want["status"] == M.OK).all() and (want["variance_kind"] == 1).all()
    want = run(eng, calls, "camera_unsized")
    assert want["status"][0] == M.OK and want["variance_kind"][0] == 1


def test_max_variance_one_float_below_and_above(eng, calls):
    """F: the float32 neighbours of an accepted pair's variance: the lower rejects, the upper accepts"""
    assert run(eng, calls, "max_variance_below")["status"][0] == M.VARIANCE_REJECTED
    assert run(eng, calls, "max_variance_above")["status"][0] == M.OK
