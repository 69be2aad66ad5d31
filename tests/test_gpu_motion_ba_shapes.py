"""lcd_refine_motion_ba and lcd_refine_motion_ba_dev (rtabmap_amd/csrc/motion_ba.hip) where the kernel's two sides, its join, its staged state,
its per-pair arguments and its gates change shape, against tests/motion_ba_model.py.  Every comparison is exact and made on both entries, the
device outputs canary-filled, the ids compared over each pair's whole to-region (test_gpu_motion_ba.check_both).  The inputs are
tests/motion_ba_inputs.py's; tests/test_motion_ba_inputs.py proves without a GPU that each takes its branch and tells the mistake it exists
for apart."""
import numpy as np
import pytest

import motion_ba_inputs as I
import motion_ba_model as M
from test_gpu_motion_ba import KW, check_both

pytestmark = pytest.mark.gpu

PRIOR = (1e-4, 4e-4)
BOTH_GATES = dict(max_inliers_mean_distance=100.0, min_inliers_distribution=1e-4)     # both figures computed, nothing rejected


@pytest.fixture(scope="module")
def eng():
    import rtabmap_amd
    e = rtabmap_amd.Engine("f32", 64)
    yield e
    assert e.vocab_count() == (0, 0) and e.sig_count() == (0, 0)            # the calls are stateless: the engine is untouched
    e.close()


def traced(p, **kw):
    a, k = I.args(p, **kw)
    k["n_inliers"] = p.get("n_inliers")
    trace = []
    return M.refine(*a, **k, trace=trace), trace


# ---- two cameras

@pytest.fixture(scope="module")
def two():
    return I.two_camera_batch()


@pytest.mark.parametrize("gates", (False, True))
@pytest.mark.parametrize("reverse", (False, True))
def test_two_different_cameras_and_a_local_transform_on_either_side(eng, two, reverse, gates):
    """the local transform on the to side, the from side, on none and on both, every intrinsic, the image size and the baseline different
    between the sides; with the gates, inliers_distribution is the to-camera's cx, cy, width and height"""
    pairs = two[::-1] if reverse else two
    want = check_both(eng, pairs, prior=PRIOR, baselines=I.TWO_BASELINES, **dict(KW, **(BOTH_GATES if gates else {})))
    assert sorted(str(p["local_side"]) for p in pairs) == ["None", "both", "from", "to"]
    assert (want["status"] == M.OK).all() and (want["lm_accepted"] > 0).all() and want["n_outliers"].all()
    assert want["inliers_distribution"].all() == gates and want["inliers_mean_distance"].all() == gates


# ---- the hand-made branch cases

@pytest.fixture(scope="module")
def branches():
    return [I.mixed_edges_pair(), I.to_only_pair(), I.late_outlier_pair(), I.between_thresholds_pair(),
            I.seeded(500, 60, outliers=2, outlier_px=(3.5, 5.0), noise=0.3)]


@pytest.mark.parametrize("reverse", (False, True))
def test_the_branch_cases_in_one_launch(eng, branches, reverse):
    """a stereo and a mono edge on one point; a point that loses its to-edge alone and is reset; a point flagged behind the second stage; a
    chi2 between delta and its square; rejected trials and the ten that end a stage"""
    pairs = branches[::-1] if reverse else branches
    want = check_both(eng, pairs, **KW)
    n_out = dict(zip(("mixed", "to_only", "late", "between", "rejected"), want["n_outliers"][::-1] if reverse else want["n_outliers"]))
    assert (want["status"] == M.OK).all()
    assert n_out["mixed"] == 0 and n_out["between"] == 1 and n_out["rejected"] > 0
    # what the model's result, which both entries equal, says of the two searched pairs (tests/test_motion_ba_inputs.py has the whole proof):
    # a point nobody planted is an outlier through its to-edge alone; a point is an outlier that only the second stage flagged
    r, trace = traced(branches[1])
    first = [e[2] for e in trace if e[0] == "flagged" and e[1] == 0][0]
    alone = [i for i, side in first if side == "to" and (i, "from") not in first]
    assert alone and not set(alone) & set(branches[1]["planted"]) and n_out["to_only"] == r["n_outliers"] and not np.isin(branches[1]["inliers"][alone], r["inliers"]).any()
    r, trace = traced(branches[2])
    late = [i for i, _ in [e[2] for e in trace if e[0] == "flagged" and e[1] == 1][0]]
    assert late and n_out["late"] == r["n_outliers"] and not np.isin(branches[2]["inliers"][late], r["inliers"]).any()


def test_the_branch_cases_without_a_kernel_beside_the_1e12_abort(eng, branches):
    want = check_both(eng, branches + [I.huge_pair()], **dict(KW, robust_delta=0.0))
    assert want["status"].tolist() == [M.OK] * 5 + [M.DIVERGED] and want["chi2_after"][5] > 1e12 and not want["n_outliers"].any()
    assert not want["transform"][5].any() and want["n_inliers"][5] == 30


def test_the_branch_cases_without_from_keypoints_and_to_points(eng, branches):
    want = check_both(eng, branches, from_points=False, to_xyz=False, **KW)
    assert (want["status"] == M.OK).all()


# ---- the join

@pytest.fixture(scope="module")
def extremes():
    return I.extreme_id_pairs()


def test_the_join_at_its_extreme_ids_and_smallest_frames(eng, extremes):
    """INT32_MIN, -1, 0, 1 and INT32_MAX as inliers, INT32_MAX the largest key next to the padding keys; one pair per way an inlier is no
    unique id of both frames with a finite from-point; frames of 0, 1 and 2 rows, those of 0 rows first, in the middle and last"""
    empty = ("rows_0_to_one", "rows_0_from", "rows_0_to_none")
    rest = [n for n in extremes if n not in empty]
    names = [empty[0]] + rest[:len(rest) // 2] + [empty[1]] + rest[len(rest) // 2:] + [empty[2]]
    assert sorted(names) == sorted(extremes)
    pairs = [extremes[n][0] for n in names]
    assert 0 in (pairs[0]["to_ids"].shape[0], pairs[-1]["to_ids"].shape[0]) and pairs[1 + len(rest) // 2]["from_ids"].shape[0] == 0
    want = check_both(eng, pairs, **KW)
    assert want["status"].tolist() == [extremes[n][1] for n in names]
    at = 0
    for k, p in enumerate(pairs):
        nt = p["to_ids"].shape[0]
        region = want["inliers"][at:at + nt]
        if want["status"][k] == M.OK:
            assert want["lm_accepted"][k] > 0 and want["transform"][k].any() and I.INT32_MAX in region[:want["n_inliers"][k]]
        else:                                                              # the ids as they came, zeros behind them, no transform
            n = max(min(p.get("n_inliers", len(p["inliers"])), nt), 0)
            assert not want["transform"][k].any() and want["n_inliers"][k] == n
            assert region.tolist() == p["inliers"][:n].tolist() + [0] * (nt - n)
        at += nt


def test_a_batch_whose_to_frames_are_all_empty(eng, extremes):
    """n_pairs > 0 and not one to-row: no inlier region, no scratch row"""
    pairs = [extremes[n][0] for n in ("rows_0_to_one", "rows_0_to_none", "rows_0_to_one")]
    want = check_both(eng, pairs, **KW)
    assert want["status"].tolist() == [M.BAD_INLIER, M.NO_INPUT, M.BAD_INLIER] and want["inliers"].shape[0] == 0 and not want["n_inliers"].any()


# ---- the staged state

@pytest.fixture(scope="module")
def staging():
    return I.staging_pairs()


@pytest.mark.parametrize("reverse", (False, True))
def test_two_scratch_pairs_and_a_staged_one_in_one_launch(eng, staging, reverse):
    """STAGE_CAP + 1 inliers in 1800 rows, 40 inliers, STAGE_CAP + 1 inliers in 1790 rows: the scratch path with a stride that is not the
    inlier count, a second pair's state behind the first one's, an LDS-path pair between them"""
    pairs = staging[::-1] if reverse else staging
    assert [p["m"] for p in staging] == [I.STAGE_CAP + 1, 40, I.STAGE_CAP + 1] and [p["to_ids"].shape[0] for p in staging] == [1800, 48, 1790]
    want = check_both(eng, pairs, **KW)
    assert (want["status"] == M.OK).all() and want["n_outliers"].all() and (want["lm_accepted"] > 0).all()


@pytest.mark.parametrize("beside", ("alone", "behind", "in_front"))
def test_8192_rows_with_few_inliers(eng, beside):
    """the state of 100 points staged over the carve that held 2 x 8192 keys; beside a pair of nine rows"""
    wide, nine = I.made("wide_pair"), I.made("nine_row_pair")
    assert wide["to_ids"].shape[0] == wide["from_ids"].shape[0] == 8192 and wide["m"] == 100 and nine["to_ids"].shape[0] == 9
    pairs = {"alone": [wide], "behind": [nine, wide], "in_front": [wide, nine]}[beside]
    want = check_both(eng, pairs, **KW)
    assert (want["status"] == M.OK).all() and want["n_outliers"].max() >= 10


# ---- per-pair arguments, more pairs than compute units

def test_320_pairs_with_their_own_prior_and_baselines(eng):
    """eight distinct pairs tiled to 320, prior variances and baselines that differ from pair to pair (nine distinct rows, so that the model
    runs 72 times), every third pair's prior variances at or below both floors"""
    distinct = I.many_pairs()
    pairs = distinct * (I.MANY_PAIRS // len(distinct))
    rows = I.per_pair_kw(pairs, period=I.MANY_PERIOD)
    assert len(pairs) == I.MANY_PAIRS == 320 and (rows["prior"][1:] != rows["prior"][:-1]).any(axis=1).all() and (rows["baselines"][1:] != rows["baselines"][:-1]).any(axis=1).all()
    want = check_both(eng, pairs, prior=rows["prior"], baselines=rows["baselines"], **KW)
    assert (want["status"] == M.OK).all() and (want["lm_accepted"] > 0).all()
    assert len({want["transform"][k].tobytes() for k in range(0, 320, 8)}) == I.MANY_PERIOD             # one pair under every row


def test_eight_pairs_with_eight_different_rows(eng):
    pairs = I.many_pairs()
    rows = I.per_pair_kw(pairs)
    want = check_both(eng, pairs, prior=rows["prior"], baselines=rows["baselines"], **dict(KW, **BOTH_GATES))
    assert (want["status"] == M.OK).all()


# ---- the gates

def test_a_to_camera_that_is_not_valid_skips_the_distribution_gate(eng):
    """cx = 0, cy < 0, width 0, height 0, each on a pair a valid camera rejects"""
    want = check_both(eng, I.gate_camera_pairs(), baselines=I.TWO_BASELINES, **dict(KW, **I.GATES_KW))
    assert (want["status"] == M.OK).all() and not want["inliers_distribution"].any() and want["inliers_mean_distance"].all()


def test_to_points_that_count_for_no_depth_and_the_first_gate_of_two(eng):
    """to-points with one coordinate NaN or +inf, with depth 0 and a negative depth; a pair whose survivors have no finite to-point, which
    skips the mean-distance gate; a pair both gates reject, which the first one does"""
    edge = [I.to_edge_pair(kind) for kind in I.TO_EDGE_KINDS]
    for p in edge:
        to_stereo = [e for e in traced(p)[1] if e[0] == "edges"][0][2]
        assert not to_stereo[list(I.TO_EDGE_ROWS)].any() and to_stereo.sum() == p["m"] - len(I.TO_EDGE_ROWS)
    none, far = I.no_finite_to_pair(), I.far_narrow_pair()
    want = check_both(eng, edge + [none, far], **dict(KW, **I.GATES_KW))
    assert want["status"].tolist() == [M.OK] * 5 + [M.MEAN_DISTANCE_REJECTED]
    assert want["inliers_mean_distance"][:4].all() and want["inliers_mean_distance"][4] == 0 and want["inliers_distribution"][:5].all()
    assert want["inliers_mean_distance"][5] > 7.5 and want["inliers_distribution"][5] == 0 and not want["transform"][5].any()
    want = check_both(eng, [none], **dict(KW, max_inliers_mean_distance=0.5))         # a bound every pair with a depth would fail
    assert want["status"][0] == M.OK and want["inliers_mean_distance"][0] == 0 and want["n_inliers"][0] > 0


# ---- the iteration count

@pytest.mark.parametrize("iterations", (1, 6))
def test_the_iteration_count_bounds_the_second_stage(eng, iterations):
    """the first stage runs its five iterations whatever the argument says"""
    pairs = I.made("count_pairs")[3:6]
    want = check_both(eng, pairs, prior=PRIOR, **dict(KW, iterations=iterations))
    ends = [{e[1]: e[2] for e in traced(p, prior_variance=PRIOR, iterations=iterations)[1] if e[0] == "stage_end"} for p in pairs]
    assert (want["status"] == M.OK).all() and all(e[0] == M.STAGE1 and 1 <= e[1] <= iterations for e in ends)
    assert ((want["lm_accepted"] >= M.STAGE1 + 1) & (want["lm_accepted"] <= M.STAGE1 + iterations)).all()
