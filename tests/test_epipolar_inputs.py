"""Each hand-made pair of epipolar_inputs.py takes the branch of the rule it was made for: read off the model's trace.  No GPU, no library."""
import numpy as np

import epipolar_inputs as I
import epipolar_model as M


def run(pair, **kw):
    trace = {}
    kw.setdefault("iterations", 60)
    return M.verify(*I.frames(pair), trace=trace, **kw), trace


def test_ids_negative_doubled_and_at_the_ends_of_the_range():
    p = I.id_cases()
    r, _ = run(p)
    assert r["matches"].tolist() == p["expect_matches"]
    assert I.INT32_MAX in r["matches"] and I.INT32_MIN not in r["matches"] and -3 not in r["matches"]
    assert 500001 not in r["matches"] and 500002 not in r["matches"] and 500003 not in r["matches"]   # doubled in from, in to, in both
    assert r["status"] == M.OK


def test_pair_counts_around_the_two_minima():
    assert run(I.with_m(7))[0]["status"] == M.FEW_PAIRS                      # m < 8 whatever match_count_min
    assert run(I.with_m(7), match_count_min=1)[0]["status"] == M.FEW_PAIRS
    r, t = run(I.with_m(8))
    assert r["status"] == M.OK and r["matches"].shape[0] == 8 and t["count"] == 8
    assert run(I.with_m(11), match_count_min=12)[0]["status"] == M.FEW_PAIRS   # m = match_count_min - 1
    assert run(I.with_m(12), match_count_min=12)[0]["status"] != M.FEW_PAIRS


def test_all_keypoints_equal_have_no_scale():
    p = I.all_equal()
    assert not M.normalisation(M.correspondences(*I.frames(p))[1][:, :2])[0]
    r, t = run(p)
    assert r["status"] == M.NO_MODEL and t == {} and not r["fundamental"].any()


def test_collinear_keypoints_leave_no_seventh_pivot():
    r, t = run(I.collinear())
    assert t["no_pivot"] == 60 and t["not_drawn"] == 0 and r["status"] == M.NO_MODEL


def test_two_free_zero_columns_give_a_cubic_without_leading_coefficient():
    r, t = run(I.c3_zero())
    assert t["no_pivot"] == 0 and t["c3_zero"] == 60 and r["status"] == M.NO_MODEL


def test_cubics_with_one_and_with_three_real_roots():
    r, t = run(I.scene(1, 120), iterations=200)
    assert t["one_root"] > 0 and t["three_roots"] > 0 and t["one_root"] + t["three_roots"] == 200 and r["status"] == M.OK


def test_a_nan_keypoint_is_a_pair_and_takes_the_model_away():
    p = I.nan_keypoint()
    r, _ = run(p)
    assert p["nan_id"] in r["matches"] and r["status"] == M.NO_MODEL and r["inliers"].size == 0


def test_a_best_count_one_below_and_at_match_count_min():
    p = I.scene(3, 100)
    r, t = run(p, match_count_min=8)
    n = t["count"]
    assert r["inliers"].shape[0] == n and 8 < n < 100
    at, _ = run(p, match_count_min=n)
    above, _ = run(p, match_count_min=n + 1)
    assert at["status"] == M.OK and above["status"] == M.FEW_INLIERS
    assert np.array_equal(at["inliers"], above["inliers"]) and np.array_equal(M.bits(at["fundamental"]), M.bits(above["fundamental"]))


def test_a_planar_scene_decides_like_a_general_one():
    assert run(I.scene(4, 120, planar=True), iterations=200)[0]["status"] == M.OK


def test_too_few_distinct_draws_invalidate_nothing_at_m_8():
    """with m = 8 a hypothesis needs seven of eight indices within 32 draws; the trace says how many did not get them"""
    _, t = run(I.with_m(8), iterations=300)
    assert t["not_drawn"] < 300
