"""Proves without a GPU, through the model's trace, that each hand-made input of tests/motion_ba_inputs.py takes the branch it exists for."""
import numpy as np

import motion_ba_inputs as I
import motion_ba_model as M


def run(p, from_points=True, to_xyz=True, **kw):
    a, k = I.args(p, from_points, to_xyz, **kw)
    k["n_inliers"] = p.get("n_inliers")
    trace = []
    return M.refine(*a, **k, trace=trace), trace


def flagged(trace, stage):
    return [e[2] for e in trace if e[0] == "flagged" and e[1] == stage][0]


def test_a_stereo_and_a_mono_edge_on_the_same_point():
    r, tr = run(I.mixed_edges_pair())
    _, from_stereo, to_stereo, present = [e for e in tr if e[0] == "edges"][0]
    assert present and from_stereo.all() and (from_stereo & ~to_stereo).any() and (from_stereo & to_stereo).any()
    assert r["status"] == M.OK


def test_no_from_keypoints_and_no_positive_baseline():
    p = I.seeded(330, 50)
    r, tr = run(p, from_points=False)
    assert [e for e in tr if e[0] == "edges"][0][3] is False and r["status"] == M.OK and r["lm_accepted"] > 0
    r, tr = run(p, baselines=(0.0, -0.1))
    _, from_stereo, to_stereo, _ = [e for e in tr if e[0] == "edges"][0]
    assert not from_stereo.any() and not to_stereo.any() and r["status"] == M.OK
    r, tr = run(p, to_xyz=False)
    assert not [e for e in tr if e[0] == "edges"][0][2].any()


def test_a_point_flagged_through_its_to_edge_alone_keeps_its_from_edge():
    p = I.to_only_pair()
    r, tr = run(p)
    first = flagged(tr, 0)
    alone = [i for i, side in first if side == "to" and (i, "from") not in first]
    # (a planted gross outlier drags its point along inside the five iterations, so that both of its edges pass delta: the planted ones
    # that are flagged are flagged through both here; the edge that leaves alone belongs to a point the pulled pose pushes over the threshold on the to side)
    assert alone and any((i, "from") in first and (i, "to") in first for i in p["planted"])
    assert all(p["inliers"][i] not in r["inliers"] for i in alone)          # an outlier although one of its edges stays
    _, _, flags, P, P0 = [e for e in tr if e[0] == "state" and e[1] == 0][0]
    _, _, cf2, ct2 = [e for e in tr if e[0] == "chi2" and e[1] == 1][0]
    for i in alone:
        assert flags[i] & M.F_TO_OUT and flags[i] & M.F_OUTLIER and not flags[i] & M.F_FROM_OUT
        assert P[i].tobytes() == P0[i].tobytes()                          # reset to its initial estimate
        assert M.from_active(flags)[i] and cf2[i] > 0 and ct2[i] == 0      # the second stage works on its from-edge alone
    assert r["status"] == M.OK and r["n_outliers"] >= len(set(i for i, _ in first))


def test_a_point_flagged_only_behind_the_second_stage():
    p = I.late_outlier_pair()
    r, tr = run(p)
    first, second = flagged(tr, 0), flagged(tr, 1)
    assert second and not {i for i, _ in second} & {i for i, _ in first}
    assert all(p["inliers"][i] not in r["inliers"] for i, _ in second)


def test_a_chi2_between_delta_and_its_square_is_flagged():
    p = I.between_thresholds_pair()
    r, tr = run(p)
    i = p["planted"][0]
    _, _, cf, ct = [e for e in tr if e[0] == "chi2" and e[1] == 0][0]
    assert (i, "to") in flagged(tr, 0) and 8.0 < ct[i] < 64.0             # g2o's kernel would still call it an inlier (chi2 <= delta^2)
    assert r["n_outliers"] == 1 and p["inliers"][i] not in r["inliers"]


def test_a_rejected_trial_restores_the_state_and_ten_end_a_stage():
    p = I.seeded(500, 60, outliers=2, outlier_px=(3.5, 5.0), noise=0.3)
    r, tr = run(p)
    trials = [e for e in tr if e[0] == "trial"]
    assert any(a[4] == "rejected" and b[4] == "accepted" and a[1:3] == b[1:3] for a, b in zip(trials, trials[1:]))
    last = [e for e in trials if e[1] == 1][-M.TRIALS:]
    assert len(last) == M.TRIALS and all(e[4] != "accepted" for e in last) and [e[3] for e in last] == list(range(M.TRIALS))
    ends = {e[1]: e for e in tr if e[0] == "stage_end"}
    assert ends[1][2] < 20 and ends[0][2] == M.STAGE1
    assert r["chi2_after"] == ends[1][3] and r["chi2_after"] <= r["chi2_before"]


def test_the_nan_and_the_1e12_abort():
    p = I.nan_pair()
    r, tr = run(p)
    assert r["status"] == M.DIVERGED and np.isnan(r["chi2_after"]) and not r["transform"].any() and list(r["inliers"]) == list(p["inliers"])
    assert [e[1] for e in tr if e[0] == "stage_end"] == [0]                # (:1954: the first stage's test)
    r, tr = run(I.huge_pair(), robust_delta=0.0)
    assert r["status"] == M.DIVERGED and r["chi2_after"] > 1e12 and np.isfinite(r["chi2_after"]) and not r["transform"].any()


def test_below_min_inliers_behind_the_filtering_and_each_gate_alone():
    pairs, expect = I.status_batch()
    few, far, narrow = pairs[6], pairs[7], pairs[8]
    r, _ = run(few, min_inliers=20)
    assert r["status"] == M.BELOW_MIN_INLIERS and len(r["inliers"]) < 20 <= len(few["inliers"]) and not r["transform"].any()
    r, _ = run(far, max_inliers_mean_distance=7.5)
    assert r["status"] == M.MEAN_DISTANCE_REJECTED and r["inliers_mean_distance"] > 7.5 and r["inliers_distribution"] == 0
    assert run(far, max_inliers_mean_distance=7.5, to_xyz=False)[0]["status"] == M.OK         # no to-points: nothing to test
    r, _ = run(narrow, min_inliers_distribution=0.01)
    assert r["status"] == M.DISTRIBUTION_REJECTED and 0 < r["inliers_distribution"] < 0.01 and r["inliers_mean_distance"] == 0
    assert run(pairs[0], min_inliers_distribution=0.01)[0]["inliers_distribution"] > 0.01


def test_the_status_batch_has_every_status():
    pairs, expect = I.status_batch()
    assert sorted(set(expect)) == list(range(7))
    assert [run(p, **I.STATUS_KW)[0]["status"] for p in pairs] == expect
