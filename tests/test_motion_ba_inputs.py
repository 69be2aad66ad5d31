"""Proves without a GPU, through the model's trace, that each hand-made input of tests/motion_ba_inputs.py takes the branch it exists for."""
import numpy as np
import pytest

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


# ---- the inputs of tests/test_gpu_motion_ba_shapes.py

def bits(r):
    """every output of a result as bytes"""
    return b"".join(np.asarray(r[k]).tobytes() for k in sorted(r))


def edges(trace):
    return [e for e in trace if e[0] == "edges"][0]


def test_every_existing_pair_keeps_its_cameras():
    for p in (I.seeded(1, 5), I.seeded(1, 5, local=True)):
        a, k = I.args(p)
        c = I.concatenate([p])
        for cam in (k["camera_from"], k["camera_to"], c["cameras_from"][0], c["cameras_to"][0]):
            assert set(cam) == set(I.camera(True, p["local"])) and all(np.array_equal(cam[n], v) for n, v in I.camera(True, p["local"]).items())


def test_the_two_cameras_share_nothing():
    for k in ("fx", "fy", "cx", "cy", "image_width", "image_height"):
        assert I.CAMERA_FROM[k] != I.CAMERA_TO[k]
    assert I.CAMERA_FROM["fx"] != I.CAMERA_FROM["fy"] and I.CAMERA_TO["fx"] != I.CAMERA_TO["fy"] and I.TWO_BASELINES[0] != I.TWO_BASELINES[1]
    pairs = I.two_camera_batch()
    assert [p["local_side"] for p in pairs] == ["to", "from", None, "both"]
    for p in pairs:
        assert ("local_transform" in p["camera_from"]) == (p["local_side"] in ("from", "both"))
        assert ("local_transform" in p["camera_to"]) == (p["local_side"] in ("to", "both"))
        a, k = I.args(p)
        assert k["camera_from"] is p["camera_from"] and k["camera_to"] is p["camera_to"]
        c = I.concatenate([p])
        assert c["cameras_from"][0] is p["camera_from"] and c["cameras_to"][0] is p["camera_to"]


@pytest.mark.parametrize("k", range(4))
def test_a_two_camera_pair_adjusts_and_tells_each_mix_up_apart(k):
    """the pair is a valid input (status OK, the planted outliers flagged, the result nearer the true transform than the start), and each way
    of taking one side for the other changes the output's bits"""
    p = I.two_camera_batch()[k]
    kw = dict(baselines=I.TWO_BASELINES, prior_variance=(1e-4, 4e-4), max_inliers_mean_distance=100.0, min_inliers_distribution=1e-4)
    r, tr = run(p, **kw)
    assert r["status"] == M.OK and r["lm_accepted"] > 0 and r["n_outliers"] >= len(p["planted"])
    assert all(p["inliers"][i] not in r["inliers"] for i in p["planted"])
    assert np.abs(r["transform"] - p["true"]).max() < 0.75 * np.abs(p["transform"] - p["true"]).max()
    assert edges(tr)[1].any() and edges(tr)[2].any()
    cf, ct = p["camera_from"], p["camera_to"]
    swapped = run(dict(p, camera_from=ct, camera_to=cf), **kw)[0]
    assert bits(swapped) != bits(r)
    moved = lambda cam, has: dict({n: v for n, v in cam.items() if n != "local_transform"}, **({"local_transform": I.PI.LOCAL} if has else {}))
    if p["local_side"] in ("from", "to"):                               # the local transform on the other side
        other = run(dict(p, camera_from=moved(cf, p["local_side"] == "to"), camera_to=moved(ct, p["local_side"] == "from")), **kw)[0]
        assert bits(other) != bits(r) and other["transform"].tobytes() != r["transform"].tobytes()
    else:                                                               # on both or on none: one side's taken away or added
        for side in ("camera_from", "camera_to"):
            other = run(dict(p, **{side: moved(p[side], p["local_side"] is None)}), **kw)[0]
            assert bits(other) != bits(r)
    assert run(p, **dict(kw, baselines=I.TWO_BASELINES[::-1]))[0]["transform"].tobytes() != r["transform"].tobytes()
    sized = run(dict(p, camera_to=dict(ct, image_width=cf["image_width"], image_height=cf["image_height"])), **kw)[0]
    assert sized["transform"].tobytes() == r["transform"].tobytes() and sized["inliers_distribution"].tobytes() != r["inliers_distribution"].tobytes()


def test_the_extreme_ids_end_as_listed():
    cases = I.extreme_id_pairs()
    for name, (p, status) in cases.items():
        r, tr = run(p)
        assert r["status"] == status, name
        if status == M.OK:
            assert r["lm_accepted"] > 0 and r["transform"].any(), name
            kept = set(r["inliers"].tolist())
            assert I.INT32_MAX in kept and (I.INT32_MIN in kept) == (I.INT32_MIN in p["inliers"].tolist()), name
        else:
            assert not r["transform"].any() and r["inliers"].tolist() == p["inliers"][:max(min(p.get("n_inliers", 1 << 30), len(p["inliers"])), 0)].tolist(), name
    both = [name for name, (p, s) in cases.items() if s == M.OK and {I.INT32_MIN, -1, 0, 1, I.INT32_MAX} <= set(p["inliers"].tolist())]
    assert "ok" in both and "ok_six" in both and "rows_2" not in both
    for name in ("ok", "ok_six"):
        p = cases[name][0]
        assert (p["from_ids"].shape[0], p["to_ids"].shape[0]) == I.T3.EXTREME_ROWS and p["from_ids"].max() == p["to_ids"].max() == I.INT32_MAX
    assert sorted((p["from_ids"].shape[0], p["to_ids"].shape[0]) for name, (p, _) in cases.items() if name.startswith("rows_")) == \
        [(0, 5), (1, 1), (1, 70), (2, 2), (2, 2), (5, 0), (5, 0)]
    # each BAD_INLIER pair has the one cause its name says
    count = lambda ids, i: int((ids == i).sum())
    p = cases["above_every_key"][0]
    assert I.INT32_MAX in p["inliers"] and p["inliers"].max() > max(p["from_ids"].max(), p["to_ids"].max())
    p = cases["below_every_key"][0]
    assert I.INT32_MIN in p["inliers"] and p["inliers"].min() < min(p["from_ids"].min(), p["to_ids"].min())
    p = cases["max_twice_in_to"][0]
    assert count(p["to_ids"], I.INT32_MAX) == 2 and count(p["from_ids"], I.INT32_MAX) == 1 and count(p["inliers"], I.INT32_MAX) == 1
    p = cases["max_twice_in_from"][0]
    assert count(p["from_ids"], I.INT32_MAX) == 2 and count(p["to_ids"], I.INT32_MAX) == 1 and count(p["inliers"], I.INT32_MAX) == 1
    p = cases["in_to_only"][0]
    assert [i for i in p["inliers"] if i not in p["from_ids"]] == [p["inliers"][-1]] and p["inliers"][-1] in p["to_ids"]
    p = cases["in_from_only"][0]
    assert [i for i in p["inliers"] if i not in p["to_ids"]] == [I.INT32_MIN + 1] and I.INT32_MIN + 1 in p["from_ids"]
    p = cases["twice_in_from"][0]
    assert sorted(count(p["from_ids"], i) for i in p["inliers"])[-2:] == [1, 2] and all(count(p["to_ids"], i) == 1 for i in p["inliers"])
    p = cases["from_point_not_finite"][0]
    assert (~np.isfinite(p["from_xyz"])).sum() == 1 and run(dict(p, from_xyz=np.nan_to_num(p["from_xyz"], posinf=1.0)))[0]["status"] == M.OK
    p, q = cases["count_negative"][0], cases["count_above_rows"][0]
    assert p["n_inliers"] == -1 and q["n_inliers"] == q["to_ids"].shape[0] + 1 == q["inliers"].shape[0] + 1
    assert run(dict(p, n_inliers=len(p["inliers"])))[0]["status"] == M.OK and run(dict(q, n_inliers=10))[0]["status"] == M.OK


@pytest.mark.parametrize("kind", I.TO_EDGE_KINDS)
def test_a_to_point_with_one_bad_coordinate_gives_a_mono_to_edge(kind):
    p = I.to_edge_pair(kind)
    rows = [int(np.flatnonzero(p["to_ids"] == p["inliers"][i])[0]) for i in I.TO_EDGE_ROWS]
    bad = ~np.isfinite(p["to_xyz"][rows])
    if kind in ("nan", "inf"):
        assert bad.sum(axis=1).tolist() == [1, 1, 1] and bad.any(axis=0).all()         # one coordinate each, every coordinate once
    else:
        assert not bad.any() and all(p["to_xyz"][r, 2] == 0 if kind == "zero" else p["to_xyz"][r, 2] < 0 for r in rows)
    r, tr = run(p, max_inliers_mean_distance=100.0)
    _, from_stereo, to_stereo, _ = edges(tr)
    special = np.zeros(p["m"], bool)
    special[list(I.TO_EDGE_ROWS)] = True
    assert from_stereo.all() and not to_stereo[special].any() and to_stereo[~special].all()
    assert r["status"] == M.OK and r["inliers_mean_distance"] > 0
    whole = I.to_edge_pair(kind)                                        # the same rows all-NaN: another mean distance where the rows are finite
    whole["to_xyz"][rows] = np.nan
    other = run(whole, max_inliers_mean_distance=100.0)[0]
    assert (other["inliers_mean_distance"] != r["inliers_mean_distance"]) == (kind in ("zero", "negative"))


def test_no_finite_to_point_skips_the_mean_distance_gate():
    p = I.no_finite_to_pair()
    r, tr = run(p, max_inliers_mean_distance=0.5)
    assert r["status"] == M.OK and r["inliers_mean_distance"] == 0 and len(r["inliers"]) > 0 and not edges(tr)[2].any()
    q = I.seeded(735, 40, nan_to=0.0)                                   # the same pair with its to-points: the gate rejects it
    assert run(q, max_inliers_mean_distance=0.5)[0]["status"] == M.MEAN_DISTANCE_REJECTED


def test_an_invalid_to_camera_skips_the_distribution_gate():
    pairs = I.gate_camera_pairs()
    assert len(pairs) == len(I.GATE_CAMERAS) == 4
    for p, cam in zip(pairs, I.GATE_CAMERAS):
        assert sum(cam[k] != I.CAMERA_TO[k] for k in cam) == 1 and (cam["cx"] <= 0 or cam["cy"] <= 0 or cam["image_width"] == 0 or cam["image_height"] == 0)
        r, _ = run(p, baselines=I.TWO_BASELINES, **I.GATES_KW)
        assert r["status"] == M.OK and r["inliers_distribution"] == 0 and r["inliers_mean_distance"] > 0
        valid = dict(p, camera_to=dict(p["camera_to"], **{k: I.CAMERA_TO[k] for k in ("cx", "cy", "image_width", "image_height")}))
        r, _ = run(valid, baselines=I.TWO_BASELINES, min_inliers_distribution=0.01)
        assert r["status"] == M.DISTRIBUTION_REJECTED and 0 < r["inliers_distribution"] < 0.01


def test_the_mean_distance_gate_is_the_first_of_the_two():
    p = I.far_narrow_pair()
    assert run(p, max_inliers_mean_distance=7.5)[0]["status"] == M.MEAN_DISTANCE_REJECTED
    assert run(p, min_inliers_distribution=0.01)[0]["status"] == M.DISTRIBUTION_REJECTED
    r, _ = run(p, **I.GATES_KW)
    assert r["status"] == M.MEAN_DISTANCE_REJECTED and r["inliers_mean_distance"] > 7.5 and r["inliers_distribution"] == 0


def test_the_per_pair_rows_differ_and_every_third_is_a_floor():
    pairs = I.many_pairs()
    assert [p["m"] for p in pairs] == list(I.MANY_SIZES) and min(I.MANY_SIZES) == 3 and max(I.MANY_SIZES) == 65
    kw = I.per_pair_kw(pairs)
    assert kw["prior"].shape == kw["baselines"].shape == (8, 2) and len({tuple(r) for r in kw["baselines"].tolist()}) == 8
    assert len({tuple(r) for r in kw["prior"].tolist()}) == 7             # (the floors take turns: the first and the third are the same row)
    tiled = I.per_pair_kw(pairs * (I.MANY_PAIRS // 8), period=I.MANY_PERIOD)
    assert tiled["prior"].shape == (I.MANY_PAIRS, 2) and len({tuple(r) for r in np.concatenate([tiled["prior"], tiled["baselines"]], axis=1).tolist()}) == I.MANY_PERIOD
    for k in range(I.MANY_PAIRS):
        lin, ang = tiled["prior"][k]
        floor = lin <= M.LINEAR_EPSILON and ang <= M.ANGULAR_EPSILON
        assert floor == (k % 3 == 0)
        if floor:
            assert M.prior_information(lin, M.LINEAR_EPSILON) == M.F(1e8) and M.prior_information(ang, M.ANGULAR_EPSILON) == M.F(1 / 3e-8)
    assert {tuple(r) for r in tiled["prior"][::3].tolist()} == set(I.PRIOR_FLOORS)
    # a pair's result depends on its row: a kernel that read another pair's would differ
    p = pairs[5]
    seen = {bits(run(p, prior_variance=tuple(tiled["prior"][k]), baselines=tuple(tiled["baselines"][k]))[0]) for k in range(I.MANY_PERIOD)}
    assert len(seen) == I.MANY_PERIOD
    b = tuple(tiled["baselines"][1])
    assert bits(run(p, baselines=b)[0]) != bits(run(p, baselines=b[::-1])[0])


def test_the_staging_pairs_leave_lds_and_the_wide_pair_does_not():
    big, small, big2 = I.staging_pairs()
    assert big["m"] == big2["m"] == I.STAGE_CAP + 1 and small["m"] == 40 <= I.STAGE_CAP
    assert (big["to_ids"].shape[0], big2["to_ids"].shape[0]) == (1800, 1790) and big["from_ids"].shape[0] == 1800
    wide, nine = I.wide_pair(), I.nine_row_pair()
    assert wide["to_ids"].shape[0] == wide["from_ids"].shape[0] == 8192 and wide["m"] == 100 and nine["to_ids"].shape[0] == 9
    for p in (big, small, big2, wide, nine):
        r, _ = run(p)
        assert r["status"] == M.OK and (r["n_outliers"] > 0) == (len(p["planted"]) > 0) and r["lm_accepted"] > 0


def test_the_iteration_count_bounds_the_second_stage_only():
    for p in I.count_pairs()[3:6]:
        ends = {}
        for it in (1, 6):
            r, tr = run(p, iterations=it)
            ends[it] = {e[1]: e[2] for e in tr if e[0] == "stage_end"}
            assert r["status"] == M.OK and ends[it][0] == M.STAGE1 and 1 <= ends[it][1] <= it
        assert ends[6][1] > 1
