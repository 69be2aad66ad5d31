"""Each input of tests/motion_pnp_inputs.py has the property it exists for.  No GPU.  What a search found is a constant there and is proven
again here."""
import numpy as np
import pytest

import motion_pnp_inputs as I
import motion_pnp_model as M

KW = dict(min_inliers=4, reproj_error=2.0, iterations=60, refine_iterations=5, variance_median_ratio=4, max_variance=0.0, seed=3)


def test_the_mixed_batch_has_its_sizes_and_its_decoys():
    for m, pair in zip(I.BATCH_SIZES, I.mixed_batch()):
        ids, P, UV, T = M.correspondences(*I.frames(pair))
        assert len(ids) == m == pair["m"] and ids.tolist() == pair["ids"].tolist()
        for side in ("from_ids", "to_ids"):                             # an id that occurs twice, ids of one side only
            vals, counts = np.unique(pair[side], return_counts=True)
            assert (counts == 2).sum() == 1
        assert len(set(pair["from_ids"].tolist()) - set(pair["to_ids"].tolist())) >= 3 and len(set(pair["to_ids"].tolist()) - set(pair["from_ids"].tolist())) >= 3
        shared = set(pair["from_ids"].tolist()) & set(pair["to_ids"].tolist())
        assert len(shared) == m + 3                                     # the two doubled ids and the one whose from-point is not finite
        assert (~np.isfinite(pair["from_xyz"]).all(axis=1)).sum() == 1
        if m >= 63:
            assert np.isnan(T).any() and np.isfinite(T).all(axis=1).sum() > m // 2
            assert ids.min() < 0                                        # negative ids take part
            # the generator's inliers reproject within a few pixels under its pose, its outliers do not as a rule
            e, front = M.reproj_error(I.true_model(pair), I.model_camera(I.CAMERA), P, UV)
            assert front.all() and (e[pair["inlier"]] < 3.0).all() and (e[~pair["inlier"]] > 3.0).mean() > 0.9


def test_the_special_pairs():
    r = M.estimate(*I.frames(I.all_outlier_pair()), **dict(KW, min_inliers=10, iterations=300))
    assert r["status"] != M.OK and r["counts"].max() < 10
    behind = I.behind_pair()
    _, P, UV, _ = M.correspondences(*I.frames(behind))
    assert len(P) == behind["m"] and (P[:, 2] < 0).all() and (P[:, 1] == 0).all() and len(set(P[:, 0].tolist())) == behind["m"]
    r = M.estimate(*I.frames(behind), **dict(KW, iterations=300))
    assert r["status"] == M.NO_MODEL and not r["counts"].any()
    seed = I.seed_with_invalid_first(4, 1)
    assert M.draw4(seed, 0, 4) is None and M.draw4(seed, 1, 4) is not None
    pair = I.mixed_batch()[6]
    for local in (None, I.LOCAL):                                       # guess_of inverts model_of_guess up to rounding
        back = M.model_of_guess(I.guess_of(I.true_model(pair), local), local)
        np.testing.assert_allclose(back, I.true_model(pair), atol=2e-6)


@pytest.mark.parametrize("name", sorted(I.REFINE_CASES))
def test_refine_cases_reach_their_branch(name):
    pair, kw = I.refine_case(name)
    r = M.estimate(*I.frames(pair), **dict(KW, **kw))
    assert I.REFINE_CASES[name][7] in r["trace"], r["trace"]
    if name == "size_members_few":
        assert {"size_changed", "members_changed", "few"} <= set(r["trace"]) and r["trace"][0] != "few"
    if name == "oscillating_guarded":
        assert "oscillating" not in r["trace"] and I.REFINE_CASES[name][:5] == I.REFINE_CASES["oscillating"][:5]
    if name == "step_sensitive":                                        # why the rule takes eight Gauss-Newton steps
        ids = [M.estimate(*I.frames(pair), **dict(KW, steps=s, **kw))["inliers"].tolist() for s in (6, 7, 8, 9, 10)]
        assert ids[0] != ids[1] and ids[1] == ids[2] == ids[3] == ids[4]


def test_the_staged_limit_and_the_big_pair():
    assert I.STAGE_CAP == {True: 3360, False: 5376}
    big = I.big_pair()
    assert big["from_ids"].shape[0] == big["to_ids"].shape[0] == 8192 == M.MAX_ROWS
    ids, _, _, _ = M.correspondences(*I.frames(big))
    assert len(ids) == 8000 > max(I.STAGE_CAP.values())


def test_the_fit_sets_are_in_general_position():
    sets = I.fit_sets()
    assert len(sets) == 27
    for s in sets:
        n = len(s["P"])
        assert 20 <= n <= 650 and n >= 8 and I.general_position(s["UV0"].astype(np.float64), s["C"])
        assert 0.5 <= s["C"][:, 2].min() and s["C"][:, 2].max() <= 10.0
        assert (s["UV0"][:, 0] >= 0).all() and (s["UV0"][:, 0] <= I.WIDTH - 1).all() and (s["UV0"][:, 1] >= 0).all() and (s["UV0"][:, 1] <= I.HEIGHT - 1).all()
        noise = s["UV1"] - s["UV0"]
        assert 0.3 < noise.std() < 0.7
        e, front = M.reproj_error(np.concatenate([s["R"], s["t"][:, None]], axis=1).reshape(12).astype(np.float32), I.model_camera(I.CAMERA), s["P"], s["UV0"])
        assert front.all() and e.max() < 0.01                           # noise-free up to fp32


# ---- the inputs of tests/test_gpu_motion_pnp_shapes.py

CAM = I.model_camera(I.CAMERA)


def estimate(call, k=0):
    cams = [call["cam"]] * len(call["pairs"]) if isinstance(call["cam"], dict) else call["cam"]
    return M.estimate(*I.frames(call["pairs"][k], call["to_xyz"]), camera=I.model_camera(cams[k]), guess=None if call["guesses"] is None else call["guesses"][k],
                      **call["kw"])


@pytest.fixture(scope="module")
def calls():
    return I.shape_calls()


def test_join_sizes_runs_extreme_ids_and_the_predicate(calls):
    sizes = I.join_size_pairs()
    for (nf, nt), pair in zip(I.JOIN_SIZES, sizes):
        assert (pair["from_ids"].shape[0], pair["to_ids"].shape[0]) == (nf, nt)
        assert len(M.correspondences(*I.frames(pair))[0]) == min(nf, nt, 60)
    assert all(I.T3.sort_length(nf) != I.T3.sort_length(nt) for nf, nt in I.JOIN_SIZES)      # two sorts of different lengths, every time
    lengths_over = {b: set() for b in (255, 511)}
    for k, pair in enumerate(I.duplicate_run_pairs()):
        runs = {side: I.T3.runs_of(pair[side]) for side in ("from_ids", "to_ids")}
        for side in runs:
            assert len(runs[side]) == 4 and (0 in runs[side]) != (k % 2 == (side == "from_ids"))       # A's run starts at 0, B's ends at the last row
            assert any(a + l == I.T3.RUN_ROWS for a, l in runs[side].items()) == (0 not in runs[side])
            for b in (63, 255, 511):
                over = [l for a, l in runs[side].items() if a <= b < b + 1 < a + l]
                assert len(over) == 1
                if b in lengths_over:
                    lengths_over[b].add(over[0])
        ids = M.correspondences(*I.frames(pair))[0]
        assert len(ids) == pair["m"] and not set(ids.tolist()) & set(pair["running"]) and len(pair["running"]) == 8
    assert lengths_over == {255: {2, 3, 5}, 511: {2, 3, 5}}
    unique, in_to, in_from = (M.correspondences(*I.frames(p))[0].tolist() for p in I.extreme_id_pairs())
    assert unique[0] == I.INT32_MIN and unique[-1] == I.INT32_MAX and len(unique) == 10
    for ids, pair in ((in_to, I.extreme_id_pairs()[1]), (in_from, I.extreme_id_pairs()[2])):
        assert I.INT32_MIN not in ids and I.INT32_MAX not in ids and len(ids) == 9
        doubled = sorted(int(i) for side in ("from_ids", "to_ids") for i, c in zip(*np.unique(pair[side], return_counts=True)) if c == 2)
        assert doubled == [I.INT32_MIN, I.INT32_MAX]
    pred = I.predicate_pair()
    ids, P, UV, _ = M.correspondences(*I.frames(pred))
    dropped = [int(pred["ids"][k]) for k in I.PREDICATE_FROM]
    assert len(ids) == I.PREDICATE_ROWS - 3 and not set(dropped) & set(ids.tolist())
    for k, (c, v) in I.PREDICATE_FROM.items():                          # one coordinate only
        p = pred["from_xyz"][pred["from_ids"] == pred["ids"][k]][0]
        assert (~np.isfinite(p)).sum() == 1 and not np.isfinite(p[c])
    assert np.isfinite(P).all() and (~np.isfinite(UV)).sum() == 3
    r = estimate(calls["join_1"], len(calls["join_1"]["pairs"]) - 1)
    held = [int(pred["ids"][k]) for k in I.PREDICATE_KEYPOINT]
    assert r["status"] == M.OK and set(held) <= set(r["matches"].tolist()) and not set(held) & set(r["inliers"].tolist())
    assert len(r["inliers"]) == len(ids) - 3
    for name in ("join_1", "join_0"):
        assert [p["from_ids"].shape[0] for p in calls[name]["pairs"]][:8] == [nf for nf, _ in I.JOIN_SIZES]
    assert {c["section"] for c in calls.values()} == set(I.SHAPE_SECTIONS)     # every call is filed under one section, every section has a call
    assert sum(len(I.section_calls(s, calls)) for s in I.SHAPE_SECTIONS) == len(calls)


def test_keypoints_that_are_not_finite_make_their_hypotheses_invalid(calls):
    """three of ten keypoints are NaN, +inf, -inf in one coordinate: hypotheses draw each of them among their three points and as the fourth,
    none of those is valid or counts anything, the others are valid and one of them wins"""
    call = calls["keypoints"]
    pair, kw = call["pairs"][0], call["kw"]
    ids, P, UV, _ = M.correspondences(*I.frames(pair))
    bad = set(I.KEYPOINT_ROWS)
    assert len(ids) == 10 and np.isfinite(P).all() and set(np.nonzero(~np.isfinite(UV).all(axis=1))[0].tolist()) == bad
    assert sorted(str(UV[k, c]) for k, (c, v) in I.KEYPOINT_ROWS.items()) == ["-inf", "inf", "nan"]
    hs, has, solutions = I.hypotheses(pair, CAM, kw["seed"], kw["iterations"])
    draws = [M.draw4(kw["seed"], int(h), 10) for h in hs]
    triple = np.array([bool(bad & set(d[:3])) for d in draws])
    fourth = np.array([d[3] in bad for d in draws]) & ~triple
    assert {k for d, t in zip(draws, triple) if t for k in d[:3]} >= bad and {d[3] for d, f in zip(draws, fourth) if f} >= bad
    assert triple.sum() >= 10 and fourth.sum() >= 3 and (~triple & ~fourth).sum() >= 2
    assert not has[triple | fourth].any() and has[~triple & ~fourth].all()
    assert not np.stack([s[0] for s in solutions])[:, triple | fourth].any()           # not one solution of any of them
    r = estimate(call)
    assert not r["counts"][hs[triple | fourth] + 1].any() and (r["counts"][hs[~triple & ~fourth] + 1] == 7).all() and r["counts"][0] == 0
    assert r["status"] == M.OK and r["best"] - 1 in hs[~triple & ~fourth].tolist() and len(r["matches"]) == 10
    assert sorted(set(r["matches"].tolist()) - set(r["inliers"].tolist())) == [int(ids[k]) for k in sorted(bad)]


@pytest.mark.parametrize("to_xyz", (False, True))
def test_layout_pairs_are_staged_and_not(to_xyz):
    staged, five, big = I.layout_pairs(to_xyz)
    cap = I.STAGE_CAP[to_xyz]
    m = [len(M.correspondences(*I.frames(p))[0]) for p in (staged, five, big)]
    assert m == [150, 5, cap + (1 if to_xyz else 4)]
    assert staged["to_ids"].shape[0] == 200 != m[0] <= cap              # staged: the stride is m, not the rows
    assert big["to_ids"].shape[0] == (8192 if to_xyz else 5500) != m[2] > cap      # from the scratch: the stride is the to-frame's rows


def test_ties_across_chunks(calls):
    tie = I.tie_pair()
    e, front = M.reproj_error(I.model_of_guess_flip(), CAM, *M.correspondences(*I.frames(tie))[1:3])
    assert not front.any()                                              # the guess sees every point behind it
    for it, full in ((255, 246), (65535, 62394)):
        r = estimate(calls["tie_%d" % it])
        assert r["best"] == 1 and r["counts"][0] == 0 and (r["counts"] == 40).sum() == full and r["counts"].max() == 40
    assert set(I.TIE_ITERATIONS) == {255, 256, 257, 511, 512, 65534, 65535}
    r = estimate(calls["tie_guess"])
    assert r["best"] == 0 and r["counts"][0] == 40 and (r["counts"] == 40).sum() > 200
    m, invalid, seed, _ = I.TIE_INVALID_FIRST
    assert seed == I.seed_with_invalid_first(m, invalid)
    r = estimate(calls["tie_invalid_first"])
    assert r["best"] == invalid + 1 and r["counts"][:invalid + 2].tolist() == [0] * (invalid + 1) + [m] and (r["counts"] == m).sum() > 100


def test_the_late_winner_and_its_cut_off(calls):
    pair = I.late_winner_pair()
    assert pair["inlier"].sum() == I.LATE_INLIERS and pair["m"] == I.LATE_ROWS
    assert I.find_late_winner(pair) == I.LATE_POSITION
    for c, iterations in I.LATE_CASES:
        r = estimate(calls["late_%d" % c])
        assert r["best"] == c and r["counts"][:c].max() < r["counts"][c] == I.LATE_INLIERS and len(r["counts"]) == iterations + 1
        assert r["status"] == M.OK
        cut = estimate(calls["cut_%d" % c])
        assert len(cut["counts"]) == c and cut["best"] < c and 0 < cut["counts"][cut["best"]] < I.LATE_INLIERS and cut["status"] == M.OK
    assert I.LATE_CASES[-1][0] == I.LATE_CASES[-1][1]                   # the very last candidate


def test_the_solver_batch_reaches_every_cell(calls):
    cells, four, none, statuses = np.zeros(8, np.int64), 0, 0, []
    for k, (name, pair) in enumerate(I.solver_pairs().items()):
        assert 4 <= pair["m"] <= 6
        hs, has, solutions = I.hypotheses(pair, CAM, I.SOLVER_KW["seed"], I.SOLVER_KW["iterations"])
        win, n_valid = I.winning_cells(solutions)
        assert ((win >= 0) == has).all()
        cells += np.bincount(win[win >= 0], minlength=8)
        four, none = four + int((n_valid == 4).sum()), none + int((n_valid == 0).sum())
        statuses.append(estimate(calls["solver"], k)["status"])
    assert (cells > 0).all() and four > 0 and none > 0 and M.NO_MODEL in statuses and M.OK in statuses
    pairs = I.solver_pairs()
    P = pairs["collinear"]["from_xyz"]
    assert not np.cross(P[1] - P[0], P[2] - P[0]).any()                 # area2 = 0 exactly
    idx = np.array([[0], [1], [2], [3]])
    assert not M.p3p(P[idx[:3]], M.bearing(CAM, pairs["collinear"]["to_points"][idx[:3]]), P[idx[3]], pairs["collinear"]["to_points"][idx[3]], CAM)[0][0]
    assert (pairs["coincident"]["from_xyz"][0] == pairs["coincident"]["from_xyz"][1]).all()
    assert set((pairs["equidistant"]["from_xyz"][:3] ** 2).sum(axis=1).tolist()) == {17.0}
    assert pairs["principal"]["to_points"][0].tolist() == [I.CX, I.CY]
    assert set(pairs["plane"]["from_xyz"][:, 2].tolist()) == {4.0}
    # behind: every hypothesis whose fourth point is row 3 has no solution, though its triple has some for any other fourth point -- what
    # they lose them to is the fourth point's place behind the camera; every other hypothesis of the pair is valid
    behind = pairs["behind"]
    seed, iterations = I.SOLVER_KW["seed"], I.SOLVER_KW["iterations"]
    hs, has, solutions = I.hypotheses(behind, CAM, seed, iterations)
    draws = np.array([M.draw4(seed, int(h), 4) for h in hs])
    fourth = draws[:, 3] == 3
    ok = np.stack([s[0] for s in solutions])
    assert fourth.sum() >= 3 and not has[fourth].any() and not ok[:, fourth].any() and has[~fourth].all()
    P, UV = behind["from_xyz"], behind["to_points"]
    idx = draws[fourth].T
    again = M.p3p(P[idx[:3]], M.bearing(CAM, UV[idx[:3]]), P[idx[0]], UV[idx[0]], CAM)          # the same triples, one of their own as the fourth
    assert again[0].all()
    for valid, _, _, models in again[2]:                                # and under each of their solutions row 3 lies behind the camera
        Z = (models[:, 8] * P[3, 0] + models[:, 9] * P[3, 1]) + models[:, 10] * P[3, 2] + models[:, 11]
        assert (Z[valid] < 0).all()
    assert np.stack([s[0] for s in again[2]]).any(axis=0).all()
    assert statuses[list(pairs).index("line")] == M.NO_MODEL
    hs, has, solutions = I.hypotheses(pairs["far_keypoint"], CAM, I.SOLVER_KW["seed"], I.SOLVER_KW["iterations"])
    ok, e = np.stack([s[0] for s in solutions]), np.stack([s[2] for s in solutions])
    far = np.array([(ok[:, h].sum() >= 2) and len(set(M.bits(e[ok[:, h], h]).tolist())) == 1 and e[ok[:, h], h][0] > 1e18 for h in range(len(hs))])
    r = estimate(calls["solver"], list(pairs).index("far_keypoint"))
    assert far.any() and r["best"] - 1 in hs[far].tolist() and r["counts"].max() == 5      # the winner is a hypothesis whose solutions tie in their error


def test_shepperd_cases_lanes_late_members_and_the_refused_step(calls):
    for pick, seeds in I.SHEPPERD_SEEDS.items():
        for s in seeds:
            r = estimate(calls["shepperd_%d_%d" % (pick, s)])
            assert r["status"] == M.OK and len(r["picks"]) >= 2 and set(r["picks"]) == {pick}
            R = I.made("shepperd_pair", s)["R"]
            assert np.trace(R) < -0.9
    for local in (False, True):
        call = calls["exact_rotations_%d" % local]
        for k, (R, pick, top) in enumerate(I.EXACT_ROTATIONS):
            r = estimate(call, k)
            model0 = M.model_of_guess(call["guesses"][k], call["cam"].get("local_transform"))
            np.testing.assert_array_equal(model0.reshape(3, 4)[:, :3], np.array(R, np.float32))    # exact in fp32, behind the local transform too
            c = [1 + np.trace(np.array(R))] + [1 + 2 * R[i][i] - np.trace(np.array(R)) for i in range(3)]
            assert max(c) == top and c.index(max(c)) == pick            # the first of the largest
            assert r["best"] == 0 and r["picks"] == [pick] and r["status"] == M.OK and len(r["inliers"]) == 60
    for k, (axis, pick, other) in enumerate(I.TIED_ROTATIONS):
        call = calls["exact_rotations_tied"]
        R = M.model_of_guess(call["guesses"][k], None).reshape(3, 4)[:, :3]
        r = estimate(call, k)
        assert R[pick - 1, pick - 1] == R[other - 1, other - 1] and pick < other
        assert r["picks"] == [pick] and r["best"] == 0 and r["status"] == M.OK and len(r["inliers"]) == 60
        d = R.diagonal()
        pivots = [np.float32(1) + ((d[0] + d[1]) + d[2]), np.float32(1) + ((d[0] - d[1]) - d[2]), np.float32(1) + ((d[1] - d[0]) - d[2]),
                  np.float32(1) + ((d[2] - d[0]) - d[1])]              # as the rule computes them
        assert pivots[pick] == pivots[other] == max(pivots) > 1.9 and sorted(pivots)[1] < 1
    for k, m in enumerate(I.LANE_SIZES):
        r = estimate(calls["lanes"], k)
        assert r["status"] == M.OK and len(r["inliers"]) == m and len(r["trace"]) >= 1 and len(r["picks"]) == len(r["trace"])
    assert I.find_late_members(range(5)) == [(s, d) for s, d in sorted(I.LATE_MEMBERS.items())]
    for s, differing in I.LATE_MEMBERS.items():
        r = estimate(calls["late_members_%d" % s])
        assert r["first_differing"] == differing and min(differing) >= 256 and r["trace"].count("members_changed") == len(differing)
        assert len(r["inliers"]) > 256 and r["status"] == M.OK
    r = estimate(calls["refused"])
    assert r["status"] == M.OK and r["best"] == 0 and len(r["inliers"]) == 6 and len(r["trace"]) == 1
    assert len(r["refused"]) == M.STEPS * len(r["trace"])               # every step of every fit
    np.testing.assert_array_equal(r["transform"], M.IDENTITY)


def test_covariance_ratios_keys_and_cameras(calls):
    for k, n in enumerate(I.RATIO_SIZES):                               # the selection is every correspondence: n of them
        assert len(estimate(calls["ratio_2"], k)["inliers"]) == n
    ks = {(n, ratio): n // ratio for n in I.RATIO_SIZES for ratio in I.RATIOS}
    for n in I.RATIO_SIZES:
        assert {2, 3, n, n + 1, (1 << 31) - 1} <= set(I.RATIOS)
        assert ks[(n, 2)] == n // 2 and ks[(n, n)] == 1 and ks[(n, n + 1)] == 0 and ks[(n, (1 << 31) - 1)] == 0
    r = estimate(calls["negative_cosine"])
    assert r["status"] == M.OK and r["angle_cos"] < 0 and 40 < (r["cosines"] < 0).sum() < 60 and (r["cosines"] > 0).any()
    keys = M.order_key(r["cosines"])
    assert (np.argsort(keys, kind="stable") == np.argsort(r["cosines"], kind="stable")).all()
    r = estimate(calls["nonfinite_to"])
    assert r["status"] == M.OK and r["variance_kind"] == 1 and not np.isfinite(r["T"]).all(axis=1).any() and len(r["inliers"]) == 60
    r = estimate(calls["zero_point"])
    at = r["inlier_index"].index(0)
    assert r["status"] == M.OK and not r["P"][0].any() and r["matches"][0] == I.zero_point_pair()["ids"][0] and r["cosines"][at] == 1.0
    for k, sign in enumerate((1, -1)):                                  # the clamps: every raw cosine is beyond the bound it is clamped to
        r = estimate(calls["clamps"], k)
        raw = I.raw_cosine(r["P"], np.float32(sign) * r["P"])
        assert r["status"] == M.OK and r["best"] == 0 and len(r["inliers"]) == 20 and (sign * raw > 1).all() and (np.abs(raw) < 1.000001).all()
        np.testing.assert_array_equal(r["model"], M.IDENTITY)
        assert (r["cosines"] == sign).all() and r["angle_cos"] == sign
    cams = calls["cameras"]["cam"]
    assert len({tuple(sorted(c.items())) for c in cams}) == len(cams) == 5
    assert [(c["cx"] <= 0, c["cy"] <= 0) for c in cams[:3]] == [(True, True), (True, False), (False, True)]
    assert cams[0]["image_width"] % 2 == 1 and cams[1]["image_height"] % 2 == 1 and cams[3]["fx"] != cams[3]["fy"] and cams[4]["fy"] < 0
    for k in range(5):
        r = estimate(calls["cameras"], k)
        assert r["status"] == M.OK and r["variance_kind"] == 1 and len(r["inliers"]) >= 25
    r = estimate(calls["camera_unsized"])
    fin = np.isfinite(r["T"][r["inlier_index"]]).all(axis=1)
    assert r["status"] == M.OK and fin.any() and (~fin).any() and calls["camera_unsized"]["cam"]["cx"] == 0.0 and "image_width" not in calls["camera_unsized"]["cam"]
    below, above = I.max_variance_bounds()
    lin = estimate(calls["negative_cosine"])["variance_lin"]
    assert np.float64(np.float32(below)) < lin < np.float64(np.float32(above)) and np.nextafter(np.float32(below), np.float32(np.inf)) in (np.float32(above), np.float32(lin))
    assert estimate(calls["max_variance_below"])["status"] == M.VARIANCE_REJECTED and estimate(calls["max_variance_above"])["status"] == M.OK
