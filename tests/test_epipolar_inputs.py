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
    """with m = 8 a hypothesis needs seven of eight indices within 32 draws; the trace says how many did not get them: at least one of
    draw_failure()'s hypotheses, and not all of them"""
    p, seed, iterations = I.draw_failure()
    assert iterations <= 60 and M.correspondences(*I.frames(p))[0].shape[0] == 8
    assert M.draw7(seed, I.DRAW_FAILURE_H, 8) is None and M.draw7(seed, 0, 8) is not None and I.DRAW_FAILURE_H < iterations
    r, t = run(p, iterations=iterations, seed=seed)
    assert 0 < t["not_drawn"] < iterations
    assert r["status"] == M.OK


def census_classes(traces):
    """the classes of the census -> {class: number of winners in it}"""
    n = lambda pred: sum(1 for t in traces if pred(t))
    classes = {}
    for r in range(3):
        classes["root %d" % r] = n(lambda t: t["root"] == r)
    for k in (1, 3):
        classes["n_roots %d" % k] = n(lambda t: t["n_roots"] == k)
    for c in range(5):
        classes["chunk %d" % c] = n(lambda t: t["best"] // 256 == c)
    for q in range(4):
        classes["lanes %d..%d" % (64 * q, 64 * q + 63)] = n(lambda t: (t["best"] % 256) // 64 == q)
    for w in range(4):
        classes["scoring wave %d" % w] = n(lambda t: (t["best"] % 256) % 4 == w)
    for s in (False, True):
        classes["lead_negative %s" % s] = n(lambda t: t["lead_negative"] == s)
    classes["disc <= 0"] = n(lambda t: t["clamped"]["disc_nonpos"])
    classes["clamped"] = n(lambda t: t["clamped"]["clamped"])
    return classes


def test_the_census_batch_has_two_winners_in_every_class():
    """Every class of winner the kernel builds differently -- the root's index, one or three real roots, the chunk (the last holds candidates
    1024 and 1025 only), the quarter of the chunk whose lanes made it, the wave that scored it, the sign flip of the returned matrix, a cubic
    without turning points -- is met by two pairs at least.  No winner with a clamped k1 or k2 was found among 20 000 scenes of the recipe
    (B bounds the cubic's roots and, by Gauss-Lucas, its derivative's too; only rounding could clamp), so that class is counted, not required."""
    pairs, iterations, seed = I.census_batch()
    assert len(pairs) <= 64 and 3 * iterations == 4 * 256 + 2
    traces = []
    for p in pairs:
        r, t = run(p, iterations=iterations, seed=seed)
        assert r["status"] == M.OK and t["best"] == t["tied"][0] and t["n_roots"] in (1, 3) and t["root"] < t["n_roots"]
        traces.append(t)
    classes = census_classes(traces)
    print("\n".join("%-20s %d" % kv for kv in classes.items()))
    for name, count in classes.items():
        assert count >= 2 or name == "clamped", (name, count)
    assert sorted(t["best"] for t in traces if t["best"] >= 1024) == [1024, 1024, 1025, 1025]


def test_ties_span_the_chunks_and_both_sides_of_candidate_255():
    """On the three clean pairs every sound hypothesis reaches all m inliers: at 300 iterations at least 50 candidates tie, in all four
    chunks, and the winner is the lowest; at 85 iterations (candidates 0 .. 254) the ties end below candidate 255, at 86 (0 .. 257) they go
    on behind it, in the second chunk.  The noisy pair's best count is reached by candidates of one chunk made by lanes of different waves
    and scored by different waves."""
    pairs, seed = I.tie_pairs()
    for p, m in zip(pairs[:3], (8, 9, 12)):
        r, t = run(p, iterations=300, seed=seed)
        assert r["status"] == M.OK and t["count"] == m
        assert len(t["tied"]) >= 50 and {c // 256 for c in t["tied"]} == {0, 1, 2, 3} and t["best"] == t["tied"][0] == min(t["tied"])
        _, t85 = run(p, iterations=85, seed=seed)
        _, t86 = run(p, iterations=86, seed=seed)
        assert t85["tied"] and max(t85["tied"]) < 255 and t85["best"] == t85["tied"][0]
        assert t86["tied"][:len(t85["tied"])] == t85["tied"] and max(t86["tied"]) > 255 and t86["best"] == t86["tied"][0]
    for iterations in (85, 86, 300):
        _, t = run(pairs[3], iterations=iterations, seed=seed)
        a = t["tied"][0]
        assert t["best"] == a and t["count"] < 40
        assert any(b // 256 == a // 256 and (b % 256) // 64 != (a % 256) // 64 and b % 4 != a % 4 for b in t["tied"][1:]), t["tied"]


SCALE_KW = dict(iterations=60, seed=5)


def scale_row(pair, k):
    r, t = run(I.scaled(pair, k), ransac_threshold=3.0 * 2.0 ** k, **SCALE_KW)
    return r, t


def test_power_of_two_scales_keep_the_inliers_until_the_squares_leave_the_normal_range():
    """scene(3, 100), the threshold scaled alike.  Scaling by a power of two is exact, so the inlier set is that of scale 1 while every
    intermediate is normal: k = -62 .. +55.  From 2^-64 down the distance squares, then thr2, go subnormal and lose bits: the counts change
    (the model keeps subnormals, as IEEE does) and the status stays LCD_EPI_OK down to 2^-70; at 2^-74 nothing is left.  From 2^+60 up the
    sum of the distances overflows.  Table, as derived here (k: status, inliers, subnormal distance squares / thr2 / winner's line error):
       0: OK 16 - - -     -20: OK 16 - - -    -62: OK 16 - - -    +20: OK 16 - - -    +55: OK 16 - - line
     -64: OK 50 dist - -  -66: OK 100 dist thr2 -   -70: OK 98 dist thr2 -   -74: NO_MODEL   +60, +62: NO_MODEL"""
    p = I.scene(3, 100)
    base, t0 = scale_row(p, 0)
    assert base["status"] == M.OK and base["inliers"].shape[0] == 16 and not any(t0["subnormal"].values())
    table = {}
    for k in (-20, -62, -64, -66, -70, -74, 20, 55, 60, 62):
        r, t = scale_row(p, k)
        table[k] = (r["status"], r["inliers"].shape[0], t.get("subnormal"))
        print("k %+3d status %d inliers %3d subnormal %s" % (k, r["status"], r["inliers"].shape[0], t.get("subnormal")))
        if k in (-20, -62, 20, 55):
            assert r["status"] == M.OK and np.array_equal(r["inliers"], base["inliers"])   # (the matrix' entries scale by 2^-2k, 2^-k and 1: not compared)
    assert [table[k][:2] for k in (-64, -66, -70)] == [(M.OK, 50), (M.OK, 100), (M.OK, 98)]
    assert all(table[k][2]["distance"] for k in (-64, -66, -70)) and table[-66][2]["thr2"] and table[-70][2]["thr2"]
    assert [table[k][:2] for k in (-74, 60, 62)] == [(M.NO_MODEL, 0)] * 3
    assert table[55][2]["line"]
    for k in (-66, -70):                                                  # with_m(8), its companion in the GPU test, is accepted under a subnormal thr2 too
        r, t = scale_row(I.with_m(8), k)
        assert r["status"] == M.OK and t["subnormal"]["thr2"]


def test_infinite_keypoints_and_nan_in_unpaired_rows():
    for side in ("from", "to"):
        for sign in (1, -1):
            p = I.inf_keypoint(sign, side)
            assert np.isinf(p[side + "_points"]).sum() == 1 and (p[side + "_points"][np.isinf(p[side + "_points"])] * sign > 0).all()
            r, t = run(p)
            assert r["status"] == M.NO_MODEL and r["matches"].shape[0] == 40 and not r["fundamental"].any() and t == {}
    p, twin = I.nan_unpaired()
    assert np.isnan(p["from_points"]).any(axis=1).sum() == 6 and np.isnan(p["to_points"]).any(axis=1).sum() == 6
    assert np.isfinite(twin["from_points"]).all() and np.isfinite(twin["to_points"]).all()
    r, q = run(p)[0], run(twin)[0]
    assert r["status"] == q["status"] == M.OK and np.array_equal(r["matches"], q["matches"]) and np.array_equal(r["inliers"], q["inliers"])
    assert np.array_equal(M.bits(r["fundamental"]), M.bits(q["fundamental"]))
