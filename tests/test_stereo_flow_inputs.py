"""Proofs, by tests/stereo_flow_model.py, that each input of tests/stereo_flow_inputs.py shows the property it is named for, and that each of
the model's deliberately wrong variants differs from the rule on at least one of them.  No GPU."""
import numpy as np

import stereo_flow_inputs as I
import stereo_flow_model as M


def _traces(c, variant=None):
    levels = M.cached_levels(c["P"], c["pair"], variant)
    out = []
    for pt in c["points"]:
        trace = {}
        result = M.track(levels, c["P"], pt, variant, trace)
        out.append((trace, result))
    return out


def _events(trace, level):
    return [e if isinstance(e, str) else e[0] for e in trace.get(level, [])]


def _right(c, variant=None):
    return I.bits(M.frame(c["pair"], c["points"], c["P"], variant=variant)["right"])


def test_level_counts_and_odd_sizes():
    sizes = []
    for pr, P, want in I.level_count_cases(np.random.default_rng(1)):
        w = pr["width"]
        levels = M.build_pyramid(pr["left"][:, :w], P["win_width"], P["win_height"], P["max_level"])
        assert len(levels) == want
        sizes += [l.shape[::-1] for l in levels]
        nxt = ((levels[-1].shape[1] + 1) // 2, (levels[-1].shape[0] + 1) // 2)
        assert len(levels) == P["max_level"] + 1 or nxt[0] <= P["win_width"] or nxt[1] <= P["win_height"]
    assert (17, 5) in sizes and (9, 5) in sizes and (17, 13) in sizes and (9, 7) in sizes          # odd levels of odd levels
    pr, P, _ = I.level_count_cases(np.random.default_rng(1))[0]
    assert ((17 + 1) // 2, (5 + 1) // 2) == (9, 3) and P["win_height"] == 3                         # 17 x 5: the next level's height EQUALS the window's


def test_window_origins_at_the_bounds_and_one_step_beyond():
    c = I.border_origin_case(np.random.default_rng(2))
    w, h = c["P"]["win_width"], c["P"]["win_height"]
    cols, rows = c["pair"]["width"], c["pair"]["left"].shape[0]
    origins, outside = set(), 0
    for (trace, (_, status, _)), pt in zip(_traces(c), c["points"]):
        ev = trace[0][0]
        if ev == "prev_outside":
            outside += 1
            assert status == 0
        else:
            origins.add(ev[1:])
    assert {o[0] for o in origins} >= {-w, cols - 1} and {o[1] for o in origins} >= {-h, rows - 1}
    assert outside == 4


def test_integer_coordinates_and_ties():
    c = I.integer_case(np.random.default_rng(3))
    for trace, _ in _traces(c):
        assert ("weights", 0.0, 0.0) in trace[0]
    c = I.tie_case(np.random.default_rng(3))
    for trace, _ in _traces(c):
        a = [e for e in trace[0] if e[0] == "weights"][0][1]
        assert a == 2.0 ** -15 and float(np.float32(a) * np.float32(16384)) == 0.5
    assert M.weights(np.float32(2.0 ** -15), np.float32(0))[:2] == (16384, 0)                     # half to even, both ties
    assert M.weights(np.float32(2.0 ** -15), np.float32(0), "half_up")[:2] == (16384, 1)


def test_flat_patch_and_the_eigenvalue_threshold():
    c = I.flat_case(np.random.default_rng(4))
    for trace, (_, status, _) in _traces(c):
        assert "det_fail" in _events(trace, 1) and "det_fail" in _events(trace, 0) and status == 0
    default = dict(c, P=M.params(win_width=5, win_height=3, max_level=1))
    for trace, (_, status, _) in _traces(default):
        assert "eig_fail" in _events(trace, 0) and status == 0
    passes, fails = I.eigen_threshold_cases(np.random.default_rng(4))
    assert M.frame(passes["pair"], passes["points"], passes["P"])["status"].tolist() == [1]
    assert M.frame(fails["pair"], fails["points"], fails["P"])["status"].tolist() == [0]
    assert np.nextafter(passes["P"]["min_eig_threshold"], np.inf) == fails["P"]["min_eig_threshold"]


def test_every_exit_of_the_iteration():
    for name, c in I.exit_cases(np.random.default_rng(5)).items():
        seen = [e for trace, _ in _traces(c) for e in _events(trace, 0)]
        assert seen.count(name) >= 10, (name, seen)


def test_leaving_the_image():
    c = I.leaving_case(np.random.default_rng(6))
    at0 = later = 0
    for trace, (_, status, _) in _traces(c):
        if "next_outside" in _events(trace, 0):
            at0 += 1
            assert status == 0
        above = [l for l in (1, 2, 3) if "next_outside" in _events(trace, l)]
        if above and "origin" in _events(trace, min(above) - 1):
            later += 1                                                   # left at a higher level, and the level below went on
    assert at0 >= 5 and later >= 5


def test_disparity_gate_and_projection_edges():
    cases = I.disparity_gate_cases(np.random.default_rng(7))
    d = cases[0]["d"]
    status = lambda c: M.frame(c["pair"], c["points"], c["P"])["status"].tolist()
    below = np.nextafter(d[0], np.float32(-np.inf))
    assert d[0] != d[1] and below < d[0]
    assert status(cases[0]) == [0, int(d[1] > d[0])]                      # d == min_disparity goes
    assert status(cases[1]) == [1, int(d[1] <= d[0])]                     # d == max_disparity stays
    assert status(cases[2]) == [0, int(d[1] <= below)]                    # one float below: d > max_disparity
    zero, zero_err, back, back_err = (M.frame(c["pair"], c["points"], c["P"]) for c in cases[3:])
    pts = cases[3]["points"]
    assert ((pts[:, 0] - zero["right"][:, 0]) == 0).all() and zero["status"].tolist() == [0, 0]
    assert ((pts[:, 0] - back["right"][:, 0]) < 0).all() and back["status"].tolist() == [0, 0]
    for fr in (zero_err, back_err):                                       # the L1 error keeps the status; the projection refuses d = 0 and d < 0
        assert fr["status"].tolist() == [1, 1] and np.isnan(fr["xyz"]).all()


def test_depth_bounds_right_cx_and_transform():
    cases = I.depth_bound_cases(np.random.default_rng(8))
    zs = []
    for k in range(0, len(cases), 4):
        free, at_min, at_max, between = (M.frame(c["pair"], c["points"], c["P"], M.KEEP_ALL, c["min_depth"], c["max_depth"])["xyz"] for c in cases[k:k + 4])
        assert np.isfinite(free).all()
        assert np.isnan(at_min[0]).all() and np.isfinite(at_max[0]).all() and np.isfinite(between[0]).all()
        zs.append(cases[k]["z"])
        kept = M.frame(cases[k]["pair"], cases[k]["points"], cases[k]["P"], M.FILTER_3D, 0.0, 0.0)["kept"]
        assert kept == [0, 1, 2]
    assert zs[1] > zs[0] * 1.3                                            # without right_cx the disparity is not corrected
    plain, tilted = cases[0], cases[8]
    a = M.frame(plain["pair"], plain["points"], plain["P"])["xyz"]
    b = M.frame(tilted["pair"], tilted["points"], tilted["P"])["xyz"]
    assert np.abs(a - b).max() > 0.1


def test_both_error_modes_and_the_pitch():
    loose, tight, tighter = (M.frame(c["pair"], c["points"], c["P"]) for c in I.error_mode_case(np.random.default_rng(9)))
    c = I.error_mode_case(np.random.default_rng(9))[0]
    eig = M.frame(c["pair"], c["points"], M.params())
    levels = M.cached_levels(c["P"], c["pair"])
    errs = np.array([float(M.track(levels, c["P"], pt)[2]) for pt in c["points"]])
    tracked = np.array([M.track(levels, c["P"], pt)[1] for pt in c["points"]]) == 1
    assert (errs[tracked] < 50).all() and (errs[tracked] >= 0.25).any() and (errs[tracked] < 1.0).any()
    assert (loose["status"] == eig["status"]).all()
    assert (tighter["status"] >= loose["status"]).all()                   # a keypoint whose error is not below the threshold KEEPS its status
    p = I.pitch_case(np.random.default_rng(9))
    assert p["pair"]["left"].shape[1] == p["pair"]["width"] + 7
    tight_pair = M.pair(np.ascontiguousarray(p["pair"]["left"][:, :40]), np.ascontiguousarray(p["pair"]["right"][:, :40]), p["pair"]["camera"])
    np.testing.assert_array_equal(I.bits(M.frame(p["pair"], p["points"], p["P"])["right"]), I.bits(M.frame(tight_pair, p["points"], p["P"])["right"]))


def test_each_wrong_variant_differs_on_a_case():
    rng = lambda: np.random.default_rng(5)
    assert (_right(I.integer_case(rng())) != _right(I.integer_case(rng()), "plain_lk")).any()
    assert (_right(I.tie_case(rng())) != _right(I.tie_case(rng()), "half_up")).any()
    assert (_right(I.border_origin_case(rng())) != _right(I.border_origin_case(rng()), "reflect_deriv")).any()
    inside = I.integer_case(rng())                                        # ... and the border variant only there
    assert (_right(inside) == _right(inside, "reflect_deriv")).all()
