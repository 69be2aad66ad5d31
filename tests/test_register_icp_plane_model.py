"""The host mirror of lcd_register_icp_plane (rtabmap_amd/host/RegistrationIcp.cpp, through c_shim.cpp) against
tests/register_icp_plane_model.py bit for bit on every hand-made case, size and block, batch and region edge under all three search values,
the refusals, what the mirror
does behind the rule, the sweep count, and the fp32 rule against an independent point-to-plane ICP.  No GPU."""
import numpy as np
import pytest

import register_icp_plane_inputs as I
import register_icp_plane_model as M
from register_icp_plane_device import model_of

F = np.float32
INTS = ("status", "stop", "iterations", "n_correspondences", "branch")
FLOATS = ("transform", "icp_transform", "correction", "ratio", "complexity", "complexity_values", "complexity_vectors", "second_eigenvalue")
# The reference's own fp32 noise: the largest entry difference between icp_plane64 (PCL's uncentred normal equations, numpy.linalg.solve,
# Rz Ry Rx, a kd-tree) run in float32 and in float64 over accuracy_pairs() was 1.23e-6 (test_the_fp32_rule_against_a_float64_icp prints
# it and asserts that it has not moved); the rule's largest difference to the float64 run was 7.68e-7.  The bound is the former times 4.
ICP64_FP32_NOISE = 1.23e-6
ICP64_BOUND = 4 * ICP64_FP32_NOISE


def mirror(p, **kw):
    from rtabmap_amd import vwdictionary as V
    return V.register_icp_plane_cpu(*I.scans(p), **kw)


def assert_same(got, want, what=""):
    assert got is not None, what
    for k in INTS:
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    for k in FLOATS:
        np.testing.assert_array_equal(I.bits(got[k]).reshape(-1), I.bits(want[k]).reshape(-1), err_msg="%s %s" % (what, k))
    assert np.float64(got["variance"]).view(np.uint64) == np.float64(want["variance"]).view(np.uint64), (what, got["variance"], want["variance"])
    np.testing.assert_array_equal(got["match"], want["match"], err_msg=what + " match")


def both(p, **kw):
    want = M.register(*I.scans(p), **kw)
    for search in (M.SEARCH_AUTO, M.SEARCH_BRUTE, M.SEARCH_GRID):
        assert_same(mirror(p, **dict(kw, search=search)), want, "search %d" % search)
    return want


@pytest.mark.parametrize("name", sorted(I.hand_cases()))
def test_the_mirror_equals_the_model_on_every_hand_made_case(name):
    p, kw = I.hand_cases()[name]
    both(p, **kw)


def test_the_mirror_equals_the_model_at_every_size():
    for p in I.size_batch():
        both(p, **I.KW)


def test_the_mirror_equals_the_model_at_the_edges():
    p, kw, c = I.complexity_edge(M)
    assert both(p, **dict(kw, min_complexity=float(c)))["branch"] == 0
    assert both(p, **dict(kw, min_complexity=float(np.nextafter(c, F(1)))))["branch"] == 1
    p, kw, d = I.gate_edge(M)
    for v in (np.nextafter(d, F(-1)), d, np.nextafter(d, F(1))):
        both(p, **dict(kw, min_normal_cos=float(v)))


def test_normals_and_coordinates_that_are_not_finite():
    p = I.with_nan_normals(I.pair(600, 600, 7, noise=0.004))
    want = both(p, **I.KW)                                                 # legal on the host entry
    assert (want["status"], want["branch"]) == (M.OK, 0) and (want["match"][[255, 256, 511]] == -1).all() and not np.isin([255, 256, 511], want["match"]).any()
    assert want["ratio"] == F(want["n_correspondences"]) / F(600)          # the denominator still counts them
    q = I.changed(p)
    q["from_xyz"][300, 1] = np.inf
    assert mirror(q, **I.KW) is None
    with pytest.raises(M.Refused):
        M.register(*I.scans(q), **I.KW)
    want = both(q, device_entry=True, **I.KW)
    assert want["match"][300] == -1 and want["ratio"] == F(want["n_correspondences"]) / F(600)


def test_8192_rows_on_both_sides():
    p = I.pair(8192, 8192, 41, noise=0.003)
    want = both(p, **dict(I.KW, max_iterations=2))
    assert (want["stop"], want["iterations"], want["branch"]) == (M.STOP_ITERATIONS, 2, 0) and want["n_correspondences"] > 2000


@pytest.mark.parametrize("bad", [dict(max_iterations=0), dict(max_laser_scans=-1), dict(search=3), dict(max_correspondence_distance=0.0),
                                 dict(max_correspondence_distance=1e200), dict(epsilon=float("nan")), dict(correspondence_ratio=1.5),
                                 dict(min_complexity=-0.1), dict(min_complexity=1.5), dict(min_complexity=float("nan")), dict(low_complexity_strategy=3),
                                 dict(low_complexity_strategy=-1), dict(normal_gate=True, min_normal_cos=float("nan")),
                                 dict(normal_gate=True, min_normal_cos=float("inf"))])
def test_refused_arguments(bad):
    p = I.pair(20, 20, 3)
    assert mirror(p, **dict(I.KW, **bad)) is None
    with pytest.raises(M.Refused):
        M.register(*I.scans(p), **dict(I.KW, **bad))


def test_a_cosine_that_is_not_finite_is_legal_while_the_gate_is_off():
    p = I.pair(40, 40, 3)
    both(p, min_normal_cos=float("nan"), **I.KW)
    big = I.raw(np.zeros((8193, 3)), np.zeros((8193, 3)), np.zeros((3, 3)), np.zeros((3, 3)))
    assert mirror(big, **I.KW) is None
    assert mirror(dict(p, guess=np.full(12, np.nan, np.float32)), **I.KW) is None


def test_the_host_side_gates():
    """RegistrationIcp.cpp:856-961 behind the rule, as for the point-to-point call: the result of the plane rule goes through the same finish()"""
    from rtabmap_amd import vwdictionary as V
    p, kw = I.hand_cases()["plane_guess_far"]
    r = mirror(p, **kw)
    t, info = V.register_icp_finish(r, max_translation=0.2, max_rotation=0.78, correspondence_ratio=0.1)
    np.testing.assert_array_equal(t, r["transform"])
    v = r["variance"] / 10.0
    np.testing.assert_array_equal(info["covariance"], np.diag([v, v, v, v / 10.0, v / 10.0, v / 10.0]))
    assert info["icp_correspondences"] == r["n_correspondences"]
    t, _ = V.register_icp_finish(r, max_translation=float(info["icp_translation"]) * 0.99, max_rotation=0.0)
    assert t is None
    for name in ("corridor_strategy_0", "parallel_normals_singular"):      # LCD_ICP_LOW_COMPLEXITY and LCD_ICP_STOP_SINGULAR: no transform
        q, kw = I.hand_cases()[name]
        t, info = V.register_icp_finish(mirror(q, **kw))
        assert t is None and info["icp_correspondences"] == 0 and np.array_equal(info["covariance"], np.eye(6))


def test_two_more_sweeps_change_no_bit_of_the_eigenvalues():
    """the sweep count of the 3 x 3 Jacobi (csrc/icp_plane_rule.h argues it): 5, 6 and 7 sweeps give the same values and complexity"""
    pairs = [p for p, _ in I.hand_cases().values()] + I.size_batch()[8:]
    seen = 0
    for p in pairs:
        for N in (p["from_normals"], M.rotate(p["guess"], p["to_normals"])):
            fin = np.isfinite(N).all(axis=1)
            a, b, c = (M.pca(N, fin, sweeps=s) for s in (M.SWEEPS, M.SWEEPS + 1, M.SWEEPS + 2))
            if not a["has"]:
                continue
            seen += 1
            for other in (b, c):
                np.testing.assert_array_equal(I.bits(a["values"]), I.bits(other["values"]))
    assert seen >= 40


def accuracy_pairs():
    """3-D room pairs in the ranges of the point-to-point accuracy check: 400 x 380 points, noise-free and with 1 cm of noise, rotations within
    0.04 rad, translations within 8 cm"""
    return [I.pair(400, 380, 500 + seed, noise=noise) for noise in (0.0, 0.01) for seed in range(6)]


def test_the_fp32_rule_against_a_float64_icp():
    """an accuracy check, not a parity claim.  The bound is four times the reference's own fp32 noise, measured here: icp_plane64 in float32
    against itself in float64 on the same pairs."""
    kw = dict(max_iterations=I.KW["max_iterations"], max_correspondence_distance=I.KW["max_correspondence_distance"])
    worst = noise = 0.0
    for p in accuracy_pairs():
        got = mirror(p, **I.KW)
        ref, _ = M.icp_plane64(p["from_xyz"], p["to_xyz"], p["to_normals"], p["guess"], **kw)
        ref32, _ = M.icp_plane64(p["from_xyz"], p["to_xyz"], p["to_normals"], p["guess"], dtype=np.float32, **kw)
        assert (got["status"], got["branch"]) == (M.OK, 0) and ref is not None and ref32 is not None
        worst = max(worst, np.abs(got["transform"].reshape(3, 4).astype(np.float64) - ref).max())
        noise = max(noise, np.abs(ref32.astype(np.float64) - ref).max())
    print("largest difference to the float64 ICP: rule %.3g, the same ICP in float32 %.3g" % (worst, noise))
    assert noise <= ICP64_FP32_NOISE * 1.0001, "the measured fp32 noise of the reference moved: the bound is stated for %.3g" % ICP64_FP32_NOISE
    assert worst <= ICP64_BOUND


# ---- the cases of the block, batch and region edges (tests/register_icp_plane_inputs.py; tests/test_register_icp_plane_inputs.py proves what
# each of them does): the mirror under all three search values against the model, whose results the two modules share

def cached(p, **kw):
    want = model_of(p, **kw)
    for search in (M.SEARCH_AUTO, M.SEARCH_BRUTE, M.SEARCH_GRID):
        assert_same(mirror(p, **dict(kw, search=search)), want, "search %d" % search)
    return want


@pytest.mark.parametrize("name", sorted(I.low_complexity_sizes()))
def test_the_mirror_equals_the_model_in_the_low_complexity_branch_at_every_block_edge(name):
    pairs, kw = I.low_complexity_sizes()[name]
    assert all(cached(p, **kw)["branch"] == 1 for p in pairs)


def test_the_mirror_equals_the_model_under_the_gate_at_every_block_edge():
    pairs, kw = I.gate_sizes()
    for p in pairs:
        want = cached(p, **kw)
        assert 0 < want["n_correspondences"] < len(want["reciprocal_pass"])


def test_the_mirror_takes_the_source_side_from_the_rows_that_take_part():
    pairs, kw = I.swap_turned_by_normals()
    for p in pairs:
        want = cached(p, **kw)
        assert want["from_is_target"] == (p["from_xyz"].shape[0] < p["to_xyz"].shape[0])


def test_the_mirror_equals_the_model_on_the_mixed_batches():
    for strategy, (pairs, kw) in I.mixed_batch().items():
        assert [(r["branch"], r["status"]) for r in (cached(p, **kw) for p in pairs)] == I.MIXED[strategy]


def test_the_mirror_skips_the_padding_of_a_region_and_the_host_rule_refuses_it():
    for region, pads, plain, kw in I.padded_regions():
        for a, b in zip(pads, plain):
            want = cached(a, device_entry=True, **kw)
            assert (want["match"][b["from_xyz"].shape[0]:] == -1).all()
            assert mirror(a, **kw) is None
            cached(b, **kw)


def test_the_mirror_skips_coordinates_that_are_not_finite_at_600_and_1100_rows():
    for p in I.non_finite_coordinates():
        assert cached(p, device_entry=True, **I.KW)["status"] == M.OK
        assert mirror(p, **I.KW) is None


@pytest.mark.parametrize("name", sorted(I.grid_edge_pairs()))
def test_the_grid_form_equals_the_model_at_its_edges_with_normals(name):
    p = I.grid_edge_pairs()[name]
    assert cached(p, **I.GRID_EDGE_KW)["branch"] == 0 and cached(p, **I.GRID_EDGE_ONCE_KW)["branch"] == 0


def test_the_mirror_equals_the_model_at_8192_rows_in_branch_1_and_under_the_gate():
    low, gate, between, kw = I.rows_8192()
    assert cached(low, **kw)["branch"] == 1
    want = cached(gate, **kw)
    assert 0 < want["n_correspondences"] < len(want["reciprocal_pass"])
    cached(between, **kw)


def test_the_mirror_equals_the_model_behind_the_filter():
    import scan_filter_model as SM
    p, kw, region = I.filter_chain()
    f = SM.filter_scans([p["from_xyz"], p["to_xyz"]], [region, region], device_entry=True, **kw)
    q = I.raw(f["xyz"][:region], f["normals"][:region], f["xyz"][region:], f["normals"][region:], p["guess"])
    assert cached(q, device_entry=True, **dict(I.KW, max_iterations=3))["status"] == M.OK
