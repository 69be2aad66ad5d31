"""What tests/register_icp_plane_inputs.py promises about its cases, shown with tests/register_icp_plane_model.py: each hand-made case takes
the branch its name says.  No GPU, no library."""
import numpy as np
import pytest

import register_icp_plane_inputs as I
import register_icp_plane_model as M

F = np.float32
_cache = {}


def run(name):
    if name not in _cache:
        p, kw = I.hand_cases()[name]
        _cache[name] = M.register(*I.scans(p), **kw)
    return _cache[name]


@pytest.mark.parametrize("name", ["plane", "plane_guess_far", "plane_swapped", "plane_3dof", "plane_stop_transform", "plane_max_laser_scans", "plane_noisy_normals"])
def test_room_pairs_take_branch_0_and_converge(name):
    r = run(name)
    assert (r["status"], r["branch"]) == (M.OK, 0) and r["complexity"] > F(0.02) and r["second_eigenvalue"] == F(1)
    assert r["n_correspondences"] >= 100 and (r["match"] >= 0).sum() == r["n_correspondences"]


def test_the_stops_and_the_ratio_gate():
    assert (run("plane_stop_iterations")["stop"], run("plane_stop_iterations")["iterations"]) == (M.STOP_ITERATIONS, 2)
    assert run("plane_stop_transform")["stop"] == M.STOP_TRANSFORM and run("plane_stop_transform")["iterations"] < run("plane")["iterations"]
    r = run("plane_below_ratio")
    assert r["status"] == M.BELOW_RATIO and not r["transform"].any() and r["icp_transform"].any()
    assert run("plane_max_laser_scans")["ratio"] == F(run("plane")["n_correspondences"]) / F(600)
    assert run("plane_swapped")["pca_from"]["oi"] > run("plane_swapped")["pca_to"]["oi"]            # the from-side is step 5's target


def test_force_3dof_is_applied_behind_the_registered_cloud():
    a, b = run("plane"), run("plane_3dof")
    assert a["n_correspondences"] == b["n_correspondences"] and a["variance"] == b["variance"]      # the same registered cloud
    Fm = b["icp_transform"]
    assert Fm[[2, 6, 8, 9, 11]].tolist() == [0, 0, 0, 0, 0] and Fm[10] == 1 and Fm[1] == -Fm[4] and not np.array_equal(a["icp_transform"], Fm)


def test_corridor_normals_have_complexity_0_and_no_vectors():
    for s in (0, 1, 2):
        r = run("corridor_exact_strategy_%d" % s)
        assert r["complexity"] == 0 and r["second_eigenvalue"] == F(1) and r["complexity_values"].tolist() == [0.25, 0, 0]
        assert (r["status"], r["branch"]) == ((M.LOW_COMPLEXITY, 0) if s == 0 else (M.OK, 1))
    r0, r1, r2 = (run("corridor_exact_strategy_%d" % s) for s in (0, 1, 2))
    assert not r0["icp_transform"].any() and r0["variance"] == 1 and (r0["match"] == -1).all() and r0["iterations"] == 0
    # strategy 1 without vectors: vp = 0, the correction keeps its rotation and loses its translation; strategy 2 keeps both
    assert r1["correction"][[3, 7, 11]].tolist() == [0, 0, 0] and np.abs(r2["correction"][[3, 7, 11]]).max() > 1e-3
    np.testing.assert_allclose(r1["correction"].reshape(3, 4)[:, :3], r2["correction"].reshape(3, 4)[:, :3], atol=1e-6)


def test_the_second_value_on_either_side_of_min_complexity():
    above, below, as_is = run("corridor_strategy_1"), run("corridor_second_below"), run("corridor_strategy_2")
    for r in (above, below, as_is):
        assert (r["status"], r["branch"]) == (M.OK, 1) and F(0) < r["complexity"] < F(0.02)
    s = above["second_eigenvalue"]
    assert F(0.02) <= s < F(0.5) and s == min(above["pca_from"]["values"][1], above["pca_to"]["values"][1])
    n1, n2 = above["complexity_vectors"][:3].astype(np.float64), above["complexity_vectors"][3:6].astype(np.float64)
    v = as_is["correction"][[3, 7, 11]].astype(np.float64)
    np.testing.assert_allclose(above["correction"][[3, 7, 11]], n1 * (v @ n1) + n2 * (v @ n2), atol=1e-5)
    np.testing.assert_allclose(below["correction"][[3, 7, 11]], n1 * (v @ n1), atol=1e-5)
    assert np.abs(n2 * (v @ n2)).max() > 1e-4                              # the two projections differ by more than the tolerance
    assert run("corridor_strategy_0")["status"] == M.LOW_COMPLEXITY and run("corridor_strategy_0")["complexity"] == above["complexity"]
    assert (run("corridor_3dof")["status"], run("corridor_3dof")["branch"]) == (M.OK, 1)


def test_parallel_normals_with_min_complexity_0_are_singular():
    r = run("parallel_normals_singular")
    assert (r["status"], r["stop"], r["branch"], r["iterations"]) == (M.NOT_CONVERGED, M.STOP_SINGULAR, 0, 0) and r["counts"][0] >= 100


def test_one_normal_is_no_pca_and_two_are_the_smallest():
    one, two, none = run("one_normal"), run("two_normals"), run("no_normal")
    assert one["pca_from"]["oi"] == 1 and not one["pca_from"]["has"] and not one["complexity_values"].any()
    assert two["pca_from"]["oi"] == 2 and two["pca_from"]["has"] and two["complexity_values"][0] > 0
    assert none["pca_from"]["oi"] == 0
    for r in (one, two, none):                                             # all rows with finite coordinates take part in branch 1
        assert (r["status"], r["branch"]) == (M.OK, 1) and r["n_correspondences"] >= 100
    # the quirk itself: the PCA sees 2 oi rows of which oi are zero -- against NumPy's covariance over those rows
    p, _ = I.hand_cases()["plane"]
    r = run("plane")
    N = p["from_normals"].astype(np.float64)
    w = np.linalg.eigvalsh(np.cov(np.vstack([N, np.zeros_like(N)]).T, bias=True))[::-1]
    np.testing.assert_allclose(r["pca_from"]["values"], w, atol=1e-6)
    assert abs(np.linalg.eigvalsh(np.cov(N.T, bias=True))[0] * 3 - r["pca_from"]["complexity"]) > 0.05


def test_equal_complexities_take_the_to_side():
    r = run("equal_complexities")
    assert r["pca_from"]["complexity"] == r["pca_to"]["complexity"] and r["branch"] == 1
    assert not np.array_equal(r["pca_from"]["vectors"], r["pca_to"]["vectors"])
    np.testing.assert_array_equal(r["complexity_vectors"], r["pca_to"]["vectors"])                  # :539: `<` is false on equality


def test_complexity_and_gate_edges_exist():
    p, kw, c = I.complexity_edge(M)
    assert M.register(*I.scans(p), **dict(kw, min_complexity=float(c)))["branch"] == 0
    assert M.register(*I.scans(p), **dict(kw, min_complexity=float(np.nextafter(c, F(1)))))["branch"] == 1
    p, kw, d = I.gate_edge(M)
    n = [M.register(*I.scans(p), **dict(kw, min_normal_cos=float(v)))["n_correspondences"] for v in (np.nextafter(d, F(-1)), d, np.nextafter(d, F(1)))]
    assert n[0] > n[1] >= n[2]


@pytest.mark.parametrize("name", ["gate_fails_among_the_first", "gate_fails_swapped"])
def test_a_failing_correspondence_among_the_first_changes_the_median(name):
    r = run(name)
    ok, d2 = r["reciprocal_pass"], r["reciprocal_d2"]
    n = r["n_correspondences"]
    assert 0 < (~ok).sum() and n == ok.sum() and not ok[:n].all() and ok[n:].any()
    as_written = np.sort(d2[:n])[n >> 1]
    of_the_passing = np.sort(d2[ok])[n >> 1]
    assert r["variance"] == 2.1981 * np.float64(as_written) and as_written != of_the_passing
    assert (r["match"] >= 0).sum() == n


def test_counts_of_0_1_and_2_take_the_variance_where_there_is_one():
    zero, one, two = run("gate_count_0"), run("gate_count_1"), run("gate_count_2")
    assert (zero["n_correspondences"], one["n_correspondences"], two["n_correspondences"]) == (0, 1, 2)
    assert zero["variance"] == 1 and zero["status"] == M.BELOW_RATIO
    assert one["variance"] == 2.1981 * np.float64(one["reciprocal_d2"][0]) and one["status"] == M.OK
    assert two["variance"] == 2.1981 * np.float64(np.sort(two["reciprocal_d2"][:2])[1])


def test_the_size_batch_reaches_every_status_of_small_pairs():
    rs = [M.register(*I.scans(p), **I.KW) for p in I.size_batch()]
    assert {M.OK, M.EMPTY, M.NOT_CONVERGED} <= {r["status"] for r in rs}
    assert {M.STOP_SINGULAR, M.STOP_FEW_CORRESPONDENCES} <= {r["stop"] for r in rs}
