"""What the cases of tests/register_icp_inputs.py rely on, proven with tests/register_icp_model.py: each hand-made case takes the branch of the
rule it is named after.  No device and no library is involved."""
import numpy as np
import pytest

import register_icp_inputs as I
import register_icp_model as M

F = np.float32


@pytest.fixture(scope="module")
def results():
    return {name: M.register(*I.scans(p), force_3dof=p["flat"], **kw) for name, (p, kw) in I.hand_cases().items()}


def test_ties_take_the_lowest_row_and_the_first_of_a_doubled_point(results):
    r = results["ties"]
    assert r["counts"] == [4] and r["match"].tolist() == [0, 2, 4, 5]       # row 0 of (0, 1) at d2 = 1, row 2 of the doubled (2, 3)


def test_the_threshold_is_inclusive_and_decided_by_one_ulp(results):
    at, above = results["d2_at_thr2"], results["d2_above_thr2"]
    assert at["counts"] == [3] and at["status"] == M.OK
    assert above["counts"] == [2] and (above["status"], above["stop"], above["iterations"]) == (M.NOT_CONVERGED, M.STOP_FEW_CORRESPONDENCES, 0)
    assert F(0.5) * F(0.5) == F(0.25) and np.nextafter(F(0.5), F(1)) ** 2 > F(0.25)


def test_two_three_and_later_fewer_correspondences(results):
    assert results["two_correspondences"]["counts"] == [2] and results["two_correspondences"]["status"] == M.NOT_CONVERGED
    assert results["three_correspondences"]["counts"][0] == 3 and results["three_correspondences"]["status"] == M.OK
    r = results["falls_below_three"]
    assert r["counts"] == [3, 2] and (r["status"], r["stop"], r["iterations"]) == (M.NOT_CONVERGED, M.STOP_FEW_CORRESPONDENCES, 1)
    assert (r["match"] == -1).all() and not r["icp_transform"].any()


def test_each_stop_is_taken(results):
    assert (results["stop_iterations"]["stop"], results["stop_iterations"]["iterations"]) == (M.STOP_ITERATIONS, 2)
    assert (results["max_iterations_1"]["stop"], results["max_iterations_1"]["iterations"]) == (M.STOP_ITERATIONS, 1)
    assert results["stop_transform"]["stop"] == M.STOP_TRANSFORM and 1 < results["stop_transform"]["iterations"] < 30
    assert results["stop_mse"]["stop"] == M.STOP_MSE and 1 < results["stop_mse"]["iterations"] < 30


def test_identical_clouds_fit_the_identity_and_stop_on_the_transform_test(results):
    """T_0 of identical clouds is the identity exactly, so with epsilon = 0 the transform test, which comes first, ends the loop; the mse is 0"""
    for name in ("identical_clouds", "identical_clouds_2d"):
        r = results[name]
        assert (r["stop"], r["iterations"]) == (M.STOP_TRANSFORM, 1) and r["mses"] == [F(0)]
        assert np.array_equal(r["icp_transform"], I.IDENTITY) and r["n_correspondences"] == 200 and r["variance"] == 0.0


def test_epsilon_is_decided_by_one_float():
    eps, below, at = I.epsilon_pair(M)
    p, kw = I.hand_cases()["stop_mse"]
    r = M.register(*I.scans(p), force_3dof=True, **dict(kw, epsilon=eps))
    s = M.register(*I.scans(p), force_3dof=True, **dict(kw, epsilon=below))
    assert (r["stop"], r["iterations"]) == (M.STOP_TRANSFORM, at)
    assert s["iterations"] > at or s["stop"] != M.STOP_TRANSFORM


def test_a_and_b_zero_give_a_pure_translation(results):
    r = results["a_b_zero"]
    T = r["models"][0]
    assert T[[0, 1, 4, 5]].tolist() == [1, 0, 0, 1] and T[3] != 0 and T[7] != 0 and T[11] == 0


def test_the_target_is_the_larger_cloud_and_b_on_equal_sizes(results):
    assert [results[n]["from_is_target"] for n in ("swap_less", "swap_equal", "swap_more")] == [False, False, True]
    for n in ("swap_less", "swap_equal", "swap_more"):
        r = results[n]
        kept = r["match"][r["match"] >= 0]
        assert len(kept) == r["n_correspondences"] >= 3 and len(set(kept.tolist())) == len(kept)


def test_the_ratio_gate(results):
    at, above, rel = results["ratio_at_equality"], results["ratio_above"], results["ratio_relative"]
    assert at["ratio"] == F(0.5) and at["status"] == M.BELOW_RATIO and not at["transform"].any() and at["icp_transform"].any() and at["correction"].any()
    assert above["ratio"] == F(0.5) and above["status"] == M.OK and above["transform"].any()
    assert rel["ratio"] == F(5) / F(6) and rel["status"] == M.OK


def test_huge_coordinates_run_through_as_no_neighbour(results):
    r = results["huge_coordinates"]
    assert r["counts"] == [3, 0] and r["status"] == M.NOT_CONVERGED


def test_the_size_batch_holds_every_size_on_both_sides():
    for flat in (True, False):
        batch = I.size_batch(flat)
        assert {p["from_xyz"].shape[0] for p in batch} >= set(I.SIZES) and {p["to_xyz"].shape[0] for p in batch} >= set(I.SIZES)
        for p in batch:
            assert np.isfinite(p["from_xyz"]).all() and np.isfinite(p["to_xyz"]).all()
            assert not flat or (not p["from_xyz"][:, 2].any() and not p["to_xyz"][:, 2].any())


def test_non_finite_rows_are_where_they_are_put():
    p = I.with_non_finite(I.pair(600, 600, False, 7))
    assert np.nonzero(~np.isfinite(p["from_xyz"]).all(axis=1))[0].tolist() == [255, 256, 511]
    assert np.nonzero(~np.isfinite(p["to_xyz"]).all(axis=1))[0].tolist() == [255, 256, 511]
