"""The host mirror of lcd_register_icp (rtabmap_amd/host/RegistrationIcp.cpp, through c_shim.cpp) against tests/register_icp_model.py bit for
bit on the hand-made cases of every branch of the rule and on batches of every size, the refusals of both entries, what the mirror does
behind the rule (the Euler-angle gate, the covariance), and the fp32 rule against a float64 ICP.  No GPU."""
import numpy as np
import pytest

import register_icp_inputs as I
import register_icp_model as M

F = np.float32
# The largest difference between an entry of out_transform under the fp32 rule and under the float64 ICP of the model (the same loop, a
# kd-tree, an SVD fit) measured on accuracy_pairs() -- 24 pairs of 400 x 380 points, 2-D and 3-D, noise-free and with 1 cm of noise,
# rotations within 0.04 rad and translations within 8 cm -- was 4.50e-7; the bound is that times the margin of 4 the design allows.
ICP64_BOUND = 4 * 4.50e-7


def mirror(p, **kw):
    from rtabmap_amd import vwdictionary as V
    return V.register_icp_cpu(*I.scans(p), **kw)


def assert_same(got, want, what=""):
    """a result of the mirror (or of the engine, cut to the pair) against the model's"""
    for k in ("status", "stop", "iterations", "n_correspondences"):
        assert int(got[k]) == want[k], (what, k, got[k], want[k])
    for k in ("transform", "icp_transform", "correction"):
        np.testing.assert_array_equal(I.bits(got[k]), I.bits(want[k]), err_msg="%s %s" % (what, k))
    assert I.bits(got["ratio"]) == I.bits(want["ratio"]), (what, got["ratio"], want["ratio"])
    assert np.float64(got["variance"]).view(np.uint64) == np.float64(want["variance"]).view(np.uint64), (what, got["variance"], want["variance"])
    np.testing.assert_array_equal(got["match"], want["match"], err_msg=what + " match")


def both(p, **kw):
    want = M.register(*I.scans(p), **kw)
    for search in (M.SEARCH_AUTO, M.SEARCH_BRUTE, M.SEARCH_GRID):
        assert_same(mirror(p, **dict(kw, search=search)), want)
    return want


@pytest.mark.parametrize("name", sorted(I.hand_cases()))
def test_the_mirror_equals_the_model_on_every_hand_made_case(name):
    p, kw = I.hand_cases()[name]
    both(p, force_3dof=p["flat"], **kw)


def test_the_mirror_equals_the_model_where_epsilon_decides():
    eps, below, _ = I.epsilon_pair(M)
    p, kw = I.hand_cases()["stop_mse"]
    a = both(p, force_3dof=True, **dict(kw, epsilon=eps))
    b = both(p, force_3dof=True, **dict(kw, epsilon=below))
    assert (a["stop"], a["iterations"]) != (b["stop"], b["iterations"])


@pytest.mark.parametrize("flat", [True, False])
def test_the_mirror_equals_the_model_at_every_size(flat):
    for p in I.size_batch(flat):
        both(p, force_3dof=flat, **I.KW)


def test_non_finite_rows_take_no_part_on_the_device_entry_and_are_refused_on_the_host_entry():
    p = I.with_non_finite(I.pair(600, 600, False, 7, noise=0.004))
    want = both(p, device_entry=True, **I.KW)
    assert want["status"] == M.OK and (want["match"][[255, 256, 511]] == -1).all() and not np.isin([255, 256, 511], want["match"]).any()
    clean = dict(p, from_xyz=np.delete(p["from_xyz"], [255, 256, 511], axis=0), to_xyz=np.delete(p["to_xyz"], [255, 256, 511], axis=0))
    assert M.register(*I.scans(clean), **I.KW)["n_correspondences"] == want["n_correspondences"]       # they count towards no size either
    assert mirror(p, **I.KW) is None
    with pytest.raises(M.Refused):
        M.register(*I.scans(p), **I.KW)
    all_bad = I.raw(np.full((4, 3), np.nan), p["to_xyz"][:10])
    assert both(all_bad, device_entry=True, **I.KW)["status"] == M.EMPTY


def test_8192_rows_on_both_sides():
    p = I.pair(8192, 8192, False, 41, noise=0.003)
    want = both(p, **dict(I.KW, max_iterations=2))
    assert (want["stop"], want["iterations"]) == (M.STOP_ITERATIONS, 2) and want["n_correspondences"] > 2000


@pytest.mark.parametrize("bad", [dict(max_iterations=0), dict(max_laser_scans=-1), dict(search=3), dict(search=-1),
                                 dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=float("inf")),
                                 dict(max_correspondence_distance=1e200), dict(epsilon=-1.0), dict(epsilon=float("nan")),
                                 dict(correspondence_ratio=1.5), dict(correspondence_ratio=-0.1)])
def test_refused_arguments(bad):
    p = I.pair(20, 20, False, 3)
    assert mirror(p, **dict(I.KW, **bad)) is None
    with pytest.raises(M.Refused):
        M.register(*I.scans(p), **dict(I.KW, **bad))


def test_refused_sizes_and_guesses():
    big = I.raw(np.zeros((8193, 3)), np.zeros((3, 3)))
    assert mirror(big, **I.KW) is None and mirror(I.raw(big["to_xyz"], big["from_xyz"]), **I.KW) is None
    p = I.pair(20, 20, False, 3)
    assert mirror(dict(p, guess=np.full(12, np.nan, np.float32)), **I.KW) is None


def test_the_host_side_gates_and_the_covariance():
    """RegistrationIcp.cpp:856-961 behind the rule: Euler angles and translation of out_correction against Icp/MaxRotation / MaxTranslation,
    variance / 10, the covariance eye x variance with the rotation block / 10"""
    from rtabmap_amd import vwdictionary as V
    p = I.pair(300, 280, False, 31, guess_off=True)
    r = mirror(p, **I.KW)
    t, info = V.register_icp_finish(r, max_translation=0.2, max_rotation=0.78, correspondence_ratio=0.1)
    c = r["correction"].astype(np.float64)
    angles = [np.arctan2(c[9], c[10]), np.arcsin(-c[8]), np.arctan2(c[4], c[0])]
    assert info["icp_translation"] == pytest.approx(np.abs(c[[3, 7, 11]]).max(), rel=1e-6)
    assert info["icp_rotation"] == pytest.approx(np.abs(angles).max(), rel=1e-5)
    np.testing.assert_array_equal(t, r["transform"])
    v = r["variance"] / 10.0
    np.testing.assert_array_equal(info["covariance"], np.diag([v, v, v, v / 10.0, v / 10.0, v / 10.0]))
    assert info["icp_correspondences"] == r["n_correspondences"] and info["icp_inliers_ratio"] == r["ratio"]
    # the gates: a limit just below what the correction is refuses, 0 switches a gate off
    t, info = V.register_icp_finish(r, max_translation=float(info["icp_translation"]) * 0.99, max_rotation=0.0)
    assert t is None and info["icp_correspondences"] == 0 and np.array_equal(info["covariance"], np.eye(6))
    t, _ = V.register_icp_finish(r, max_translation=0.0, max_rotation=float(info["icp_rotation"]) * 0.99)
    assert t is None
    t, _ = V.register_icp_finish(r, max_translation=0.0, max_rotation=0.0)
    assert t is not None
    # below the ratio: the information is filled, the transform is not
    low, kw = I.hand_cases()["ratio_at_equality"]
    t, info = V.register_icp_finish(mirror(low, **kw), correspondence_ratio=0.5)
    assert t is None and info["icp_correspondences"] == 5 and info["icp_inliers_ratio"] == F(0.5)
    # not converged: nothing
    few, kw = I.hand_cases()["two_correspondences"]
    t, info = V.register_icp_finish(mirror(few, **kw))
    assert t is None and info["icp_correspondences"] == 0 and np.array_equal(info["covariance"], np.eye(6))


@pytest.mark.parametrize("name", sorted(I.grid_edge_pairs()))
def test_the_grid_form_equals_the_model_at_its_edges(name):
    """every target in one cell, targets on cell faces and corners, a nearest target in a diagonal neighbour cell, equal distances across two
    cells, a flat scan and one with a point off the plane, and coordinates beyond the key's cell range on either side (the brute form inside
    a GRID call): the model is brute force, the mirror runs under AUTO (brute at these sizes), BRUTE and GRID"""
    p = I.grid_edge_pairs()[name]
    for flat in (False, True):
        want = both(p, force_3dof=flat, **I.GRID_KW)
        assert want["n_correspondences"] >= 3


def test_equal_distances_across_two_cells_go_to_the_lower_row():
    p = I.grid_edge_pairs()["equal_across_cells"]
    from rtabmap_amd import vwdictionary as V
    got = V.register_icp_cpu(*I.scans(p), search=M.SEARCH_GRID, **dict(I.GRID_KW, max_iterations=1, max_correspondence_distance=0.125))
    want = M.register(*I.scans(p), **dict(I.GRID_KW, max_iterations=1, max_correspondence_distance=0.125))
    assert_same(got, want)
    cells, h = V.register_icp_cells(p["to_xyz"][:, 0], I.GRID_THR)
    assert h == F(0.265625) and cells[0] != cells[1]                       # the two candidates of row 0 lie in different cells
    d = p["from_xyz"][0] - p["to_xyz"][:2]
    assert (d * d).sum(axis=1).tolist() == [0.015625, 0.015625]             # at the same d2, exactly


def test_no_pair_within_the_threshold_sits_more_than_one_cell_apart():
    """the cell function against brute force, in the fp32 arithmetic the search uses: coordinates at and a few ulps around cell edges from
    -65 534 to 65 534 cells, -0.0 and +0.0 among them, each against partners at and a few ulps around the threshold to either side; every
    pair whose double(d2) <= thr2 must lie in the same or in neighbouring cells, and a partner one cell size away may not (the margin is
    not vacuous)"""
    from rtabmap_amd import vwdictionary as V
    for thr in (0.25, 0.3, 0.1, 0.05, 1.0, 7.3e-4, 123.456):
        h = F(F(thr) * F(1.0625))
        ks = np.concatenate([np.arange(-40, 41), [-65534, -65533, -30000, -1025, 1023, 4097, 30001, 65533, 65534]]).astype(np.float32)
        edge = ks * h
        base = np.concatenate([edge] + [np.nextafter(edge, s * np.float32(np.inf)) for s in (-1, 1)] +
                              [edge + s * np.float32(thr) * np.float32(f) for s in (-1, 1) for f in (0.25, 0.5, 0.999)] + [np.array([0.0, -0.0], np.float32)])
        t = np.float32(thr)
        steps = [t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(9e9)), t * np.float32(0.999999), t * np.float32(1.000001), t * np.float32(0.5)]
        steps = np.array([s * sign for s in steps for sign in (1, -1)], np.float32)
        p = np.repeat(base, len(steps))
        q = (p + np.tile(steps, len(base))).astype(np.float32)
        dx = p - q
        d2 = (dx * dx + np.float32(0)) + np.float32(0)
        near = d2.astype(np.float64) <= np.float64(thr) * np.float64(thr)
        cp, hh = V.register_icp_cells(p, thr)
        cq, _ = V.register_icp_cells(q, thr)
        assert hh == h
        ok = (cp > -2 ** 31) & (cq > -2 ** 31)
        assert near.sum() > 300 and (near & ok).sum() > 300
        assert (np.abs(cp - cq)[near & ok] <= 1).all(), thr
        assert np.abs(cp - cq)[ok].max() == 1 and (cp[ok] != cq[ok]).any()
        far = (p + h * np.float32(2.01)).astype(np.float32)
        cf, _ = V.register_icp_cells(far, thr)
        assert (np.abs(cf - cp)[(cf > -2 ** 31) & ok & (np.abs(ks).max() > 0)] >= 2).all()
        out, _ = V.register_icp_cells(np.array([65535.5 * h, -65536 * h, np.inf, np.nan], np.float32), thr)
        assert (out == -2 ** 31).all()


def test_auto_is_the_grid_from_the_measured_size_on():
    """AUTO and GRID agree with BRUTE on either side of the threshold (the forms cannot be told apart by results: that is the point)"""
    for n in (1023, 1024, 1025):
        p = I.pair(n, n, True, 900 + n, noise=0.004)
        both(p, force_3dof=True, **dict(I.KW, max_iterations=3))


def accuracy_pairs():
    return [I.pair(400, 380, flat, 500 + seed, noise=noise) for flat in (True, False) for noise in (0.0, 0.01) for seed in range(6)]


def test_the_fp32_rule_against_a_float64_icp():
    """an accuracy check, not a parity claim: the same loop in float64 with a kd-tree and an SVD fit, written independently"""
    worst = 0.0
    for p in accuracy_pairs():
        got = mirror(p, force_3dof=p["flat"], **I.KW)
        ref, _ = M.icp64(*I.scans(p), max_iterations=I.KW["max_iterations"], force_3dof=p["flat"], max_correspondence_distance=I.KW["max_correspondence_distance"])
        assert got["status"] == M.OK and ref is not None
        worst = max(worst, np.abs(got["transform"].reshape(3, 4).astype(np.float64) - ref).max())
    print("largest difference to the float64 ICP: %.3g" % worst)
    assert worst <= ICP64_BOUND
