"""What tests/register_icp_plane_inputs.py promises about its cases, shown with tests/register_icp_plane_model.py: each hand-made case takes
the branch its name says, and each case of the block, batch and region edges the branch, swap side, search form or failure pattern it is
named for.  No GPU, no library."""
import numpy as np
import pytest

import register_icp_plane_inputs as I
import register_icp_plane_model as M
from register_icp_plane_device import model_of

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


# ---- the branches at block, batch and region edges: each case takes the branch, swap side, search form or failure pattern it is named for

def test_the_low_complexity_sizes_complete_a_registration_in_branch_1():
    sets = I.low_complexity_sizes()
    pairs, kw = sets["strategy_1"]
    assert sorted(p["from_xyz"].shape[0] for p in pairs[0::2]) == sorted(I.EDGE_SIZES) == sorted(p["to_xyz"].shape[0] for p in pairs[1::2])
    for p in pairs:
        assert abs(p["from_xyz"].shape[0] - p["to_xyz"].shape[0]) == 20
        r = model_of(p, **kw)
        assert (r["branch"], r["status"]) == (1, M.OK) and F(0) < r["complexity"] < F(kw["min_complexity"])
        assert r["second_eigenvalue"] >= F(kw["min_complexity"]) and r["n_correspondences"] >= 100
    for name in ("second_below", "strategy_2", "force_3dof"):
        assert sets[name][0] is pairs
        for p in pairs:
            r = model_of(p, **sets[name][1])
            assert (r["branch"], r["status"]) == (1, M.OK) and r["n_correspondences"] >= 90 and r["complexity"] > F(0)
            assert (r["second_eigenvalue"] >= F(sets[name][1]["min_complexity"])) == (name != "second_below")
    # the three variants do something else than strategy 1 does
    for p in pairs[:2]:
        a = model_of(p, **kw)
        for name in ("second_below", "strategy_2", "force_3dof"):
            assert not np.array_equal(a["icp_transform"], model_of(p, **sets[name][1])["icp_transform"]), name
    (flat,), kw = sets["exact_zero"]
    r = model_of(flat, **kw)
    assert (flat["from_xyz"].shape[0], flat["to_xyz"].shape[0]) == (513, 493)
    assert (r["branch"], r["status"], r["complexity"], r["second_eigenvalue"]) == (1, M.OK, 0, 1) and r["n_correspondences"] >= 100


def test_the_gate_sizes_fail_in_the_first_trip_in_a_later_one_and_among_the_first():
    pairs, kw = I.gate_sizes()
    sides = set()
    for p in pairs:
        r = model_of(p, **kw)
        ok, rows, n = r["reciprocal_pass"], r["reciprocal_rows"], r["n_correspondences"]
        n_source = p["to_xyz" if r["from_is_target"] else "from_xyz"].shape[0]
        assert (r["branch"], r["status"]) == (0, M.OK) and r["from_is_target"] == (p["from_xyz"].shape[0] > p["to_xyz"].shape[0])
        assert 0 < ok.sum() < len(ok) and n == ok.sum()
        assert (rows[~ok] < 256).any() and ((rows[~ok] >= 512).any() or n_source <= 512)
        assert not ok[:n].all() and ok[n:].any()                          # a failing one among the first `count`, a passing one behind them
        if n_source > 256:                                                # a failing correspondence in a later trip than a passing one
            assert rows[~ok].max() >= 256 and rows[ok].min() < 256
        sides.add((bool(r["from_is_target"]), n_source > 512))
    assert sides == {(True, False), (False, False), (True, True), (False, True)}


def test_non_finite_normals_turn_the_source_side():
    pairs, kw = I.swap_turned_by_normals()
    for p, raw_says in zip(pairs, (True, False)):
        nf, nt = p["from_xyz"].shape[0], p["to_xyz"].shape[0]
        part = [int(np.isfinite(p[k]).all(axis=1).sum()) for k in ("from_normals", "to_normals")]
        assert (nf > nt) == raw_says and sorted(part) == [225, 280] and max(nf, nt) == 300
        r = model_of(p, **kw)
        other = model_of(p, source_is_to=raw_says, **kw)
        assert (r["branch"], r["status"]) == (0, M.OK) and r["from_is_target"] == (part[0] > part[1]) == (not raw_says)
        # what the other decision would change: reciprocity and the cosine are symmetric, so neither the matches nor their number -- the median
        # over the first `count` in the other side's row order is another
        np.testing.assert_array_equal(r["match"], other["match"])
        assert r["n_correspondences"] == other["n_correspondences"] and not r["reciprocal_pass"][:r["n_correspondences"]].all()
        assert np.float64(r["variance"]).view(np.uint64) != np.float64(other["variance"]).view(np.uint64)
        assert I.bits(r["ratio"]) == I.bits(F(r["n_correspondences"]) / F(300))


def test_the_mixed_batches_hold_what_their_docstring_lists():
    batches = I.mixed_batch()
    assert batches[0][0] is batches[1][0]
    for strategy, (pairs, kw) in batches.items():
        assert kw["low_complexity_strategy"] == strategy
        got = [(model_of(p, **kw)["branch"], model_of(p, **kw)["status"]) for p in pairs]
        assert got == I.MIXED[strategy]
    assert set(I.MIXED[0]) == {(0, M.OK), (0, M.LOW_COMPLEXITY), (0, M.BELOW_RATIO), (0, M.NOT_CONVERGED)}
    assert set(I.MIXED[1]) == {(b, s) for b in (0, 1) for s in (M.OK, M.BELOW_RATIO, M.NOT_CONVERGED)} | {(1, M.EMPTY)}
    rows = [max(p["from_xyz"].shape[0], p["to_xyz"].shape[0]) for p in batches[0][0]]
    assert rows.index(max(rows)) == 4 and [p["from_xyz"].shape[0] for p in batches[0][0][:3]] == [513, 400, 0]
    stops = {model_of(p, **batches[1][1])["stop"] for p in batches[1][0]}
    assert M.STOP_FEW_CORRESPONDENCES in stops


def test_the_padding_of_a_region_takes_part_in_nothing():
    forms = set()
    for region, pads, plain, kw in I.padded_regions():
        for a, b in zip(pads, plain):
            nf, nt = b["from_xyz"].shape[0], b["to_xyz"].shape[0]
            assert a["from_xyz"].shape == a["to_normals"].shape == (region, 3) and nf < region and nt < region
            for k, n in (("from_xyz", nf), ("from_normals", nf), ("to_xyz", nt), ("to_normals", nt)):
                assert np.isnan(a[k][n:]).all() and np.array_equal(a[k][:n], b[k])
            ra, rb = model_of(a, device_entry=True, **kw), model_of(b, **kw)
            for k in ("status", "stop", "iterations", "n_correspondences", "branch"):
                assert ra[k] == rb[k], k
            for k in ("transform", "icp_transform", "correction", "ratio", "complexity", "complexity_values", "complexity_vectors", "second_eigenvalue"):
                np.testing.assert_array_equal(I.bits(ra[k]), I.bits(rb[k]), err_msg=k)
            assert np.float64(ra["variance"]).view(np.uint64) == np.float64(rb["variance"]).view(np.uint64)
            assert np.array_equal(ra["match"][:nf], rb["match"]) and (ra["match"][nf:] == -1).all()
            assert (ra["branch"], ra["status"]) == (0, M.OK) and ra["n_correspondences"] >= 100
            with pytest.raises(M.Refused):
                M.register(*I.scans(a), **kw)
            forms.add((region, nf >= 1024, nt >= 1024))                   # which of the two searched sides AUTO takes in the grid form
    assert forms == {(1024, False, False), (2048, True, True), (2048, False, True)}


def test_the_grid_edges_take_branch_0_with_their_normals():
    import register_icp_inputs as I0
    cases = I.grid_edge_pairs()
    assert set(cases) == {k for k, p in I0.grid_edge_pairs().items() if not p["flat"]} | {"diagonal_neighbour_singular"}
    for name, p in cases.items():
        for k in ("from_normals", "to_normals"):
            np.testing.assert_allclose(np.linalg.norm(p[k].astype(np.float64), axis=1), 1.0, atol=1e-6)
            assert len(np.unique(p[k], axis=0)) == p[k].shape[0]           # no two rows share a normal
        r = model_of(p, **I.GRID_EDGE_KW)
        assert r["branch"] == 0 and r["counts"][0] >= 3, name
        # four correspondences do not hold the plane fit's six unknowns: those two pairs end in STOP_SINGULAR, after a first search (and, for
        # equal_across_cells, a first fit) that the counts still show.  The three copies of diagonal_neighbour complete two fits; then their
        # arbitrary normals have carried the twelve rows out of reach.  The others complete every iteration.
        singular = name in ("diagonal_neighbour_singular", "equal_across_cells")
        assert (r["stop"] == M.STOP_SINGULAR) == singular, name
        if name == "diagonal_neighbour":
            assert (r["stop"], r["iterations"], r["counts"][0]) == (M.STOP_FEW_CORRESPONDENCES, 2, 12)
        elif not singular:
            assert (r["status"], r["iterations"]) == (M.OK, I.GRID_EDGE_KW["max_iterations"]), name
        # with one iteration every pair that is not singular at once hands its first fit -- the normals of the rows the first search found -- over
        # to the outputs
        once = model_of(p, **I.GRID_EDGE_ONCE_KW)
        assert once["branch"] == 0 and (once["stop"] == M.STOP_SINGULAR) == (name == "diagonal_neighbour_singular"), name
        if name != "diagonal_neighbour_singular":
            assert (once["stop"], once["iterations"]) == (M.STOP_ITERATIONS, 1) and once["icp_transform"].any(), name
    assert model_of(cases["faces_and_corners"], **I.GRID_EDGE_KW)["iterations"] >= 1
    assert model_of(cases["diagonal_neighbour"], **I.GRID_EDGE_KW)["iterations"] >= 1
    assert model_of(cases["equal_across_cells"], **I.GRID_EDGE_KW)["iterations"] == 1
    # the three copies of diagonal_neighbour keep what it is named for: a from-row whose nearest target lies in a cell that differs along all three axes
    p = cases["diagonal_neighbour"]
    row, _ = M.nearest(p["from_xyz"], np.ones(12, bool), p["to_xyz"], np.ones(15, bool))
    cells = lambda x: np.floor(x.astype(np.float64) / I.GRID_CELL)
    diagonal = (cells(p["from_xyz"]) != cells(p["to_xyz"][row])).all(axis=1)
    assert diagonal.sum() >= 3 and {int(i) // 4 for i in np.flatnonzero(diagonal)} == {0, 1, 2}


def test_non_finite_coordinates_at_600_and_1100_rows():
    a, b, few = I.non_finite_coordinates()
    for p, n in ((a, 600), (b, 1100)):
        r = model_of(p, device_entry=True, **I.KW)
        assert (r["branch"], r["status"]) == (0, M.OK) and (r["match"][[255, 256, 511]] == -1).all() and not np.isin([255, 511], r["match"]).any()
        assert I.bits(r["ratio"]) == I.bits(F(r["n_correspondences"]) / F(n - 2))
        with pytest.raises(M.Refused):
            M.register(*I.scans(p), **I.KW)
    r = model_of(few, device_entry=True, **I.KW)
    rows = [int(np.isfinite(few[k]).all(axis=1).sum()) for k in ("from_xyz", "to_xyz")]
    assert rows[0] == 1095 and rows[1] < 150 and (r["branch"], r["status"], r["from_is_target"]) == (0, M.OK, True)
    assert I.bits(r["ratio"]) == I.bits(F(r["n_correspondences"]) / F(1095))


def test_the_8192_row_pairs_take_branch_1_and_fail_the_gate_somewhere():
    low, gate, between, kw = I.rows_8192()
    assert (low["from_xyz"].shape[0], low["to_xyz"].shape[0], gate["from_xyz"].shape[0], gate["to_xyz"].shape[0]) == (8192, 8100, 8192, 8000)
    assert kw["max_iterations"] == 2 and kw["normal_gate"]
    r = model_of(low, **kw)
    assert (r["branch"], r["status"], r["stop"], r["iterations"]) == (1, M.OK, M.STOP_ITERATIONS, 2) and r["n_correspondences"] > 2000
    assert F(0) < r["complexity"] < F(0.02) <= r["second_eigenvalue"]
    r = model_of(gate, **kw)
    assert (r["branch"], r["status"], r["stop"], r["iterations"]) == (0, M.OK, M.STOP_ITERATIONS, 2)
    assert 0 < r["reciprocal_pass"].sum() < len(r["reciprocal_pass"]) and r["n_correspondences"] > 2000
    assert (r["reciprocal_rows"][~r["reciprocal_pass"]] >= 7936).any() and not r["reciprocal_pass"][:r["n_correspondences"]].all()
    assert model_of(between, **kw)["branch"] == 0


def test_the_filter_leaves_more_than_1024_points_in_a_region_of_2048():
    import scan_filter_model as SM
    p, kw, region = I.filter_chain()
    f = SM.filter_scans([p["from_xyz"], p["to_xyz"]], [region, region], device_entry=True, **kw)
    assert region == 2048 and (f["status"] == SM.OK).all() and 1100 <= f["count"].min() and f["count"].max() <= 1900
    assert np.isnan(f["xyz"][f["count"][0]:region]).all() and np.isnan(f["normals"][region + f["count"][1]:]).all()
    r = M.register(f["xyz"][:region], f["normals"][:region], f["xyz"][region:], f["normals"][region:], p["guess"], device_entry=True, **dict(I.KW, max_iterations=3))
    assert (r["branch"], r["status"]) == (0, M.OK) and r["n_correspondences"] >= 300
