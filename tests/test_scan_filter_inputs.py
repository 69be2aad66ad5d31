"""Each hand-made scan of tests/scan_filter_inputs.py does what it is named for, proven with tests/scan_filter_model.py (no GPU)."""
import numpy as np

import scan_filter_inputs as I
import scan_filter_model as M

C = I.cases()


def run(name, k=0, **over):
    c = C[name]
    cap = None if c["caps"] is None else c["caps"][k]
    return M.filter_scan(c["scans"][k], cap, device_entry=True, **dict(c["kw"], **over))


def test_steps_at_n_equal_to_step_and_one_above():
    assert [run("step_2", k)["count"] for k in range(3)] == [2, 1, 20]     # n == step: no downsampling; n == step + 1: n / step = 1
    assert [run("step_3", k)["count"] for k in range(3)] == [3, 1, 13]
    np.testing.assert_array_equal(run("step_3", 2)["xyz"][:13], C["step_3"]["scans"][2][0:39:3])


def test_the_range_is_strict_on_both_bounds():
    b = I.on_the_bounds()
    r = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
    assert r[0] == 25 and r[1] < 25 < r[2] and r[3] == 25
    kept = lambda res: [int(np.flatnonzero((b == row).all(axis=1))[0]) for row in res["xyz"][:res["count"]]]
    assert kept(run("range_min")) == [0, 2, 3, 5, 6]                       # r == 25 stays, one float below goes
    assert kept(run("range_max")) == [0, 1, 3, 4]                          # r == 25 stays, one float above goes
    assert kept(run("range_both")) == [0, 2, 3, 5]                         # r == 100 stays as well
    assert kept(run("range_negative_min")) == kept(run("range_max"))       # a negative bound is off
    assert kept(run("range_2d")) == [0, 1, 3, 4, 6]                          # z takes no part: (3, 4, 100) stays, (0, 0, 5) too


def test_rows_that_are_not_finite_keep_their_sampling_slot():
    r = run("not_finite_rows")
    scan = C["not_finite_rows"]["scans"][0]
    np.testing.assert_array_equal(I.bits(r["xyz"][:r["count"]]), I.bits(scan[2:300:2][np.arange(1, 150) != 128]))   # rows 0 and 256 are sampled and dropped
    assert r["count"] == 148 and run("not_finite_rows_voxel_normals")["stage_counts"][0] == 297
    try:
        M.filter_scan(scan, downsampling_step=2)
        assert False
    except M.Refused as e:
        assert e.code == M.INVALID


def test_voxel_cases():
    r = run("one_voxel_513")
    assert r["stage_counts"].tolist() == [513, 1, 1]
    s = np.float32(0)
    for v in C["one_voxel_513"]["scans"][0][:, 0]:
        s = s + v
    assert I.bits(r["xyz"][0, 0]) == I.bits(s / np.float32(513))             # the running sum in row order
    assert run("every_row_its_voxel")["count"] == 9 * 8 * 7
    assert run("runs")["count"] == 5
    neg = run("negative_coordinates")
    assert (C["negative_coordinates"]["scans"][0] < 0).all() and 1 < neg["count"] < 300
    m = run("multiples_of_the_leaf")
    assert m["count"] == 120                                                 # a multiple of the leaf opens its own cell: no two rows merge
    x = np.sort(np.unique(m["xyz"][:120, 0]))
    np.testing.assert_array_equal(x, np.array([-0.75, -0.5, -0.25, 0, 0.25, 0.5], np.float32))
    assert [run("grid_too_large", k)["status"] for k in range(2)] == [M.GRID_TOO_LARGE, M.OK]
    assert run("grid_too_large")["stage_counts"].tolist() == [2, 0, 0]
    assert run("cell_beyond_int32")["status"] == M.GRID_TOO_LARGE


def test_floor_is_not_truncation():
    r = M.filter_scan(np.array([[-0.01, 0, 0], [0.01, 0, 0]], np.float32), voxel_size=0.1)
    assert r["count"] == 2                                                   # cells -1 and 0; a truncation would merge them


def test_k_mode_cases():
    for k in (1, 2):
        assert [run("k_%d" % k, s)["status"] for s in range(3)] == [M.EMPTY] * 3
        assert run("k_%d" % k)["stage_counts"].tolist() == [300, 300, 0]
    for k in (3, 5, 8, 9, 16, 17, 32):
        assert [run("k_%d" % k, s)["status"] for s in range(3)] == [M.OK, M.OK, M.EMPTY]     # 4 rows: min(K, |C|) = 4 (K >= 4) or 3; 2 rows: none
    lat = C["k_lattice_ties"]["scans"][0]
    d = M.dist2(lat, lat)
    assert (np.sort(d, axis=1)[:, 4] == np.sort(d, axis=1)[:, 5]).any()      # the fifth and sixth neighbour are equally far: the row decides
    nb = M.neighbours_k(lat, 5)
    assert (nb[:, 0] == np.arange(100)).all()                                # p itself first: d2 = 0
    dup = C["k_duplicates"]["scans"][0]
    assert (M.neighbours_k(dup, 5)[::3, :3] == np.arange(0, 180, 3)[:, None] + np.arange(3)).all()
    col = run("k_collinear")
    assert col["status"] == M.OK and np.isfinite(col["normals"][:20]).all()
    assert (np.abs((col["normals"][:20] * np.array([1, 2, 0], np.float32)).sum(axis=1)) < 1e-5).all()   # perpendicular to the line
    flat = run("k_flat_z0")
    np.testing.assert_array_equal(flat["normals"][:64], np.tile(np.array([0, 0, 1], np.float32), (64, 1)))   # the flip's dot product is exactly 0: not negated


def test_radius_mode_cases():
    lat = C["radius_lattice"]["scans"][0]
    inside = M.dist2(lat, lat) <= np.float32(1)
    assert (inside.sum(axis=1) >= 4).all() and (M.dist2(lat, lat)[inside] == 1).any()   # the six lattice neighbours sit on d2 == r^2
    assert run("radius_lattice")["count"] == 100
    sp = run("radius_sparse")
    assert 0 < sp["count"] < sp["stage_counts"][1] == 200                    # rows with fewer than three neighbours go


def test_ground_rule_cases():
    a, b = run("ground_up", ground_normals_up=0.0), run("ground_up")
    turned = (I.bits(a["normals"]) != I.bits(b["normals"])).any(axis=1)
    assert turned.any() and (a["xyz"][turned, 2] < 10).all() and (a["xyz"][~turned & (np.arange(400) < a["count"]), 2] >= 10).any()
    above = run("ground_up", 1)                                              # a ceiling at z = 12 seen from the origin: its normals point down and stay
    assert (above["normals"][:64, 2] == -1).all()
    scan, kw, up_equal, up_below = I.ground_edge(M)
    e, l = M.filter_scan(scan, ground_normals_up=up_equal, **kw), M.filter_scan(scan, ground_normals_up=up_below, **kw)
    assert (I.bits(e["normals"]) != I.bits(l["normals"])).any() and up_below < up_equal


def test_capacity_cases():
    assert [run("capacity_exact", k)["status"] for k in range(2)] == [M.OK, M.OK]
    short = run("capacity_one_short")
    assert short["status"] == M.NO_ROOM and short["count"] == 0 and short["stage_counts"].tolist() == [64, 64, 64] and np.isnan(short["xyz"]).all()
    assert run("capacity_one_short_normals", 1)["status"] == M.NO_ROOM and run("capacity_zero")["status"] == M.NO_ROOM
    big = run("larger_region")
    assert big["status"] == M.OK and (I.bits(big["xyz"][big["count"]:]) == 0x7FC00000).all() and (I.bits(big["normals"][big["count"]:]) == 0x7FC00000).all()
