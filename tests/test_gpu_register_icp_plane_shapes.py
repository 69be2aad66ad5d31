"""GPU tests of lcd_register_icp_plane and lcd_register_icp_plane_dev (rtabmap_amd/csrc/register_icp_plane.hip) where a workgroup's path, the
batch around it or the region it reads changes shape: the low-complexity branch and the gate at every block edge and at 8192 rows, the
source side of step 5 turned by normals that are not finite, branches side by side in one launch, NaN-padded regions in both search forms,
the scan filter feeding the grid form, and the grid form's edges with normals.  tests/test_register_icp_plane_inputs.py proves on the CPU
that every case does what it is named for.  Every comparison is exact: every int, and every float and double bit for bit, against
tests/register_icp_plane_model.py."""
import numpy as np
import pytest
import torch

import register_icp_plane_inputs as I
import register_icp_plane_model as M
from register_icp_plane_device import (LCD_ERR_INVALID, PER_PAIR, SEARCHES, expected, model_of, assert_same, outputs_dev, run_dev, run_host, check_both, refused)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import rtabmap_amd
    e = rtabmap_amd.Engine("f32", 64)
    yield e
    assert e.vocab_count() == (0, 0) and e.sig_count() == (0, 0)
    e.close()


def check_dev(eng, pairs, what="", **kw):
    """the device entry alone, under the three searches, with the refusals of that entry in the model"""
    want = expected(pairs, device_entry=True, **kw)
    for search in SEARCHES:
        assert_same(run_dev(eng, pairs, search=search, **kw), want, "%s dev, search %d" % (what, search))
    return want


def test_the_low_complexity_branch_at_every_block_edge(eng):
    """corridor pairs of 255, 256, 257, 511, 512, 513 and 1025 rows against 20 fewer, both ways round, in ONE batch per parameter set:
    GroupBackend's fit, reciprocal, median and set_registered inside the plane kernel's carve, then limit_translation with both vectors, with
    the first alone and without any (complexity 0 exactly), strategy 2 and force_3dof"""
    for name, (pairs, kw) in I.low_complexity_sizes().items():
        want = check_both(eng, pairs, name, searches=SEARCHES, **kw)
        assert (want["branch"] == 1).all() and (want["status"] == M.OK).all()


def test_the_gate_at_every_block_edge(eng):
    """room pairs of the same sizes with every fifth from-normal negated: the rank across one to five trips, the cut at `count`, the median over
    the first `count` with failing correspondences among them and in later trips than passing ones, the source on either side"""
    pairs, kw = I.gate_sizes()
    want = check_both(eng, pairs, "gate", searches=SEARCHES, **kw)
    assert (want["branch"] == 0).all()
    for p, n in zip(pairs, want["n_correspondences"]):
        assert 0 < n < len(model_of(p, **kw)["reciprocal_pass"])


def test_8192_rows_in_the_low_complexity_branch_and_under_the_gate(eng):
    low, gate, between, kw = I.rows_8192()
    for name, p, branch in (("corridor", low, 1), ("gate", gate, 0)):
        want = expected([p], **kw)
        assert want["branch"][0] == branch and want["stop"][0] == M.STOP_ITERATIONS and want["n_correspondences"][0] > 2000
        for search in SEARCHES:
            assert_same(run_dev(eng, [p], search=search, **kw), want, "8192 %s dev, search %d" % (name, search))
        assert_same(run_host(eng, [p], **kw), want, "8192 %s host" % name)
    r = model_of(gate, **kw)
    assert 0 < r["reciprocal_pass"].sum() < len(r["reciprocal_pass"])
    batch = [low, between, gate]
    assert_same(run_dev(eng, batch, **kw), expected(batch, **kw), "8192 in both branches, a small pair between")


def test_non_finite_normals_turn_the_source_side(eng):
    """300 rows against 280 of which 225 against 280 take part: step 5 compares the latter, and under the gate the variance shows it"""
    pairs, kw = I.swap_turned_by_normals()
    want = check_both(eng, pairs, "turned", searches=SEARCHES, **kw)
    for k, p in enumerate(pairs):
        other = model_of(p, source_is_to=not model_of(p, **kw)["from_is_target"], **kw)
        assert np.float64(want["variance"][k]).view(np.uint64) != np.float64(other["variance"]).view(np.uint64)
        assert I.bits(want["ratio"][k]) == I.bits(np.float32(want["n_correspondences"][k]) / np.float32(300))


def test_branches_side_by_side_in_one_launch(eng):
    """branch 0, branch 1, the early return of strategy 0 and the EMPTY return in neighbouring workgroups that share the stride and the LDS
    size of the largest pair, which stands in the middle; then the same batches reversed"""
    for strategy, (pairs, kw) in I.mixed_batch().items():
        want = check_both(eng, pairs, "mixed, strategy %d" % strategy, searches=SEARCHES, **kw)
        assert list(zip(want["branch"].tolist(), want["status"].tolist())) == I.MIXED[strategy]
        back = check_both(eng, pairs[::-1], "mixed and reversed, strategy %d" % strategy, searches=SEARCHES, **kw)
        for k in PER_PAIR:
            np.testing.assert_array_equal(np.ascontiguousarray(back[k][::-1]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8), err_msg=k)


def test_nan_padded_regions_in_both_search_forms(eng):
    """sides as lcd_filter_scans_dev leaves them: regions of 1 024 rows whose points stay brute under AUTO, regions of 2 048 rows with more
    than 1 024 points (grid under AUTO) and with fewer on one side; the sort is sized by the region, the search by the rows that take part"""
    for region, pads, plain, kw in I.padded_regions():
        want = check_dev(eng, pads, "regions of %d" % region, **kw)
        unpadded = expected(plain, **kw)
        for k in PER_PAIR:
            np.testing.assert_array_equal(np.ascontiguousarray(want[k]).view(np.uint8), np.ascontiguousarray(unpadded[k]).view(np.uint8), err_msg=k)
        assert (want["status"] == M.OK).all()
        refused(LCD_ERR_INVALID, run_host, eng, pads, **kw)


def test_the_filter_feeds_the_grid_form(eng):
    """two scans are filtered into regions of 2 048 rows that more than 1 024 voxels fill; lcd_register_icp_plane_dev then takes out_offsets
    as the pair's offsets, nothing read back in between, under AUTO (the grid form by the rows that take part) and GRID: the result equals
    the two models chained"""
    import scan_filter_model as SM
    p, fkw, region = I.filter_chain()
    want_f = SM.filter_scans([p["from_xyz"], p["to_xyz"]], [region, region], device_entry=True, **fkw)
    assert (want_f["status"] == SM.OK).all() and 1100 <= want_f["count"].min() and want_f["count"].max() <= 1900
    x = torch.from_numpy(np.concatenate([p["from_xyz"], p["to_xyz"]])).cuda()
    off, oo = [0, p["from_xyz"].shape[0], x.shape[0]], [0, region, 2 * region]
    f = dict(xyz=torch.full((2 * region, 3), 7.0, dtype=torch.float32, device="cuda"), normals=torch.full((2 * region, 3), 7.0, dtype=torch.float32, device="cuda"),
             count=torch.full((2,), -7, dtype=torch.int32, device="cuda"), stage_counts=torch.full((2, 3), -7, dtype=torch.int32, device="cuda"),
             status=torch.full((2,), -7, dtype=torch.int32, device="cuda"))
    outs = {search: outputs_dev(1, region) for search in (M.SEARCH_AUTO, M.SEARCH_GRID)}
    torch.cuda.synchronize()
    kw = dict(I.KW, max_iterations=3)
    eng.filter_scans_dev(x, off, oo, f, **fkw)
    for search, out in outs.items():
        eng.register_icp_plane_dev(f["xyz"][:region], f["normals"][:region], [0, region], f["xyz"][region:], f["normals"][region:], [0, region], p["guess"][None], out,
                                   search=search, **kw)
    eng.synchronize()
    np.testing.assert_array_equal(f["count"].cpu().numpy(), want_f["count"])
    np.testing.assert_array_equal(I.bits(f["xyz"].cpu().numpy()), I.bits(want_f["xyz"]))
    np.testing.assert_array_equal(I.bits(f["normals"].cpu().numpy()), I.bits(want_f["normals"]))
    q = I.raw(want_f["xyz"][:region], want_f["normals"][:region], want_f["xyz"][region:], want_f["normals"][region:], p["guess"])
    want = expected([q], device_entry=True, **kw)
    assert want["status"][0] == M.OK and want["branch"][0] == 0 and want["n_correspondences"][0] >= 300
    for search, out in outs.items():
        assert_same({k: v.cpu().numpy() for k, v in out.items()}, want, "behind the filter, search %d" % search)


def test_the_grid_edges_through_the_plane_kernel(eng):
    """register_icp_inputs.grid_edge_pairs() with a normal a row that is a function of the row index: targets on faces and corners, a nearest
    target in a diagonal neighbour cell, equal distances across cells, a target beyond the key range (brute inside a GRID call), a from-row
    beyond it (walks the target) -- fit_plane reads the normal of the row found.  With three iterations and with one, which hands the first
    fit to the outputs.  Then coordinates that are not finite at 600 and 1 100 rows under all three searches, on the device entry"""
    pairs = list(I.grid_edge_pairs().values())
    for kw in (I.GRID_EDGE_KW, I.GRID_EDGE_ONCE_KW):
        want = check_both(eng, pairs, "grid edges", searches=SEARCHES, **kw)
        assert (want["branch"] == 0).all() and {M.OK, M.NOT_CONVERGED} == set(want["status"].tolist())
    bad = I.non_finite_coordinates()
    want = check_dev(eng, bad, "non-finite coordinates", **I.KW)
    assert (want["status"] == M.OK).all()
    refused(LCD_ERR_INVALID, run_host, eng, bad, **I.KW)
