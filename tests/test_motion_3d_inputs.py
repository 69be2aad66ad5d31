"""Every input of tests/motion_3d_inputs.py has the property it exists for, shown with the NumPy model alone.  No GPU."""
import numpy as np
import pytest

import motion_3d_inputs as I
import motion_3d_model as M


def test_mixed_batch_has_the_sizes_duplicates_and_one_sided_ids():
    batch = I.mixed_batch()
    assert tuple(p["m"] for p in batch) == I.BATCH_SIZES
    for p in batch:
        ids, P, Q = M.correspondences(*I.frames(p))
        assert ids.tolist() == p["ids"].tolist() and len(ids) == p["m"]
        f, t = p["from_ids"].tolist(), p["to_ids"].tolist()
        assert any(f.count(i) == 2 and t.count(i) == 1 for i in set(f))             # twice in from, once in to
        assert any(t.count(i) == 2 and f.count(i) == 1 for i in set(t))             # once in from, twice in to
        assert len(set(f) - set(t)) >= 3 and len(set(t) - set(f)) >= 3              # ids of one side only
        assert p["from_ids"].shape[0] > p["m"] and (np.diff(p["from_ids"]) < 0).any()   # shuffled rows
    assert any((p["ids"] < 0).any() for p in batch)                                 # the rule has no sign test
    assert [m for m in I.BATCH_SIZES if m in (63, 64, 65, 255, 256, 257)] == [63, 64, 65, 255, 256, 257]   # around a wave and a workgroup


def test_the_batch_reaches_every_status_but_no_model():
    seen = set()
    for p in I.mixed_batch():
        seen.add(M.estimate(*I.frames(p), min_inliers=4, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=1)["status"])
    assert {M.OK, M.FEW_CORRESPONDENCES} <= seen
    r = M.estimate(*I.frames(I.all_outlier_pair()), min_inliers=10, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=1)
    assert r["counts"].max() < 10 and r["status"] in (M.BELOW_MIN_INLIERS, M.FEW_INLIERS)
    assert M.estimate(*I.frames(I.exact_pair(3)), min_inliers=3, iterations=1, refine_iterations=0, seed=I.seed_with_invalid_first(3, 1))["status"] == M.NO_MODEL


def test_exact_pair_ties_every_hypothesis():
    r = M.estimate(*I.frames(I.exact_pair(40)), min_inliers=3, inlier_distance=0.1, iterations=64, refine_iterations=0, seed=5)
    assert (r["counts"] == 40).all()
    np.testing.assert_array_equal(r["transform"], np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32))


def test_seed_with_invalid_first():
    for invalid in (1, 2):
        seed = I.seed_with_invalid_first(3, invalid)
        assert all(M.draw3(seed, h, 3) is None for h in range(invalid)) and M.draw3(seed, invalid, 3) is not None
        assert all(M.draw3(s, 0, 3) is not None for s in range(min(seed, 200)))      # it is the first such seed (checked up to 200)


def test_overflow_refit_pair():
    p = I.overflow_refit_pair()
    ids, P, Q = M.correspondences(*I.frames(p))
    assert len(ids) == p["m"] and np.isfinite(P).all() and np.isfinite(Q).all()
    assert np.isnan(M.fit_set(P, Q)).any()                                           # the fit of all of them overflows
    idx = np.array(M.draw3(1, 0, p["m"]))
    assert np.isfinite(M.fit3(P[idx][:, None], Q[idx][:, None])).all()               # a hypothesis does not
    r = M.estimate(*I.frames(p), min_inliers=3, inlier_distance=I.OVERFLOW_DISTANCE, iterations=20, refine_iterations=5, seed=1)
    assert (r["counts"] == p["m"]).all() and r["trace"] == ["empty"]


@pytest.mark.parametrize("name", sorted(I.REFINE_CASES))
def test_refine_cases_reach_their_branch(name):
    pair, kw = I.refine_case(name)
    assert I.REFINE_CASES[name][6] in M.estimate(*I.frames(pair), **kw)["trace"]


def test_fit_sets_are_well_conditioned():
    sets = I.fit_sets()
    assert len(sets) >= 20
    for P, Q in sets:
        assert len(P) >= 6 and np.sort(M.kabsch64(P, Q)[2])[1] / len(P) > I.SIGMA_FLOOR
    # what the floor is for: points on a line are refused
    line = np.outer(np.arange(8.0), [1.0, 2.0, 3.0]).astype(np.float32)
    assert not I.well_conditioned(line, line) and not I.well_conditioned(sets[0][0][:5], sets[0][1][:5])


def test_big_pair_is_beyond_the_staging():
    p = I.big_pair()
    assert p["from_ids"].shape[0] == 8192 and p["to_ids"].shape[0] == 8192
    assert len(M.correspondences(*I.frames(p))[0]) == 8000 > I.STAGE_CAP == 5248
    assert I.BATCH_SIZES[-1] < I.STAGE_CAP                                           # the mixed batch is on the staged path
