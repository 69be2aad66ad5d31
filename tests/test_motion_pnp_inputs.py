"""Each input of tests/motion_pnp_inputs.py has the property it exists for.  No GPU.  What a search found is a constant there and is proven
again here."""
import numpy as np
import pytest

import motion_pnp_inputs as I
import motion_pnp_model as M

KW = dict(min_inliers=4, reproj_error=2.0, iterations=60, refine_iterations=5, variance_median_ratio=4, max_variance=0.0, seed=3)


def test_the_mixed_batch_has_its_sizes_and_its_decoys():
    for m, pair in zip(I.BATCH_SIZES, I.mixed_batch()):
        ids, P, UV, T = M.correspondences(*I.frames(pair))
        assert len(ids) == m == pair["m"] and ids.tolist() == pair["ids"].tolist()
        for side in ("from_ids", "to_ids"):                             # an id that occurs twice, ids of one side only
            vals, counts = np.unique(pair[side], return_counts=True)
            assert (counts == 2).sum() == 1
        assert len(set(pair["from_ids"].tolist()) - set(pair["to_ids"].tolist())) >= 3 and len(set(pair["to_ids"].tolist()) - set(pair["from_ids"].tolist())) >= 3
        shared = set(pair["from_ids"].tolist()) & set(pair["to_ids"].tolist())
        assert len(shared) == m + 3                                     # the two doubled ids and the one whose from-point is not finite
        assert (~np.isfinite(pair["from_xyz"]).all(axis=1)).sum() == 1
        if m >= 63:
            assert np.isnan(T).any() and np.isfinite(T).all(axis=1).sum() > m // 2
            assert ids.min() < 0                                        # negative ids take part
            # the generator's inliers reproject within a few pixels under its pose, its outliers do not as a rule
            e, front = M.reproj_error(I.true_model(pair), I.model_camera(I.CAMERA), P, UV)
            assert front.all() and (e[pair["inlier"]] < 3.0).all() and (e[~pair["inlier"]] > 3.0).mean() > 0.9


def test_the_special_pairs():
    r = M.estimate(*I.frames(I.all_outlier_pair()), **dict(KW, min_inliers=10, iterations=300))
    assert r["status"] != M.OK and r["counts"].max() < 10
    behind = I.behind_pair()
    _, P, UV, _ = M.correspondences(*I.frames(behind))
    assert len(P) == behind["m"] and (P[:, 2] < 0).all() and (P[:, 1] == 0).all() and len(set(P[:, 0].tolist())) == behind["m"]
    r = M.estimate(*I.frames(behind), **dict(KW, iterations=300))
    assert r["status"] == M.NO_MODEL and not r["counts"].any()
    seed = I.seed_with_invalid_first(4, 1)
    assert M.draw4(seed, 0, 4) is None and M.draw4(seed, 1, 4) is not None
    pair = I.mixed_batch()[6]
    for local in (None, I.LOCAL):                                       # guess_of inverts model_of_guess up to rounding
        back = M.model_of_guess(I.guess_of(I.true_model(pair), local), local)
        np.testing.assert_allclose(back, I.true_model(pair), atol=2e-6)


@pytest.mark.parametrize("name", sorted(I.REFINE_CASES))
def test_refine_cases_reach_their_branch(name):
    pair, kw = I.refine_case(name)
    r = M.estimate(*I.frames(pair), **dict(KW, **kw))
    assert I.REFINE_CASES[name][7] in r["trace"], r["trace"]
    if name == "size_members_few":
        assert {"size_changed", "members_changed", "few"} <= set(r["trace"]) and r["trace"][0] != "few"
    if name == "oscillating_guarded":
        assert "oscillating" not in r["trace"] and I.REFINE_CASES[name][:5] == I.REFINE_CASES["oscillating"][:5]
    if name == "step_sensitive":                                        # why the rule takes eight Gauss-Newton steps
        ids = [M.estimate(*I.frames(pair), **dict(KW, steps=s, **kw))["inliers"].tolist() for s in (6, 7, 8, 9, 10)]
        assert ids[0] != ids[1] and ids[1] == ids[2] == ids[3] == ids[4]


def test_the_staged_limit_and_the_big_pair():
    assert I.STAGE_CAP == {True: 3360, False: 5376}
    big = I.big_pair()
    assert big["from_ids"].shape[0] == big["to_ids"].shape[0] == 8192 == M.MAX_ROWS
    ids, _, _, _ = M.correspondences(*I.frames(big))
    assert len(ids) == 8000 > max(I.STAGE_CAP.values())


def test_the_fit_sets_are_in_general_position():
    sets = I.fit_sets()
    assert len(sets) == 27
    for s in sets:
        n = len(s["P"])
        assert 20 <= n <= 650 and n >= 8 and I.general_position(s["UV0"].astype(np.float64), s["C"])
        assert 0.5 <= s["C"][:, 2].min() and s["C"][:, 2].max() <= 10.0
        assert (s["UV0"][:, 0] >= 0).all() and (s["UV0"][:, 0] <= I.WIDTH - 1).all() and (s["UV0"][:, 1] >= 0).all() and (s["UV0"][:, 1] <= I.HEIGHT - 1).all()
        noise = s["UV1"] - s["UV0"]
        assert 0.3 < noise.std() < 0.7
        e, front = M.reproj_error(np.concatenate([s["R"], s["t"][:, None]], axis=1).reshape(12).astype(np.float32), I.model_camera(I.CAMERA), s["P"], s["UV0"])
        assert front.all() and e.max() < 0.01                           # noise-free up to fp32
