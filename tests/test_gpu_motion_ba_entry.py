"""The entry with the reference's shape, MotionBA::refine through VWDictionaryHip.refine_motion_ba (host/MotionBA.cpp, c_shim.cpp's hmba_refine),
against tests/motion_ba_model.py: the multimaps turned into arrays, the prior taken from the PnP's covariance inputs, the baselines, the
survivors put in the inliers' place, and the lending dictionary untouched."""
import numpy as np
import pytest

import motion_ba_inputs as I
import motion_ba_model as M

pytestmark = pytest.mark.gpu

# (name, pair, kpts_a, words3b, (variance kind, linear variance, cosine), local, overrides) -> the status the model gives
CASES = (
    ("plain", dict(seed=80, m=70, outliers=6), True, True, (1, 1e-4, 0.9995), False, {}),
    ("no from keypoints", dict(seed=81, m=64, outliers=5), False, True, (1, 2e-4, 1.0), False, {}),              # acos(1) = 0: the angular floor
    ("no to points", dict(seed=82, m=90, outliers=7), True, False, (2, 3e-4, 1.0), True, {}),                    # kind 2: one variance for all six
    ("identity information", dict(seed=83, m=65, outliers=5), True, True, (0, 1.0, 1.0), True, {}),             # kind 0: NULL prior_variance
    ("other baselines", dict(seed=84, m=60, outliers=4), True, True, (1, 1e-4, 0.0), False, dict(baselines=(0.12, 0.0))),
    ("below min inliers", dict(seed=85, m=24, outliers=6), True, True, (1, 1e-4, 0.999), False, dict(min_inliers=20)),
    ("mean distance", dict(seed=86, m=50, depth=(8.0, 10.0)), True, True, (1, 1e-4, 0.999), False, dict(max_inliers_mean_distance=7.5)),
    ("distribution", dict(seed=87, m=50), True, True, (1, 1e-4, 0.999), True, dict(min_inliers_distribution=0.5)),
)


def prior_of(kind, lin, cosine):
    """motion_pnp_covariance's diagonal entries 0 and 3 (Motion2D.cpp)"""
    return None if kind == 0 else (lin, 2.1981 * np.arccos(cosine)) if kind == 1 else (lin, lin)


def test_the_reference_shaped_entry_through_the_dictionary():
    from rtabmap_amd import synth
    from rtabmap_amd.vwdictionary import VWDictionaryHip
    h = VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
    h.add_new_words(synth.vocab_surf(50, seed=8), 1)
    h.update()
    before = (h.index_ids(), h.visual_words, h.indexed_words, h.not_indexed_words, h.total_active_references)
    seen = set()
    for name, spec, kpts_a, words3b, (kind, lin, cosine), local, over in CASES:
        spec = dict(spec)
        p = I.seeded(spec.pop("seed"), spec.pop("m"), local=local, **spec)
        # an id twice in the from-frame and one twice in the to-frame (neither an inlier): the multimaps hold them, the rule ignores them
        p["from_ids"][int(np.flatnonzero(~np.isin(p["from_ids"], p["inliers"]))[0])] = p["from_ids"][int(np.flatnonzero(~np.isin(p["from_ids"], p["inliers"]))[1])]
        p["to_ids"][int(np.flatnonzero(~np.isin(p["to_ids"], p["inliers"]))[0])] = p["to_ids"][int(np.flatnonzero(~np.isin(p["to_ids"], p["inliers"]))[1])]
        kw = dict(min_inliers=1, iterations=20, pixel_variance=1.0, robust_delta=8.0, max_inliers_mean_distance=0.0, min_inliers_distribution=0.0,
                  baselines=(I.BASELINE, I.BASELINE))
        kw.update(over)
        cam = I.camera(True, local)
        want = M.refine(p["from_ids"], p["from_xyz"], p["to_ids"], p["to_points"], p["inliers"], p["transform"], from_points=p["from_points"] if kpts_a else None,
                        to_xyz=p["to_xyz"] if words3b else None, prior_variance=prior_of(kind, lin, cosine), camera_from=cam, camera_to=cam, **kw)
        t, survivors, info = h.refine_motion_ba((p["from_ids"], p["from_xyz"]), (p["to_ids"], p["to_points"]), p["inliers"], p["transform"],
                                                kpts_a=p["from_points"] if kpts_a else None, words3b=p["to_xyz"] if words3b else None, variance_kind=kind,
                                                variance_lin=lin, angle_cos=cosine, camera_from=cam, camera_to=cam, **kw)
        seen.add(want["status"])
        assert info["status"] == want["status"], name
        assert (t is None) == (want["status"] != M.OK), name
        if t is not None:
            np.testing.assert_array_equal(t.view(np.uint32), want["transform"].view(np.uint32), err_msg=name)
        assert survivors == want["inliers"].tolist(), name
        assert np.float32(info["inliers_mean_distance"]).tobytes() == np.float32(want["inliers_mean_distance"]).tobytes(), name
        assert np.float32(info["inliers_distribution"]).tobytes() == np.float32(want["inliers_distribution"]).tobytes(), name
        if want["status"] == M.OK:
            assert (want["n_outliers"] > 0 or not kpts_a) and len(survivors) == len(p["inliers"]) - want["n_outliers"], name
    assert seen == {M.OK, M.BELOW_MIN_INLIERS, M.MEAN_DISTANCE_REJECTED, M.DISTRIBUTION_REJECTED}
    # an inlier id twice in the from-frame: LCD_BA_BAD_INLIER, no transform, the inliers as they came; then a call the engine refuses
    p = I.seeded(88, 30)
    p["from_ids"][int(np.flatnonzero(~np.isin(p["from_ids"], p["inliers"]))[0])] = p["inliers"][4]
    t, survivors, info = h.refine_motion_ba((p["from_ids"], p["from_xyz"]), (p["to_ids"], p["to_points"]), p["inliers"], p["transform"], kpts_a=p["from_points"],
                                            words3b=p["to_xyz"], camera_from=I.camera(True), camera_to=I.camera(True), min_inliers=1)
    assert t is None and info["status"] == M.BAD_INLIER and survivors == p["inliers"].tolist()
    t, survivors, info = h.refine_motion_ba((p["from_ids"], p["from_xyz"]), (p["to_ids"], p["to_points"]), p["inliers"], p["transform"], kpts_a=p["from_points"],
                                            words3b=p["to_xyz"], camera_from=I.camera(True), camera_to=I.camera(True), pixel_variance=0.0)
    assert t is None
    assert (h.index_ids(), h.visual_words, h.indexed_words, h.not_indexed_words, h.total_active_references) == before
    h.close()
