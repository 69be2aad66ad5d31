"""tests/motion_3d_model.py on hand-made cases with hand-computed values, every branch of the refinement loop reached by a constructed input,
the host mirror (rtabmap_amd/host/Motion3D.cpp, through c_shim.cpp) against the model bit for bit, and the fp32 fit against a float64 SVD fit.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import motion_3d_inputs as I
import motion_3d_model as M

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(min_inliers=4, inlier_distance=0.1, iterations=60, refine_iterations=5, seed=3)
# the largest difference between an entry of the fp32 fit and of the float64 SVD fit measured on I.fit_sets() (27 sets of 20 .. 650 inliers,
# coordinates within +-3) was 2.06e-7; the bound is that times the margin of 4 the design allows for other seeds and scales
FIT64_BOUND = 4 * 2.06e-7


def mirror(pair, **kw):
    from rtabmap_amd import vwdictionary as V
    return V.motion3d_cpu(*I.frames(pair), **kw)


def assert_same(got, want):
    """a result of the mirror (or of the engine, cut to the pair) against the model's"""
    assert int(got["status"]) == want["status"]
    np.testing.assert_array_equal(I.bits(got["transform"]), I.bits(want["transform"]))
    assert np.float64(got["variance"]).view(np.uint64) == np.float64(want["variance"]).view(np.uint64)
    assert list(got["matches"]) == list(want["matches"]) and list(got["inliers"]) == list(want["inliers"])


def both(pair, **kw):
    want = M.estimate(*I.frames(pair), **kw)
    assert_same(mirror(pair, **kw), want)
    return want


def frame_pair(f_ids, f_xyz, t_ids, t_xyz):
    return dict(from_ids=np.array(f_ids, np.int32), from_xyz=np.array(f_xyz, np.float32).reshape(-1, 3), to_ids=np.array(t_ids, np.int32),
                to_xyz=np.array(t_xyz, np.float32).reshape(-1, 3))


def test_unique_ids_and_the_predicate():
    """7 twice in from and once in to, 9 once in from and twice in to, a NaN, an infinity and a zero point on either side: none takes part;
    the rest comes out in ascending id, negative ids first"""
    nan, inf = float("nan"), float("inf")
    pair = frame_pair([5, 7, 7, 9, 11, 13, 15, 17, -3, 2, 21, 23], [[1, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [nan, 1, 1], [1, 1, 1], [0, 0, 0], [1, 1, 1], [0, 2, 0], [0, 0, 3], [1, inf, 1], [0, 0, -0.0]],
                      [7, 5, 9, 9, 11, 13, 15, 17, 2, -3, 99, 21, 23], [[1, 1, 1], [1, 0, 0], [3, 3, 3], [4, 4, 4], [1, 1, 1], [1, -inf, 1], [1, 1, 1], [0, -0.0, 0], [0, 0, 3], [0, 2, 0], [5, 5, 5], [1, 1, 1], [1, 1, 1]])
    ids, P, Q = M.correspondences(*I.frames(pair))
    assert ids.tolist() == [-3, 2, 5]
    np.testing.assert_array_equal(P, np.array([[0, 2, 0], [0, 0, 3], [1, 0, 0]], np.float32))
    np.testing.assert_array_equal(P, Q)
    r = both(pair, min_inliers=3, inlier_distance=0.1, iterations=4, refine_iterations=0, seed=0)
    assert r["status"] == M.OK and r["inliers"].tolist() == [-3, 2, 5]
    np.testing.assert_array_equal(r["transform"], np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32))      # to == from: the identity, exactly
    assert r["variance"] == 0.0
    r = both(pair, min_inliers=4, inlier_distance=0.1, iterations=4, refine_iterations=0, seed=0)
    assert r["status"] == M.FEW_CORRESPONDENCES and r["matches"].tolist() == [-3, 2, 5] and len(r["inliers"]) == 0 and r["variance"] == 1.0
    assert not r["transform"].any()


def test_two_three_and_min_inliers():
    two = I.exact_pair(2)
    for min_inliers in (1, 2):                                          # the guard size() >= 3 is its own
        assert both(two, min_inliers=min_inliers, inlier_distance=0.1, iterations=5, refine_iterations=5, seed=0)["status"] == M.FEW_CORRESPONDENCES
    three = I.exact_pair(3)
    r = both(three, min_inliers=1, inlier_distance=0.1, iterations=5, refine_iterations=5, seed=0)
    assert r["status"] == M.OK and len(r["inliers"]) == 3
    ten = I.exact_pair(10)
    assert both(ten, min_inliers=11, inlier_distance=0.1, iterations=5, refine_iterations=5, seed=0)["status"] == M.FEW_CORRESPONDENCES
    r = both(ten, min_inliers=10, inlier_distance=0.1, iterations=5, refine_iterations=5, seed=0)
    assert r["status"] == M.OK and len(r["inliers"]) == 10
    # six points that move together among twelve: inliers and variance are returned, the transform is not
    half = I.exact_pair(12)
    half["to_xyz"][6:] = half["to_xyz"][6:] * F(-3) + F(40)
    for min_inliers, status in ((6, M.OK), (7, M.BELOW_MIN_INLIERS)):
        r = both(half, min_inliers=min_inliers, inlier_distance=0.1, iterations=100, refine_iterations=5, seed=0)
        assert r["status"] == status and r["inliers"].tolist() == [1, 2, 3, 4, 5, 6] and r["variance"] == 0.0
        assert r["transform"].any() == (status == M.OK)


def test_a_known_rotation_is_recovered():
    """a quarter turn about z and the shift (1, 2, 3), exact in fp32: the pose is the inverse, R^T and -R^T t.  Tolerances from the format: a
    rotation entry carries a few roundings of values <= 1 (8 ulp of 1 = 1e-6); a translation entry is that error times a centroid of norm
    <= 14 (coordinates within +-8), 1e-5"""
    pair = I.exact_pair(9)
    p = pair["from_xyz"]
    pair["to_xyz"] = np.stack([-p[:, 1] + 1, p[:, 0] + 2, p[:, 2] + 3], axis=1).astype(np.float32)
    r = both(pair, min_inliers=9, inlier_distance=0.01, iterations=20, refine_iterations=5, seed=1)
    assert r["status"] == M.OK and len(r["inliers"]) == 9
    pose, model = r["transform"].reshape(3, 4), r["model"].reshape(3, 4)
    np.testing.assert_allclose(pose[:, :3], [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], rtol=0, atol=1e-6)
    np.testing.assert_allclose(pose[:, 3], [-2, 1, -3], rtol=0, atol=1e-5)
    np.testing.assert_allclose(model[:, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], rtol=0, atol=1e-6)
    np.testing.assert_allclose(model[:, 3], [1, 2, 3], rtol=0, atol=1e-5)


def test_sums_and_draws_by_hand():
    # (e0 + e2) + e1 with e1 = half an ulp of 1 and e2 = three quarters: 1 + 0.75 ulp rounds to 1 + ulp, the tie behind it to 1 + 2 ulp;
    # left to right the tie 1 + 0.5 ulp falls to 1 and the sum is 1 + ulp
    e = np.array([1.0, 2.0 ** -24, 1.5 * 2.0 ** -24], np.float32)
    assert M.lane_sum(e) == F(1) + F(2.0 ** -22) and M.sum3(*e) == M.lane_sum(e)
    assert (e[0] + e[1]) + e[2] == F(1) + F(2.0 ** -23)
    assert M.lane_sum(np.array([-0.0], np.float32)).view(np.uint32) == 0              # the lanes start at +0
    big = np.arange(1, 601, dtype=np.float32)
    lanes = [F(0)] * 256
    for i, v in enumerate(big):
        lanes[i % 256] = lanes[i % 256] + v
    s = 128
    while s:
        lanes = [lanes[l] + lanes[l + s] for l in range(s)]
        s //= 2
    assert M.lane_sum(big) == lanes[0]
    x = 1                                                                             # mix(1) by hand, step by step
    x ^= x >> 16; x = (x * 0x7feb352d) & M.M32; x ^= x >> 15; x = (x * 0x846ca68b) & M.M32; x ^= x >> 16
    assert M.mix(0) == 0 and M.mix(1) == x and M.mix(1 << 32 | 1) == x
    d = M.draw3(5, 0, 1000)
    assert len(set(d)) == 3 and all(0 <= v < 1000 for v in d)
    base = (M.mix(5) * 3) & M.M32
    assert d[0] == M.mix(base) % 1000
    assert M.draw3(5, 0, 2) is None and M.draw3(5, 0, 1) is None                       # never three distinct among two


def test_ties_go_to_the_lowest_hypothesis_and_an_invalid_draw_never_wins():
    exact = I.exact_pair(12)
    r = both(exact, min_inliers=3, inlier_distance=0.1, iterations=50, refine_iterations=0, seed=9)
    assert (r["counts"] == 12).all() and r["best"] == 0
    # a tie between different models: six noisy correspondences, all inside the threshold for several hypotheses
    noisy = I.random_pair(np.random.default_rng(4), 6, outliers=0.0, noise=0.01, decoys=False)
    r = both(noisy, min_inliers=3, inlier_distance=0.2, iterations=30, refine_iterations=0, seed=2)
    top = np.nonzero(r["counts"] == r["counts"].max())[0]
    assert len(top) >= 2 and r["best"] == top[0]
    later = M.estimate(*I.frames(noisy), min_inliers=3, inlier_distance=0.2, iterations=1, refine_iterations=0, seed=(2 + int(top[1])) & M.M32)
    assert (I.bits(later["transform"]) != I.bits(r["transform"])).any()                # hypothesis top[1] alone is another model
    # m = 3 and a seed whose hypothesis 0 finds no three distinct indices in 16 draws
    seed = I.seed_with_invalid_first(3, 1)
    three = I.exact_pair(3)
    assert M.draw3(seed, 0, 3) is None and M.draw3(seed, 1, 3) is not None
    assert both(three, min_inliers=3, inlier_distance=0.1, iterations=1, refine_iterations=0, seed=seed)["status"] == M.NO_MODEL
    r = both(three, min_inliers=3, inlier_distance=0.1, iterations=2, refine_iterations=0, seed=seed)
    assert r["status"] == M.OK and r["best"] == 1 and r["counts"].tolist() == [0, 3]


@pytest.mark.parametrize("name", sorted(I.REFINE_CASES))
def test_refinement_branches(name):
    pair, kw = I.refine_case(name)
    r = both(pair, **kw)
    assert I.REFINE_CASES[name][6] in r["trace"]
    for refine in I.REFINE:
        r = both(pair, **dict(kw, refine_iterations=refine))
        assert len(r["trace"]) <= max(refine, 0) + 1 and (refine > 0) == bool(r["trace"])


def test_refinement_empty_selection_on_the_first_pass():
    pair = I.overflow_refit_pair()
    kw = dict(min_inliers=3, inlier_distance=I.OVERFLOW_DISTANCE, iterations=20, seed=1)
    r = both(pair, refine_iterations=0, **kw)
    assert r["status"] == M.OK and len(r["inliers"]) == pair["m"]
    for refine in (1, 5):                                               # 1: the break; 5: the continue, whose condition leaves the loop
        r = both(pair, refine_iterations=refine, **kw)
        assert r["trace"] == ["empty"] and r["status"] == M.FEW_INLIERS and len(r["inliers"]) == 0 and r["variance"] == 1.0


def test_host_mirror_equals_the_model_on_the_generators():
    for pair in I.mixed_batch():
        for iterations in I.ITERATIONS:
            for refine in I.REFINE:
                both(pair, min_inliers=4, inlier_distance=0.1, iterations=iterations, refine_iterations=refine, seed=iterations + refine)
    r = both(I.all_outlier_pair(), **KW)
    assert r["status"] != M.OK or len(r["inliers"]) < 8
    both(I.exact_pair(300), **KW)


def test_host_mirror_equals_the_model_where_the_kernel_changes_shape():
    """the inputs of tests/test_gpu_motion_3d_shapes.py (but the largest): the mirror joins with a std::map, picks with a comparison of keys
    and selects the median with nth_element, the model does each its own way"""
    kw = dict(min_inliers=3, inlier_distance=0.1, iterations=50, refine_iterations=2, seed=1)
    for pair in I.asymmetric_pairs() + I.duplicate_run_pairs() + I.extreme_id_pairs() + [I.predicate_pair()]:
        both(pair, **kw)
    m, invalid, seed = I.TIE_INVALID_FIRST
    for iterations in I.TIE_ITERATIONS:
        assert both(I.exact_pair(m), min_inliers=3, inlier_distance=0.1, iterations=iterations, refine_iterations=0, seed=seed)["best"] == invalid
    for h, iterations in I.LATE_CASES + tuple((h, h) for h in I.CUT_OFF):
        both(I.late_winner_pair(), **I.late_kw(h, iterations))
    for seed in sorted(I.LATE_MEMBERS):
        both(I.late_members_pair(seed), seed=seed, **I.LATE_MEMBERS_KW)
    for pair, kw in I.select_cases().values():
        both(pair, **kw)
    for kw in I.scratch_table_kws():
        both(I.scratch_table_pair(), **kw)


def test_host_mirror_refuses_what_the_entry_refuses():
    pair = I.exact_pair(5)
    for bad in (dict(iterations=0), dict(iterations=65536), dict(min_inliers=0), dict(refine_iterations=-1), dict(inlier_distance=0.0),
                dict(inlier_distance=-1.0), dict(inlier_distance=float("nan")), dict(inlier_distance=float("inf"))):
        kw = dict(KW, **bad)
        assert mirror(pair, **kw) is None
        with pytest.raises(M.Refused):
            M.estimate(*I.frames(pair), **kw)
    assert mirror(I.exact_pair(8193), **KW) is None
    empty = frame_pair([], [], [], [])
    assert mirror(empty, **KW)["status"] == M.FEW_CORRESPONDENCES


def test_fp32_fit_against_a_float64_svd_fit():
    """the rule estimates what it should: every entry of the fp32 fit of a well-conditioned inlier set within FIT64_BOUND of the float64
    Kabsch fit of the same set (no parity claim)"""
    sets = I.fit_sets()
    assert len(sets) >= 20
    worst = 0.0
    for P, Q in sets:
        m = M.fit_set(P, Q).reshape(3, 4).astype(np.float64)
        R, t, _ = M.kabsch64(P, Q)
        worst = max(worst, np.abs(m[:, :3] - R).max(), np.abs(m[:, 3] - t).max())
    print("fp32 fit against float64 Kabsch: worst entry difference %.3e" % worst)
    assert worst <= FIT64_BOUND


def test_abi_of_the_new_struct():
    from rtabmap_amd import capi
    assert ctypes.sizeof(capi.LcdMotion3dArgs) == 136 and capi.LcdMotion3dArgs.inlier_distance.offset == 24 and capi.LcdMotion3dArgs.out_inliers.offset == 128
    src = open(os.path.join(ROOT, "rtabmap_amd", "csrc", "motion_3d.hip")).read()
    assert re.search(r"static_assert\(sizeof\(lcd_motion_3d_args\) == 136\b", src)
    header = open(os.path.join(ROOT, "include", "lcd.h")).read()
    assert int(re.search(r"#define LCD_ABI_VERSION (\d+)", header).group(1)) == 7
    assert int(re.search(r"#define LCD_M3D_SWEEPS (\d+)", header).group(1)) == M.SWEEPS
    rule = open(os.path.join(ROOT, "rtabmap_amd", "csrc", "motion_3d_rule.h")).read()
    assert int(re.search(r"constexpr int SWEEPS = (\d+)", rule).group(1)) == M.SWEEPS
    assert (capi.LCD_M3D_OK, capi.LCD_M3D_FEW_CORRESPONDENCES, capi.LCD_M3D_NO_MODEL, capi.LCD_M3D_FEW_INLIERS, capi.LCD_M3D_BELOW_MIN_INLIERS) == \
           (M.OK, M.FEW_CORRESPONDENCES, M.NO_MODEL, M.FEW_INLIERS, M.BELOW_MIN_INLIERS)
