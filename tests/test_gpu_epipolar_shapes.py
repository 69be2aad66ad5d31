"""lcd_verify_epipolar and lcd_verify_epipolar_dev where a call shows one candidate of 3 x iterations: winners on every root, chunk and wave
(the census), ties across chunks and waves, scenes times powers of two down to subnormal squares and up to overflow, non-finite keypoints, the
ends of iterations, seed and match_count_min, ids kept in the scratch, and hypotheses without seven distinct draws.  Everything is compared
with the NumPy model (epipolar_model.py) exactly -- ints and float bits -- through both entries with canary-filled outputs;
test_epipolar_inputs.py proves on the CPU that each input is of the class it is here for."""
import numpy as np
import pytest

import epipolar_inputs as I
import epipolar_model as M
from test_gpu_epipolar import KW, check_both, eng, run_dev, run_host  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def census():
    return I.census_batch()


def test_the_winners_cover_every_root_chunk_and_wave(eng, census):
    """46 pairs of 1 026 candidates each: winners on roots 0, 1 and 2, on cubics with one and three real roots, in chunks 0 .. 3 and in the last
    chunk of two, made by lanes of every wave and scored by every wave, with and without the sign flip"""
    pairs, iterations, seed = census
    want = check_both(eng, pairs, "census", iterations=iterations, seed=seed)
    assert (want["status"] == M.OK).all()
    check_both(eng, pairs[::-1], "census reversed", iterations=iterations, seed=seed)


@pytest.mark.parametrize("iterations", (85, 86, 300))
def test_ties_take_the_lowest_candidate_across_chunks_and_waves(eng, iterations):
    """up to 119 candidates reach the best count, in all four chunks at 300 iterations and on both sides of candidate 255 at 86"""
    pairs, seed = I.tie_pairs()
    want = check_both(eng, pairs, "ties %d" % iterations, iterations=iterations, seed=seed)
    assert want["n_inliers"][:3].tolist() == [8, 9, 12]


def scale_pairs(k):
    return [I.scaled(I.scene(3, 100), k), I.scaled(I.with_m(8), k)]


def device_inliers(eng, pairs, **kw):
    """the device entry's inlier ids, pair by pair"""
    got = run_dev(eng, pairs, **kw)
    first = np.concatenate([[0], np.cumsum([p["to_ids"].shape[0] for p in pairs])])
    return [got["inliers"][first[j]:first[j] + got["n_inliers"][j]].tolist() for j in range(len(pairs))]


@pytest.fixture(scope="module")
def inliers_at_scale_one(eng):
    ids = device_inliers(eng, scale_pairs(0), **KW)
    assert [len(i) for i in ids] == [16, 8]
    return ids


@pytest.mark.parametrize("k", (-74, -70, -66, -64, -62, -20, 20, 55, 60))
def test_power_of_two_scales(eng, inliers_at_scale_one, k):
    """scene(3, 100) and with_m(8) times 2^k, the threshold scaled alike.  From 2^-64 down the distance squares and thr2 are subnormal: a
    device that flushed them, or rounded / or sqrt otherwise, would differ from the model here.  For k in -62, -20, +20, +55 the scaling is
    exact all the way, and the device's inlier ids are those it gave itself at scale 1."""
    pairs = scale_pairs(k)
    kw = dict(KW, ransac_threshold=3.0 * 2.0 ** k)
    want = check_both(eng, pairs, "scale 2^%d" % k, **kw)
    assert want["status"].tolist() == ([M.NO_MODEL] * 2 if k in (-74, 60) else [M.OK] * 2)
    if k in (-62, -20, 20, 55):
        assert device_inliers(eng, pairs, **kw) == inliers_at_scale_one


def test_non_finite_keypoints(eng):
    pairs = [I.inf_keypoint(sign, side) for side in ("from", "to") for sign in (1, -1)]
    want = check_both(eng, pairs, "infinite keypoints")
    assert want["status"].tolist() == [M.NO_MODEL] * 4 and want["n_pairs"].tolist() == [40] * 4 and not want["fundamental"].any()
    nan, twin = I.nan_unpaired()
    want = check_both(eng, [nan, twin], "NaN in unpaired rows")
    assert want["status"].tolist() == [M.OK, M.OK] and M.bits(want["fundamental"][0]).tolist() == M.bits(want["fundamental"][1]).tolist()
    got = run_dev(eng, [nan, twin], **KW)
    n = nan["to_ids"].shape[0]
    assert got["fundamental"][0].tobytes() == got["fundamental"][1].tobytes() and got["n_inliers"][0] == got["n_inliers"][1]
    assert np.array_equal(got["inliers"][:n], got["inliers"][n:]) and np.array_equal(got["matches"][:n], got["matches"][n:])


def test_iteration_and_seed_extremes(eng, census):
    """65 535 iterations are 768 chunks less three candidates; seed + h wraps past 2^32 within the first sixteen hypotheses"""
    check_both(eng, [I.with_m(10)], "65535 iterations", iterations=65535)
    for seed in (0, 0xFFFFFFFF, 0xFFFFFFF0):
        check_both(eng, census[0][:4], "seed %#x" % seed, iterations=300, seed=seed)


def test_match_count_min_below_and_far_above_eight(eng):
    """below 8 the rule's own minimum of eight pairs decides; 2^31 - 1 is above every count"""
    pairs = [I.with_m(7), I.with_m(8), I.scene(3, 100)]
    for match_count_min in (1, 7):
        want = check_both(eng, pairs, "match_count_min %d" % match_count_min, match_count_min=match_count_min)
        assert want["status"].tolist() == [M.FEW_PAIRS, M.OK, M.OK] and want["n_pairs"].tolist() == [7, 8, 100]
    want = check_both(eng, pairs, "match_count_min 2^31 - 1", match_count_min=2 ** 31 - 1)
    assert want["status"].tolist() == [M.FEW_PAIRS] * 3 and want["n_pairs"].tolist() == [7, 8, 100]


def test_two_8192_row_pairs_without_out_matches(eng):
    """without out_matches a pair's ids go to the eighth word of its scratch rows; the second pair's scratch starts 8 x 8 192 words in"""
    pairs = [I.scene(77, 100, extra=8092), I.scene(78, 8192, outliers=0.5, extra=0)]
    assert [p["to_ids"].shape[0] for p in pairs] == [8192, 8192]
    want = check_both(eng, pairs, "8192 rows twice", leave_out=("matches",), iterations=10)
    assert want["n_pairs"].tolist() == [100, 8192] and want["n_inliers"][1] > 0
    check_both(eng, pairs, "8192 rows twice", leave_out=("matches", "fundamental"), iterations=10)


def test_hypotheses_without_seven_distinct_draws(eng):
    """hypothesis 3 of 60 finds no seven distinct indices among eight within its 32 draws: its three candidates are skipped, the rest decide"""
    p, seed, iterations = I.draw_failure()
    want = check_both(eng, [p], "draw failure", iterations=iterations, seed=seed)
    assert want["status"].tolist() == [M.OK]
    others = [I.scene(100 + m, m, outliers=0.3, extra=4) for m in (9, 63, 64, 65)]
    want = check_both(eng, others[:3] + [p] + others[3:], "draw failure as pair 3 of 5", iterations=iterations, seed=seed)
    assert want["status"][3] == M.OK and want["n_pairs"].tolist() == [9, 63, 64, 8, 65]
