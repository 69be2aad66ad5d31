"""CPU-only: tests/feature_select_model.py on hand-made cases whose answers follow from the reference's text (Features2d.cpp:293-516,
Memory.cpp:5951-6059), and the host mirror (rtabmap_amd/host/FeatureSelect.cpp, through the shim) against the model."""
import numpy as np
import pytest

import feature_select_inputs as I
import feature_select_model as M

DENORMAL = float(np.float32(1e-45))


def test_equal_responses_the_higher_index_wins_on_both_sides_of_the_cut():
    r = [2.0, 1.0, 1.0, 1.0, 1.0, 3.0]
    # the multimap walked backwards: 5 (3.0), 0 (2.0), then the equal ones 4, 3, 2, 1
    assert M.select_frame(r, 3, M.BY_RESPONSE) == [5, 0, 4]
    assert M.select_frame(r, 4, M.BY_RESPONSE) == [5, 0, 4, 3]
    assert M.select_frame(r, 4, M.KEEP_ORDER) == [0, 3, 4, 5]            # 1 and 2 lose to 3 and 4
    assert M.select_frame([1.0] * 5, 2, M.KEEP_ORDER) == [3, 4]
    assert M.select_frame([-1.0, 1.0, -1.0], 1, M.BY_RESPONSE) == [2]     # fabs: both signs are one group


def test_signed_zeros_and_denormals():
    r = [0.0, -0.0, DENORMAL, -DENORMAL, 0.0]
    assert M.select_frame(r, 2, M.BY_RESPONSE) == [3, 2]                  # a denormal is above zero; equal magnitudes: the higher index
    assert M.select_frame(r, 4, M.BY_RESPONSE) == [3, 2, 4, 1]            # -0.0 equals 0.0: index decides
    assert M.select_frame(r, 3, M.KEEP_ORDER) == [2, 3, 4]


def test_the_cut_sizes():
    r = [5.0, 1.0, 4.0, 2.0, 3.0]
    assert M.select_frame(r, 5, M.BY_RESPONSE) == [0, 1, 2, 3, 4]         # n == max: not cut, and NOT sorted
    assert M.select_frame(r, 4, M.BY_RESPONSE) == [0, 2, 4, 3]            # n == max + 1
    assert M.select_frame(r, 4, M.KEEP_ORDER) == [0, 2, 3, 4]
    assert M.select_frame(r, 1, M.BY_RESPONSE) == [0] and M.select_frame(r, 1, M.KEEP_ORDER) == [0]
    for order in (M.KEEP_ORDER, M.BY_RESPONSE):
        assert M.select_frame(r, 0, order) == [0, 1, 2, 3, 4] and M.select_frame(r, -3, order) == [0, 1, 2, 3, 4]
        assert M.select_frame([], 3, order) == []
    assert M.select_frame(r, 7, M.BY_RESPONSE) == [0, 1, 2, 3, 4]         # a frame that is not cut keeps its own order


def _grid_frame(points, response=None):
    n = len(points)
    return np.arange(1, n + 1, dtype=np.float32) if response is None else np.asarray(response, np.float32), np.asarray(points, np.float32)


def test_grid_cells_keep_their_strongest():
    # 2 x 2 cells of 50 x 50 pixels on 100 x 100, max 4 -> perCell 1.  Cell (0,0) holds 3, (0,1) holds 1 (exactly perCell), (1,1) holds 2
    # (perCell + 1), (1,0) is empty.
    r, p = _grid_frame([(10, 10), (20, 20), (30, 30), (60, 10), (60, 60), (70, 70)], [1, 3, 2, 1, 5, 5])
    assert M.select_frame(r, 4, M.KEEP_ORDER, (2, 2), (100, 100), p) == [1, 3, 5]     # equal responses in (1,1): index 5 beats 4
    # perCell == 0 (max 3 over 4 cells): the inner call's maxKeypoints > 0 fails, every cell stays whole
    assert M.select_frame(r, 3, M.KEEP_ORDER, (2, 2), (100, 100), p) == [0, 1, 2, 3, 4, 5]
    # the whole-frame early exit comes first: n <= max selects everything, even what the grid could not place
    outside = np.array([(10, 10), (150, 10)], np.float32)
    assert M.select_frame([1, 2], 2, M.KEEP_ORDER, (2, 2), (100, 100), outside) == [0, 1]
    assert M.select_frame([1, 2], 0, M.KEEP_ORDER, (2, 2), (1, 1), outside) == [0, 1]
    with pytest.raises(M.Refused):
        M.select_frame(r, 4, M.BY_RESPONSE, (2, 2), (100, 100), p)                    # no compacting grid variant


def test_truncation_at_a_cell_edge_and_below_zero():
    assert M.cell_of((49.99, 50.0), (100, 100), (2, 2)) == (1, 0)         # int(49.99) = 49 -> col 0; int(50.0) = 50 -> row 1
    assert M.cell_of((-0.5, -0.99), (100, 100), (2, 2)) == (0, 0)         # int(-0.5) = 0
    assert M.cell_of((-1.5, 0.0), (100, 100), (2, 2)) == (0, 0)           # -1 / 50 = 0 in C: still column 0
    assert M.cell_of((-50.0, 0.0), (100, 100), (2, 2)) is None            # -50 / 50 = -1
    assert M.cell_of((float("nan"), 0.0), (100, 100), (2, 2)) == (0, 0)
    # 640 x 480 over 3 x 5: cells of 128 x 160, 640 divides, 480 divides; 641 x 482 leaves a strip
    assert M.cell_of((639.9, 479.9), (640, 480), (3, 5)) == (2, 4)
    assert M.cell_of((640.0, 10.0), (641, 482), (3, 5)) is None           # the remainder strip: col 640 / 128 = 5
    assert M.cell_of((10.0, 480.0), (641, 482), (3, 5)) is None           # row 480 / 160 = 3
    r, p = _grid_frame([(10, 10), (20, 20), (640, 10), (30, 30)])
    with pytest.raises(M.Refused):
        M.select_frame(r, 3, M.KEEP_ORDER, (3, 5), (641, 482), p)         # the reference asserts, the host entry refuses
    assert M.select_frame(r, 3, M.KEEP_ORDER, (3, 5), (641, 482), p, device=True) == [0, 1, 3]   # perCell 0; the strip's point is never selected
    with pytest.raises(M.Refused):
        M.select_frame(r, 3, M.KEEP_ORDER, (3, 5), (5, 482), p)           # width <= grid_cols


def test_nan_is_refused_on_the_host_and_ordered_by_its_bits_on_the_device():
    r = np.array([1.0, np.nan, np.inf, 2.0], np.float32)
    with pytest.raises(M.Refused):
        M.select_frame(r, 2, M.BY_RESPONSE)
    with pytest.raises(M.Refused):
        M.select_frame(r, 9, M.BY_RESPONSE)
    assert M.select_frame(r, 2, M.BY_RESPONSE, device=True) == [1, 2]
    assert M.select_frame(r, 3, M.KEEP_ORDER, device=True) == [1, 2, 3]


def test_expansion():
    # codes with a first id: -(k+1) -> first + k; an id stands; id 0 is no word
    np.testing.assert_array_equal(M.expand_frame(6, [0, 2, 3, 5], [7, -1, 0, -2], 100), [7, -1, 100, -2, -3, 101])
    # without a first id a code is no word
    np.testing.assert_array_equal(M.expand_frame(6, [0, 2, 3, 5], [7, -1, 0, -2], 0), [7, -1, -2, -3, -4, -5])
    np.testing.assert_array_equal(M.expand_frame(6, [0, 2, 3, 5], [7, -1, 0, -2], -4), [7, -1, -2, -3, -4, -5])
    np.testing.assert_array_equal(M.expand_frame(4, [], [], 5), [-1, -2, -3, -4])                 # count == 0: the _badSignRatio list
    np.testing.assert_array_equal(M.expand_frame(3, [2, 0, 1], [4, 5, 6]), [5, 6, 4])              # count == n: nothing negative
    with pytest.raises(M.Refused):
        M.expand_frame(3, [3], [4])
    np.testing.assert_array_equal(M.expand_frame(3, [3, -1, 1], [4, 4, 9], device=True), [-1, 9, -2])
    np.testing.assert_array_equal(M.expand_batch([0, 3, 3, 5], [1, 0, 2], [1, 0, 0, 1, 0], [-1, 0, 0, 8, 0], [50, 0, 0]), [-1, 50, -2, -1, 8])


# ---------------------------------------------------------------------------------------------------------------- the host mirror
def _mirror_select(frame, max_features, grid):
    from rtabmap_amd import vwdictionary as V
    mask = V.limit_keypoints(frame["response"], frame.get("points"), max_features, frame.get("image_size", (0, 0)), *grid)
    return None if mask is None else np.flatnonzero(mask).tolist()


def test_host_mirror_equals_the_model():
    """FeatureSelect::limitKeypoints (both forms) and expandWordIds through the Python wrapper, over the generators' frames"""
    from rtabmap_amd import vwdictionary as V
    rng = np.random.default_rng(5)
    frames = [I.tied_frame(rng, n) for n in (0, 1, 2, 63, 64, 65, 257, 1000)] + [I.cut_in_tie_frame(rng, 300, 100), I.all_equal_frame(200)]
    for f in frames:
        n = len(f["response"])
        for mx in sorted({-1, 0, 1, 2, 64, 100, 500, max(n - 1, 1), n, n + 1}):
            assert _mirror_select(f, mx, (1, 1)) == M.select_frame(f["response"], mx, M.KEEP_ORDER), (n, mx)
            assert V.limit_keypoints_compact(f["response"], mx).tolist() == M.select_frame(f["response"], mx, M.BY_RESPONSE), (n, mx)
    for grid, size in I.GRIDS:
        for mx in (16, 50, 200):
            g = I.grid_frame(rng, 600, size, grid, mx)
            assert _mirror_select(g, mx, grid) == M.select_frame(g["response"], mx, M.KEEP_ORDER, grid, size, g["points"]), (grid, size, mx)
    # refusals: NaN, the remainder strip, an image not larger than the grid; the early exit looks at none of them
    bad = I.grid_frame(rng, 100, (641, 482), (3, 5), 30)
    bad["points"][7] = (640.5, 10.0)
    assert _mirror_select(bad, 30, (3, 5)) is None and _mirror_select(bad, 100, (3, 5)) == list(range(100))
    assert V.limit_keypoints([1.0, float("nan"), 2.0], None, 1) is None and V.limit_keypoints_compact([1.0, float("nan")], 1) is None
    assert V.limit_keypoints([1.0, 2.0, 3.0], [(0, 0)] * 3, 2, (5, 100), 2, 5) is None
    for n in (0, 1, 64, 500):
        e = I.expansion_frame(rng, n)
        for first in (0, 1000):
            np.testing.assert_array_equal(V.expand_word_ids(n, e["index"], e["word_ids"], first), M.expand_frame(n, e["index"], e["word_ids"], first))
    assert V.expand_word_ids(3, [3], [5]) is None and V.expand_word_ids(3, [-1], [5]) is None
