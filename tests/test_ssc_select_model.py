"""The LCD_SELECT_SSC rule without a GPU: the scalars by hand, the tie rule, and the host mirror (rtabmap_amd/host/FeatureSelect.cpp through
the host library) against tests/ssc_select_model.py on every generator, in both output orders, with the refusals."""
import numpy as np
import pytest

import ssc_select_inputs as I
import ssc_select_model as M


# max_features, (width, height) -> m, high, Kmin, Kmax.  By hand, (640, 480):
#   2:   2 * 0.1f = 0.2f -> round 0, m = 2; exp1 = 1124, exp2 = 2489608, sqrt = 1577.849..; -(1124 - 1577.849..) / 1 = 453.849.. -> 454;
#        2 -+ 0.2f = 1.8f, 2.2f -> 2, 2
#   5:   5 * 0.1f is the float 0.5 exactly -> round 1 (away from zero), m = 4; exp2 = 4951056, sqrt = 2225.096..; 1097.096.. / 3 = 365.69..
#        -> 366; 4 -+ 0.4f = 3.6f, 4.4f -> 4, 4
#   15:  15 * 0.1f is the float 1.5 exactly -> round 2, m = 13; exp2 = 16027572, sqrt = 4003.445..; 2857.445.. / 12 = 238.12.. -> 238;
#        13 -+ 1.3000001f = 11.7f, 14.3f -> 12, 14
#   500: 50 -> m = 450; exp2 = 553853960, sqrt = 23534.102..; 21514.102.. / 449 = 47.915.. -> 48; 450 -+ 45 = 405, 495
SCALARS = [
    (2, (640, 480), (2, 454, 2, 2)), (5, (640, 480), (4, 366, 4, 4)), (15, (640, 480), (13, 238, 12, 14)), (500, (640, 480), (450, 48, 405, 495)),
    (2, (33, 17), (2, 17, 2, 2)), (5, (33, 17), (4, 13, 4, 4)), (15, (33, 17), (13, 8, 12, 14)), (500, (33, 17), (450, 0, 405, 495)),
]


@pytest.mark.parametrize("mx,size,want", SCALARS)
def test_scalars_by_hand(mx, size, want):
    assert M.scalars(mx, *size) == want


def test_low_by_hand():
    assert [M.low_of(n, 13) for n in (16, 51, 52, 116, 117, 8192)] == [1, 1, 2, 2, 3, 25]      # 52 / 13 = 4, 117 / 13 = 9
    assert M.low_of(1000, 450) == 1 and M.low_of(1800, 450) == 2


def _hand_frame():
    """seven features on a 20 x 20 image, max 6 -> m = 6 - round(0.6f) = 5, Kmin = round(4.5f) = 5, Kmax = round(5.5f) = 6; exp1 = 50, exp2 =
    80 + 20 + 400 + 400 + 400 - 800 + 8000 = 8500, sqrt = 92.19..; (50 - 92.19..) / 4 = -10.5.. -> high = 11; low = max(1, floor(sqrt(7 / 5))) = 1.
    The order by response is A B C D E F G.
    width 6 (1 + 10 / 2, c = 3): cells (row, col) A (0,0), B (0,1), C (0,2), D (3,3), E (6,6), F (6,0), G (0,0).  A selected; B, C within 2
      columns of A; D three rows and columns from A; E three from D; F six columns from E, three rows from D; G in A's cell -> 4 < Kmin: high = 5.
    width 3 (1 + 4 / 2, c = 1.5): A (0,0), B (0,3), C (0,5), D (6,6), E (13,13), F (12,0), G (1,1).  A; B three columns away: selected; C two
      columns from B: covered; D, E, F; G beside A: covered -> 5: found."""
    pts = np.array([(1, 1), (5, 1), (8, 1), (10, 10), (20, 20), (1, 19), (2, 2)], np.float32)
    resp = np.array([6, 5, 4, 3, 2, 1, 0.5], np.float32)
    return dict(response=resp, points=pts, image_size=(20, 20))


def test_hand_made_frame():
    f = _hand_frame()
    assert M.scalars(6, 20, 20) == (5, 11, 5, 6)
    tr = {}
    kept = M.select_frame(f["response"], 6, M.BY_RESPONSE, f["image_size"], f["points"], trace=tr)
    assert (tr["widths"], tr["sizes"], tr["exit"], tr["low"]) == ([6, 3], [4, 5], "found", 1)
    assert kept == [0, 1, 3, 4, 5]


def test_tie_rule():
    """equal responses go by the lower index; -0.0 is +0.0; the order is by the SIGNED response"""
    r = np.array([1.0, -3.0, 1.0, 0.0, -0.0, 2.0, -0.0, 0.0, I.DENORMAL, -I.DENORMAL], np.float32)
    assert M.order_of(r) == [5, 0, 2, 8, 3, 4, 6, 7, 9, 1]
    # all in one cell but two: among equal responses the lower index is the one selected
    f = _hand_frame()
    f["response"] = np.ones(7, np.float32)
    assert M.select_frame(f["response"], 6, M.BY_RESPONSE, f["image_size"], f["points"]) == [0, 1, 3, 4, 5]
    f["points"][:] = f["points"][::-1].copy()                             # G F E D C B A: at width 3 C comes before B now and covers it, G covers A
    assert M.select_frame(f["response"], 6, M.BY_RESPONSE, f["image_size"], f["points"]) == [0, 1, 2, 3, 4]


def _mirror(f, mx, order):
    from rtabmap_amd import vwdictionary as V
    if order == M.BY_RESPONSE:
        got = V.limit_keypoints_compact(f["response"], mx, points=f["points"], image_size=f["image_size"], ssc=True)
        return None if got is None else got.tolist()
    got = V.limit_keypoints(f["response"], f["points"], mx, f["image_size"], ssc=True)
    return None if got is None else np.flatnonzero(got).tolist()


@pytest.mark.parametrize("order", [M.KEEP_ORDER, M.BY_RESPONSE])
def test_mirror_equals_the_model_on_every_generator(order):
    frames = [I.named(nm[0]) for nm in I.NAMED] + [(_hand_frame(), 6), (_hand_frame(), 7), (_hand_frame(), 0), (_hand_frame(), 2)]
    rng = np.random.default_rng(3)
    for seed in range(12):
        size = I.SIZES[seed % len(I.SIZES)]
        n = int(rng.integers(3, 400))
        frames.append(((I.uniform_frame, I.integer_frame, I.clustered_frame)[seed % 3](rng, n, size), int(rng.integers(2, n + 3))))
    for k, (f, mx) in enumerate(frames):
        assert _mirror(f, mx, order) == M.select_frame(f["response"], mx, order, f["image_size"], f["points"]), "frame %d" % k


def test_mirror_refusals():
    from rtabmap_amd import vwdictionary as V
    f = _hand_frame()
    for order in (M.KEEP_ORDER, M.BY_RESPONSE):
        assert _mirror(f, 1, order) is None                                                    # max_features == 1
        for size in ((0, 20), (20, 0), (16385, 20), (20, 16385)):
            assert _mirror(dict(f, image_size=size), 5, order) is None
        for bad in ((-0.5, 1.0), (1.0, -1e-40), (20.5, 1.0), (1.0, 21.0), (np.nan, 1.0), (1.0, np.inf)):
            g = dict(f, points=f["points"].copy())
            g["points"][2] = bad
            assert _mirror(g, 5, order) is None, bad
            with pytest.raises(M.Refused):
                M.select_frame(g["response"], 5, order, g["image_size"], g["points"])
            assert _mirror(g, 7, order) == list(range(7))                                      # not cut: nothing is looked at
        g = dict(f, response=f["response"].copy())
        g["response"][1] = np.nan
        assert _mirror(g, 5, order) is None
    assert V.limit_keypoints(f["response"], f["points"], 5, f["image_size"], grid_rows=2, grid_cols=2, ssc=True) is None
    assert V.limit_keypoints_compact(f["response"], 5, points=None, image_size=f["image_size"], ssc=True) is None
    with pytest.raises(M.Refused):
        M.select_frame(f["response"], 1, M.KEEP_ORDER, f["image_size"], f["points"])


def test_device_definitions_in_the_model():
    """a feature whose cell is outside an iteration's mask is not selected in it and covers nothing; NaN responses are ordered by their bits"""
    f = _hand_frame()
    f["points"][0] = (-1.0, 1.0)                                          # A leaves.  width 6: B, D, E, F (C and G beside B); width 3: the same four
    tr = {}                                                               # (G two columns from B); width 1: cells far apart, all six -> found
    kept = M.select_frame(f["response"], 6, M.BY_RESPONSE, f["image_size"], f["points"], device=True, trace=tr)
    assert (tr["widths"], tr["sizes"]) == ([6, 3, 1], [4, 4, 6]) and kept == [1, 2, 3, 4, 5, 6]
    r = np.array([1.0, np.nan, -np.nan, np.inf, -np.inf], np.float32)
    assert M.order_of(r) == [1, 3, 0, 4, 2]
