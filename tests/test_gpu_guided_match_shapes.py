"""GPU tests of lcd_match_guided at the code's own boundaries (rtabmap_amd/csrc/guided_match.hip): the candidate list's drain at 64 entries,
a window that holds every target, the 8192-row limit, points at exactly the radius, the arithmetic without fused multiply-add, ties, the
ratios 0 / 0.8 / 1, the first-come rule under full contention, NaN points, out-of-range corners on the device entry, and the error table.
Inputs and their properties: tests/guided_match_inputs.py (asserted without a GPU in tests/test_guided_match_inputs.py)."""
import ctypes as C

import numpy as np
import pytest

import guided_match_inputs as I
import guided_match_model as M

pytestmark = pytest.mark.gpu

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
COMBOS = [(d, n) for d in (M.P2F, M.F2P) for n in (M.RATIO, M.NEAREST)]


def _both(eng, oracle, pairs, what, **kw):
    """host and device entry against the model"""
    kw.setdefault("radius", I.RADIUS)
    kw.setdefault("nndr", 0.8)
    kw.setdefault("nn_type", M.RATIO)
    kw.setdefault("direction", M.P2F)
    exp = I.expected_batch(oracle, pairs, kw["radius"], kw["nndr"], kw["nn_type"], kw["direction"])
    I.assert_same(I.run_dev(eng, pairs, **kw), exp, what + " dev")
    I.assert_same(I.run_host(eng, pairs, **kw), exp, what + " host")
    return exp


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("f32", 128), ("f32", 96), ("u8", 32), ("u8", 48)])
def test_windows_of_63_64_65_128_129_candidates(oracle, dtype, dim):
    import rtabmap_amd
    eng = rtabmap_amd.Engine(dtype, dim)
    for direction, nn_type in COMBOS:
        pair = I.window_case(oracle, dtype, dim, direction)
        exp = _both(eng, oracle, [pair], direction, nn_type=nn_type, direction=direction)
        assert exp["count"].tolist() == I.WINDOW_COUNTS
        assert sorted(set(I.best_behind_first_drain(oracle, pair, direction))) == [False, True]
    eng.close()


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_a_radius_that_covers_every_target(oracle, dtype, dim):
    import rtabmap_amd
    pair = I.general_case(oracle, dtype, dim, 1100, 1100, 1100)
    eng = rtabmap_amd.Engine(dtype, dim)
    for direction in (M.P2F, M.F2P):
        exp = _both(eng, oracle, [pair], direction, radius=1000.0, direction=direction)
        assert (exp["count"] >= 1098).sum() >= 1098                       # everything but the points planted far outside the image
    eng.close()


def test_8192_rows_on_every_side_and_the_limit(oracle):
    """one pair at 8192 x 8192 x 8192, radius 40 (about 126 candidates per window); 8193 on any side is refused, nothing written"""
    import rtabmap_amd
    from rtabmap_amd import capi
    pair = I.general_pair("f32", 64, 8192, 8192, 8192, 5)
    eng = rtabmap_amd.Engine("f32", 64)
    exp = I.expected_batch(oracle, [pair], I.RADIUS, 0.8, M.RATIO, M.P2F)
    assert M.outcomes(exp, M.P2F) == I.ALL_OUTCOMES and exp["count"].max() > 128
    I.assert_same(I.run_dev(eng, [pair]), exp, "dev")
    I.assert_same(I.run_host(eng, [I.swapped(pair)], direction=M.F2P, with_dist=False), dict(exp, owner=None), "host, roles exchanged")
    big, pts, rows = np.zeros((8193, 64), np.float32), np.zeros((8193, 2), np.float32), np.zeros(8193, np.int32)
    small = (big[:4], big[:4], pts[:4], rows[:4], pts[:4])
    over = [(big, big[:4], pts[:4], rows[:4], pts[:4]),                   # 8193 from-rows, to-rows, corners
            (big[:4], big, pts[:4], rows[:4], pts),
            (big[:4], big[:4], pts, rows, pts[:4])]
    for k, p in enumerate(over):
        for direction in (M.P2F, M.F2P):
            for run in (I.run_host, I.run_dev):
                with pytest.raises(capi.LcdError) as err:
                    run(eng, [small, p], direction=direction)
                assert err.value.status == LCD_ERR_UNSUPPORTED, k
    I.assert_same(I.run_host(eng, [pair]), exp, "afterwards")
    eng.close()


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_points_at_exactly_the_radius_and_without_fma(oracle, dtype, dim):
    import rtabmap_amd
    eng = rtabmap_amd.Engine(dtype, dim)
    grid = I.grid_pair(dtype, dim, 1)
    exp = _both(eng, oracle, [grid], "grid", radius=5.0)
    assert exp["count"].tolist() == [3, 3, 3]
    assert _both(eng, oracle, [grid], "grid", radius=5.0, direction=M.F2P)["count"].tolist() == [0, 0, 0, 0, 0, 1, 1, 1] * 3
    pair = I.no_fma_case(dtype, dim)
    assert I.fma_matters(pair) > 0
    for direction in (M.P2F, M.F2P):
        _both(eng, oracle, [pair], "no fma " + direction, nn_type=M.NEAREST, direction=direction)
    eng.close()


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("f32", 61), ("u8", 32), ("u8", 48)])
def test_duplicated_descriptors_inside_windows(oracle, dtype, dim):
    import rtabmap_amd
    eng = rtabmap_amd.Engine(dtype, dim)
    pair = I.tie_pair(dtype, dim, 2)
    for p, direction in ((pair, M.P2F), (I.swapped(pair), M.F2P)):
        exp = _both(eng, oracle, [p], "ratio", nndr=1.0, direction=direction)
        assert I.ties(exp) == (6, 6) and (exp["match"] < 0).sum() >= 12   # d1 == d2 never passes, at zero either
        exp = _both(eng, oracle, [p], "nearest", nn_type=M.NEAREST, direction=direction)
        assert (exp["match"] >= 0).sum() >= 12
    eng.close()


@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("u8", 32)])
def test_ratios_0_08_and_1(oracle, dtype, dim):
    import rtabmap_amd
    pair = I.general_case(oracle, dtype, dim, 300, 280, 300)
    eng = rtabmap_amd.Engine(dtype, dim)
    for direction in (M.P2F, M.F2P):
        n = []
        for nndr in (0.0, 0.8, 1.0):
            exp = _both(eng, oracle, [pair], "nndr %g" % nndr, nndr=nndr, direction=direction)
            n.append(int(((exp["count"] >= 2) & (exp["match"] >= 0)).sum()))
        assert n[0] == 0 < n[1] < n[2]                                    # at 0 only single candidates match
    eng.close()


def test_every_corner_choosing_one_to_row_nan_points_and_a_permutation(oracle):
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", 64)
    one = I.one_row_pair("f32", 64, 4)
    exp = _both(eng, oracle, [one], "one row")
    assert (exp["match"] == 2).all() and exp["owner"].tolist() == [-1, -1, 0]
    assert (np.diff(one[3]) < 0).any()
    nan = I.nan_pair(oracle, "f32", 64)
    for direction in (M.P2F, M.F2P):
        exp = _both(eng, oracle, [nan, one], "nan " + direction, direction=direction)
        assert (exp["count"] == 0).sum() >= 40
    eng.close()


def test_the_device_entry_never_follows_a_from_row_out_of_range(oracle):
    """corner_from_row outside [0, nf): the host entry refuses the call, the device entry treats the corner as no candidate"""
    import rtabmap_amd
    from rtabmap_amd import capi
    frm, to, corners, cfr, pts = I.general_case(oracle, "f32", 64, 300, 280, 300)
    cfr = cfr.copy()
    cfr[0::9] = 300
    cfr[4::9] = -1
    cfr[7::27] = 1 << 30
    pair = (frm, to, corners, cfr, pts)
    eng = rtabmap_amd.Engine("f32", 64)
    for direction in (M.P2F, M.F2P):
        exp = I.expected_batch(oracle, [pair], I.RADIUS, 0.8, M.RATIO, direction)
        I.assert_same(I.run_dev(eng, [pair], direction=direction), exp, direction)
        with pytest.raises(capi.LcdError) as err:
            I.run_host(eng, [pair], direction=direction)
        assert err.value.status == LCD_ERR_INVALID
    bad = (cfr < 0) | (cfr >= 300)
    exp = I.expected_batch(oracle, [pair], I.RADIUS, 0.8, M.RATIO, M.P2F)
    assert (exp["count"][bad] == 0).all() and (exp["match"][bad] == -1).all() and (exp["count"][~bad] > 0).any()
    eng.close()


def test_errors_leave_nothing_written_and_the_handle_usable(oracle):
    import rtabmap_amd
    from rtabmap_amd import capi
    eng = rtabmap_amd.Engine("f32", 64)
    pair = I.general_case(oracle, "f32", 64, 33, 31, 65)
    frm, to, corners, cfr, pts = pair
    good = I.expected_batch(oracle, [pair], I.RADIUS, 0.8, M.RATIO, M.P2F)
    keep = []

    def call(entry="lcd_match_guided", n_pairs=1, fo=(0, 33), to_off=(0, 65), co=(0, 31), direction=0, nn_type=0, radius=40.0, size=None, null=(), rows=cfr):
        offs = [None if o is None else np.asarray(o, np.int64) for o in (fo, to_off, co)]
        outs = [np.full(128, -7, np.int32), np.full(128, -7, np.int32), np.full(256, -7.0, np.float32), np.full(128, -7, np.int32)]
        a = capi.LcdGuidedArgs(C.sizeof(capi.LcdGuidedArgs) if size is None else size, direction, nn_type, n_pairs, radius, 0.8)
        vals = dict(from_rows=frm, to_rows=to, corners=corners, corner_from_row=rows, to_points=pts, from_offsets=offs[0], to_offsets=offs[1],
                    corner_offsets=offs[2], out_count=outs[0], out_match=outs[1], out_dist=outs[2], out_to_owner=outs[3])
        keep.append(vals)
        for k, v in vals.items():
            setattr(a, k, None if v is None or k in null else v.ctypes.data)
        rc = getattr(eng.L, entry)(eng.h, C.byref(a))
        assert all((o == -7).all() for o in outs), "written"
        return rc

    bad_rows = cfr.copy()
    bad_rows[5] = 33
    cases = [
        (LCD_ERR_UNSUPPORTED, dict(n_pairs=65536)),
        (LCD_ERR_INVALID, dict(n_pairs=-1)),
        (LCD_ERR_INVALID, dict(fo=(1, 33))),                                             # offsets: not starting at 0, decreasing, missing
        (LCD_ERR_INVALID, dict(n_pairs=2, fo=(0, 33, 20), to_off=(0, 30, 65), co=(0, 10, 31))),
        (LCD_ERR_INVALID, dict(n_pairs=2, fo=(0, 20, 33), to_off=(0, 30, 65), co=(0, 31, 10))),
        (LCD_ERR_INVALID, dict(co=None)),
        (LCD_ERR_INVALID, dict(to_off=None)),
        (LCD_ERR_INVALID, dict(radius=float("nan"))),                                    # radius: not finite, zero, negative
        (LCD_ERR_INVALID, dict(radius=float("inf"))),
        (LCD_ERR_INVALID, dict(radius=0.0)),
        (LCD_ERR_INVALID, dict(radius=-40.0)),
        (LCD_ERR_INVALID, dict(size=112)),                                               # wrong struct_size / direction / nn_type
        (LCD_ERR_INVALID, dict(direction=2)),
        (LCD_ERR_INVALID, dict(nn_type=2)),
        (LCD_ERR_INVALID, dict(nn_type=-1)),
        (LCD_ERR_INVALID, dict(null=("from_rows",))),                                    # NULL where rows exist
        (LCD_ERR_INVALID, dict(null=("to_rows",))),
        (LCD_ERR_INVALID, dict(null=("corners",))),
        (LCD_ERR_INVALID, dict(null=("corner_from_row",))),
        (LCD_ERR_INVALID, dict(null=("to_points",))),
        (LCD_ERR_INVALID, dict(null=("out_count",))),
        (LCD_ERR_INVALID, dict(null=("out_match",))),
        (LCD_ERR_INVALID, dict(null=("out_to_owner",))),
        (LCD_ERR_INVALID, dict(rows=bad_rows)),                                          # host entry: a from-row outside [0, nf)
    ]
    for want, kw in cases:
        assert call(**kw) == want, kw
        assert eng.L.lcd_last_error(eng.h)
        I.assert_same(I.run_host(eng, [pair]), good, "usable after %r" % (kw,))
    assert call(n_pairs=0, fo=None, to_off=None, co=None) == 0                           # no pairs: LCD_OK, nothing touched
    for kw in (dict(size=112), dict(radius=0.0), dict(direction=2), dict(n_pairs=65536), dict(null=("out_match",))):
        assert call(entry="lcd_match_guided_dev", **kw) in (LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED), kw    # refused before any pointer is followed
    I.assert_same(I.run_dev(eng, [pair]), good, "usable")
    # a handle of a sharded vocabulary
    eng.set_option("shard_append", 1)
    for entry in ("lcd_match_guided", "lcd_match_guided_dev"):
        assert call(entry=entry) == LCD_ERR_UNSUPPORTED
    eng.close()
    # padded rows: the device entry refuses the handle, the host entry serves it
    pad = rtabmap_amd.Engine("u8", 5)
    p5 = I.general_case(oracle, "u8", 5, 33, 31, 65)
    with pytest.raises(capi.LcdError) as err:
        I.run_dev(pad, [p5])
    assert err.value.status == LCD_ERR_UNSUPPORTED
    I.assert_same(I.run_host(pad, [p5]), I.expected_batch(oracle, [p5], I.RADIUS, 0.8, M.RATIO, M.P2F), "padded host")
    pad.close()
