"""The rule of lcd_track_flow without a GPU: the host mirror (rtabmap_amd/host/FlowTrack.cpp) against tests/flow_track_model.py bit for
bit on every generator, the four wrong variants told from the rule, the single-property inputs proven to reach their branches, the keep
rule on its bounds, and the ABI of the new structs."""
import ctypes
import os
import re

import numpy as np
import pytest

import flow_track_inputs as I
import flow_track_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("x_only", "row_major", "osc_x", "stop_float")


def _mirror(c, as_device=True):
    from rtabmap_amd import vwdictionary as V
    pr = c["pair"]
    return V.flow_track_cpu(pr["from"], pr["to"], c["points"], c["P"], pr["max_level"], c["initial"] if pr["use_initial"] else None, width=pr["width"],
                            as_device=as_device)


def _assert_mirror(c, what=""):
    pr = c["pair"]
    want = M.run_pair(pr, c["points"], c["P"], c["initial"], device=True)
    got = _mirror(c)
    np.testing.assert_array_equal(got["status"], want["status"], err_msg=what)
    np.testing.assert_array_equal(I.bits(got["track"]), I.bits(want["track"]), err_msg=what)
    np.testing.assert_array_equal(I.bits(got["err"]), I.bits(want["err"]), err_msg=what)
    assert got["kept"].tolist() == want["kept"], what
    return want


def _traces(c, variant=None):
    levels = M.cached_levels(c["P"], c["pair"])
    out = []
    for k, pt in enumerate(c["points"]):
        tr = {}
        res = M.track(levels, c["P"], pt, None if not c["pair"]["use_initial"] else c["initial"][k], variant, tr)
        out.append((tr, res))
    return out


def test_abi_of_the_new_structs():
    from rtabmap_amd import capi
    assert ctypes.sizeof(capi.LcdFlowPair) == 48 and ctypes.sizeof(capi.LcdFlowParams) == 40 and ctypes.sizeof(capi.LcdTrackFlowArgs) == 128
    src = open(os.path.join(ROOT, "rtabmap_amd", "csrc", "flow_track.hip")).read()
    assert re.search(r"static_assert\(sizeof\(lcd_track_flow_args\) == 128\b", src)
    assert "gather_kept_rows" in src and "block_rank(keep" in src and "stereo_pyramid_kernel" in src and "__syncthreads" not in src.split("flow_keep_kernel")[0]
    rule = open(os.path.join(ROOT, "rtabmap_amd", "csrc", "flow_track_rule.h")).read()
    assert '#include "stereo_flow_rule.h"' in rule and "fp contract(off)" in rule and "reflect101(int" not in rule      # shared, not copied
    L = capi.load()
    assert L.lcd_track_flow and L.lcd_track_flow_dev
    fp = capi.flow_params()
    assert (fp.win_width, fp.win_height, fp.iterations, fp.eps, fp.use_min_eigenvals, fp.min_eig_threshold, fp.error_threshold) == (16, 16, 30, 0.01, 1, 1e-4, 20.0)


def test_lane_tree_sum_is_the_engines_order():
    """against a plain statement of rtabmap_amd/host/LaneSum.h's laneTreeSum<64>, on lengths around the passes; and not the row-major chain"""
    rng = np.random.default_rng(0)
    differs = 0
    for n in (1, 9, 63, 64, 65, 128, 256, 961):
        t = (rng.integers(-2000, 2000, n) * rng.integers(-2000, 2000, n)).astype(np.int32)
        part = [np.float32(0)] * 64
        for i in range(n):
            part[i % 64] = part[i % 64] + np.float32(t[i])
        s = 32
        while s >= 1:
            for l in range(s):
                part[l] = part[l] + part[l + s]
            s //= 2
        assert (I.bits(M.lane_tree_sum(t)) == I.bits(part[0])).all()
        differs += int((I.bits(M.lane_tree_sum(t)) != I.bits(M.S.ordered_sum(t))).any())
    assert differs >= 1


@pytest.mark.parametrize("max_level,use_initial", [(0, 0), (3, 0), (2, 1), (0, 1)])
@pytest.mark.parametrize("width,height,win_w,win_h", I.SHAPES)
def test_host_mirror_equals_the_model(width, height, win_w, win_h, max_level, use_initial):
    rng = np.random.default_rng(width + win_w + max_level)
    tracked = 0
    for pad in (0, 5):
        pr, pts, ini = I.random_pair(rng, width, height, 120, win_w, win_h, pad=pad, max_level=max_level, use_initial=use_initial)
        for mode in (1, 0):
            P = M.params(win_width=win_w, win_height=win_h, use_min_eigenvals=mode, error_threshold=2.0)
            tracked += int(_assert_mirror(I.case(pr, pts, P, ini), what=str((pad, mode)))["status"].sum())
    assert tracked > 150


def test_host_mirror_on_the_single_property_inputs():
    for k, c in enumerate(I.all_cases(np.random.default_rng(5))):
        _assert_mirror(c, what="case %d" % k)


def test_each_wrong_variant_differs_from_the_rule_on_some_generator():
    """... so the GPU tests, which run the same generators, tell a kernel that implements a variant from one that implements the rule"""
    cases = I.all_cases(np.random.default_rng(5))                         # exactly what test_gpu_flow_track.py's test_single_property_inputs runs
    told = {v: 0 for v in VARIANTS}
    for c in cases:
        want = M.run_pair(c["pair"], c["points"], c["P"], c["initial"], device=True)
        for v in VARIANTS:
            got = M.run_pair(c["pair"], c["points"], c["P"], c["initial"], device=True, variant=v)
            told[v] += int(not (np.array_equal(I.bits(got["track"]), I.bits(want["track"])) and np.array_equal(got["status"], want["status"]) and
                                np.array_equal(I.bits(got["err"]), I.bits(want["err"]))))
    assert all(told[v] >= 1 for v in VARIANTS), told


def test_the_single_property_inputs_reach_their_branches():
    rng = np.random.default_rng(5)
    ex = I.exit_cases(rng)
    exits = {name: [tr[0][-1] for tr, _ in _traces(c)] for name, c in ex.items()}
    assert exits["cap"].count("cap") >= 20 and exits["eps"].count("eps") >= 20 and exits["oscillation"].count("oscillation") >= 5
    lv = I.leaving_case(rng)
    tr = _traces(lv)
    assert sum(1 for t, r in tr if t[0] and t[0][-1] == "next_outside" and r[1] == 0) >= 3          # leaving at level 0: status 0
    assert sum(1 for t, r in tr if any(t[l] and t[l][-1] == "next_outside" for l in (1, 2, 3) if l in t) and ("origin" in [e[0] for e in t[0] if isinstance(e, tuple)])) >= 3
    g = I.eigen_gate_cases(rng)
    t0, t1, t2 = (_traces(c)[0] for c in g)
    assert "eig_fail" not in t0[0][0] and t0[1][1] == 1
    assert "eig_fail" in t1[0][0] and t1[1][1] == 0
    assert "eig_fail" in t2[0][1] and "eig_fail" not in t2[0][0] and t2[1][1] == 1                     # the gate closes above level 0 only
    f0, f1 = I.flat_case(rng)
    assert all("det_fail" in t[0] and r[1] == 0 for t, r in _traces(f0)) and all("eig_fail" in t[0] and r[1] == 0 for t, r in _traces(f1))
    assert all(("weights", 2.0 ** -15, 2.0 ** -15) in t[0] for t, _ in _traces(I.tie_case(rng)))
    b = I.border_origin_case(rng)
    origins = [e[1:] for t, _ in _traces(b) for e in t[0] if isinstance(e, tuple) and e[0] == "origin"]
    assert any(o[0] == -5 for o in origins) and any(o[0] == 39 for o in origins) and any(o[1] == -3 for o in origins) and any(o[1] == 23 for o in origins)
    assert sum(1 for t, _ in _traces(b) if t[0] == ["prev_outside"]) >= 4
    kb = I.keep_bound_case(rng)
    fr = M.run_pair(kb["pair"], kb["points"], kb["P"], kb["initial"])
    assert fr["status"].all() and np.array_equal(I.bits(fr["track"]), I.bits(kb["initial"]))            # iterations = 0: the corner stays on the bound
    assert fr["kept"] == [1, 2, 3, 6, 7, 8, 10]
    e20, e0, eq, above = I.error_mode_cases(rng)
    full = M.run_pair(e20["pair"], e20["points"], e20["P"])
    assert len(full["kept"]) > 30 and M.run_pair(e0["pair"], e0["points"], e0["P"])["kept"] == []
    one = M.run_pair(eq["pair"], eq["points"], eq["P"])
    assert one["status"].tolist() == [1] and np.float32(eq["P"]["error_threshold"]) == one["err"][0] and one["kept"] == []
    assert M.run_pair(above["pair"], above["points"], above["P"])["kept"] == [0]
    for c in I.initial_cases(rng):
        fr = M.run_pair(c["pair"], c["points"], c["P"], c["initial"])
        plain = M.run_pair(I.with_(c["pair"], use_initial=0), c["points"], c["P"])
        assert not np.array_equal(I.bits(fr["track"]), I.bits(plain["track"])) and 10 < len(fr["kept"]) < 50
    cut = I.level_cut_case(rng)
    assert len(M.cached_levels(cut["P"], cut["pair"])) == 2


def test_keep_rule_on_its_bounds():
    P = M.params(use_min_eigenvals=0, error_threshold=20.0)
    lo = np.nextafter(np.float32(0), np.float32(-1))
    for to, status, err, want in (((40.0, 5.0), 1, 1.0, False), ((np.nextafter(np.float32(40), np.float32(0)), 5.0), 1, 1.0, True), ((0.0, 0.0), 1, 1.0, True),
                                  ((-0.0, -0.0), 1, 1.0, True), ((lo, 5.0), 1, 1.0, False), ((5.0, 24.0), 1, 1.0, False), ((5.0, lo), 1, 1.0, False),
                                  ((np.nan, 5.0), 1, 1.0, False), ((5.0, np.nan), 1, 1.0, False), ((np.inf, 5.0), 1, 1.0, False), ((5.0, 5.0), 0, 1.0, False),
                                  ((5.0, 5.0), 1, 20.0, False), ((5.0, 5.0), 1, np.nextafter(np.float32(20), np.float32(0)), True), ((5.0, 5.0), 1, np.nan, False)):
        assert M.keep(P, to, status, np.float32(err), 40, 24) == want, (to, status, err)
    assert M.keep(M.params(), (5.0, 5.0), 1, np.float32(1e9), 40, 24)                                  # minEig mode: the error gates nothing


def test_host_mirror_refuses_what_the_engine_refuses():
    from rtabmap_amd import vwdictionary as V
    rng = np.random.default_rng(2)
    pr, pts, ini = I.random_pair(rng, 64, 48, 5)
    f, t = pr["from"], pr["to"]
    for pt in I.wild_points():
        assert V.flow_track_cpu(f, t, [pt]) is None
        assert V.flow_track_cpu(f, t, pts[:1], initial=[pt]) is None
        with pytest.raises(M.Refused):
            M.run_pair(pr, [pt])
        got = V.flow_track_cpu(f, t, [pt], as_device=True)
        assert got["status"].tolist() == [0] and np.isnan(got["track"]).all() and got["kept"].tolist() == [] and got["err"].tolist() == [0.0]
        assert M.run_pair(pr, [pt], device=True)["status"].tolist() == [0]
    for change in (dict(win_width=2), dict(win_height=32), dict(win_width=64), dict(eps=float("nan")), dict(error_threshold=float("nan"))):
        assert V.flow_track_cpu(f, t, pts, change) is None, change
        with pytest.raises(M.Refused):
            M.run_pair(pr, pts, M.params(**change))
    for ml in (-1, 9):
        assert V.flow_track_cpu(f, t, pts, max_level=ml) is None
        with pytest.raises(M.Refused):
            M.run_pair(I.with_(pr, max_level=ml), pts)
    assert V.flow_track_cpu(f, t, np.zeros((0, 2), np.float32))["track"].shape == (0, 2)
    # the clamps of the stereo rule: 150 iterations are 100, eps 20 is 10, negative ones are 0
    for a, b in ((dict(iterations=150, eps=0.0), dict(iterations=100, eps=0.0)), (dict(eps=20.0), dict(eps=10.0)), (dict(iterations=-3), dict(iterations=0)),
                 (dict(eps=-1.0, iterations=3), dict(eps=0.0, iterations=3))):
        np.testing.assert_array_equal(I.bits(M.run_pair(pr, pts, M.params(**a))["track"]), I.bits(M.run_pair(pr, pts, M.params(**b))["track"]))
        _assert_mirror(I.case(pr, pts, M.params(**a)))
