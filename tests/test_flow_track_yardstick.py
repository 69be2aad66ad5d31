"""The accuracy of lcd_track_flow's rule against an independent float64 tracker (tests/flow_track_yardstick.py), without a GPU."""
import numpy as np

import flow_track_model as M
import flow_track_yardstick as Y


def test_accuracy_against_the_float64_yardstick():
    """Smooth random textures resampled at a known 2-D shift (integer and fractional, both axes, 64 x 48 and 160 x 120), the points more than
    the window from the border, the reference's defaults (16 x 16, three levels).  The yardstick's largest error against the truth is
    recorded in DESIGN.md 4u: 0.0433 pixels, at the shift (-2.6, 1.8) on 160 x 120; the rule's is 0.0432 there, and both trackers keep every
    point of every scene.  The yardstick's own error stays within 0.5 .. 1.25 of the recorded value; the rule's largest error over the points
    both trackers keep stays within 4 x the recorded value; a texture counts only if the yardstick keeps at least 95 % of its points."""
    worst_yardstick = worst_rule = 0.0
    for width, height, shift in Y.SCENES:
        a, b, pts, truth = Y.scene(width, height, shift)
        q, kept = Y.track(a, b, pts)
        assert kept.mean() >= 0.95
        fr = M.run_pair(M.pair(a, b, width, 3), pts, M.params())
        tracked = np.zeros(len(pts), bool)
        tracked[fr["kept"]] = True
        both = kept & tracked
        ey = float(np.linalg.norm(q - truth, axis=1)[kept].max())
        er = float(np.linalg.norm(fr["track"].astype(np.float64) - truth, axis=1)[both].max())
        print("%d x %d shift %s: yardstick %.6f kept %.3f, rule %.6f kept %.3f" % (width, height, shift, ey, kept.mean(), er, tracked.mean()))
        assert both.sum() >= 0.9 * len(pts)
        worst_yardstick, worst_rule = max(worst_yardstick, ey), max(worst_rule, er)
    print("yardstick %.6f rule %.6f recorded %.4f" % (worst_yardstick, worst_rule, Y.YARDSTICK_ERROR))
    assert 0.5 * Y.YARDSTICK_ERROR <= worst_yardstick <= 1.25 * Y.YARDSTICK_ERROR
    assert worst_rule <= Y.FACTOR * Y.YARDSTICK_ERROR
