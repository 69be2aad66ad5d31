"""How the Gauss-Newton step count of lcd_estimate_motion_pnp's rule was chosen (profiles/motion_pnp.txt).  CPU only: the host
mirror's motion_pnp_cpu with its `steps` argument over the generators of tests/motion_pnp_inputs.py.

    python tools/motion_pnp_steps.py

Prints, for K = 1 .. 10, in how many of the calls the outputs (status, both id lists and their counts) with K steps differ from those with
K + 1 and with K + 2, then the smallest K that two more steps do not change and the rule's count, one more; and the largest difference between
an entry of the fp32 fit and of a float64 least-squares fit over the inlier sets, with the minimal solver's worst held-out reprojection."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import motion_pnp_inputs as I  # noqa: E402
import motion_pnp_model as M  # noqa: E402
from rtabmap_amd import vwdictionary as V  # noqa: E402


def calls():
    out = []
    base = dict(min_inliers=4, reproj_error=2.0, variance_median_ratio=4, max_variance=0.0)
    for pair in I.mixed_batch():
        for iterations in (1, 300):
            for refine in I.REFINE:
                out.append((pair, dict(base, iterations=iterations, refine_iterations=refine, seed=5)))
    for name in I.REFINE_CASES:
        pair, kw = I.refine_case(name)
        out.append((pair, dict(base, **kw)))
    out.append((I.all_outlier_pair(), dict(base, iterations=300, refine_iterations=5, seed=3)))
    rng = np.random.default_rng(77)
    for j in range(20):
        out.append((I.random_pair(rng, int(rng.integers(30, 400))), dict(base, min_inliers=10, iterations=300, refine_iterations=5, seed=j)))
    return out


def key(r):
    return (r["status"], r["matches"].tobytes(), r["inliers"].tobytes())


def cpu(pair, steps, **kw):
    return V.motion_pnp_cpu(*I.frames(pair), camera=(I.FX, I.FY, I.CX, I.CY), image_size=(I.WIDTH, I.HEIGHT), steps=steps, **kw)


def main():
    cases = calls()
    res = {s: [key(cpu(p, s, **kw)) for p, kw in cases] for s in range(1, 13)}
    stable = None
    for s in range(1, 11):
        d1 = sum(a != b for a, b in zip(res[s], res[s + 1]))
        d2 = sum(a != b for a, b in zip(res[s], res[s + 2]))
        print("steps %2d: differs from %2d in %2d and from %2d in %2d of %d calls" % (s, s + 1, d1, s + 2, d2, len(cases)))
        if stable is None and d1 == 0 and d2 == 0:
            stable = s
    print("smallest count that two more steps do not change: %s; the rule takes one more: %s (motion_pnp_rule.h has %d)" %
          (stable, None if stable is None else stable + 1, M.STEPS))
    sets = I.fit_sets()
    r, t, p, n = M.fit_deviation(sets, I.model_camera(I.CAMERA))
    print("fp32 fit from the P3P start against float64 least squares, %d fits over %d sets of %d .. %d points: worst rotation entry %.3e, worst translation "
          "entry %.3e; P3P: worst held-out reprojection %.3e px" % (n, len(sets), min(len(s["P"]) for s in sets), max(len(s["P"]) for s in sets), r, t, p))


if __name__ == "__main__":
    main()
