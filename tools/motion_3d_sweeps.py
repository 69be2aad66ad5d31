"""How the Jacobi sweep count of lcd_estimate_motion_3d's rule was chosen (profiles/motion_3d.txt).  CPU only: the host mirror's
motion3d_cpu with its `sweeps` argument over the generators of tests/motion_3d_inputs.py.

    python tools/motion_3d_sweeps.py

Prints, for s = 1 .. 10, in how many of the calls the outputs (status, transform bits, variance bits, both id lists) with s sweeps differ from
those with s + 1 and with s + 2, then the smallest s that two more sweeps do not change and the rule's count, one more; and the largest
difference between an entry of the fp32 fit and of a float64 SVD fit over the well-conditioned inlier sets."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import motion_3d_inputs as I  # noqa: E402
import motion_3d_model as M  # noqa: E402
from rtabmap_amd import vwdictionary as V  # noqa: E402


def calls():
    out = []
    for pair in I.mixed_batch():
        for iterations in (1, 300):
            for refine in I.REFINE:
                out.append((pair, dict(min_inliers=4, inlier_distance=0.1, iterations=iterations, refine_iterations=refine, seed=5)))
    out += [I.refine_case(name) for name in I.REFINE_CASES]
    out.append((I.all_outlier_pair(), dict(min_inliers=4, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=3)))
    rng = np.random.default_rng(77)
    for j in range(20):
        out.append((I.random_pair(rng, int(rng.integers(30, 400))), dict(min_inliers=10, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=j)))
    return out


def key(r):
    return (r["status"], M.bits(r["transform"]).tobytes(), float(r["variance"]), r["matches"].tobytes(), r["inliers"].tobytes())


def main():
    cases = calls()
    res = {s: [key(V.motion3d_cpu(*I.frames(p), sweeps=s, **kw)) for p, kw in cases] for s in range(1, 13)}
    stable = None
    for s in range(1, 11):
        d1 = sum(a != b for a, b in zip(res[s], res[s + 1]))
        d2 = sum(a != b for a, b in zip(res[s], res[s + 2]))
        print("sweeps %2d: differs from %2d in %2d and from %2d in %2d of %d calls" % (s, s + 1, d1, s + 2, d2, len(cases)))
        if stable is None and d1 == 0 and d2 == 0:
            stable = s
    print("smallest count that two more sweeps do not change: %s; the rule takes one more: %s (motion_3d_rule.h has %d)" %
          (stable, None if stable is None else stable + 1, M.SWEEPS))
    worst = 0.0
    sets = I.fit_sets()
    for P, Q in sets:
        m = M.fit_set(P, Q).reshape(3, 4).astype(np.float64)
        R, t, _ = M.kabsch64(P, Q)
        worst = max(worst, np.abs(m[:, :3] - R).max(), np.abs(m[:, 3] - t).max())
    print("fp32 fit against a float64 SVD fit, %d well-conditioned inlier sets of %d .. %d: worst entry difference %.3e" %
          (len(sets), min(len(p) for p, _ in sets), max(len(p) for p, _ in sets), worst))


if __name__ == "__main__":
    main()
