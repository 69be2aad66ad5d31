"""Measures lcd_estimate_motion_mono_dev against the round trip a caller has without it: ids and keypoints to the host, motion_mono_cpu on one
core, results back to the device.  Both paths are compared bit for bit first.  Five rounds of the median of 50 calls after 10 warm-up calls,
at m = 100 and m = 500 correspondences and batches of 1, 8 and 64 pairs; one JSON line per cell, then a table.

    python tools/bench_motion_mono.py [--iterations 1000] [--calls 50] [--rounds 5] [--short-round-trip]

Both paths follow that protocol.  At 64 pairs a round trip takes up to 1.9 s, so the protocol's 260 calls of it take eight minutes a cell;
--short-round-trip measures the round trip with fewer calls (10 at one pair, 3 from 8 pairs on, after 1 warm-up call) and says so in its
output (round_trip_calls).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--short-round-trip", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="*", default=[100, 500])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 64])
    a = ap.parse_args()
    import torch
    import rtabmap_amd
    from rtabmap_amd import vwdictionary as V
    import motion_mono_inputs as I

    eng = rtabmap_amd.Engine("f32", 64)
    kw = dict(min_inliers=20, iterations=a.iterations, reproj_threshold=2.0, variance_median_ratio=4, max_variance=1e30, distance_threshold=50.0, seed=1)
    rows = []
    for m in a.sizes:
        for nb in a.batches:
            pairs = [I.scene(7000 + 31 * m + k, m + 2, outliers=0.4, noise=0.5) for k in range(nb)]
            fi, fp, f3, fo, ti, tp, to = I.batch(pairs)
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
            d = dict(fi=t(fi), fp=t(fp), f3=t(f3), ti=t(ti), tp=t(tp))
            n = ti.shape[0]
            i32 = lambda k: torch.zeros((k,), dtype=torch.int32, device="cuda")
            out = dict(transform=torch.zeros((nb, 12), device="cuda"), status=i32(nb), n_matches=i32(nb), n_inliers=i32(nb),
                       variance=torch.zeros((nb,), dtype=torch.float64, device="cuda"), matches=i32(n), inliers=i32(n), points3=torch.zeros((n, 3), device="cuda"))
            cams = [I.CAMERA_DICT] * nb

            def device():
                eng.estimate_motion_mono_dev(d["fi"], d["fp"], fo, d["ti"], d["tp"], to, cams, out["transform"], out["status"], out["n_matches"],
                                             out["n_inliers"], out["variance"], out["matches"], out["inliers"], out["points3"], d_from_points3=d["f3"], **kw)
                eng.synchronize()

            def round_trip():
                h = {k: v.cpu().numpy() for k, v in d.items()}
                res = []
                for k in range(nb):
                    f, g = slice(fo[k], fo[k + 1]), slice(to[k], to[k + 1])
                    res.append(V.motion_mono_cpu(h["fi"][f], h["fp"][f], h["ti"][g], h["tp"][g], I.CAMERA, from_points3=h["f3"][f], **kw))
                back = torch.from_numpy(np.stack([r["transform"] for r in res])).cuda()
                torch.cuda.synchronize()
                return res, back

            device()
            res, _ = round_trip()
            got = {k: v.cpu().numpy() for k, v in out.items()}
            for k, r in enumerate(res):                                 # bit for bit first
                assert got["status"][k] == r["status"] and got["transform"][k].tobytes() == r["transform"].tobytes(), (m, nb, k)
                assert got["inliers"][to[k]:to[k] + len(r["inliers"])].tolist() == r["inliers"].tolist()
                assert got["points3"][to[k]:to[k] + len(r["inliers"])].tobytes() == r["points3"].tobytes()
                assert np.float64(got["variance"][k]).tobytes() == np.float64(r["variance"]).tobytes()

            def measure(fn, calls, warmup):
                for _ in range(warmup):
                    fn()
                meds = []
                for _ in range(a.rounds):
                    ts = []
                    for _ in range(calls):
                        t0 = time.perf_counter()
                        fn()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    meds.append(statistics.median(ts))
                return meds

            dev_ms = measure(device, a.calls, a.warmup)
            cpu_calls = max(3, min(a.calls, int(2000 / max(nb * a.iterations * 0.2, 1)))) if a.short_round_trip else a.calls
            cpu_ms = measure(round_trip, cpu_calls, 1 if a.short_round_trip else a.warmup)
            row = dict(m=m, batch=nb, iterations=a.iterations, device_ms=[round(v, 3) for v in dev_ms], round_trip_ms=[round(v, 3) for v in cpu_ms],
                       round_trip_calls=cpu_calls, ok=int(sum(r["status"] == 0 for r in res)))
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("%5s %6s %28s %28s" % ("m", "batch", "device ms (min .. max)", "round trip ms (min .. max)"))
    for r in rows:
        print("%5d %6d %12.3f .. %12.3f %12.3f .. %12.3f" % (r["m"], r["batch"], min(r["device_ms"]), max(r["device_ms"]), min(r["round_trip_ms"]),
                                                            max(r["round_trip_ms"])))
    eng.close()


if __name__ == "__main__":
    main()
