"""Times lcd_refine_motion_ba_dev next to the only path the engine offered a caller who holds both frames and the PnP's outputs in device
memory before: synchronise, the PnP's outputs (inliers, counts, transforms) to the host, the rule on the CPU on one core (motion_ba_cpu of the
host mirror, the same arithmetic, over frames the host already holds), then the results back to the device.  Needs a GPU.

    python tools/bench_motion_ba.py [--reps 50] [--warmup 10] [--rounds 5] [--out profiles/motion_ba_bench.txt]

Per case and path, from a synchronised stream to a synchronised stream, after warm-up calls, in `rounds` rounds of `reps` repetitions:
  dev_ms    lcd_refine_motion_ba_dev, what the caller waits for
  trip_ms   the round trip through the host
Reported per call: the median of the rounds' medians and their spread (lowest .. highest round).  The expectation -- the device entry, in a
batch of 8 or more, no slower than the round trip beyond the round trip's own spread over the rounds -- is evaluated and printed as it comes
out; the single-pair figure is reported whatever it is.  The two paths' results are compared bit for bit before a number is reported.  One
JSON line per case; --out also writes them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KW = dict(min_inliers=20, iterations=20, pixel_variance=1.0, robust_delta=8.0, max_inliers_mean_distance=0.0, min_inliers_distribution=0.0)
OUTS = ("transform", "status", "inliers", "n_inliers", "n_outliers", "chi2_before", "chi2_after", "lm_accepted", "inliers_mean_distance", "inliers_distribution")


def summary(round_medians_ms):
    m = np.asarray(round_medians_ms, np.float64)
    return {"median": round(float(np.median(m)), 4), "low": round(float(m.min()), 4), "high": round(float(m.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import rtabmap_amd
    from rtabmap_amd import vwdictionary as V
    import motion_ba_inputs as I

    eng = rtabmap_amd.Engine("f32", 64)
    cam = I.camera(True)
    lines = []
    for m in (300, 1000):
        for n_pairs in (1, 8, 64):
            rng = np.random.default_rng(1000 * m + n_pairs)
            pairs = [I.pair(rng, m, outliers=m // 10) for _ in range(n_pairs)]
            c = I.concatenate(pairs)
            nt = c["to_ids"].shape[0]
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            d = {k: dev(c[k]) for k in ("from_ids", "from_xyz", "from_points", "to_ids", "to_points", "to_xyz", "inliers", "n_inliers", "transforms")}
            types = dict(transform=((n_pairs, 12), torch.float32), status=((n_pairs,), torch.int32), inliers=((nt,), torch.int32),
                         n_inliers=((n_pairs,), torch.int32), n_outliers=((n_pairs,), torch.int32), chi2_before=((n_pairs,), torch.float64),
                         chi2_after=((n_pairs,), torch.float64), lm_accepted=((n_pairs,), torch.int32),
                         inliers_mean_distance=((n_pairs,), torch.float32), inliers_distribution=((n_pairs,), torch.float32))
            o = {k: torch.zeros(s, dtype=t, device="cuda") for k, (s, t) in types.items()}
            o2 = {k: torch.zeros(s, dtype=t, device="cuda") for k, (s, t) in types.items()}

            def device_path():
                eng.refine_motion_ba_dev(d["from_ids"], d["from_xyz"], c["from_offsets"], d["to_ids"], d["to_points"], c["to_offsets"], d["inliers"],
                                         d["n_inliers"], d["transforms"], [cam] * n_pairs, [cam] * n_pairs, *[o[k] for k in OUTS],
                                         d_from_points=d["from_points"], d_to_xyz=d["to_xyz"], default_baseline=I.BASELINE, **KW)
                eng.synchronize()

            def round_trip():
                eng.synchronize()
                inl, cnt, tr = d["inliers"].cpu().numpy(), d["n_inliers"].cpu().numpy(), d["transforms"].cpu().numpy()
                res = dict(transform=np.zeros((n_pairs, 12), np.float32), status=np.zeros(n_pairs, np.int32), inliers=np.zeros(nt, np.int32),
                           n_inliers=np.zeros(n_pairs, np.int32), n_outliers=np.zeros(n_pairs, np.int32), chi2_before=np.zeros(n_pairs, np.float64),
                           chi2_after=np.zeros(n_pairs, np.float64), lm_accepted=np.zeros(n_pairs, np.int32),
                           inliers_mean_distance=np.zeros(n_pairs, np.float32), inliers_distribution=np.zeros(n_pairs, np.float32))
                for k, p in enumerate(pairs):
                    t0 = int(c["to_offsets"][k])
                    r = V.motion_ba_cpu(p["from_ids"], p["from_xyz"], p["to_ids"], p["to_points"], inl[t0:t0 + cnt[k]], tr[k], from_points=p["from_points"],
                                        to_xyz=p["to_xyz"], camera_from=cam, camera_to=cam, baselines=(I.BASELINE, I.BASELINE), **KW)
                    for name in res:
                        if name == "inliers":
                            res[name][t0:t0 + len(r["inliers"])] = r["inliers"]
                        elif name == "n_inliers":
                            res[name][k] = len(r["inliers"])
                        else:
                            res[name][k] = r[name]
                for name in res:
                    o2[name].copy_(torch.from_numpy(res[name]))
                torch.cuda.synchronize()

            device_path()
            round_trip()
            for name in OUTS:                                            # bit for bit before a number is reported
                a, b = o[name].cpu().numpy(), o2[name].cpu().numpy()
                assert a.tobytes() == b.tobytes(), (m, n_pairs, name)
            timed = {}
            for label, fn in (("dev_ms", device_path), ("trip_ms", round_trip)):
                for _ in range(args.warmup):
                    fn()
                meds = []
                for _ in range(args.rounds):
                    ts = []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        fn()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    meds.append(float(np.median(ts)))
                timed[label] = summary(meds)
            spread = timed["trip_ms"]["high"] - timed["trip_ms"]["low"]
            line = dict(inliers=m, pairs=n_pairs, **timed, accepted_steps=int(o["lm_accepted"].sum().item()),
                        expectation_holds=bool(timed["dev_ms"]["median"] <= timed["trip_ms"]["median"] + spread) if n_pairs >= 8 else None)
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
