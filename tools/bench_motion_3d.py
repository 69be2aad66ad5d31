"""Times lcd_estimate_motion_3d_dev next to the only path the engine offered a caller who holds both frames' word ids and 3-D points in device
memory before: synchronise, both frames to the host, the rule on the CPU (motion3d_cpu of the host mirror, the same arithmetic), then the
transform, the counts and the id lists back.  Both sides run in the same process on the same data (needs an MI355X; there is no CPU fallback).

    python tools/bench_motion_3d.py [--reps 60] [--warmup 10] [--rounds 5] [--out profiles/motion_3d_bench.txt]

Cases: pairs of 300 and of 1000 correspondences, 40 % of them outliers, 300 iterations, 5 refinement passes, threshold 0.1; 1, 8 and 64
pairs per call; and one pair of 5000 and one of 6000 correspondences, whose coordinates the kernel does and does not stage in LDS.  Per case `rounds` rounds; a round times, each as the median over `reps` repetitions after `warmup`:
  wall_ms   a host clock from "ids and points are complete on the device" (a synchronised stream) to "transforms, counts and id lists are
            complete on the device" (the stream synchronised again), for the device entry and the round trip alike
  dev_ms    HIP events on the engine's stream around ONE call of the device entry
  host_ms   lcd_estimate_motion_3d over host arrays (the host entry: staging, one copy in, the launch, one copy out)
  cpu_ms    motion3d_cpu alone over the pairs, no copies (what the round trip spends computing)
Reported per call and, for dev_ms and host_ms, per pair: the median of the rounds' medians and their spread (lowest .. highest round).  The
expectation -- the device entry's wall_ms, in a batch of 8 or more, no larger than the round trip's beyond that baseline's own spread over
the rounds -- is evaluated and printed as it comes out.  The two paths' results are compared bit for bit before a number is reported.
One JSON line per case; --out also writes the table."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KW = dict(min_inliers=20, inlier_distance=0.1, iterations=300, refine_iterations=5, seed=1)


def summary(round_medians_ms):
    m = np.asarray(round_medians_ms, np.float64)
    return {"median": round(float(np.median(m)), 4), "low": round(float(m.min()), 4), "high": round(float(m.max()), 4)}


def make_pair(rng, m, outliers=0.4, noise=0.01):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    angle = rng.uniform(0.2, 1.2)
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    P = rng.uniform(-3, 3, (m, 3))
    Q = P @ R.T + rng.uniform(-1, 1, 3) + rng.normal(size=(m, 3)) * noise
    out = rng.random(m) < outliers
    Q[out] = rng.uniform(-3, 3, (int(out.sum()), 3))
    ids = (rng.permutation(4 * m)[:m] + 1).astype(np.int32)
    perm = rng.permutation(m)
    return ids, P.astype(np.float32), ids[perm], Q.astype(np.float32)[perm]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 50 or a.rounds < 5:
        sys.exit("bench_motion_3d.py: at least 50 repetitions and 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_motion_3d.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    from rtabmap_amd import vwdictionary as V

    stream = torch.cuda.Stream()
    lines = []
    # the last two are one side and the other of what the kernel stages in LDS (5248 correspondences)
    for m, n_pairs in ((300, 1), (300, 8), (300, 64), (1000, 1), (1000, 8), (1000, 64), (5000, 1), (6000, 1)):
        name = "%d x (%d correspondences, 40 %% outliers, 300 iterations)" % (n_pairs, m)
        rng = np.random.default_rng(m + n_pairs)
        pairs = [make_pair(rng, m) for _ in range(n_pairs)]
        off = np.arange(0, m * n_pairs + 1, m, dtype=np.int64)
        fi, fx, ti, tx = (np.ascontiguousarray(np.concatenate([p[k] for p in pairs])) for k in range(4))
        N = fi.shape[0]
        eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_fi, d_fx, d_ti, d_tx = (torch.from_numpy(x).cuda() for x in (fi, fx, ti, tx))
            mk = lambda: dict(t=torch.zeros((n_pairs, 12), device="cuda"), s=torch.zeros(n_pairs, dtype=torch.int32, device="cuda"),
                              nm=torch.zeros(n_pairs, dtype=torch.int32, device="cuda"), ni=torch.zeros(n_pairs, dtype=torch.int32, device="cuda"),
                              v=torch.zeros(n_pairs, dtype=torch.float64, device="cuda"), m=torch.zeros(N, dtype=torch.int32, device="cuda"),
                              i=torch.zeros(N, dtype=torch.int32, device="cuda"))
            d, b = mk(), mk()
        stream.synchronize()

        def dev():
            eng.estimate_motion_3d_dev(d_fi, d_fx, off, d_ti, d_tx, off, d["t"], d["s"], d["nm"], d["ni"], d["v"], d["m"], d["i"], **KW)

        def cpu(h_fi, h_fx, h_ti, h_tx):
            t, s, nm, ni = np.zeros((n_pairs, 12), np.float32), np.zeros(n_pairs, np.int32), np.zeros(n_pairs, np.int32), np.zeros(n_pairs, np.int32)
            v, om, oi = np.zeros(n_pairs, np.float64), np.zeros(N, np.int32), np.zeros(N, np.int32)
            for k in range(n_pairs):
                lo, hi = k * m, (k + 1) * m
                r = V.motion3d_cpu(h_fi[lo:hi], h_fx[lo:hi], h_ti[lo:hi], h_tx[lo:hi], **KW)
                t[k], s[k], v[k], nm[k], ni[k] = r["transform"], r["status"], r["variance"], len(r["matches"]), len(r["inliers"])
                om[lo:lo + nm[k]], oi[lo:lo + ni[k]] = r["matches"], r["inliers"]
            return t, s, nm, ni, v, om, oi

        def round_trip():
            with torch.cuda.stream(stream):
                stream.synchronize()
                res = cpu(d_fi.cpu().numpy(), d_fx.cpu().numpy(), d_ti.cpu().numpy(), d_tx.cpu().numpy())
                for key, x in zip(("t", "s", "nm", "ni", "v", "m", "i"), res):
                    b[key].copy_(torch.from_numpy(x), non_blocking=True)

        def host():
            eng.estimate_motion_3d(fi, fx, off, ti, tx, off, **KW)

        def cpu_only():
            cpu(fi, fx, ti, tx)

        kinds = {"dev": dev, "round trip": round_trip, "host entry": host, "motion3d_cpu": cpu_only}
        med = {k: {"wall_ms": [], "dev_ms": []} for k in kinds}
        for rnd in range(a.rounds):
            for k, call in kinds.items():
                reps, warm = a.reps, a.warmup
                wall, devt = [], []
                for i in range(warm + reps):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    call()
                    stream.synchronize()
                    if i >= warm:
                        wall.append((time.perf_counter() - t0) * 1e3)
                med[k]["wall_ms"].append(float(np.median(wall)))
                if k != "dev":
                    continue
                for i in range(a.warmup + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record()
                        call()
                        e1.record()
                    e1.synchronize()
                    if i >= a.warmup:
                        devt.append(e0.elapsed_time(e1))
                med[k]["dev_ms"].append(float(np.median(devt)))
        for key in ("s", "nm", "ni", "m", "i"):                     # the two paths agree, bit for bit, on what was timed
            assert torch.equal(d[key], b[key]), key
        assert torch.equal(d["t"].view(torch.int32), b["t"].view(torch.int32)) and torch.equal(d["v"].view(torch.int64), b["v"].view(torch.int64))
        inliers = d["ni"].cpu().numpy().tolist()
        eng.close()
        res = {"case": name, "pairs": n_pairs, "correspondences": m, "reps": a.reps, "rounds": a.rounds, "inliers": inliers[:8], "launches_per_call": 1}
        for k in kinds:
            res[k] = {e: summary(v) for e, v in med[k].items() if v}
            res[k]["per_pair_ms"] = round(res[k]["dev_ms" if k == "dev" else "wall_ms"]["median"] / n_pairs, 4)
        base, dv = res["round trip"]["wall_ms"], res["dev"]["wall_ms"]
        res["dev"]["no_slower_than_round_trip"] = bool(dv["median"] <= base["median"] + (base["high"] - base["low"]))
        res["copies_saved_ms"] = round(base["median"] - res["motion3d_cpu"]["wall_ms"]["median"], 4)
        print(json.dumps(res), flush=True)
        lines.append("    %s: inliers %s" % (name, inliers[:8]))
        for k in kinds:
            for e, v in res[k].items():
                if isinstance(v, dict):
                    lines.append("    %-14s %-8s median %9.4f ms per call   rounds %9.4f .. %9.4f   per pair %8.4f ms" %
                                 (k, e, v["median"], v["low"], v["high"], v["median"] / n_pairs))
        lines.append("    round trip minus motion3d_cpu (the copies and the synchronisation the device entry saves): %.4f ms" % res["copies_saved_ms"])
        lines.append("    dev no slower than the host round trip beyond its spread: %s" % res["dev"]["no_slower_than_round_trip"])
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
