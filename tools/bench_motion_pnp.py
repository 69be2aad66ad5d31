"""Times lcd_estimate_motion_pnp_dev next to the only path the engine offered a caller who holds both frames in device memory before:
synchronise, both frames to the host, the rule on the CPU (motion_pnp_cpu of the host mirror, the same arithmetic), then the results back to
the device.  Needs a GPU.

    python tools/bench_motion_pnp.py [--reps 60] [--warmup 10] [--rounds 5] [--out profiles/motion_pnp_bench.txt]

Per case and path, from a synchronised stream to a synchronised stream, after warm-up calls, in `rounds` rounds of `reps` repetitions:
  wall_ms   what the caller waits for
  dev_ms    the device entry between two events on the stream (the launch and the job table's copy)
  host_ms   lcd_estimate_motion_pnp over host arrays (the host entry: staging, one copy in, the launch, one copy out)
Reported per call and per pair: the median of the rounds' medians and their spread (lowest .. highest round).  The expectation -- the device
entry's wall_ms, in a batch of 8 or more, no larger than the round trip's beyond that baseline's own spread over the rounds -- is evaluated
and printed as it comes out.  The two paths' results are compared bit for bit before a number is reported.  The last two cases lie on
either side of what the kernel stages in LDS with to_xyz (3360 correspondences).  One JSON line per case; --out also writes
the table."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KW = dict(min_inliers=20, reproj_error=2.0, iterations=300, refine_iterations=1, variance_median_ratio=4, max_variance=0.0, seed=1)
FX, FY, CX, CY, W, H = 525.0, 525.0, 319.5, 239.5, 640, 480
CAMERA = dict(fx=FX, fy=FY, cx=CX, cy=CY, image_width=W, image_height=H)


def summary(round_medians_ms):
    m = np.asarray(round_medians_ms, np.float64)
    return {"median": round(float(np.median(m)), 4), "low": round(float(m.min()), 4), "high": round(float(m.max()), 4)}


def make_pair(rng, m, outliers=0.4, noise=0.5):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    angle = rng.uniform(0.05, 0.5)
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    t = rng.uniform(-0.5, 0.5, 3)
    z = rng.uniform(0.5, 10.0, m)
    u, v = rng.uniform(0, W - 1, m), rng.uniform(0, H - 1, m)
    C = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], axis=1)
    P = (C - t) @ R
    UV = np.stack([u, v], axis=1) + rng.normal(size=(m, 2)) * noise
    out = rng.random(m) < outliers
    UV[out] = np.stack([rng.uniform(0, W - 1, int(out.sum())), rng.uniform(0, H - 1, int(out.sum()))], axis=1)
    ids = (rng.permutation(4 * m)[:m] + 1).astype(np.int32)
    perm = rng.permutation(m)
    return ids, P.astype(np.float32), ids[perm], UV.astype(np.float32)[perm], C.astype(np.float32)[perm]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 50 or a.rounds < 5:
        sys.exit("bench_motion_pnp.py: at least 50 repetitions and 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_motion_pnp.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    from rtabmap_amd import vwdictionary as V

    stream = torch.cuda.Stream()
    lines = []
    for m, n_pairs in ((300, 1), (300, 8), (300, 64), (1000, 1), (1000, 8), (1000, 64), (3300, 1), (3400, 1)):
        name = "%d x (%d correspondences, 40 %% outliers, 300 iterations, 1 pass)" % (n_pairs, m)
        rng = np.random.default_rng(m + n_pairs)
        pairs = [make_pair(rng, m) for _ in range(n_pairs)]
        off = np.arange(0, m * n_pairs + 1, m, dtype=np.int64)
        fi, fx, ti, tp, tx = (np.ascontiguousarray(np.concatenate([p[k] for p in pairs])) for k in range(5))
        N = fi.shape[0]
        eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_fi, d_fx, d_ti, d_tp, d_tx = (torch.from_numpy(x).cuda() for x in (fi, fx, ti, tp, tx))
            mk = lambda: dict(t=torch.zeros((n_pairs, 12), device="cuda"), s=torch.zeros(n_pairs, dtype=torch.int32, device="cuda"),
                              nm=torch.zeros(n_pairs, dtype=torch.int32, device="cuda"), ni=torch.zeros(n_pairs, dtype=torch.int32, device="cuda"),
                              vl=torch.zeros(n_pairs, dtype=torch.float64, device="cuda"), vc=torch.zeros(n_pairs, dtype=torch.float64, device="cuda"),
                              vk=torch.zeros(n_pairs, dtype=torch.int32, device="cuda"), m=torch.zeros(N, dtype=torch.int32, device="cuda"),
                              i=torch.zeros(N, dtype=torch.int32, device="cuda"))
            d, b = mk(), mk()
        stream.synchronize()

        def dev():
            eng.estimate_motion_pnp_dev(d_fi, d_fx, off, d_ti, d_tp, off, CAMERA, d["t"], d["s"], d["nm"], d["ni"], d["vl"], d["vc"], d["vk"], d["m"], d["i"],
                                        d_to_xyz=d_tx, **KW)

        def cpu(h_fi, h_fx, h_ti, h_tp, h_tx):
            t, s, nm, ni = np.zeros((n_pairs, 12), np.float32), np.zeros(n_pairs, np.int32), np.zeros(n_pairs, np.int32), np.zeros(n_pairs, np.int32)
            vl, vc, vk, om, oi = np.zeros(n_pairs, np.float64), np.zeros(n_pairs, np.float64), np.zeros(n_pairs, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
            for k in range(n_pairs):
                lo, hi = k * m, (k + 1) * m
                r = V.motion_pnp_cpu(h_fi[lo:hi], h_fx[lo:hi], h_ti[lo:hi], h_tp[lo:hi], h_tx[lo:hi], camera=(FX, FY, CX, CY), image_size=(W, H), **KW)
                t[k], s[k], vl[k], vc[k], vk[k], nm[k], ni[k] = r["transform"], r["status"], r["variance_lin"], r["angle_cos"], r["variance_kind"], len(r["matches"]), len(r["inliers"])
                om[lo:lo + nm[k]], oi[lo:lo + ni[k]] = r["matches"], r["inliers"]
            return t, s, nm, ni, vl, vc, vk, om, oi

        def round_trip():
            with torch.cuda.stream(stream):
                stream.synchronize()
                res = cpu(d_fi.cpu().numpy(), d_fx.cpu().numpy(), d_ti.cpu().numpy(), d_tp.cpu().numpy(), d_tx.cpu().numpy())
                for key, x in zip(("t", "s", "nm", "ni", "vl", "vc", "vk", "m", "i"), res):
                    b[key].copy_(torch.from_numpy(x), non_blocking=True)

        def host():
            eng.estimate_motion_pnp(fi, fx, off, ti, tp, off, CAMERA, to_xyz=tx, **KW)

        kinds = {"dev": dev, "round trip": round_trip, "host entry": host}
        med = {k: {"wall_ms": [], "dev_ms": []} for k in kinds}
        for rnd in range(a.rounds):
            for k, call in kinds.items():
                wall, devt = [], []
                for i in range(a.warmup + a.reps):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    call()
                    stream.synchronize()
                    if i >= a.warmup:
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
        for key in ("s", "nm", "ni", "vk", "m", "i"):               # the two paths agree, bit for bit, on what was timed
            assert torch.equal(d[key], b[key]), key
        assert torch.equal(d["t"].view(torch.int32), b["t"].view(torch.int32))
        assert torch.equal(d["vl"].view(torch.int64), b["vl"].view(torch.int64)) and torch.equal(d["vc"].view(torch.int64), b["vc"].view(torch.int64))
        inliers = d["ni"].cpu().numpy().tolist()
        eng.close()
        res = {"case": name, "pairs": n_pairs, "correspondences": m, "reps": a.reps, "rounds": a.rounds, "inliers": inliers[:8], "launches_per_call": 1}
        for k in kinds:
            res[k] = {e: summary(v) for e, v in med[k].items() if v}
            res[k]["per_pair_ms"] = round(res[k]["dev_ms" if k == "dev" else "wall_ms"]["median"] / n_pairs, 4)
        base, dv = res["round trip"]["wall_ms"], res["dev"]["wall_ms"]
        res["dev"]["no_slower_than_round_trip"] = bool(dv["median"] <= base["median"] + (base["high"] - base["low"]))
        print(json.dumps(res), flush=True)
        lines.append("    %s: inliers %s" % (name, inliers[:8]))
        for k in kinds:
            for e, v in res[k].items():
                if isinstance(v, dict):
                    lines.append("    %-14s %-8s median %9.4f ms per call   rounds %9.4f .. %9.4f   per pair %8.4f ms" %
                                 (k, e, v["median"], v["low"], v["high"], v["median"] / n_pairs))
        lines.append("    dev no slower than the host round trip beyond its spread: %s" % res["dev"]["no_slower_than_round_trip"])
        if a.out:                                                   # after every case: a run that is cut short leaves what it measured
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
