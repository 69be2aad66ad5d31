"""Times lcd_verify_epipolar_dev next to the round trip a caller of the appearance-only mode had before it: word ids and keypoints of both
signatures from the device to the host, the rule on one core (epipolar_cpu, the engine's own arithmetic compiled for the host), the
decisions back to the device.  Both sides run in the same process on the same data (needs an MI355X; there is no CPU fallback).

    python tools/bench_epipolar.py [--m 100 500] [--batches 1 8 64] [--iterations 1000] [--reps 50] [--warmup 10] [--rounds 5] [--out FILE]

Per case (m correspondences a pair with 40 % outliers, `batch` pairs a call) `rounds` rounds; a round times, each as the median over `reps`
repetitions after `warmup`, a host clock from "ids and keypoints are complete on the device" (a synchronised stream) to "the statuses are
complete on the device" (the stream synchronised again), for the device entry and for the round trip alike.  Reported per call: the median
of the rounds' medians and their spread (lowest .. highest round).  The expectation -- in a batch of 8 or more the device entry is no slower
than the round trip beyond the round trip's own spread over the rounds -- is evaluated and printed as it comes out; the single-pair figure
stands beside it and is expected to be latency-bound (one workgroup behind a chain of barriers).  The two paths' results are compared bit for
bit before a number is reported.  One JSON line per case; --out also writes the table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(round_medians_ms):
    m = np.asarray(round_medians_ms, np.float64)
    return {"median": round(float(np.median(m)), 4), "low": round(float(m.min()), 4), "high": round(float(m.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[100, 500])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 50 or a.rounds < 5:
        sys.exit("bench_epipolar.py: at least 50 repetitions and 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_epipolar.py: needs a GPU")
    import epipolar_inputs as I
    import rtabmap_amd
    from rtabmap_amd import vwdictionary as V
    eng = rtabmap_amd.Engine("f32", 64)
    kw = dict(match_count_min=8, iterations=a.iterations, ransac_threshold=3.0, seed=0)
    lines = ["%5s %6s | %28s | %28s | %s" % ("m", "batch", "device entry ms (low .. high)", "host round trip ms (low .. high)", "batch >= 8: no slower beyond the spread")]
    for m in a.m:
        for batch in a.batches:
            pairs = [I.scene(3000 + 100 * k + m, m, outliers=0.4, extra=10) for k in range(batch)]
            fi, fp, fo, ti, tp, to = I.batch(pairs)
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
            d_fi, d_fp, d_ti, d_tp = dev(fi), dev(fp), dev(ti), dev(tp)
            d_f = torch.zeros((batch, 9), device="cuda")
            d_st, d_np, d_ni = (torch.zeros(batch, dtype=torch.int32, device="cuda") for _ in range(3))
            d_m, d_in = (torch.zeros(ti.shape[0], dtype=torch.int32, device="cuda") for _ in range(2))

            def device_entry():
                eng.verify_epipolar_dev(d_fi, d_fp, fo, d_ti, d_tp, to, d_f, d_st, d_np, d_ni, d_m, d_in, **kw)
                eng.synchronize()

            def round_trip():
                h_fi, h_fp, h_ti, h_tp = d_fi.cpu().numpy(), d_fp.cpu().numpy(), d_ti.cpu().numpy(), d_tp.cpu().numpy()
                res = [V.epipolar_cpu(h_fi[fo[k]:fo[k + 1]], h_fp[fo[k]:fo[k + 1]], h_ti[to[k]:to[k + 1]], h_tp[to[k]:to[k + 1]], **kw) for k in range(batch)]
                status = torch.tensor([r["status"] for r in res], dtype=torch.int32).cuda()
                torch.cuda.synchronize()
                return res, status

            # ---- the same bits first
            device_entry()
            res, status = round_trip()
            g_f, g_st, g_m, g_in, g_ni = d_f.cpu().numpy(), d_st.cpu().numpy(), d_m.cpu().numpy(), d_in.cpu().numpy(), d_ni.cpu().numpy()
            for k, r in enumerate(res):
                assert g_st[k] == r["status"] and g_ni[k] == r["inliers"].shape[0], (m, batch, k)
                assert np.array_equal(g_m[to[k]:to[k] + r["matches"].shape[0]], r["matches"]) and np.array_equal(g_in[to[k]:to[k] + g_ni[k]], r["inliers"])
                assert g_f[k].view(np.uint32).tobytes() == r["fundamental"].view(np.uint32).tobytes(), (m, batch, k)
            assert np.array_equal(status.cpu().numpy(), g_st)

            def timed(fn):
                rounds = []
                for _ in range(a.rounds):
                    for _ in range(a.warmup):
                        fn()
                    t = []
                    for _ in range(a.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        t.append(1e3 * (time.perf_counter() - t0))
                    rounds.append(float(np.median(t)))
                return summary(rounds)

            d, h = timed(device_entry), timed(round_trip)
            holds = None if batch < 8 else bool(d["median"] <= h["median"] + (h["high"] - h["low"]))
            rec = dict(m=m, batch=batch, iterations=a.iterations, inliers=[int(v) for v in g_ni[:4]], device_ms=d, round_trip_ms=h, expectation_holds=holds)
            print(json.dumps(rec), flush=True)
            lines.append("%5d %6d | %9.4f (%8.4f .. %8.4f) | %9.4f (%8.4f .. %8.4f) | %s" % (m, batch, d["median"], d["low"], d["high"], h["median"], h["low"], h["high"],
                                                                                  "-" if holds is None else ("holds" if holds else "DOES NOT HOLD")))
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
    eng.close()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
