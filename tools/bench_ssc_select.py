"""Times lcd_select_features_dev with LCD_SELECT_SSC (Kp/SSC, the square covering) next to what a caller whose extractor leaves its output in
device memory had before: synchronise, responses and points to the host, the host mirror's SSC (FeatureSelect::limitKeypointsSSC), the
index list back, a plain gather of the rows on the device.  Both sides run in the same process on the same data (needs an MI355X; there
is no CPU fallback).

    python tools/bench_ssc_select.py [--reps 50] [--warmup 10] [--rounds 5] [--out profiles/ssc_select_bench.txt]

Cases (SURF rows, 64 floats, uniform points on 640 x 480): 1, 8 and 64 frames of 2000 -> 500 and of 8000 -> 1000.  Per case `rounds`
rounds; a round times, each as the median over `reps` repetitions after `warmup`:
  wall_ms   a host clock from "the extractor's output is complete on the device" (a synchronised stream) to "the selected rows are
            complete on the device" (the stream synchronised again), for the device entry and for the host round trip alike
  dev_ms    HIP events on the engine's stream around ONE call of the device entry
Reported per call: the median of the rounds' medians and their spread (lowest .. highest round).  The expectation -- from 8 frames on,
the device entry's wall_ms no larger than the host round trip's beyond that baseline's own spread over the rounds; the single frame is
reported only -- is evaluated and printed as it comes out.  The two paths' results are compared bit for bit before a number is reported.
One JSON line per case; --out also writes the table."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH, HEIGHT = 640, 480


def summary(round_medians_ms):
    m = np.asarray(round_medians_ms, np.float64)
    return {"median": round(float(np.median(m)), 4), "low": round(float(m.min()), 4), "high": round(float(m.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 30 or a.rounds < 5:
        sys.exit("bench_ssc_select.py: at least 30 repetitions and 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ssc_select.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    from rtabmap_amd import synth, vwdictionary as V

    cases = [(n, mx, nf) for n, mx in ((2000, 500), (8000, 1000)) for nf in (1, 8, 64)]
    stream = torch.cuda.Stream()
    lines = []
    for n, mx, n_frames in cases:
        name = "%d x (%d -> %d)" % (n_frames, n, mx)
        rng = np.random.default_rng(n + n_frames)
        N = n * n_frames
        off = np.arange(0, N + 1, n, dtype=np.int64)
        resp = (rng.random(N) * 100).astype(np.float32)
        resp[rng.random(N) < 0.2] = 25.0                                   # ties
        pts = (rng.random((N, 2)) * np.array([WIDTH, HEIGHT])).astype(np.float32)
        rows = np.tile(synth.vocab_surf(n, seed=n), (n_frames, 1))
        size = [(WIDTH, HEIGHT)] * n_frames
        eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_resp, d_pts, d_rows = (torch.from_numpy(x).cuda() for x in (resp, pts, rows))
            d_count = torch.zeros(n_frames, dtype=torch.int32, device="cuda")
            d_index = torch.zeros(N, dtype=torch.int32, device="cuda")
            d_out = torch.zeros_like(d_rows)
            b_out = torch.zeros_like(d_rows)                               # the baseline's gathered rows, frame f at off[f]
        stream.synchronize()
        state = {}

        def select_dev():
            eng.select_features_dev(d_resp, off, mx, d_count, d_index, image_size=size, d_points=d_pts, d_rows=d_rows, d_out_rows=d_out, ssc=True)

        def select_round_trip():
            with torch.cuda.stream(stream):
                stream.synchronize()
                h_resp, h_pts = d_resp.cpu().numpy(), d_pts.cpu().numpy()
                kept = []
                for f in range(n_frames):
                    s = slice(int(off[f]), int(off[f + 1]))
                    kept.append(np.flatnonzero(V.limit_keypoints(h_resp[s], h_pts[s], mx, (WIDTH, HEIGHT), ssc=True)).astype(np.int64))
                state["kept"] = kept
                flat = np.concatenate([k + int(off[f]) for f, k in enumerate(kept)])
                gathered = d_rows.index_select(0, torch.from_numpy(flat).cuda(non_blocking=True))
                at = 0
                for f, k in enumerate(kept):
                    b_out[int(off[f]):int(off[f]) + k.shape[0]] = gathered[at:at + k.shape[0]]
                    at += k.shape[0]

        kinds = {"select dev": select_dev, "select round trip": select_round_trip}
        med = {k: {"wall_ms": [], "dev_ms": []} for k in kinds}
        for rnd in range(a.rounds):
            for k, call in kinds.items():
                wall, dev = [], []
                for i in range(a.warmup + a.reps):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    call()
                    stream.synchronize()
                    if i >= a.warmup:
                        wall.append((time.perf_counter() - t0) * 1e3)
                med[k]["wall_ms"].append(float(np.median(wall)))
                if not k.endswith("dev"):
                    continue
                for i in range(a.warmup + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record()
                        call()
                        e1.record()
                    e1.synchronize()
                    if i >= a.warmup:
                        dev.append(e0.elapsed_time(e1))
                med[k]["dev_ms"].append(float(np.median(dev)))
        # the two paths agree on what was timed
        count, index = d_count.cpu().numpy(), d_index.cpu().numpy()
        for f in range(n_frames):
            a0, c = int(off[f]), int(count[f])
            np.testing.assert_array_equal(index[a0:a0 + c], state["kept"][f])
            assert (index[a0 + c:a0 + n] == -1).all()
            assert torch.equal(d_out[a0:a0 + c], b_out[a0:a0 + c])
        eng.close()
        res = {"case": name, "frames": n_frames, "reps": a.reps, "rounds": a.rounds, "selected": count.tolist()[:8], "launches_per_call": 1}
        for k in kinds:
            res[k] = {e: summary(v) for e, v in med[k].items() if v}
        base, dev = res["select round trip"]["wall_ms"], res["select dev"]["wall_ms"]
        verdict = bool(dev["median"] <= base["median"] + (base["high"] - base["low"]))
        res["select dev"]["no_slower_than_round_trip"] = verdict
        res["select dev"]["asked"] = n_frames >= 8
        print(json.dumps(res), flush=True)
        lines.append("    %s: selected %s%s" % (name, count.tolist()[:8], " ..." if n_frames > 8 else ""))
        for k in kinds:
            for e, v in res[k].items():
                if isinstance(v, dict):
                    lines.append("    %-22s %-18s %-8s median %9.4f ms per call   rounds %9.4f .. %9.4f" % (name, k, e, v["median"], v["low"], v["high"]))
        lines.append("    %-22s %-18s no slower than the host round trip beyond its spread: %s%s" % (name, "select dev", verdict, "" if n_frames >= 8 else " (reported, not asked)"))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
