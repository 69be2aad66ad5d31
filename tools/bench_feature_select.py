"""Times lcd_select_features_dev and lcd_expand_word_ids_dev next to the only path the engine offered a caller whose extractor leaves its
output in device memory before: synchronise, responses to the host, the host mirror's selection (FeatureSelect::limitKeypoints), the index
list back, a gather on the device -- and for the expansion: ids and index list to the host, FeatureSelect::expandWordIds, the list back.
Both sides run in the same process on the same data (needs an MI355X; there is no CPU fallback).

    python tools/bench_feature_select.py [--reps 60] [--warmup 10] [--rounds 5] [--out profiles/feature_select_bench.txt]

Cases (SURF rows, 64 floats): 1000 -> 500 (the reference's defaults), 5000 -> 1000, 16384 -> 500, a 4 x 4 grid at 1000 -> 500 on 640 x 480,
and eight frames of 1000 -> 500 in one call.  Per case `rounds` rounds; a round times, each as the median over `reps` repetitions after
`warmup`:
  wall_ms   a host clock from "the extractor's output is complete on the device" (a synchronised stream) to "the selected rows / expanded
            ids are complete on the device" (the stream synchronised again), for the device entry and for the host round trip alike
  dev_ms    HIP events on the engine's stream around ONE call of the device entry
Reported per call: the median of the rounds' medians and their spread (lowest .. highest round).  The expectation -- the device entry's
wall_ms no larger than the host round trip's beyond that baseline's own spread over the rounds -- is evaluated and printed as it comes out.
The two paths' results are compared before a number is reported.  One JSON line per case; --out also writes the table."""
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
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 50 or a.rounds < 5:
        sys.exit("bench_feature_select.py: at least 50 repetitions and 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_feature_select.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    from rtabmap_amd import synth, vwdictionary as V

    cases = [("1000 -> 500", 1000, 500, (1, 1), 1), ("5000 -> 1000", 5000, 1000, (1, 1), 1), ("16384 -> 500", 16384, 500, (1, 1), 1),
             ("1000 -> 500, grid 4x4", 1000, 500, (4, 4), 1), ("8 x (1000 -> 500)", 1000, 500, (1, 1), 8)]
    stream = torch.cuda.Stream()
    lines = []
    for name, n, mx, grid, n_frames in cases:
        rng = np.random.default_rng(n + n_frames)
        N = n * n_frames
        off = np.arange(0, N + 1, n, dtype=np.int64)
        resp = (rng.random(N) * 100).astype(np.float32)
        resp[rng.random(N) < 0.2] = 25.0                                   # ties
        pts = (rng.random((N, 2)) * np.array([WIDTH - 1, HEIGHT - 1])).astype(np.float32)
        rows = synth.vocab_surf(N, seed=n)
        size = [(WIDTH, HEIGHT)] * n_frames
        with_grid = grid != (1, 1)
        eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_resp, d_pts, d_rows = (torch.from_numpy(x).cuda() for x in (resp, pts, rows))
            d_count = torch.zeros(n_frames, dtype=torch.int32, device="cuda")
            d_index = torch.zeros(N, dtype=torch.int32, device="cuda")
            d_out = torch.zeros_like(d_rows)
            b_out = torch.zeros_like(d_rows)                               # the baseline's gathered rows, frame f at off[f]
            d_words = torch.from_numpy(rng.integers(1, 50000, N).astype(np.int32)).cuda()
            d_all, b_all = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
        stream.synchronize()
        state = {}

        def select_dev():
            eng.select_features_dev(d_resp, off, mx, d_count, d_index, grid=grid, image_size=size if with_grid else None,
                                    d_points=d_pts if with_grid else None, d_rows=d_rows, d_out_rows=d_out)

        def select_round_trip():
            with torch.cuda.stream(stream):
                stream.synchronize()
                h_resp = d_resp.cpu().numpy()
                h_pts = d_pts.cpu().numpy() if with_grid else None
                kept = []
                for f in range(n_frames):
                    s = slice(int(off[f]), int(off[f + 1]))
                    mask = V.limit_keypoints(h_resp[s], None if h_pts is None else h_pts[s], mx, (WIDTH, HEIGHT), grid[0], grid[1])
                    kept.append(np.flatnonzero(mask).astype(np.int64))
                state["kept"] = kept
                for f in range(n_frames):
                    idx = torch.from_numpy(kept[f] + int(off[f])).cuda(non_blocking=True)
                    b_out[int(off[f]):int(off[f]) + kept[f].shape[0]] = d_rows.index_select(0, idx)

        def expand_dev():
            eng.expand_word_ids_dev(off, d_count, d_index, d_words, d_all)

        def expand_round_trip():
            with torch.cuda.stream(stream):
                stream.synchronize()
                h_words, h_index, h_count = d_words.cpu().numpy(), d_index.cpu().numpy(), d_count.cpu().numpy()
                out = np.empty(N, np.int32)
                for f in range(n_frames):
                    a0, c = int(off[f]), int(h_count[f])
                    out[a0:a0 + n] = V.expand_word_ids(n, h_index[a0:a0 + c], h_words[a0:a0 + c])
                b_all.copy_(torch.from_numpy(out), non_blocking=True)

        kinds = {"select dev": select_dev, "select round trip": select_round_trip, "expand dev": expand_dev, "expand round trip": expand_round_trip}
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
        assert torch.equal(d_all, b_all)
        eng.close()
        res = {"case": name, "frames": n_frames, "reps": a.reps, "rounds": a.rounds, "selected": count.tolist(), "launches_per_call": 1}
        for k in kinds:
            res[k] = {e: summary(v) for e, v in med[k].items() if v}
        for what in ("select", "expand"):
            base, dev = res[what + " round trip"]["wall_ms"], res[what + " dev"]["wall_ms"]
            res[what + " dev"]["no_slower_than_round_trip"] = bool(dev["median"] <= base["median"] + (base["high"] - base["low"]))
        print(json.dumps(res), flush=True)
        lines.append("    %s: %d frame(s), selected %s" % (name, n_frames, count.tolist()))
        for k in kinds:
            for e, v in res[k].items():
                if isinstance(v, dict):
                    lines.append("    %-24s %-18s %-8s median %8.4f ms per call   rounds %8.4f .. %8.4f" % (name, k, e, v["median"], v["low"], v["high"]))
        for what in ("select", "expand"):
            lines.append("    %-24s %-18s no slower than the host round trip beyond its spread: %s" % (name, what + " dev", res[what + " dev"]["no_slower_than_round_trip"]))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
