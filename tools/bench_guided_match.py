"""Times the guided two-frame matching of lcd_match_guided next to the only matchers the engine offered such a caller before, lcd_match_pairs
in cross-check and in dictionary mode, on the same pairs in the same process (needs an MI355X; there is no CPU fallback).

    python tools/bench_guided_match.py [--reps 60] [--warmup 10] [--rounds 5] [--out profiles/guided_match.txt]

Cases: 300 + 300 SURF, 400 + 400 ORB, 1000 + 1000 SURF and a batch of 8 pairs of 300 + 300 SURF, keypoints uniform in 640 x 480, every
from-row projected (a corner per from-row, 2 px off its keypoint), 3/4 of the to-rows noisy copies of from-rows 3 px from the projection,
radius 40.  Per case `rounds` rounds; a round times, each as the median over `reps` repetitions after `warmup`:
  guided p2f / f2p   lcd_match_guided(_dev), ratio rule 0.8, projected-to-frame (the reference's default) and frame-to-projected
  cross_check        lcd_match_pairs(_dev), LCD_MATCH_CROSS_CHECK
  dictionary         lcd_match_pairs(_dev), LCD_MATCH_DICTIONARY
host_ms is a host clock around the host entry (rows in, results out, one synchronisation), dev_ms HIP events on the engine's stream around
ONE call of the device entry.  Reported per pair: the median of the rounds' medians and their spread (lowest .. highest round).  The
expectation -- guided no slower than the global cross-check beyond that baseline's spread over the rounds -- is evaluated and printed as it
comes out.  The two entries' results are compared before a number is reported.  One JSON line per case; --out also writes the table."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH, HEIGHT, RADIUS = 640.0, 480.0, 40.0


def make_pair(kind, rows, seed):
    """-> (from, to, corners, corner_from_row, to_points)"""
    from rtabmap_amd import synth
    rng = np.random.default_rng(seed)
    n_copy = rows * 3 // 4
    src = rng.permutation(rows)[:n_copy]
    if kind == "orb":
        a = rng.integers(0, 256, (rows, 32), dtype=np.uint8)
        b = np.concatenate([a[src] ^ np.packbits(rng.random((n_copy, 256)) < 0.02, axis=1), rng.integers(0, 256, (rows - n_copy, 32), dtype=np.uint8)])
    else:
        a = synth.vocab_surf(rows, seed=seed)
        b = a[src] + rng.standard_normal((n_copy, 64)).astype(np.float32) * np.float32(0.02)
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        b = np.concatenate([b, synth.vocab_surf(rows - n_copy, seed=seed + 1)]).astype(np.float32)
    size = np.array([WIDTH, HEIGHT])
    key_from = rng.random((rows, 2)) * size
    corners = (key_from + rng.standard_normal((rows, 2)) * 2.0).astype(np.float32)
    pts = np.concatenate([corners[src] + rng.standard_normal((n_copy, 2)) * 3.0, rng.random((rows - n_copy, 2)) * size]).astype(np.float32)
    return np.ascontiguousarray(a), np.ascontiguousarray(b), corners, np.arange(rows, dtype=np.int32), pts


def summary(round_medians_ms, per):
    m = np.asarray(round_medians_ms, np.float64) / per
    return {"median": round(float(np.median(m)), 4), "low": round(float(m.min()), 4), "high": round(float(m.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 50 or a.rounds < 5:
        sys.exit("bench_guided_match.py: at least 50 repetitions and 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_guided_match.py needs a GPU: nothing is measured without one")
    import rtabmap_amd

    cases = [("surf 300+300", "surf", 300, 1), ("orb 400+400", "orb", 400, 1), ("surf 1000+1000", "surf", 1000, 1), ("surf 8 x (300+300)", "surf", 300, 8)]
    stream = torch.cuda.Stream()
    lines = []
    for name, kind, rows, n_pairs in cases:
        pairs = [make_pair(kind, rows, 1000 + 7 * k) for k in range(n_pairs)]
        f, t, c, r, p = (np.concatenate([x[k] for x in pairs]) for k in range(5))
        off = np.arange(0, (n_pairs + 1) * rows, rows, dtype=np.int64)
        eng = rtabmap_amd.Engine("u8" if kind == "orb" else "f32", f.shape[1], stream=stream.cuda_stream)
        d_f, d_t, d_c, d_r, d_p = (torch.from_numpy(x).cuda() for x in (f, t, c, r, p))
        n = f.shape[0]
        i32 = lambda: torch.zeros(n, dtype=torch.int32, device="cuda")
        g_out = {d: (i32(), i32(), torch.zeros((n, 2), dtype=torch.float32, device="cuda"), i32()) for d in ("projected_to_frame", "frame_to_projected")}
        m_out = {"cross_check": (i32(), torch.zeros(n, dtype=torch.float32, device="cuda")), "dictionary": (i32(), i32())}
        kinds = {
            "guided p2f": (lambda: eng.match_guided(f, t, c, r, p, off, off, off, RADIUS, 0.8, "ratio", "projected_to_frame"),
                           lambda: eng.match_guided_dev(d_f, d_t, d_c, d_r, d_p, off, off, off, *g_out["projected_to_frame"], radius=RADIUS, direction="projected_to_frame")),
            "guided f2p": (lambda: eng.match_guided(f, t, c, r, p, off, off, off, RADIUS, 0.8, "ratio", "frame_to_projected"),
                           lambda: eng.match_guided_dev(d_f, d_t, d_c, d_r, d_p, off, off, off, *g_out["frame_to_projected"], radius=RADIUS, direction="frame_to_projected")),
            "cross_check": (lambda: eng.match_pairs(f, t, off, off, "cross_check"), lambda: eng.match_pairs_dev(d_f, d_t, off, off, *m_out["cross_check"], "cross_check")),
            "dictionary": (lambda: eng.match_pairs(f, t, off, off, "dictionary"), lambda: eng.match_pairs_dev(d_f, d_t, off, off, *m_out["dictionary"], "dictionary")),
        }
        med = {k: {"host_ms": [], "dev_ms": []} for k in kinds}
        got = {}
        for rnd in range(a.rounds):
            for k, (host_call, dev_call) in kinds.items():
                host, dev = [], []
                for i in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    got[k] = host_call()
                    if i >= a.warmup:
                        host.append((time.perf_counter() - t0) * 1e3)
                for i in range(a.warmup + a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record()
                        dev_call()
                        e1.record()
                    e1.synchronize()
                    if i >= a.warmup:
                        dev.append(e0.elapsed_time(e1))
                med[k]["host_ms"].append(float(np.median(host)))
                med[k]["dev_ms"].append(float(np.median(dev)))
        # the two entries agree on what was timed
        for d, k in (("projected_to_frame", "guided p2f"), ("frame_to_projected", "guided f2p")):
            o = [x.cpu().numpy() for x in g_out[d]]
            np.testing.assert_array_equal(o[0], got[k][0]); np.testing.assert_array_equal(o[1], got[k][1])
            np.testing.assert_array_equal(o[2].view(np.uint32), got[k][2].view(np.uint32))
            if d == "projected_to_frame":
                np.testing.assert_array_equal(o[3], got[k][3])
        np.testing.assert_array_equal(m_out["cross_check"][0].cpu().numpy(), got["cross_check"][0])
        np.testing.assert_array_equal(m_out["dictionary"][1].cpu().numpy(), got["dictionary"][1])
        eng.close()
        count = got["guided p2f"][0]
        res = {"case": name, "pairs": n_pairs, "reps": a.reps, "rounds": a.rounds, "candidates_per_window": round(float(count.mean()), 1),
               "matched_p2f": int((got["guided p2f"][3] >= 0).sum()), "matched_cross_check": int((got["cross_check"][0] >= 0).sum())}
        for k in kinds:
            res[k] = {e: summary(v, n_pairs) for e, v in med[k].items()}
        base = res["cross_check"]["dev_ms"]
        for k in ("guided p2f", "guided f2p"):
            res[k]["no_slower_than_cross_check_dev"] = bool(res[k]["dev_ms"]["median"] <= base["median"] + (base["high"] - base["low"]))
        print(json.dumps(res), flush=True)
        lines.append("    %s: %.1f candidates per window; matched %d (guided p2f) / %d (cross-check) of %d to-rows" %
                     (name, res["candidates_per_window"], res["matched_p2f"], res["matched_cross_check"], n))
        for k in kinds:
            for e in ("host_ms", "dev_ms"):
                v = res[k][e]
                lines.append("    %-20s %-12s %-8s median %8.4f ms per pair   rounds %8.4f .. %8.4f" % (name, k, e, v["median"], v["low"], v["high"]))
        for k in ("guided p2f", "guided f2p"):
            lines.append("    %-20s %-12s no slower than cross_check dev_ms beyond its spread: %s" % (name, k, res[k]["no_slower_than_cross_check_dev"]))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
