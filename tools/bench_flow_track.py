"""Times lcd_track_flow_dev next to the only path the engine offered a caller who registers two frames by optical flow (Vis/CorType = 1)
and whose images and corners lie in device memory before: synchronise, both images and the corners to the host, the host mirror on one core
(flow_track_cpu: the tracker and the keep step), then both corner lists, the index list and the counts back and a gather of the payload on
the device.  Both sides run in the same process on the same data (needs an MI355X; there is no CPU fallback).

    python tools/bench_flow_track.py [--reps 50] [--warmup 5] [--rounds 5] [--out profiles/flow_track_bench.txt]

Cases (the reference's Vis/CorFlow* defaults: 16 x 16, three levels, 30 iterations; a 16-byte payload: the word id and the from-side 3-D
point): 1000 and 5000 corners on 640 x 480, eight pairs of 1000 in one call, and 1000 corners with start positions and max_level 0 (the
guess is set).  Per case `rounds` rounds; a round times, each as the median over `reps` repetitions after `warmup`:
  wall_ms   a host clock from "corners and images are complete on the device" (a synchronised stream) to "both corner lists, counts and the
            compacted payload are complete on the device" (the stream synchronised again), for the device entry and the round trip alike
  dev_ms    HIP events on the engine's stream around ONE call of the device entry
Reported per call: the median of the rounds' medians and their spread (lowest .. highest round), and the device time per corner.  The
expectation -- the device entry's wall_ms no larger than the host round trip's beyond that baseline's own spread over the rounds -- is
evaluated and printed as it comes out.  The two paths' results are compared bit for bit before a number is reported.  One JSON line per
case; --out also writes the table."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summary(round_medians_ms):
    m = np.asarray(round_medians_ms, np.float64)
    return {"median": round(float(np.median(m)), 4), "low": round(float(m.min()), 4), "high": round(float(m.max()), 4)}


def image_pair(rng, width, height):
    """a smooth random texture and the same scene moved by a flow that grows from (1, -1) to (6, 3) pixels down the image"""
    a = rng.standard_normal((height + 16, width + 64))
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    for _ in range(3):
        a = sum(k[i] * np.roll(a, i - 2, 0) for i in range(5))
        a = sum(k[i] * np.roll(a, i - 2, 1) for i in range(5))
    a = (a - a.min()) / (a.max() - a.min()) * 255.0
    x = np.arange(width)[None, :] + 32.0
    y = np.arange(height)[:, None] + 8.0
    xs = x - np.linspace(1.0, 6.0, height)[:, None]
    ys = y - np.linspace(-1.0, 3.0, height)[:, None] + 0.0 * x
    i0, j0 = np.floor(xs).astype(int), np.floor(ys).astype(int)
    t, u = xs - i0, ys - j0
    to = (a[j0, i0] * (1 - t) + a[j0, i0 + 1] * t) * (1 - u) + (a[j0 + 1, i0] * (1 - t) + a[j0 + 1, i0 + 1] * t) * u
    return np.rint(a[8:8 + height, 32:32 + width]).astype(np.uint8), np.rint(to).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 20 or a.rounds < 5:
        sys.exit("bench_flow_track.py: at least 20 repetitions and 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_flow_track.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    from rtabmap_amd import vwdictionary as V

    width, height, aux_bytes = 640, 480, 16
    # name, corners per pair, pairs, max_level, use_initial
    cases = [("1000 on 640x480", 1000, 1, 3, 0), ("5000 on 640x480", 5000, 1, 3, 0), ("8 x (1000 on 640x480)", 1000, 8, 3, 0),
             ("1000, initial, level 0", 1000, 1, 0, 1)]
    stream = torch.cuda.Stream()
    lines = []
    for name, n, n_pairs, max_level, use_initial in cases:
        rng = np.random.default_rng(n + n_pairs + max_level)
        N = n * n_pairs
        off = np.arange(0, N + 1, n, dtype=np.int64)
        imgs = [image_pair(rng, width, height) for _ in range(n_pairs)]
        pts = (np.array([20.0, 20.0]) + rng.random((N, 2)) * np.array([width - 41, height - 41])).astype(np.float32)
        flow = np.stack([np.interp(pts[:, 1], [0, height - 1], [1.0, 6.0]), np.interp(pts[:, 1], [0, height - 1], [-1.0, 3.0])], 1)
        ini = (pts + flow + rng.uniform(-1.0, 1.0, pts.shape)).astype(np.float32) if use_initial else None
        aux = rng.integers(0, 256, (N, aux_bytes), dtype=np.uint8)
        eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_from = [torch.from_numpy(f).cuda() for f, _ in imgs]
            d_to = [torch.from_numpy(t).cuda() for _, t in imgs]
            d_pts, d_aux = torch.from_numpy(pts).cuda(), torch.from_numpy(aux).cuda()
            d_ini = None if ini is None else torch.from_numpy(ini).cuda()
            d_count, d_index = torch.zeros(n_pairs, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
            d_kf, d_kt, d_ka = torch.zeros((N, 2), device="cuda"), torch.zeros((N, 2), device="cuda"), torch.zeros_like(d_aux)
            b_count, b_index, b_kf, b_kt, b_ka = torch.zeros_like(d_count), torch.zeros_like(d_index), torch.zeros_like(d_kf), torch.zeros_like(d_kt), torch.zeros_like(d_ka)
        stream.synchronize()
        pairs = [{"from": f, "to": t, "max_level": max_level, "use_initial": use_initial} for f, t in zip(d_from, d_to)]

        def dev():
            eng.track_flow_dev(d_pts, off, pairs, d_count, d_index, d_kf, d_kt, d_initial=d_ini, d_aux=d_aux, aux_bytes=aux_bytes, d_out_aux=d_ka)

        def round_trip():
            with torch.cuda.stream(stream):
                stream.synchronize()
                h_pts = d_pts.cpu().numpy()
                h_ini = None if d_ini is None else d_ini.cpu().numpy()
                kf, kt = np.zeros((N, 2), np.float32), np.zeros((N, 2), np.float32)
                index, count = np.full(N, -1, np.int32), np.zeros(n_pairs, np.int32)
                kept_all = []
                for f in range(n_pairs):
                    h_from, h_to = d_from[f].cpu().numpy(), d_to[f].cpu().numpy()
                    a0 = int(off[f])
                    p = h_pts[a0:a0 + n]
                    got = V.flow_track_cpu(h_from, h_to, p, None, max_level, None if h_ini is None else h_ini[a0:a0 + n])
                    kept = got["kept"]
                    k = kept.shape[0]
                    kf[a0:a0 + k], kt[a0:a0 + k], index[a0:a0 + k], count[f] = p[kept], got["track"][kept], kept, k
                    kept_all.append(kept)
                b_kf.copy_(torch.from_numpy(kf), non_blocking=True)
                b_kt.copy_(torch.from_numpy(kt), non_blocking=True)
                b_index.copy_(torch.from_numpy(index), non_blocking=True)
                b_count.copy_(torch.from_numpy(count), non_blocking=True)
                for f in range(n_pairs):
                    idx = torch.from_numpy(kept_all[f].astype(np.int64) + int(off[f])).cuda(non_blocking=True)
                    b_ka[int(off[f]):int(off[f]) + kept_all[f].shape[0]] = d_aux.index_select(0, idx)

        def events(call, reps, warmup):
            t = []
            for i in range(warmup + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    e0.record()
                    call()
                    e1.record()
                e1.synchronize()
                if i >= warmup:
                    t.append(e0.elapsed_time(e1))
            return float(np.median(t))

        # the two paths agree, bit for bit, before anything is timed
        dev()
        round_trip()
        stream.synchronize()
        count = d_count.cpu().numpy()
        assert torch.equal(d_count, b_count) and torch.equal(d_index, b_index)
        for f in range(n_pairs):
            a0, c = int(off[f]), int(count[f])
            assert torch.equal(d_kf[a0:a0 + c].view(torch.int32), b_kf[a0:a0 + c].view(torch.int32))
            assert torch.equal(d_kt[a0:a0 + c].view(torch.int32), b_kt[a0:a0 + c].view(torch.int32)) and torch.equal(d_ka[a0:a0 + c], b_ka[a0:a0 + c])

        kinds = {"dev": (dev, a.reps), "round trip": (round_trip, max(5, a.reps // 5))}      # the round trip takes long: a fifth of the repetitions
        med = {k: {"wall_ms": [], "dev_ms": []} for k in kinds}
        for rnd in range(a.rounds):
            for k, (call, reps) in kinds.items():
                wall = []
                warm = a.warmup if k == "dev" else 1
                for i in range(warm + reps):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    call()
                    stream.synchronize()
                    if i >= warm:
                        wall.append((time.perf_counter() - t0) * 1e3)
                med[k]["wall_ms"].append(float(np.median(wall)))
                if k == "dev":
                    med[k]["dev_ms"].append(events(call, a.reps, a.warmup))
        res = {"case": name, "pairs": n_pairs, "reps": a.reps, "rounds": a.rounds, "kept": count.tolist()}
        for k in kinds:
            res[k] = {e: summary(v) for e, v in med[k].items() if v}
        base, d = res["round trip"]["wall_ms"], res["dev"]["wall_ms"]
        res["dev"]["no_slower_than_round_trip"] = bool(d["median"] <= base["median"] + (base["high"] - base["low"]))
        res["dev"]["us_per_corner"] = round(res["dev"]["dev_ms"]["median"] * 1e3 / N, 4)
        res["round trip"]["us_per_corner"] = round(base["median"] * 1e3 / N, 4)
        print(json.dumps(res), flush=True)
        lines.append("    %s: %d pair(s), kept %s" % (name, n_pairs, count.tolist()))
        for k in kinds:
            for e, v in res[k].items():
                if isinstance(v, dict):
                    lines.append("    %-24s %-11s %-8s median %9.4f ms per call   rounds %9.4f .. %9.4f" % (name, k, e, v["median"], v["low"], v["high"]))
        lines.append("    %-24s per corner: dev_ms %.4f us, round trip wall %.4f us" % (name, res["dev"]["us_per_corner"], res["round trip"]["us_per_corner"]))
        lines.append("    %-24s dev no slower than the host round trip beyond its spread: %s" % (name, res["dev"]["no_slower_than_round_trip"]))
        eng.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
