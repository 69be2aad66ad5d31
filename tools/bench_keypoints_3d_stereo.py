"""Times lcd_keypoints_3d_stereo_dev next to the only path the engine offered a stereo caller whose extractor and camera leave their output
in device memory before: synchronise, both images and the keypoints to the host, the host mirror on one core
(StereoOpticalFlowHip::computeCorrespondences with updateStatus, generateKeypoints3DStereo, filterKeypointsByDepth), then points, index list
and counts back and a gather of the descriptors on the device.  Both sides run in the same process on the same data (needs an MI355X; there
is no CPU fallback).

    python tools/bench_keypoints_3d_stereo.py [--reps 50] [--warmup 5] [--rounds 5] [--out profiles/keypoints_3d_stereo_bench.txt]

Cases (SURF rows, 64 floats, the reference's Stereo/* defaults, the 3-D filter): 1000 keypoints on 640 x 480 and on 1241 x 376 (KITTI),
5000 keypoints on 640 x 480, and eight frames of 1000 in one call.  Per case `rounds` rounds; a round times, each as the median over `reps`
repetitions after `warmup`:
  wall_ms   a host clock from "keypoints and images are complete on the device" (a synchronised stream) to "points, counts and compacted
            rows are complete on the device" (the stream synchronised again), for the device entry and the round trip alike
  dev_ms    HIP events on the engine's stream around ONE call of the device entry
Reported per call: the median of the rounds' medians and their spread (lowest .. highest round).  The expectation -- the device entry's
wall_ms no larger than the host round trip's beyond that baseline's own spread over the rounds -- is evaluated and printed as it comes out.
The two paths' results are compared bit for bit before a number is reported.  Behind the cases a breakdown by HIP events on 640 x 480: one
keypoint and 1000, with max_level 0, 2 and 5 (one keypoint leaves the pyramid and the fixed costs; the rest is the tracker's and the
emit's).  One JSON line per case; --out also writes the table."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIN_DEPTH, MAX_DEPTH = 0.5, 40.0
TILT = [0.0, 0.0, 1.0, 0.05, -1.0, 0.0, 0.0, -0.1, 0.0, -1.0, 0.0, 0.3]


def summary(round_medians_ms):
    m = np.asarray(round_medians_ms, np.float64)
    return {"median": round(float(np.median(m)), 4), "low": round(float(m.min()), 4), "high": round(float(m.max()), 4)}


def stereo_pair(rng, width, height):
    """a smooth random texture and the same scene seen with a disparity that grows from 2 to 30 pixels down the image"""
    a = rng.standard_normal((height, width + 64))
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    for _ in range(3):
        a = sum(k[i] * np.roll(a, i - 2, 0) for i in range(5))
        a = sum(k[i] * np.roll(a, i - 2, 1) for i in range(5))
    a = (a - a.min()) / (a.max() - a.min()) * 255.0
    x = np.arange(width)[None, :] + 32.0
    d = np.linspace(2.0, 30.0, height)[:, None]
    xs = x + d
    i0 = np.floor(xs).astype(int)
    t = xs - i0
    rows = np.arange(height)[:, None]
    right = a[rows, i0] * (1 - t) + a[rows, i0 + 1] * t
    left = a[:, 32:32 + width]
    return np.rint(left).astype(np.uint8), np.rint(right).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 50 or a.rounds < 5:
        sys.exit("bench_keypoints_3d_stereo.py: at least 50 repetitions and 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_keypoints_3d_stereo.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    from rtabmap_amd import synth, vwdictionary as V

    # name, keypoints per frame, width, height, frames
    cases = [("1000 on 640x480", 1000, 640, 480, 1), ("1000 on 1241x376", 1000, 1241, 376, 1), ("5000 on 640x480", 5000, 640, 480, 1),
             ("8 x (1000 on 640x480)", 1000, 640, 480, 8)]
    stream = torch.cuda.Stream()
    lines = []
    for name, n, width, height, n_frames in cases:
        rng = np.random.default_rng(n + n_frames + width)
        N = n * n_frames
        off = np.arange(0, N + 1, n, dtype=np.int64)
        cam = dict(fx=718.0, fy=718.0, cx=width / 2 - 0.5, cy=height / 2 - 0.5, right_cx=width / 2 - 0.5, baseline=0.54, transform=TILT)
        pairs = [stereo_pair(rng, width, height) for _ in range(n_frames)]
        pts = (np.array([20.0, 8.0]) + rng.random((N, 2)) * np.array([width - 41, height - 17])).astype(np.float32)
        rows = synth.vocab_surf(N, seed=n)
        eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_left = [torch.from_numpy(l).cuda() for l, _ in pairs]
            d_right = [torch.from_numpy(r).cuda() for _, r in pairs]
            d_pts, d_rows = torch.from_numpy(pts).cuda(), torch.from_numpy(rows).cuda()
            d_count, d_index = torch.zeros(n_frames, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
            d_xyz, d_out_pts, d_out = torch.zeros((N, 3), device="cuda"), torch.zeros((N, 2), device="cuda"), torch.zeros_like(d_rows)
            b_count, b_index = torch.zeros_like(d_count), torch.zeros_like(d_index)
            b_xyz, b_out_pts, b_out = torch.zeros_like(d_xyz), torch.zeros_like(d_out_pts), torch.zeros_like(d_rows)
        stream.synchronize()
        images = [dict(left=l, right=r, camera=cam) for l, r in zip(d_left, d_right)]

        def dev(params=None, points=d_pts, offsets=off, imgs=images):
            eng.keypoints_3d_stereo_dev(points, offsets, imgs, d_count, d_index, d_xyz, params=params, filter="filter_3d", min_depth=MIN_DEPTH,
                                        max_depth=MAX_DEPTH, d_rows=d_rows, d_out_points=d_out_pts, d_out_rows=d_out)

        def round_trip():
            with torch.cuda.stream(stream):
                stream.synchronize()
                h_pts = d_pts.cpu().numpy()
                xyz, index, count = np.zeros((N, 3), np.float32), np.full(N, -1, np.int32), np.zeros(n_frames, np.int32)
                out_pts = np.zeros((N, 2), np.float32)
                kept_all = []
                for f in range(n_frames):
                    h_left, h_right = d_left[f].cpu().numpy(), d_right[f].cpu().numpy()
                    a0 = int(off[f])
                    p = h_pts[a0:a0 + n]
                    right, status = V.stereo_correspondences(h_left, h_right, p)
                    x = V.generate_keypoints_3d_stereo(p, right, cam, status, MIN_DEPTH, MAX_DEPTH)
                    kept = V.filter_keypoints_by_depth_3d(x, MIN_DEPTH, MAX_DEPTH)
                    k = kept.shape[0]
                    xyz[a0:a0 + k], out_pts[a0:a0 + k], index[a0:a0 + k], count[f] = x[kept], p[kept], kept, k
                    kept_all.append(kept)
                b_xyz.copy_(torch.from_numpy(xyz), non_blocking=True)
                b_index.copy_(torch.from_numpy(index), non_blocking=True)
                b_count.copy_(torch.from_numpy(count), non_blocking=True)
                b_out_pts.copy_(torch.from_numpy(out_pts), non_blocking=True)
                for f in range(n_frames):
                    idx = torch.from_numpy(kept_all[f].astype(np.int64) + int(off[f])).cuda(non_blocking=True)
                    b_out[int(off[f]):int(off[f]) + kept_all[f].shape[0]] = d_rows.index_select(0, idx)

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

        kinds = {"dev": dev, "round trip": round_trip}
        med = {k: {"wall_ms": [], "dev_ms": []} for k in kinds}
        for rnd in range(a.rounds):
            for k, call in kinds.items():
                wall = []
                for i in range(a.warmup + a.reps):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    call()
                    stream.synchronize()
                    if i >= a.warmup:
                        wall.append((time.perf_counter() - t0) * 1e3)
                med[k]["wall_ms"].append(float(np.median(wall)))
                if k == "dev":
                    med[k]["dev_ms"].append(events(call, a.reps, a.warmup))
        # the two paths agree, bit for bit, on what was timed
        dev()
        stream.synchronize()
        count = d_count.cpu().numpy()
        assert torch.equal(d_count, b_count)
        for f in range(n_frames):
            a0, c = int(off[f]), int(count[f])
            assert torch.equal(d_index[a0:a0 + n], b_index[a0:a0 + n])
            assert torch.equal(d_xyz[a0:a0 + c].view(torch.int32), b_xyz[a0:a0 + c].view(torch.int32))
            assert torch.equal(d_out_pts[a0:a0 + c], b_out_pts[a0:a0 + c]) and torch.equal(d_out[a0:a0 + c], b_out[a0:a0 + c])
        res = {"case": name, "frames": n_frames, "reps": a.reps, "rounds": a.rounds, "kept": count.tolist()}
        for k in kinds:
            res[k] = {e: summary(v) for e, v in med[k].items() if v}
        base, d = res["round trip"]["wall_ms"], res["dev"]["wall_ms"]
        res["dev"]["no_slower_than_round_trip"] = bool(d["median"] <= base["median"] + (base["high"] - base["low"]))
        print(json.dumps(res), flush=True)
        lines.append("    %s: %d frame(s), kept %s" % (name, n_frames, count.tolist()))
        for k in kinds:
            for e, v in res[k].items():
                if isinstance(v, dict):
                    lines.append("    %-24s %-11s %-8s median %9.4f ms per call   rounds %9.4f .. %9.4f" % (name, k, e, v["median"], v["low"], v["high"]))
        lines.append("    %-24s dev no slower than the host round trip beyond its spread: %s" % (name, res["dev"]["no_slower_than_round_trip"]))
        if name == "1000 on 640x480":                                      # where the time goes: one keypoint against 1000, by the top level
            one_off = np.array([0, 1], np.int64)
            for max_level in (0, 2, 5):
                p = dict(max_level=max_level)
                t1 = events(lambda: dev(p, d_pts[:1], one_off), a.reps, a.warmup)
                tn = events(lambda: dev(p), a.reps, a.warmup)
                out = {"breakdown": name, "max_level": max_level, "dev_ms_1_keypoint": round(t1, 4), "dev_ms_1000_keypoints": round(tn, 4)}
                print(json.dumps(out), flush=True)
                lines.append("    breakdown %-14s max_level %d   dev_ms with 1 keypoint %8.4f   with 1000 %8.4f" % (name, max_level, t1, tn))
        eng.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
