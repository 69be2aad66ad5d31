"""Times lcd_keypoints_3d_dev next to the only path the engine offered an RGB-D caller whose extractor and camera leave their output in
device memory before: synchronise, keypoints and the depth image to the host, the host mirror (Keypoints3D::generateKeypoints3DDepth and
filterKeypointsByDepth), then points, index list and counts back and a gather of the descriptors on the device.  Both sides run in the
same process on the same data (needs an MI355X; there is no CPU fallback).

    python tools/bench_keypoints_3d.py [--reps 60] [--warmup 10] [--rounds 5] [--out profiles/keypoints_3d_bench.txt]

Cases (SURF rows, 64 floats): 1000 keypoints on a 640 x 480 u16 image with and without the 3-D filter, the same with four cameras on
2560 x 480, 5000 keypoints on an f32 image, and eight frames of 1000 in one call.  Per case `rounds` rounds; a round times, each as the
median over `reps` repetitions after `warmup`:
  wall_ms   a host clock from "keypoints and depth image are complete on the device" (a synchronised stream) to "points, counts and
            compacted rows are complete on the device" (the stream synchronised again), for the device entry and the round trip alike
  dev_ms    HIP events on the engine's stream around ONE call of the device entry
Reported per call: the median of the rounds' medians and their spread (lowest .. highest round).  The expectation -- the device entry's
wall_ms no larger than the host round trip's beyond that baseline's own spread over the rounds -- is evaluated and printed as it comes out.
The two paths' results are compared bit for bit before a number is reported.  One JSON line per case; --out also writes the table."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIN_DEPTH, MAX_DEPTH = 0.5, 3.5
TILT = [0.0, 0.0, 1.0, 0.05, -1.0, 0.0, 0.0, -0.1, 0.0, -1.0, 0.0, 0.3]


def summary(round_medians_ms):
    m = np.asarray(round_medians_ms, np.float64)
    return {"median": round(float(np.median(m)), 4), "low": round(float(m.min()), 4), "high": round(float(m.max()), 4)}


def depth_image(rng, width, height, f32):
    yy, xx = np.mgrid[0:height, 0:width]
    z = 2.5 + 1.4 * np.sin(xx * 0.011) * np.cos(yy * 0.013)
    z = z * (1 + 0.004 * rng.standard_normal(z.shape))
    hole = rng.random(z.shape) < 0.1
    if f32:
        d = z.astype(np.float32)
        d[hole] = np.nan
        return d
    d = np.round(z * 1000).astype(np.uint16)
    d[hole] = 0
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 50 or a.rounds < 5:
        sys.exit("bench_keypoints_3d.py: at least 50 repetitions and 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_keypoints_3d.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    from rtabmap_amd import synth, vwdictionary as V

    # name, keypoints per frame, width, height, cameras, f32, filter, frames
    cases = [("1000 on 640x480 u16, 3-D filter", 1000, 640, 480, 1, False, "filter_3d", 1),
             ("1000 on 640x480 u16, no filter", 1000, 640, 480, 1, False, "keep_all", 1),
             ("1000 on 2560x480 u16, 4 cameras, 3-D filter", 1000, 2560, 480, 4, False, "filter_3d", 1),
             ("1000 on 2560x480 u16, 4 cameras, no filter", 1000, 2560, 480, 4, False, "keep_all", 1),
             ("5000 on 640x480 f32, 3-D filter", 5000, 640, 480, 1, True, "filter_3d", 1),
             ("8 x (1000 on 640x480 u16), 3-D filter", 1000, 640, 480, 1, False, "filter_3d", 8)]
    stream = torch.cuda.Stream()
    lines = []
    for name, n, width, height, n_cam, f32, flt, n_frames in cases:
        rng = np.random.default_rng(n + n_frames + n_cam)
        N = n * n_frames
        filtered = flt != "keep_all"
        off = np.arange(0, N + 1, n, dtype=np.int64)
        sub = width // n_cam
        cams = [dict(fx=525.0 + c, fy=525.0 + c, cx=sub / 2 - 0.5 + c, cy=height / 2 - 0.5, transform=TILT) for c in range(n_cam)]
        depths = [depth_image(rng, width, height, f32) for _ in range(n_frames)]
        pts = (rng.random((N, 2)) * np.array([width - 1, height - 1])).astype(np.float32)
        rows = synth.vocab_surf(N, seed=n)
        eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_depth = [torch.from_numpy(d.view(np.int16) if not f32 else d).cuda() for d in depths]
            d_pts, d_rows = torch.from_numpy(pts).cuda(), torch.from_numpy(rows).cuda()
            d_count, d_index = torch.zeros(n_frames, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
            d_xyz, d_out_pts, d_out = torch.zeros((N, 3), device="cuda"), torch.zeros((N, 2), device="cuda"), torch.zeros_like(d_rows)
            b_count, b_index = torch.zeros_like(d_count), torch.zeros_like(d_index)
            b_xyz, b_out_pts, b_out = torch.zeros_like(d_xyz), torch.zeros_like(d_out_pts), torch.zeros_like(d_rows)
        stream.synchronize()
        images = [dict(data=d, cameras=cams, type=1 if f32 else 0) for d in d_depth]
        state = {}

        def dev():
            eng.keypoints_3d_dev(d_pts, off, images, d_count, d_index, d_xyz, filter=flt, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH,
                                 d_rows=d_rows if filtered else None, d_out_points=d_out_pts, d_out_rows=d_out)

        def round_trip():
            with torch.cuda.stream(stream):
                stream.synchronize()
                h_pts = d_pts.cpu().numpy()
                xyz, index, count = np.zeros((N, 3), np.float32), np.full(N, -1, np.int32), np.zeros(n_frames, np.int32)
                out_pts = np.zeros((N, 2), np.float32)
                kept_all = []
                for f in range(n_frames):
                    h_depth = d_depth[f].cpu().numpy()
                    h_depth = h_depth if f32 else h_depth.view(np.uint16)
                    a0 = int(off[f])
                    p = h_pts[a0:a0 + n]
                    x = V.generate_keypoints_3d_depth(p, h_depth, cams, MIN_DEPTH, MAX_DEPTH)
                    kept = V.filter_keypoints_by_depth_3d(x, MIN_DEPTH, MAX_DEPTH) if filtered else np.arange(n, dtype=np.int32)
                    k = kept.shape[0]
                    xyz[a0:a0 + k], out_pts[a0:a0 + k], index[a0:a0 + k], count[f] = x[kept], p[kept], kept, k
                    kept_all.append(kept)
                state["kept"] = kept_all
                b_xyz.copy_(torch.from_numpy(xyz), non_blocking=True)
                b_index.copy_(torch.from_numpy(index), non_blocking=True)
                b_count.copy_(torch.from_numpy(count), non_blocking=True)
                if filtered:
                    b_out_pts.copy_(torch.from_numpy(out_pts), non_blocking=True)
                    for f in range(n_frames):
                        idx = torch.from_numpy(kept_all[f].astype(np.int64) + int(off[f])).cuda(non_blocking=True)
                        b_out[int(off[f]):int(off[f]) + kept_all[f].shape[0]] = d_rows.index_select(0, idx)

        kinds = {"dev": dev, "round trip": round_trip}
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
        # the two paths agree, bit for bit, on what was timed
        count = d_count.cpu().numpy()
        assert torch.equal(d_count, b_count)
        for f in range(n_frames):
            a0, c = int(off[f]), int(count[f])
            assert torch.equal(d_index[a0:a0 + n], b_index[a0:a0 + n])
            assert torch.equal(d_xyz[a0:a0 + c].view(torch.int32), b_xyz[a0:a0 + c].view(torch.int32))
            if filtered:
                assert torch.equal(d_out_pts[a0:a0 + c], b_out_pts[a0:a0 + c]) and torch.equal(d_out[a0:a0 + c], b_out[a0:a0 + c])
        eng.close()
        res = {"case": name, "frames": n_frames, "reps": a.reps, "rounds": a.rounds, "kept": count.tolist(), "launches_per_call": 1}
        for k in kinds:
            res[k] = {e: summary(v) for e, v in med[k].items() if v}
        base, d = res["round trip"]["wall_ms"], res["dev"]["wall_ms"]
        res["dev"]["no_slower_than_round_trip"] = bool(d["median"] <= base["median"] + (base["high"] - base["low"]))
        print(json.dumps(res), flush=True)
        lines.append("    %s: %d frame(s), kept %s" % (name, n_frames, count.tolist()))
        for k in kinds:
            for e, v in res[k].items():
                if isinstance(v, dict):
                    lines.append("    %-46s %-11s %-8s median %8.4f ms per call   rounds %8.4f .. %8.4f" % (name, k, e, v["median"], v["low"], v["high"]))
        lines.append("    %-46s dev no slower than the host round trip beyond its spread: %s" % (name, res["dev"]["no_slower_than_round_trip"]))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
