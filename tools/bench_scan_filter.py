"""Times lcd_filter_scans_dev on one GPU against the host round trip through filter_scans_cpu, the float64 kd-tree pipeline of the accuracy
test, and the ICP call that follows on the same scans.  Medians over rounds, as tools/bench_register_icp.py --plane reports them.

    python tools/bench_scan_filter.py [--rounds 5] [--reps 20] [--budget 4] [--out profiles/scan_filter_timing.txt]

Shapes: 1, 8 and 64 scans of 2 000, 8 000 and 16 384 raw points of the room scene (5 mm noise) at leaf 0.05 and K = 5 -- 16 384 points also at leaf
0.1, because at 0.05 more than 8 192 voxels reach the normals --, and one radius case.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(v):
    return {"median": float(np.median(v)), "low": float(np.min(v)), "high": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--budget", type=float, default=4.0, help="seconds a CPU path may take per round; it walks fewer scans and is scaled")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rtabmap_amd
    from rtabmap_amd import capi, vwdictionary as V
    import register_icp_plane_inputs as PI
    import scan_filter_model as M

    stream = torch.cuda.Stream()
    shapes = [(ns, n, 0.05, dict(normal_k=5)) for n in (2000, 8000, 16384) for ns in (1, 8, 64)]
    shapes += [(ns, 16384, 0.1, dict(normal_k=5)) for ns in (1, 8, 64)] + [(8, 8000, 0.05, dict(normal_radius=0.15))]
    lines = []
    for ns, n, leaf, nkw in shapes:
        kw = dict(voxel_size=leaf, **nkw)
        name = "%d x %d points, leaf %.2f, %s" % (ns, n, leaf, "K = %d" % nkw["normal_k"] if "normal_k" in nkw else "radius %.2f" % nkw["normal_radius"])
        scans = []
        for k in range(ns):
            rng = np.random.default_rng(9000 + 64 * n + k)
            scans.append((PI.room(rng, n)[0] + rng.normal(0, 0.005, (n, 3)) + np.array([-2, -1.5, -1.2])).astype(np.float32))
        cap = min(n, 8192)
        x = np.concatenate(scans)
        off, oo = np.arange(ns + 1, dtype=np.int64) * n, np.arange(ns + 1, dtype=np.int64) * cap
        eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
        i32 = torch.int32
        with torch.cuda.stream(stream):
            d_x = torch.from_numpy(x).cuda()
            mk = lambda: dict(xyz=torch.zeros((ns * cap, 3), device="cuda"), normals=torch.zeros((ns * cap, 3), device="cuda"),
                              count=torch.zeros(ns, dtype=i32, device="cuda"), stage_counts=torch.zeros((ns, 3), dtype=i32, device="cuda"),
                              status=torch.zeros(ns, dtype=i32, device="cuda"))
            d, b = mk(), mk()
            n_pairs = max(ns // 2, 1)
            icp = {}
            for key, w, dt in capi.Engine.ICP_PLANE_OUT:
                tdt = {np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}[dt]
                icp[key] = torch.zeros((n_pairs, w) if w else (n_pairs,), dtype=tdt, device="cuda")
            icp["match"] = torch.zeros(n_pairs * cap, dtype=i32, device="cuda")
        stream.synchronize()
        cpu_scans = [ns]
        ident = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (n_pairs, 1))
        po = np.arange(n_pairs + 1, dtype=np.int64) * cap

        def dev():
            eng.filter_scans_dev(d_x, off, oo, d, **kw)

        def icp_after():                                                # scan i of the first half against scan i of the second (a single scan against itself); the offsets are the regions'
            first = n_pairs * cap if ns > 1 else 0
            eng.register_icp_plane_dev(d["xyz"], d["normals"], po, d["xyz"][first:], d["normals"][first:], po, ident, icp, max_iterations=30,
                                       max_correspondence_distance=0.1)

        def cpu(h_x):
            res = {k: np.zeros(tuple(v.shape), v.cpu().numpy().dtype) for k, v in b.items()}
            for k in range(cpu_scans[0]):
                r = V.filter_scans_cpu(h_x[off[k]:off[k + 1]], capacity=cap, **kw)
                res["xyz"][oo[k]:oo[k + 1]], res["normals"][oo[k]:oo[k + 1]] = r["xyz"], r["normals"]
                res["count"][k], res["status"][k], res["stage_counts"][k] = r["count"], r["status"], r["stage_counts"]
            return res

        def round_trip():
            with torch.cuda.stream(stream):
                stream.synchronize()
                res = cpu(d_x.cpu().numpy())
                for key in b:
                    b[key].copy_(torch.from_numpy(res[key]), non_blocking=True)

        def cpu_only():
            cpu(x)

        def kd64():
            if "normal_k" in nkw:
                for s in scans[:cpu_scans[0]]:
                    M.pipeline64(s, leaf, nkw["normal_k"])

        cpu_scans[0] = 1
        t0 = time.perf_counter()
        cpu_only()
        one = time.perf_counter() - t0
        cpu_scans[0] = int(min(ns, max(1, a.budget / 3 // max(one, 1e-6))))
        scale = ns / cpu_scans[0]
        dev()
        stream.synchronize()
        status = d["status"].cpu().numpy()
        kinds = {"dev": dev, "round trip": round_trip, "filter_scans_cpu": cpu_only}
        if "normal_k" in nkw:
            kinds["kd-tree float64"] = kd64
        if (status == 0).all() and int(d["count"].max()) <= 8192:
            kinds["icp behind it"] = icp_after
        med = {k: {"wall_ms": [], "dev_ms": []} for k in kinds}
        for rnd in range(a.rounds):
            for k, call in kinds.items():
                factor = scale if k in ("round trip", "filter_scans_cpu", "kd-tree float64") else 1.0
                on_dev = k in ("dev", "icp behind it")
                stream.synchronize()
                t0 = time.perf_counter()
                call()
                stream.synchronize()
                once = time.perf_counter() - t0
                reps = a.reps if k == "dev" else int(min(a.reps, max(1, a.budget // max(once, 1e-6))))
                warm = min(a.warmup, reps // 2)
                wall, devt = [once * 1e3 * factor] if reps == 1 else [], []
                for i in range(warm + reps if reps > 1 else 0):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    call()
                    stream.synchronize()
                    if i >= warm:
                        wall.append((time.perf_counter() - t0) * 1e3 * factor)
                med[k]["wall_ms"].append(float(np.median(wall)))
                if not on_dev:
                    continue
                for i in range(warm + max(reps, 3)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record()
                        call()
                        e1.record()
                    e1.synchronize()
                    if i >= warm:
                        devt.append(e0.elapsed_time(e1))
                med[k]["dev_ms"].append(float(np.median(devt)))
        dev()
        stream.synchronize()
        p = cpu_scans[0]
        for key in b:                                                   # the two paths agree, bit for bit, on what was timed
            cut = p * cap if key in ("xyz", "normals") else p
            assert torch.equal(d[key][:cut].contiguous().view(torch.uint8), b[key][:cut].contiguous().view(torch.uint8)), key
        stages = d["stage_counts"].cpu().numpy()
        eng.close()
        res = {"case": name, "scans": ns, "points": n, "rounds": a.rounds, "cpu_scans": p, "status": status[:8].tolist(), "stage_counts": stages[0].tolist(),
               "launches_per_call": 3}
        for k in kinds:
            res[k] = {e: summary(v) for e, v in med[k].items() if v}
        print(json.dumps(res), flush=True)
        lines.append("    %s: status %s, stage counts of scan 0 %s; CPU paths over %d of %d scans%s" %
                     (name, status[:8].tolist(), stages[0].tolist(), p, ns, "" if p == ns else " and scaled"))
        for k in kinds:
            for e, v in res[k].items():
                lines.append("    %-18s %-8s median %11.4f ms per call   rounds %11.4f .. %11.4f   per scan %10.4f ms" %
                             (k, e, v["median"], v["low"], v["high"], v["median"] / ns))
        if a.out:                                                       # after every case: what is done is kept if a later case is cut short
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
