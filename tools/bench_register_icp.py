"""Times lcd_register_icp_dev next to the only path the engine offered a caller who holds both laser scans in device memory before:
synchronise, both scans to the host, the rule on the CPU (register_icp_cpu of the host mirror, the same arithmetic, brute force), then the
results back.  A second baseline is the float64 ICP of tests/register_icp_model.py over scipy's kd-tree (PCL's search is a kd-tree, and brute
force flatters the device); its results are not compared, it is another computation.  All run in the same process on the same data (needs
an MI355X; there is no CPU fallback).

    python tools/bench_register_icp.py [--reps 60] [--warmup 10] [--rounds 5] [--budget 1.5] [--out profiles/register_icp_bench.txt]

Cases: 2-D scans of 360 and 1081 points and 3-D clouds of 2000 and 8000 points, 30 iterations at the most, 1, 8 and 64 pairs per call, under
LCD_ICP_SEARCH_AUTO; --curve instead times one pair per call under the brute and the grid form over the target size (the AUTO threshold).  Per case `rounds` rounds; a round
times, each as the median over the repetitions after the warm-up:
  wall_ms   a host clock from "both scans are complete on the device" (a synchronised stream) to "every output is complete on the device"
            (the stream synchronised again), for the device entry and the round trip alike
  dev_ms    HIP events on the engine's stream around ONE call of the device entry
  host_ms   lcd_register_icp over host arrays (the host entry: staging, one copy in, the launch, one copy out)
  cpu_ms    register_icp_cpu alone over the pairs, no copies (what the round trip spends computing)
  kd64_ms   the float64 kd-tree ICP alone over the pairs
A path whose single call is long gets fewer repetitions: as many as fit --budget seconds a round, three at the least (warmed up by a fifth
as many calls), and a single call where one alone takes longer than the budget; the number is reported.  The device entry's wall time always gets
the full `reps` after `warmup`.  The CPU paths walk the pairs one
after the other; where one call of them over all pairs would take more than a third of the budget they are timed over the first
`cpu_pairs` pairs and scaled by pairs / cpu_pairs, which the output says.  The device entry's results are compared
bit for bit with the round trip's (over the pairs it computed) before a number is reported.  The expectation -- the device entry's wall_ms,
in a batch of 8 or more, no larger than the round trip's beyond that baseline's own spread over the rounds -- is evaluated and printed as it
comes out.  One JSON line per case; --out also writes the table.

--plane times lcd_register_icp_plane_dev instead, by the same method, on 1, 8 and 64 pairs of 2000 and 8000 3-D points with normals: dev_ms and
wall_ms of the device entry, the host round trip through register_icp_plane_cpu (results compared bit for bit), the float64 point-to-plane ICP
of tests/register_icp_plane_model.py over scipy's kd-tree, and lcd_register_icp_dev (point to point) on the same pairs; both device entries
also per iteration of the pair that took the most (a call lasts as long as its slowest workgroup)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KW = dict(max_iterations=30, max_correspondence_distance=0.3, epsilon=0.0, correspondence_ratio=0.1)
OUTS = ("transform", "icp_transform", "correction", "status", "stop", "iterations", "n_correspondences", "ratio", "variance", "match")


def summary(round_medians_ms):
    m = np.asarray(round_medians_ms, np.float64)
    return {"median": round(float(np.median(m)), 4), "low": round(float(m.min()), 4), "high": round(float(m.max()), 4)}


def curve(a, torch, rtabmap_amd, I, stream):
    """device time of ONE pair per call under LCD_ICP_SEARCH_BRUTE and LCD_ICP_SEARCH_GRID over the target size, at most 5 iterations (the number taken is
    reported): where the grid form overtakes the brute form is icp_rule.h's AUTO_GRID_ROWS"""
    lines = []
    for flat, sizes in ((False, (256, 512, 768, 1024, 1536, 2048, 4096, 8192)), (True, (256, 360, 512, 768, 1081, 1536, 2048))):
        for n in sizes:
            p = I.pair(n, n, flat, 7000 + 64 * n, noise=0.005)
            fx, fo, tx, to, gs = I.concatenate([p])
            eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
            with torch.cuda.stream(stream):
                d_fx, d_tx = torch.from_numpy(fx).cuda(), torch.from_numpy(tx).cuda()
                outs = {s: [torch.zeros((1, 12), device="cuda") for _ in range(3)] + [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(4)] +
                           [torch.zeros(1, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"),
                            torch.zeros(n, dtype=torch.int32, device="cuda")] for s in (1, 2)}
            stream.synchronize()
            res = {"case": "curve", "flat": flat, "points": n}
            for search, name in ((1, "brute"), (2, "grid")):
                rounds = []
                for rnd in range(a.rounds):
                    t = []
                    for i in range(a.warmup + a.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        with torch.cuda.stream(stream):
                            e0.record()
                            eng.register_icp_dev(d_fx, fo, d_tx, to, gs, *outs[search], **dict(KW, max_iterations=5, force_3dof=flat, search=search))
                            e1.record()
                        e1.synchronize()
                        if i >= a.warmup:
                            t.append(e0.elapsed_time(e1))
                    rounds.append(float(np.median(t)))
                res[name] = summary(rounds)
            for x, y in zip(outs[1], outs[2]):                         # the two forms agree bit for bit
                assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
            res["iterations"] = int(outs[1][5].cpu()[0])
            eng.close()
            print(json.dumps(res), flush=True)
            lines.append("    curve %s %5d points, %d iterations: brute %9.4f ms (%9.4f .. %9.4f)   grid %9.4f ms (%9.4f .. %9.4f)" %
                         ("2-D" if flat else "3-D", n, res["iterations"], res["brute"]["median"], res["brute"]["low"], res["brute"]["high"],
                          res["grid"]["median"], res["grid"]["low"], res["grid"]["high"]))
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as fh:
                    fh.write("\n".join(lines) + "\n")


def plane(a, torch, rtabmap_amd, stream):
    from rtabmap_amd import capi, vwdictionary as V
    import register_icp_plane_inputs as IP
    import register_icp_plane_model as MP
    kw = dict(IP.KW)
    p2p_kw = {k: kw[k] for k in ("max_iterations", "max_correspondence_distance", "epsilon", "correspondence_ratio")}
    names = [k for k, _, _ in capi.Engine.ICP_PLANE_OUT] + ["match"]
    tdt = {np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}
    lines = []
    for n in (2000, 8000):
        for n_pairs in (1, 8, 64):
            pairs = [IP.pair(n, n, 7000 + 64 * n + k, noise=0.005) for k in range(n_pairs)]
            fx, fn, fo, tx, tn, to, gs = IP.concatenate(pairs)
            eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
            with torch.cuda.stream(stream):
                d_fx, d_fn, d_tx, d_tn = (torch.from_numpy(x).cuda() for x in (fx, fn, tx, tn))
                d = {k: torch.zeros((n_pairs, w) if w else (n_pairs,), dtype=tdt[dt], device="cuda") for k, w, dt in capi.Engine.ICP_PLANE_OUT}
                d["match"] = torch.zeros(fx.shape[0], dtype=torch.int32, device="cuda")
                q = [torch.zeros((n_pairs, 12), device="cuda") for _ in range(3)] + [torch.zeros(n_pairs, dtype=torch.int32, device="cuda") for _ in range(4)] + \
                    [torch.zeros(n_pairs, dtype=torch.float32, device="cuda"), torch.zeros(n_pairs, dtype=torch.float64, device="cuda"),
                     torch.zeros(fx.shape[0], dtype=torch.int32, device="cuda")]
            stream.synchronize()

            def dev():
                eng.register_icp_plane_dev(d_fx, d_fn, fo, d_tx, d_tn, to, gs, d, **kw)

            def p2p():
                eng.register_icp_dev(d_fx, fo, d_tx, to, gs, *q, **p2p_kw)

            def events(call):
                rounds = []
                for rnd in range(a.rounds):
                    t = []
                    for i in range(a.warmup + a.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        with torch.cuda.stream(stream):
                            e0.record()
                            call()
                            e1.record()
                        e1.synchronize()
                        if i >= a.warmup:
                            t.append(e0.elapsed_time(e1))
                    rounds.append(float(np.median(t)))
                return rounds

            def wall(call, reps, warm, factor=1.0):
                rounds = []
                for rnd in range(a.rounds):
                    t = []
                    for i in range(warm + reps):
                        stream.synchronize()
                        t0 = time.perf_counter()
                        call()
                        stream.synchronize()
                        if i >= warm:
                            t.append((time.perf_counter() - t0) * 1e3 * factor)
                    rounds.append(float(np.median(t)))
                return rounds

            def cpu(h):
                out = []
                for k in range(cpu_pairs):
                    out.append(V.register_icp_plane_cpu(h[0][fo[k]:fo[k + 1]], h[1][fo[k]:fo[k + 1]], h[2][to[k]:to[k + 1]], h[3][to[k]:to[k + 1]], gs[k], **kw))
                return out

            def round_trip():
                stream.synchronize()
                res = cpu([x.cpu().numpy() for x in (d_fx, d_fn, d_tx, d_tn)])
                with torch.cuda.stream(stream):
                    back[0] = torch.from_numpy(np.stack([r["transform"] for r in res])).cuda()
                return res

            def kd64():
                for p in pairs[:cpu_pairs]:
                    MP.icp_plane64(p["from_xyz"], p["to_xyz"], p["to_normals"], p["guess"], max_iterations=kw["max_iterations"],
                                   max_correspondence_distance=kw["max_correspondence_distance"])

            back = [None]
            cpu_pairs = 1
            t0 = time.perf_counter()
            first = round_trip()
            one_pair = time.perf_counter() - t0
            cpu_pairs = int(min(n_pairs, max(1, a.budget / 3 // max(one_pair, 1e-6))))
            scale = n_pairs / cpu_pairs
            cpu_reps = int(min(a.reps, max(3, a.budget // max(one_pair * cpu_pairs, 1e-6)))) if one_pair * cpu_pairs <= a.budget else 1
            res = {"case": "%d x (3-D clouds with normals, %d points a side, at most 30 iterations)" % (n_pairs, n), "pairs": n_pairs, "points": n,
                   "rounds": a.rounds, "reps": a.reps, "cpu_reps": cpu_reps, "cpu_pairs": cpu_pairs, "launches_per_call": 1}
            res["plane dev_ms"] = summary(events(dev))
            res["plane wall_ms"] = summary(wall(dev, a.reps, a.warmup))
            res["point-to-point dev_ms"] = summary(events(p2p))
            res["round trip wall_ms"] = summary(wall(round_trip, cpu_reps, 1 if cpu_reps > 1 else 0, scale))
            res["kd-tree float64 wall_ms"] = summary(wall(kd64, cpu_reps, 1 if cpu_reps > 1 else 0, scale))
            stream.synchronize()
            got = {k: v.cpu().numpy() for k, v in d.items()}
            for k, r in enumerate(round_trip()):                       # the two paths agree, bit for bit, on what was timed
                for key in names[:-1]:
                    assert np.array_equal(np.ascontiguousarray(got[key][k]).view(np.uint8), np.ascontiguousarray(r[key], got[key].dtype).view(np.uint8)), key
                assert np.array_equal(got["match"][fo[k]:fo[k + 1]], r["match"])
            it_plane, it_p2p = got["iterations"].tolist(), q[5].cpu().numpy().tolist()
            res["iterations"] = {"plane": it_plane[:8], "point-to-point": it_p2p[:8], "branch": got["branch"].tolist()[:8]}
            res["per iteration dev_ms"] = {"plane": round(res["plane dev_ms"]["median"] / max(max(it_plane), 1), 4),
                                           "point-to-point": round(res["point-to-point dev_ms"]["median"] / max(max(it_p2p), 1), 4)}
            base, dv = res["round trip wall_ms"], res["plane wall_ms"]
            res["dev no slower than the round trip"] = bool(dv["median"] <= base["median"] + (base["high"] - base["low"]))
            eng.close()
            print(json.dumps(res), flush=True)
            lines.append("    %s: CPU paths over %d of %d pairs%s, %d repetitions of them" % (res["case"], cpu_pairs, n_pairs, "" if cpu_pairs == n_pairs else " and scaled", cpu_reps))
            lines.append("    iterations plane %s, point to point %s" % (it_plane[:8], it_p2p[:8]))
            for k in ("plane dev_ms", "plane wall_ms", "point-to-point dev_ms", "round trip wall_ms", "kd-tree float64 wall_ms"):
                v = res[k]
                lines.append("    %-26s median %11.4f ms per call   rounds %11.4f .. %11.4f   per pair %10.4f ms" % (k, v["median"], v["low"], v["high"], v["median"] / n_pairs))
            lines.append("    per iteration of the slowest pair: plane %.4f ms, point to point %.4f ms; dev no slower than the round trip beyond its spread: %s" %
                         (res["per iteration dev_ms"]["plane"], res["per iteration dev_ms"]["point-to-point"], res["dev no slower than the round trip"]))
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as fh:
                    fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=1.5)
    ap.add_argument("--out", default="")
    ap.add_argument("--curve", action="store_true", help="only the two search forms' curves over the target size")
    ap.add_argument("--plane", action="store_true", help="lcd_register_icp_plane_dev instead: 3-D clouds with normals")
    a = ap.parse_args()
    if a.reps < 50 or a.rounds < 5:
        sys.exit("bench_register_icp.py: at least 50 repetitions and 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_register_icp.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    from rtabmap_amd import vwdictionary as V
    import register_icp_inputs as I
    import register_icp_model as M

    stream = torch.cuda.Stream()
    lines = []
    if a.curve:
        return curve(a, torch, rtabmap_amd, I, stream)
    if a.plane:
        return plane(a, torch, rtabmap_amd, stream)
    cases = [(flat, n, n_pairs, "") for flat, n in ((True, 360), (True, 1081), (False, 2000), (False, 8000)) for n_pairs in (1, 8, 64)]
    for flat, n, n_pairs, tag in cases:
        name = "%s%d x (%s, %d points a side, at most 30 iterations)" % (tag, n_pairs, "2-D scans" if flat else "3-D clouds", n)
        pairs = [I.pair(n, n, flat, 7000 + 64 * n + k, noise=0.005) for k in range(n_pairs)]
        fx, fo, tx, to, gs = I.concatenate(pairs)
        kw = dict(KW, force_3dof=flat)
        eng = rtabmap_amd.Engine("f32", 64, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            d_fx, d_tx = torch.from_numpy(fx).cuda(), torch.from_numpy(tx).cuda()
            f32, i32 = torch.float32, torch.int32
            mk = lambda: dict(transform=torch.zeros((n_pairs, 12), device="cuda"), icp_transform=torch.zeros((n_pairs, 12), device="cuda"),
                              correction=torch.zeros((n_pairs, 12), device="cuda"), status=torch.zeros(n_pairs, dtype=i32, device="cuda"),
                              stop=torch.zeros(n_pairs, dtype=i32, device="cuda"), iterations=torch.zeros(n_pairs, dtype=i32, device="cuda"),
                              n_correspondences=torch.zeros(n_pairs, dtype=i32, device="cuda"), ratio=torch.zeros(n_pairs, dtype=f32, device="cuda"),
                              variance=torch.zeros(n_pairs, dtype=torch.float64, device="cuda"), match=torch.zeros(fx.shape[0], dtype=i32, device="cuda"))
            d, b = mk(), mk()
        stream.synchronize()
        cpu_pairs = [n_pairs]

        def dev():
            eng.register_icp_dev(d_fx, fo, d_tx, to, gs, *(d[k] for k in OUTS), **kw)

        def cpu(h_fx, h_tx):
            p = cpu_pairs[0]
            res = {k: np.zeros(tuple(b[k].shape), b[k].cpu().numpy().dtype) for k in OUTS}
            for k in range(p):
                r = V.register_icp_cpu(h_fx[fo[k]:fo[k + 1]], h_tx[to[k]:to[k + 1]], gs[k], **kw)
                for key in OUTS[:-1]:
                    res[key][k] = r[key]
                res["match"][fo[k]:fo[k + 1]] = r["match"]
            return res

        def round_trip():
            with torch.cuda.stream(stream):
                stream.synchronize()
                res = cpu(d_fx.cpu().numpy(), d_tx.cpu().numpy())
                for key in OUTS:
                    b[key].copy_(torch.from_numpy(res[key]), non_blocking=True)

        def host():
            eng.register_icp(fx, fo, tx, to, gs, **kw)

        def cpu_only():
            cpu(fx, tx)

        def kd64():
            for p in pairs[:cpu_pairs[0]]:
                M.icp64(*I.scans(p), max_iterations=kw["max_iterations"], force_3dof=flat, max_correspondence_distance=kw["max_correspondence_distance"])

        # one pair on the CPU tells how many pairs a call of the CPU paths may walk
        cpu_pairs[0] = 1
        t0 = time.perf_counter()
        cpu_only()
        one_pair = time.perf_counter() - t0
        cpu_pairs[0] = int(min(n_pairs, max(1, a.budget / 3 // max(one_pair, 1e-6))))
        scale = n_pairs / cpu_pairs[0]

        kinds = {"dev": dev, "round trip": round_trip, "host entry": host, "register_icp_cpu": cpu_only, "kd-tree float64": kd64}
        med = {k: {"wall_ms": [], "dev_ms": []} for k in kinds}
        used = {}
        for rnd in range(a.rounds):
            for k, call in kinds.items():
                factor = scale if k in ("round trip", "register_icp_cpu", "kd-tree float64") else 1.0
                stream.synchronize()
                t0 = time.perf_counter()
                call()
                stream.synchronize()
                once = time.perf_counter() - t0
                reps = int(min(a.reps, max(3, a.budget // max(once, 1e-6)))) if once <= a.budget else 1
                if k == "dev":
                    reps = a.reps                                          # the claim rests on it: always the full protocol
                warm = min(a.warmup, max(1, reps // 5)) if reps > 1 else 0
                used[k] = reps
                wall, devt = [], []
                if reps == 1:                                              # a call longer than the budget: the call just made is the sample
                    wall.append(once * 1e3 * factor)
                for i in range(warm + reps if reps > 1 else 0):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    call()
                    stream.synchronize()
                    if i >= warm:
                        wall.append((time.perf_counter() - t0) * 1e3 * factor)
                med[k]["wall_ms"].append(float(np.median(wall)))
                if k != "dev":
                    continue
                ev_reps = int(min(a.reps, max(3, a.budget // max(once, 1e-6))))      # (the events' window is budgeted like the other paths)
                for i in range(warm + ev_reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(stream):
                        e0.record()
                        call()
                        e1.record()
                    e1.synchronize()
                    if i >= warm:
                        devt.append(e0.elapsed_time(e1))
                med[k]["dev_ms"].append(float(np.median(devt)))
        p, rows = cpu_pairs[0], int(fo[cpu_pairs[0]])
        for key in OUTS:                                               # the two paths agree, bit for bit, on what was timed
            cut = rows if key == "match" else p
            assert torch.equal(d[key][:cut].contiguous().view(torch.uint8), b[key][:cut].contiguous().view(torch.uint8)), key
        iterations = d["iterations"].cpu().numpy().tolist()
        eng.close()
        res = {"case": name, "pairs": n_pairs, "points": n, "flat": flat, "rounds": a.rounds, "reps": used, "cpu_pairs": p, "iterations": iterations[:8],
               "launches_per_call": 1}
        for k in kinds:
            res[k] = {e: summary(v) for e, v in med[k].items() if v}
            res[k]["per_pair_ms"] = round(res[k]["dev_ms" if k == "dev" else "wall_ms"]["median"] / n_pairs, 4)
        base, dv = res["round trip"]["wall_ms"], res["dev"]["wall_ms"]
        res["dev"]["no_slower_than_round_trip"] = bool(dv["median"] <= base["median"] + (base["high"] - base["low"]))
        print(json.dumps(res), flush=True)
        lines.append("    %s: iterations %s; repetitions %s; CPU paths over %d of %d pairs%s" %
                     (name, iterations[:8], used, p, n_pairs, "" if p == n_pairs else " and scaled"))
        for k in kinds:
            for e, v in res[k].items():
                if isinstance(v, dict):
                    lines.append("    %-16s %-8s median %11.4f ms per call   rounds %11.4f .. %11.4f   per pair %10.4f ms" %
                                 (k, e, v["median"], v["low"], v["high"], v["median"] / n_pairs))
        lines.append("    dev no slower than the host round trip beyond its spread: %s" % res["dev"]["no_slower_than_round_trip"])
        if a.out:                                                      # after every case: what is done is kept if a later case is cut short
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
