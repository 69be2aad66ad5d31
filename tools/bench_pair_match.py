"""Times the two-frame descriptor matching of lcd_match_pairs next to the way a caller had to do it before (needs an MI355X; there is no
CPU fallback).

    python tools/bench_pair_match.py [--reps 60] [--warmup 10] [--out profiles/pair_match.txt]

Per case -- 300 + 300 SURF and 400 + 400 ORB (the sizes of INTEGRATION.md 2d), 1000 + 1000 SURF (Vis/MaxFeatures), and a batch of 8 pairs of
300 + 300 SURF -- and per mode (dictionary, cross-check), the median over `reps` repetitions after `warmup`, with the 10th and 90th
percentile as the spread:
  host_ms     lcd_match_pairs: host rows in, ids out, one synchronisation (a host clock around the call)
  dev_ms      lcd_match_pairs_dev: HIP events on the engine's stream around ONE call (table copy + the two launches)
and, for the dictionary mode of the single pairs, the caller's earlier options in the same process on the same inputs:
  temp_ms     a temporary VWDictionaryHip per pair: create / addNewWords / update / addNewWords / clear / close
  clear_ms    one long-lived VWDictionaryHip: addNewWords / update / addNewWords / clear per pair
Every timed result is compared with the others' (the ids must agree) before a number is reported.  Prints one JSON line per case; --out also
writes the table as text."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_pair(kind, rows, seed):
    """3/4 noisy copies of the from-rows (sigma 0.02, or 2 % bit flips) plus 1/4 fresh rows, as tests/test_gpu_stream.py's frame pair"""
    from rtabmap_amd import synth
    rng = np.random.default_rng(seed)
    if kind == "orb":
        a = rng.integers(0, 256, (rows, 32), dtype=np.uint8)
        b = a[rng.permutation(rows)[: rows * 3 // 4]] ^ np.packbits(rng.random((rows * 3 // 4, 256)) < 0.02, axis=1)
        b = np.concatenate([b, rng.integers(0, 256, (rows - rows * 3 // 4, 32), dtype=np.uint8)])
    else:
        a = synth.vocab_surf(rows, seed=seed)
        b = a[rng.permutation(rows)[: rows * 3 // 4]] + rng.standard_normal((rows * 3 // 4, 64)).astype(np.float32) * np.float32(0.02)
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        b = np.concatenate([b, synth.vocab_surf(rows - rows * 3 // 4, seed=seed + 1)]).astype(np.float32)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def stats(samples_ms, per):
    s = np.sort(np.asarray(samples_ms, np.float64)) / per
    return {"median": round(float(np.median(s)), 4), "p10": round(float(s[int(0.1 * (len(s) - 1))]), 4), "p90": round(float(s[int(np.ceil(0.9 * (len(s) - 1)))]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 50:
        sys.exit("bench_pair_match.py: at least 50 repetitions")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pair_match.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    from rtabmap_amd.vwdictionary import VWDictionaryHip

    cases = [("surf 300+300", "surf", 300, 1), ("orb 400+400", "orb", 400, 1), ("surf 1000+1000", "surf", 1000, 1), ("surf 8 x (300+300)", "surf", 300, 8)]
    stream = torch.cuda.Stream()
    lines = []
    for name, kind, rows, n_pairs in cases:
        pairs = [make_pair(kind, rows, 1000 + 7 * k) for k in range(n_pairs)]
        f = np.concatenate([p[0] for p in pairs]); t = np.concatenate([p[1] for p in pairs])
        fo = np.arange(0, (n_pairs + 1) * rows, rows, dtype=np.int64); to = fo.copy()
        eng = rtabmap_amd.Engine("u8" if kind == "orb" else "f32", f.shape[1], stream=stream.cuda_stream)
        d_f, d_t = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda()
        res = {"case": name, "pairs": n_pairs, "reps": a.reps}
        for mode in ("dictionary", "cross_check"):
            o1 = torch.zeros(f.shape[0] if mode == "dictionary" else t.shape[0], dtype=torch.int32, device="cuda")
            o2 = torch.zeros(t.shape[0], dtype=torch.int32 if mode == "dictionary" else torch.float32, device="cuda")
            host, dev = [], []
            for r in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                got = eng.match_pairs(f, t, fo, to, mode)
                if r >= a.warmup:
                    host.append((time.perf_counter() - t0) * 1e3)
            for r in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    e0.record()
                    eng.match_pairs_dev(d_f, d_t, fo, to, o1, o2, mode)
                    e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    dev.append(e0.elapsed_time(e1))
            np.testing.assert_array_equal(o1.cpu().numpy(), got[0])                    # the two entries agree on what was timed
            np.testing.assert_array_equal(o2.cpu().numpy().view(np.uint32), np.ascontiguousarray(got[1]).view(np.uint32))
            res[mode] = {"host_ms": stats(host, n_pairs), "dev_ms": stats(dev, n_pairs)}
            if mode == "dictionary":
                ref = got
        eng.close()
        if n_pairs == 1:
            temp, clear = [], []
            for r in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                h = VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
                fw = h.add_new_words(f, 1); h.update(); tw = h.add_new_words(t, 2); h.clear(); h.close()
                if r >= a.warmup:
                    temp.append((time.perf_counter() - t0) * 1e3)
            assert fw == ref[0].tolist() and tw == ref[1].tolist()
            h = VWDictionaryHip(nndr=0.8, new_words_compared_together=True)
            for r in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                fw = h.add_new_words(f, 1); h.update(); tw = h.add_new_words(t, 2); h.clear()
                if r >= a.warmup:
                    clear.append((time.perf_counter() - t0) * 1e3)
            assert fw == ref[0].tolist() and tw == ref[1].tolist()
            h.close()
            res["dictionary"]["temp_ms"] = stats(temp, 1)
            res["dictionary"]["clear_ms"] = stats(clear, 1)
        print(json.dumps(res), flush=True)
        for mode in ("dictionary", "cross_check"):
            for k, v in res[mode].items():
                lines.append("    %-20s %-12s %-9s median %8.4f ms per pair   p10 %8.4f   p90 %8.4f" % (name, mode, k, v["median"], v["p10"], v["p90"]))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
