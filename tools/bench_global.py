"""Times the global-descriptor comparison (lcd_compare_to_dev) against a device-to-device copy of the same bytes (needs an MI355X; there
is no CPU fallback).

    python tools/bench_global.py                           # 100 000 signatures x 4096 floats (NetVLAD): 1.64 GB of rows
    python tools/bench_global.py --out profiles/global_similarity_timing.txt

What is timed, with HIP events on the engine's stream after a warm-up of the same calls:
  compare_ms      one lcd_compare_to_dev (the words branch's two launches with an EMPTY word list + the row pass), mean over `calls`
  row_pass GB/s   the row matrix's bytes (slots x stride x 4) / compare_ms: the row pass streams the matrix once, everything else is small
  copy GB/s       a device-to-device copy of the same number of bytes in the same process (read + write: bytes x 2 / time), the yardstick
                  for what HBM gives a plain streaming kernel here
Prints one JSON line; --out also writes the three figures as text."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--signatures", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=4096, help="signatures per lcd_sig_set_global_bulk call")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.calls < 20:
        sys.exit("bench_global.py: at least 20 timed calls")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_global.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    n, dim = a.signatures, a.dim
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=n + 64)
    ids = np.arange(1, n + 1, dtype=np.int32)
    eng.sig_add_bulk(ids, np.arange(n + 1, dtype=np.int64), (np.arange(n) % 1000 + 1).astype(np.int32))       # one word each
    rng = np.random.default_rng(1)
    for first in range(0, n, a.chunk):
        m = min(a.chunk, n - first)
        rows = rng.standard_normal((m, dim)).astype(np.float32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        eng.sig_set_global_bulk(0, ids[first:first + m], rows)
    q = rng.standard_normal(dim).astype(np.float32)
    q /= np.linalg.norm(q)
    stream = torch.cuda.ExternalStream(eng.L.lcd_stream(eng.h))
    d_q = torch.from_numpy(q).cuda()
    d_w = torch.zeros(0, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(n + 64, dtype=torch.float32, device="cuda")
    stride = (dim + 3) // 4 * 4
    nbytes = n * stride * 4
    src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    torch.cuda.synchronize()

    def timed(fn):
        with torch.cuda.stream(stream):
            for _ in range(a.warmup):
                fn()
            b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            b.record(stream)
            for _ in range(a.calls):
                fn()
            e.record(stream)
        e.synchronize()
        return b.elapsed_time(e) / a.calls

    compare_ms = timed(lambda: eng.compare_to_dev(d_w, [d_q], d_out))
    copy_ms = timed(lambda: dst.copy_(src))
    compare_ms2 = timed(lambda: eng.compare_to_dev(d_w, [d_q], d_out))          # again behind the copy: the spread a difference has to exceed
    eng.synchronize()
    got = d_out[:n].cpu().numpy()
    res = {"signatures": n, "dim": dim, "row_bytes": nbytes, "calls": a.calls,
           "compare_ms": round(compare_ms, 4), "compare_ms_2": round(compare_ms2, 4),
           "row_pass_gbs": round(nbytes / compare_ms / 1e6, 1), "row_pass_gbs_2": round(nbytes / compare_ms2 / 1e6, 1),
           "copy_ms": round(copy_ms, 4), "copy_gbs_read_plus_write": round(2 * nbytes / copy_ms / 1e6, 1),
           "min_value": float(got.min()), "max_value": float(got.max())}
    eng.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write("lcd_compare_to_dev, %d signatures x %d floats (%.2f GB of rows), %d calls after %d\n" % (n, dim, nbytes / 1e9, a.calls, a.warmup))
            f.write("compare: %.4f ms (again behind the copy: %.4f ms) = %.1f GB/s of rows (%.1f)\n" % (compare_ms, compare_ms2, res["row_pass_gbs"], res["row_pass_gbs_2"]))
            f.write("device-to-device copy of the same bytes: %.4f ms = %.1f GB/s read + write\n" % (copy_ms, res["copy_gbs_read_plus_write"]))


if __name__ == "__main__":
    main()
