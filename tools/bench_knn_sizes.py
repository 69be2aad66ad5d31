#!/usr/bin/env python
"""2-NN kernel time by vocabulary size (HIP events around the filter / scan launch, lcd_profile_*), 500 queries.
Default: SURF rows at 49k words (headline), 125k (one GPU's shard of config 4) and 1M (config 4 on one GPU).
  --dtype u8 --dim 32 --rows 20000,200000,1000000 --knn-mode valu,hamming_mfma    binary rows, the modes' launches alternated in one process
  --dtype f32 --dim 128 --knn-mode valu,bf16,f16                                   SIFT-sized rows: the scan against the two matrix-core arms
Every arm's line names the kernel lcd_profile_read reported for it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtabmap_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--knn-mode", default=os.environ.get("KNN_MODE") or "default", help="comma-separated names of rtabmap_amd.capi.KNN_MODES; several: alternated arms")
    ap.add_argument("--dtype", default="f32", choices=["f32", "u8"])
    ap.add_argument("--dim", type=int, default=0, help="floats or bytes per row (default 64 floats / 32 bytes)")
    ap.add_argument("--rows", default="49000,125000,1000000")
    a = ap.parse_args()
    q, reps = 500, 30
    dim = a.dim or (64 if a.dtype == "f32" else 32)
    rng = np.random.default_rng(0)
    out = []
    for n in [int(x) for x in a.rows.split(",")]:
        if a.dtype == "f32":
            v = rng.standard_normal((n, dim)).astype(np.float32)
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            qs = (v[rng.integers(0, n, q)] + rng.standard_normal((q, dim)).astype(np.float32) * np.float32(0.02)).astype(np.float32)
        else:
            v = rng.integers(0, 256, (n, dim), dtype=np.uint8)
            qs = v[rng.integers(0, n, q)] ^ np.packbits(rng.random((q, dim * 8)) < 0.1, axis=1)
        ids = np.arange(1, n + 1, dtype=np.int32)
        d_q = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
        arms = []
        for mode in a.knn_mode.split(","):
            eng = rtabmap_amd.Engine(a.dtype, dim, vocab_capacity=n, knn_mode=mode)
            for first in range(0, n, 250_000):
                eng.vocab_append(v[first:first + 250_000], ids[first:first + 250_000])
            arms.append({"mode": mode, "eng": eng, "d_w": torch.zeros(q * 2, dtype=torch.int32, device="cuda"),
                         "d_d": torch.zeros(q * 2, dtype=torch.float32, device="cuda"), "wall": 0.0})
        for _ in range(5):
            for arm in arms:
                arm["eng"].knn2_dev(d_q.data_ptr(), q, arm["d_w"].data_ptr(), arm["d_d"].data_ptr())
        for arm in arms:
            arm["eng"].synchronize()
        for arm in arms[1:]:
            assert torch.equal(arm["d_w"], arms[0]["d_w"]) and torch.equal(arm["d_d"], arms[0]["d_d"]), "the arms' results differ"
        for arm in arms:
            arm["eng"].profile_begin(reps)
        for _ in range(reps):
            for arm in arms:
                t0 = time.perf_counter()
                arm["eng"].knn2_dev(d_q.data_ptr(), q, arm["d_w"].data_ptr(), arm["d_d"].data_ptr())
                arm["eng"].synchronize()
                arm["wall"] += time.perf_counter() - t0
        for arm in arms:
            ms, ns, name = arm["eng"].profile_read()
            r = {"rows": n, "dtype": a.dtype, "dim": dim, "knn_mode": arm["mode"], "kernel": name, "filter_ms": ms, "knn2_call_ms": arm["wall"] / reps * 1e3,
                 "table_gbps": n * ((256 if dim == 64 else 4 * dim) if a.dtype == "f32" else dim) / (ms * 1e-3) / 1e9,     # (64 floats: the 256-byte operand rows; other float rows are read as they are)
                 "fallback_queries": arm["eng"].stats()["knn_last_fallback_queries"], "max_err_ratio": arm["eng"].stats()["knn_max_err_ratio"]}
            if a.dtype == "f32":
                r["algorithmic_tflops"] = 2.0 * q * n * dim / (ms * 1e-3) / 1e12
            else:
                r["bit_compares_per_s"] = q * n * dim * 8.0 / (ms * 1e-3)
            out.append(r)
            arm["eng"].close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
