#!/usr/bin/env python
"""Config 3 of BASELINE.json (ORB 256-bit Hamming 2-NN, 200k-word vocabulary, 500 descriptors/frame, 1 GPU): kernel time of
the Hamming 2-NN scan (events around it, lcd_profile_*) + the device frame path.  Prints one JSON line per --knn-mode.

  --knn-mode valu,hamming_mfma    two engines in one process, their launches alternated (same clocks, same neighbours on the chip):
                                  the exact vector-ALU scan (knn2_hamming_kernel) against the matrix-core scan (knn2_hamming_mfma_kernel);
                                  the results of the two are compared before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

I8_PEAK_OPS = 256 * 4 * 2 * 32 * 32 * 32 / 32 * 2.4e9     # v_mfma_i32_32x32x32_i8: 2 * 32^3 operations in 32 cycles per SIMD, 1024 SIMDs, 2.4 GHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--knn-mode", default="default", help="comma-separated lcd_knn_mode names of rtabmap_amd.capi.KNN_MODES; several: alternated arms")
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--queries", type=int, default=500)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    import torch
    import rtabmap_amd
    from rtabmap_amd import synth
    modes = a.knn_mode.split(",")
    n_words, q, n_sig = a.rows, a.queries, int(os.environ.get("ORB_SIGS", "20000"))
    vocab = synth.vocab_orb(n_words)
    words = synth.zipf_words(n_sig, q, n_words, seed=5)
    frames = [torch.from_numpy(synth.frame_from_signature(vocab, words[i * 7], seed=i, sigma=0.05)).cuda() for i in range(16)]
    cap = n_sig + 4096
    arms = []
    for mode in modes:
        stream = torch.cuda.Stream()
        eng = rtabmap_amd.Engine("u8", 32, vocab_capacity=n_words + 1024, sig_capacity=n_sig + 4096, stream=stream.cuda_stream, knn_mode=mode)
        eng.vocab_append(vocab, np.arange(1, n_words + 1, dtype=np.int32))
        eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
        arms.append({"mode": mode, "eng": eng, "keep": stream, "d_w": torch.zeros(q * 2, dtype=torch.int32, device="cuda"),
                     "d_d": torch.zeros(q * 2, dtype=torch.float32, device="cuda"), "d_words": torch.zeros(q, dtype=torch.int32, device="cuda"),
                     "d_like": torch.zeros(cap, dtype=torch.float32, device="cuda"), "wall": 0.0})
    for i in range(5):
        for arm in arms:
            arm["eng"].knn2_dev(frames[i].data_ptr(), q, arm["d_w"].data_ptr(), arm["d_d"].data_ptr())
    torch.cuda.synchronize()
    for arm in arms[1:]:                    # faster and different is not faster
        assert torch.equal(arm["d_w"], arms[0]["d_w"]) and torch.equal(arm["d_d"], arms[0]["d_d"]), "the arms' results differ"
    for arm in arms:
        arm["eng"].profile_begin(a.reps)
    for i in range(a.reps):
        for arm in arms:
            arm["eng"].knn2_dev(frames[i % 16].data_ptr(), q, arm["d_w"].data_ptr(), arm["d_d"].data_ptr())
            arm["eng"].synchronize()        # (the arms never share the chip)
    # whole frames, in alternated blocks
    for i in range(10):
        for arm in arms:
            arm["eng"].frame_dev(frames[i % 16].data_ptr(), q, n_sig + 1 + i, float(n_sig + 1), arm["d_words"].data_ptr(), arm["d_like"].data_ptr(), cap)
            arm["eng"].sig_remove(1 + i)
    torch.cuda.synchronize()
    block = 50
    for first in range(0, a.steps, block):
        for arm in arms:
            t0 = time.perf_counter()
            for i in range(first, min(first + block, a.steps)):
                arm["eng"].frame_dev(frames[i % 16].data_ptr(), q, n_sig + 11 + i, float(n_sig + 1), arm["d_words"].data_ptr(), arm["d_like"].data_ptr(), cap)
                arm["eng"].sig_remove(11 + i)
            torch.cuda.synchronize()
            arm["wall"] += time.perf_counter() - t0
    for arm in arms:
        ms, n, name = arm["eng"].profile_read()
        wall = arm["wall"]
        out = {"config": "ORB 256-bit Hamming 2-NN, %d words, %d desc/frame, %d signatures" % (n_words, q, n_sig), "knn_mode": arm["mode"], "kernel": name,
               "kernel_ms": ms, "samples": n, "bit_compares_per_s": q * n_words * 256 / (ms * 1e-3),
               "algorithmic_gbps": (n_words * 32 + q * 48) / (ms * 1e-3) / 1e9, "frame_ms": 1e3 * wall / a.steps, "frames_per_s": a.steps / wall}
        if "mfma" in name:                  # 2 * q * rows * 256 integer operations on the i8 matrix pipe
            out["i8_ops_per_s"] = 2.0 * q * n_words * 256 / (ms * 1e-3)
            out["i8_peak_ops_per_s"] = I8_PEAK_OPS
        else:                               # 8 xor + 8 bcnt + 3 key/min/max per (query, row) pair
            out["valu_lane_ops_per_s"] = q * n_words * 19.0 / (ms * 1e-3)
            out["valu_peak_lane_ops_per_s"] = 256 * 4 * 32 * 2.4e9
        print(json.dumps(out))
        arm["eng"].close()


if __name__ == "__main__":
    main()
