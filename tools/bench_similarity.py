"""Times the pair similarity next to the TF-IDF likelihood on the same index (needs an MI355X; there is no CPU fallback).

    python tools/bench_similarity.py                       # 100 000 signatures x 500 words over 49 000 words, a 500-word query
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_similarity.py --calls 50     # kernel times, in a run of its own

What is timed (host clock around work that ends in a synchronise, after a warm-up of the same calls):
  similarity_dev_us     lcd_similarity_dev enqueued `calls` times back to back, one synchronise: query reduction + scoring launch per call
  similarity_host_us    lcd_similarity for ONE signature id: staging, the same two launches, gather, download, synchronise
  likelihood_host_us    lcd_likelihood for the same id: staging, frame_words_kernel + score_kernel, gather, download, synchronise
  first_call_ms         the first similarity call of the handle: it also fills slot_nv for every sealed bucket (once per bucket)
The two host calls differ only in their kernels, so their difference is the difference of the launches; the kernels' own times
(sim_query_kernel, sim_score_kernel against frame_words_kernel, score_kernel) come from the rocprofv3 run.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--signatures", type=int, default=100000)
    ap.add_argument("--words", type=int, default=49000)
    ap.add_argument("--sig-words", type=int, default=500)
    ap.add_argument("--query-words", type=int, default=500)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_similarity.py needs a GPU: nothing is measured without one")
    import rtabmap_amd
    from rtabmap_amd import synth
    words = synth.zipf_words(a.signatures, a.sig_words, a.words, seed=100000)
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=a.signatures + 64)
    eng.sig_add_bulk(np.arange(1, a.signatures + 1, dtype=np.int32), np.arange(0, (a.signatures + 1) * a.sig_words, a.sig_words, dtype=np.int64),
                     words.reshape(-1))
    q = synth.zipf_words(1, a.query_words, a.words, seed=7)[0].astype(np.int32)
    one = np.array([a.signatures // 2], np.int32)
    N = float(a.signatures)
    d_q = torch.from_numpy(q).cuda()
    d_out = torch.zeros(a.signatures + 64, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    eng.similarity(q, one)
    first_ms = (time.perf_counter() - t0) * 1e3

    def timed(fn, sync_each):
        for _ in range(a.warmup):
            fn()
        eng.synchronize()
        t = time.perf_counter()
        for _ in range(a.calls):
            fn()
        if not sync_each:
            eng.synchronize()
        return (time.perf_counter() - t) / a.calls * 1e6

    res = {
        "signatures": a.signatures, "words": a.words, "sig_words": a.sig_words, "query_words": a.query_words, "calls": a.calls,
        "unique_query_words": int(np.unique(q).size),
        "first_call_ms": round(first_ms, 3),
        "similarity_dev_us": round(timed(lambda: eng.similarity_dev(d_q, d_out), False), 2),
        "similarity_host_us": round(timed(lambda: eng.similarity(q, one), True), 2),
        "likelihood_host_us": round(timed(lambda: eng.likelihood(q, one, N), True), 2),
    }
    # the same again, the other way round: the spread between the two passes is what a difference has to exceed
    res["likelihood_host_us_2"] = round(timed(lambda: eng.likelihood(q, one, N), True), 2)
    res["similarity_host_us_2"] = round(timed(lambda: eng.similarity(q, one), True), 2)
    res["similarity_dev_us_2"] = round(timed(lambda: eng.similarity_dev(d_q, d_out), False), 2)
    sim = eng.similarity(q, np.arange(1, a.signatures + 1, dtype=np.int32))
    eng.synchronize()
    np.testing.assert_array_equal(d_out[: a.signatures].cpu().numpy(), sim)          # the two entries agree on what was timed
    res["max_similarity"] = float(sim.max())
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
