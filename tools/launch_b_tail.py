#!/usr/bin/env python
"""Timing experiment: what the workgroups of launch B do behind the re-rank's barrier, per workgroup.  Build a variant with the stamps,
    python tools/build_variant.py btail -DLCD_B_TIMING                        (when a phase's stores were ISSUED)
    python tools/build_variant.py btailack -DLCD_B_TIMING -DLCD_RR_ACKSTAMP   (every stamp behind stores first waits for their acknowledgement)
and run with LCD_LIB_PATH=rtabmap_amd/liblcd_hip_btail.so.  The headline configuration in its growth phase (49 000 words, 10^5 signatures, frames of
500 descriptors that each create ~150 words, appended on the device); the stamps of CAPTURES launches B are read (a launch overwrites the one
before it: frames are submitted, the stream -- not the handle -- is synchronised, the newest launch B is a full one) and pooled."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtabmap_amd  # noqa: E402
from rtabmap_amd import capi, synth  # noqa: E402

ROLES = ["re-rank", "row writer", "sealed bucket", "open bucket"]


def dist(v):
    return "median %5.2f  p90 %5.2f  max %5.2f  (n=%d)" % (np.median(v), np.percentile(v, 90), v.max(), len(v)) if len(v) else "-"


def main():
    n_words, q, n_sig = 49000, 500, int(os.environ.get("N_SIG", "100000"))
    captures = int(os.environ.get("CAPTURES", "6"))
    vocab = synth.vocab_surf(n_words)
    words = synth.zipf_words(n_sig, q, n_words, seed=100000)
    eng = rtabmap_amd.Engine("f32", 64, vocab_capacity=n_words + 65536, sig_capacity=n_sig + 4096, pipeline=True, knn_mode=os.environ.get("KNN_MODE") or None)
    eng.vocab_append(vocab, np.arange(1, n_words + 1, dtype=np.int32))
    eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * q, q, dtype=np.int64), words.reshape(-1))
    d_words = torch.zeros(q, dtype=torch.int32, device="cuda")
    cap = n_sig + 4096
    d_like = torch.zeros(cap, dtype=torch.float32, device="cuda")
    lib = capi.load()
    for f in ("lcd_debug_b_timing", "lcd_debug_rr_timing", "lcd_debug_rr_tail", "lcd_debug_b_role"):
        assert hasattr(lib, f), "the library has no stamps: build a variant with -DLCD_B_TIMING and point LCD_LIB_PATH at it"
    n_frames = 12 * captures + 8
    frames = [torch.from_numpy(synth.frame_from_signature(vocab, words[i * 11], seed=i)).cuda() for i in range(n_frames)]
    recs, gi = [], 0
    for rep in range(captures):
        for i in range(12):
            eng.frame_dev(frames[gi].data_ptr(), q, n_sig + 1 + gi, float(n_sig + 1), d_words.data_ptr(), d_like.data_ptr(), cap, incremental=True,
                          new_words_compared=True, nndr=0.8, first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO if hasattr(capi, "LCD_NEW_WORD_IDS_AUTO") else -1,
                          append_new_words=True)
            gi += 1
        torch.cuda.synchronize()                       # NOT eng.synchronize(): the newest launch B must be a full one
        bb = (ctypes.c_ulonglong * (2 * 4096))(); rr = (ctypes.c_ulonglong * (8 * 512))(); rt = (ctypes.c_ulonglong * (4 * 512))(); ro = (ctypes.c_uint * 4096)()
        assert lib.lcd_debug_b_timing(bb, 2 * 4096) == 0 and lib.lcd_debug_rr_timing(rr, 8 * 512) == 0
        assert lib.lcd_debug_rr_tail(rt, 4 * 512) == 0 and lib.lcd_debug_b_role(ro, 4096) == 0
        b = np.frombuffer(bb, dtype=np.uint64).reshape(-1, 2).astype(np.float64)
        r8 = np.frombuffer(rr, dtype=np.uint64).reshape(-1, 8).astype(np.float64)
        t4 = np.frombuffer(rt, dtype=np.uint64).reshape(-1, 4).astype(np.float64)
        role = np.frombuffer(ro, dtype=np.uint32)
        idx = np.nonzero((b[:, 1] > b[:, 1].max() - 20000) & (b[:, 1] >= b[:, 0]))[0]       # the newest launch: ends within 200 us of the last one
        t0 = b[idx, 0].min()
        for w in idx:
            rec = {"rep": rep, "wg": int(w), "role": int(role[w]), "start": (b[w, 0] - t0) / 100.0, "end": (b[w, 1] - t0) / 100.0}
            if w < 512 and role[w] <= 1:
                rec.update(barrier=(r8[w, 6] - t0) / 100.0, results=(r8[w, 7] - t0) / 100.0, xcd=int(t4[w, 3]))
                if role[w] == 0:
                    rec.update(first=(r8[w, 0] - t0) / 100.0, bits=(t4[w, 0] - t0) / 100.0, n_cand=int(t4[w, 1]), n_list=int(t4[w, 2]))
            recs.append(rec)
    eng.synchronize()
    eng.close()
    print("# %d launches B pooled; us; a workgroup's times count from its launch's first workgroup start" % captures)
    for ri, nme in enumerate(ROLES):
        sel = [r for r in recs if r["role"] == ri]
        if not sel:
            continue
        print("%-13s start %s" % (nme, dist(np.array([r["start"] for r in sel]))))
        print("%-13s end   %s" % ("", dist(np.array([r["end"] for r in sel]))))
        print("%-13s end - start %s" % ("", dist(np.array([r["end"] - r["start"] for r in sel]))))
    rk = [r for r in recs if r["role"] == 0 and "bits" in r and r["barrier"] > 0]
    if rk:
        a = lambda k: np.array([r[k] for r in rk])
        print("re-rank workgroups behind their barrier (thread 0's half):")
        print("  barrier - start               %s" % dist(a("barrier") - a("start")))
        print("  results stored - barrier      %s" % dist(a("results") - a("barrier")))
        print("  bit row + list - results      %s" % dist(a("bits") - a("results")))
        print("  end - bit row + list          %s" % dist(a("end") - a("bits")))
        print("  end - barrier                 %s" % dist(a("end") - a("barrier")))
        print("  candidate rows                %s" % dist(a("n_cand")))
        print("  list entries                  %s" % dist(a("n_list")))
        tail = a("end") - a("barrier")
        for x in range(8):
            m = a("xcd") == x
            if m.any():
                print("  XCD %d: end - barrier %s" % (x, dist(tail[m])))
        c = np.corrcoef(np.vstack([tail, a("n_cand"), a("n_list"), a("start")]))[0]
        print("  correlation of end - barrier with: candidate rows %.2f, list entries %.2f, workgroup start %.2f" % (c[1], c[2], c[3]))
    wk = [r for r in recs if r["role"] == 1 and "barrier" in r and r["barrier"] > 0]
    if wk:
        a = lambda k: np.array([r[k] for r in wk])
        print("row writers: rows staged - start %s" % dist(a("barrier") - a("start")))
        print("             stores issued - rows staged %s" % dist(a("results") - a("barrier")))
        print("             end - stores issued %s" % dist(a("end") - a("results")))
    print("the ten workgroups that ended last (any launch): launch, index, role, XCD, start, barrier, results, bit row + list, end, candidate rows, list entries")
    for r in sorted(recs, key=lambda r: -r["end"])[:10]:
        print("  %d %4d %-13s xcd %s  start %5.2f  barrier %s  results %s  bits %s  end %5.2f  n_cand %s  n_list %s" % (
            r["rep"], r["wg"], ROLES[r["role"]], r.get("xcd", "-"), r["start"], "%5.2f" % r["barrier"] if "barrier" in r else "    -",
            "%5.2f" % r["results"] if "results" in r else "    -", "%5.2f" % r["bits"] if "bits" in r else "    -", r["end"], r.get("n_cand", "-"), r.get("n_list", "-")))
    ends = {}
    for r in recs:
        ends.setdefault(r["rep"], []).append((r["end"], r["role"]))
    print("who ends each launch: " + "  ".join("%d: %s %.2f" % (k, ROLES[max(v)[1]], max(v)[0]) for k, v in sorted(ends.items())))
    print("last end per role and launch: " + "  ".join("%d: " % k + "/".join("%.1f" % max([e for e, ro in v if ro == ri] or [0.0]) for ri in range(4)) for k, v in sorted(ends.items())))


if __name__ == "__main__":
    main()
