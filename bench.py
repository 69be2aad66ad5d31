#!/usr/bin/env python
"""bench.py -- loop-closure candidates/sec of the MI355X engine on BASELINE.json's headline configuration.

One STEP = one query frame through the hot path, inputs already resident in HBM:
    500 SURF-64 descriptors -> exact 2-NN against the 49k-word vocabulary + NNDR + same-frame resolution
    (VWDictionary::addNewWords) -> the frame's references registered in the inverted index (existing and new words) and the
    oldest signature retired (memory stays at 100k signatures, as Rtabmap's WM->LTM transfer keeps it) -> TF-IDF likelihood of
    the frame against every signature (Memory::computeLikelihood).
    candidates/sec = frames/sec x N_signatures.

`python bench.py --gpus N`: N == 1 runs in this process; N > 1 starts N ranks itself (one per GPU) unless a launcher
(torch.distributed.run) already did -- RANK / WORLD_SIZE in the environment.  N > 1 (`--parallelism auto`): from 100 000 words per
GPU up (config 4: 1M words over 8 GPUs) the north-star split -- ONE frame stream, the vocabulary and its postings sharded by
word-id range, an all-gather of the per-rank 2-NN candidates and an int64 all-reduce of the partial likelihood per frame (RCCL),
`"scaling": "strong"`; below that (the 49k-word headline: a 12.5 MB vocabulary, to which two exchanges per frame only add latency)
one independent frame stream per GPU with no data-path collective, `"scaling": "weak"`.  The other split is measured in the same
run and reported next to it (`config.shard_value` / `config.replicas_value`).

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the --steps steps and prints the headline (`metric`, `value`,
`unit`, `higher_is_better`, `dtype`, `ms_per_step`, ...); `--dump-outputs DIR` also writes what the last timed step computed
(DIR/<name>.npy: the frame's word ids and its likelihood vector), the inputs being seeded, so that two builds can be compared.
Everything else takes `--full`: `roofline` is the dominant kernel of the step, `roofline_score` / `roofline_knn` are the two big
kernels under fixed keys (HIP events around each launch inside the timed region, on the stream it is launched on);
`cpu_baseline` times the reference-style CPU path on this box's host cores in the same run (three variants); `parity` re-runs
frames of this configuration through a fresh engine and the oracle side by side; the step distribution, the steady-state and
secondary measurements, the HBM counter passes, the secondary legs and (N > 1) the other parallelism.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

LCD_NEW_WORD_IDS_AUTO = -1          # include/lcd.h: lcd_frame_args.first_new_word_id, the device numbers the frame's new words

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_WORDS, N_SIG, Q, DIM = 49000, 100000, 500, 64
NNDR = 0.8
# MI355X peaks (/opt/skills/guides/MI355X_MICROARCH.md): fp32 matrix/vector 157.3 TFLOP/s, bf16 MFMA 2.5 PFLOP/s dense, HBM3E 8 TB/s
PEAK_F32_TFLOPS = 157.3
PEAK_BF16_TFLOPS = 2500.0
PEAK_HBM_GBPS = 8000.0
PMC_PROFILE = os.path.join(ROOT, "profiles", "r05_pmc.json")


DIAG = set()
# the matrix-core filter of every SURF engine of this run: the one-product fp16 filter (LCD_KNN_F16, what the north star names for the SURF
# L2-distance GEMM) unless --knn-mode says otherwise; every mode returns the same bits (exact re-rank + certificate + exact redo)
KNN_MODE = "f16"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# ----------------------------------------------------------------------------------------------------------------- launch
def spawn_ranks(n, argv):
    """N > 1 without a launcher: start N copies of this script, one rank per GPU (ranks share GPUs round-robin when the box has
    fewer -- then the collectives go over gloo, a functional check only)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    for p in procs:
        rc = max(rc, p.wait())
    sys.exit(rc)


# ----------------------------------------------------------------------------------------------------------------- pieces
def make_state(n_sig):
    from rtabmap_amd import synth
    vocab = synth.vocab_surf(N_WORDS)
    words = synth.zipf_words(n_sig, Q, N_WORDS, seed=100000)
    return vocab, words


def load_engine(eng, vocab, words, owned=None):
    """Bulk-load the vocabulary and the signature memory (Memory::loadDataFromDb).  Returns the load time of the signatures."""
    n_sig = words.shape[0]
    eng.vocab_append(vocab, np.arange(1, N_WORDS + 1, dtype=np.int32))
    offsets = np.arange(0, (n_sig + 1) * Q, Q, dtype=np.int64)
    t0 = time.perf_counter()
    eng.sig_add_bulk(np.arange(1, n_sig + 1, dtype=np.int32), offsets, words.reshape(-1))
    return time.perf_counter() - t0


class Stepper:
    """The bench step on one engine: frame t registered as signature n_sig + 1 + t, the oldest signature retired."""

    def __init__(self, eng, torch, d_frames, n_sig, cap, want_like=True, log_frames=0, append=True):
        self.eng, self.d_frames, self.n_sig, self.cap = eng, d_frames, n_sig, cap
        self.d_words = torch.zeros(Q, dtype=torch.int32, device="cuda")
        # log_frames > 0: every frame's word ids are kept (one row each) so that the oracle can replay what THIS engine registered
        self.d_words_log = torch.zeros((log_frames, Q), dtype=torch.int32, device="cuda") if log_frames else None
        self.log_base = self.d_words_log.data_ptr() if log_frames else 0
        self.n_calls = 0
        self.d_like = torch.zeros(cap, dtype=torch.float32, device="cuda") if want_like else None
        self.next_sig, self.oldest, self.first_new = n_sig + 1, 1, N_WORDS + 1
        self.ptrs = [f.data_ptr() for f in d_frames]
        # append: VWDictionary::update()'s append branch inside the step (the words a frame creates are vocabulary rows before the next
        # frame is searched, as Memory::preUpdate has it, Memory.cpp:1004-1016)
        self.args = eng.frame_args(q=Q, flags=3, nndr_ratio=NNDR, N=float(n_sig + 1), d_word_ids=self.d_words.data_ptr(),
                                   d_likelihood=self.d_like.data_ptr(), likelihood_capacity=cap,
                                   append_new_words=1 if (append and "no-new" not in DIAG) else 0)
        # the words a frame creates are numbered ON THE DEVICE, as ++_lastWordId numbers them (VWDictionary.cpp:1188): nothing is read back between
        # frames, and the ids are the reference's integers (LCD_NEW_WORD_IDS_AUTO, include/lcd.h); the id of every logged frame's first new word
        # is kept beside its word ids (the -(k+1) codes of d_word_ids are that id + k)
        self.auto_ids = bool(self.args.append_new_words) and "bound-ids" not in DIAG
        self.d_first_log = torch.zeros(max(log_frames, 0) + 1, dtype=torch.int32, device="cuda")
        if self.auto_ids:
            eng.set_option("next_word_id", N_WORDS + 1)

    def __call__(self, i):
        a = self.args
        a.d_descriptors = self.ptrs[i % len(self.ptrs)]
        a.sig_id = self.next_sig
        a.first_new_word_id = 0 if "no-new" in DIAG else (LCD_NEW_WORD_IDS_AUTO if self.auto_ids else self.first_new)
        if self.log_base and self.n_calls < self.d_words_log.shape[0]:
            a.d_word_ids = self.log_base + self.n_calls * Q * 4
            a.d_first_new_word_id = self.d_first_log.data_ptr() + self.n_calls * 4
        elif self.log_base:
            a.d_word_ids = self.d_words.data_ptr()
            a.d_first_new_word_id = self.d_first_log.data_ptr() + (self.d_first_log.shape[0] - 1) * 4
        self.n_calls += 1
        self.eng.frame_dev_args(a)
        if "no-retire" not in DIAG:
            self.eng.sig_remove(self.oldest)
        self.next_sig += 1
        self.oldest += 1
        self.first_new += Q          # (only without the device's numbering: an upper bound per frame, ids only have to ascend)

    def last_word_ids(self):
        """The device buffer the last call wrote its word ids to (a row of the log while the log has room)."""
        if self.log_base and 0 < self.n_calls <= self.d_words_log.shape[0]:
            return self.d_words_log[self.n_calls - 1]
        return self.d_words


# Bayes/PredictionLC as BayesFilter::setPredictionLC parses the default string (reference Parameters.h:363; uStr2Float -> double)
PREDICTION_LC = np.asarray([0.1, 0.36, 0.30, 0.16, 0.062, 0.0151, 0.00255, 0.000324, 2.5e-05, 1.3e-06, 4.8e-08, 1.2e-09, 1.9e-11, 2.2e-13,
                            1.7e-15, 8.5e-18, 2.9e-20, 6.9e-23], dtype=np.float32).astype(np.float64)
STM = 30          # Mem/STMSize default: the newest signatures are not loop-closure candidates


def chain_neighbors(first, last, lo):
    """Neighbour lists (Memory::getNeighborsId on an odometry chain) of the signatures first..last, naming ids >= lo and <= the signature
    itself (a list is handed over when its signature appears; the engine completes the older signatures' lists)."""
    depth = PREDICTION_LC.shape[0] - 1
    ids = np.arange(first, last + 1, dtype=np.int64)
    d = np.arange(depth - 1, -1, -1, dtype=np.int64)                       # margins depth-1 .. 0  <->  neighbours id-(depth-1) .. id
    nbr = ids[:, None] - d[None, :]
    keep = nbr >= lo
    counts = keep.sum(axis=1)
    off = np.zeros(ids.shape[0] + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return ids.astype(np.int32), off, nbr[keep].astype(np.int32), np.broadcast_to(d[None, :], nbr.shape)[keep].astype(np.int32)


class BayesStepper(Stepper):
    """The step followed by the rest of Rtabmap::process' loop-closure decision on the device: adjustLikelihood, the Bayes filter's
    update over the working memory and the highest hypothesis (32 bytes out); the new signature's neighbour list goes in behind it."""

    def __init__(self, eng, torch, d_frames, n_sig, cap):
        super().__init__(eng, torch, d_frames, n_sig, cap)
        eng.bayes_configure(PREDICTION_LC, 0.9)
        t0 = time.perf_counter()
        eng.bayes_set_neighbors(*chain_neighbors(1, n_sig, 1))
        eng.synchronize()
        self.lists_load_s = time.perf_counter() - t0
        self.d_res = torch.zeros(8, dtype=torch.int32, device="cuda")
        self.args.exclude_recent = STM
        depth = PREDICTION_LC.shape[0] - 1
        self.one_id = np.array([self.next_sig], np.int32)
        self.one_off = np.array([0, depth], np.int64)
        self.one_base = -np.arange(depth - 1, -1, -1, dtype=np.int32)
        self.one_nbr = np.zeros(depth, np.int32)
        self.one_mg = np.arange(depth - 1, -1, -1, dtype=np.int32)
        self.one_prep = eng.bayes_neighbors_prepared(self.one_id, self.one_off, self.one_nbr, self.one_mg)
        self.args.d_bayes = self.d_res.data_ptr()

    def __call__(self, i):
        sid = self.next_sig
        super().__call__(i)
        # the new signature's list: itself and the depth - 1 signatures before it (chain_neighbors(sid, sid, oldest), without the numpy work)
        self.one_nbr[:] = self.one_base + sid
        self.eng.bayes_set_neighbors_prepared(self.one_prep)
        self.one_id[0] = sid + 1


def timed_loop(torch, dist, world, stream, step, steps, warmup, profile_eng=None, eng=None, per_step_events=True, prof_n=0):
    """warmup untimed steps, then exactly `steps` steps bracketed by barrier + synchronize; an event per step for the distribution.
    eng: the engine the steps run on -- its events are recorded in call order (lcd_record_event: a threaded handle enqueues the index
    stage of a frame after lcd_frame_dev returned) and it is drained (lcd_synchronize) before the clock stops."""
    for i in range(warmup):
        step(i)
    if eng is not None:
        eng.synchronize()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    for e in evs:
        e.record(stream)                                # creates the underlying hipEvent_t
    torch.cuda.synchronize()
    rec = (lambda e: eng.record_event(e.cuda_event)) if eng is not None else (lambda e: e.record(stream))
    mid = rec if per_step_events else (lambda e: None)          # an event per step costs a few microseconds of stream time each
    if profile_eng is not None:
        # HIP events around the dominant launch of some timed steps (prof_n of them; default a tenth, at least 3): a bracketed launch costs the
        # stream ~12 us of gaps (6-7 in front of it, 5-6 behind it: profiles/r06_dispatch_timeline.txt), so the timed region brackets ONE launch per
        # sampled frame -- the headline one in twenty frames -- and the other samples / the other big kernel are taken in the steps right behind it
        profile_eng.profile_begin(int(os.environ.get("LCD_BENCH_PROF_N", prof_n if prof_n else max(3, steps // 10))))
    t0 = time.perf_counter()
    rec(evs[0])
    for i in range(steps):
        step(warmup + i)
        (rec if i == steps - 1 else mid)(evs[i + 1])
    host_enqueue = time.perf_counter() - t0
    if eng is not None:
        eng.synchronize()
    t_eng = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_dev1 = time.perf_counter() - t0
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if os.environ.get("LCD_BENCH_SYNC_BREAKDOWN"):
        log("[bench] timed region: enqueue done %.1f us, lcd_synchronize returned %.1f, torch.cuda.synchronize %.1f, second %.1f; device span (events) %.1f"
            % (1e6 * host_enqueue, 1e6 * t_eng, 1e6 * t_dev1, 1e6 * wall, 1e3 * evs[0].elapsed_time(evs[steps])))
    per_step = np.array([evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]) if per_step_events else np.zeros(0)
    if world > 1:
        t = torch.tensor([wall], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())
    return {"wall": wall, "dev_ms": evs[0].elapsed_time(evs[steps]), "host_enqueue": host_enqueue, "per_step_ms": per_step}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy, float32 kept, anything else as float64 (integer ids are exact).  An array over its
    share of the 64 MB is replaced by a fixed, seeded sample of its elements, written beside it with their flat indices (<name>_index.npy)."""
    os.makedirs(out_dir, exist_ok=True)
    share = (DUMP_MAX_BYTES - 4096 * len(arrays)) // max(len(arrays), 1)
    for name, a in arrays.items():
        a = np.asarray(a)
        a = a.astype(np.float32 if a.dtype == np.float32 else np.float64)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // (a.itemsize + 8), replace=False))
            np.save(os.path.join(out_dir, name + "_index.npy"), idx.astype(np.float64))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)


# The pass / fail rule for Rtabmap::adjustLikelihood's value on the replays (the advisor's round-5 finding: the check must gate, not inform).
ADJ_GATE_NOTE = ("adjusted_value_ok = for every sampled frame: |device - formula with exactly rounded (double) statistics| <= 1e-4 relative AND "
                 "|device - reference value with its float statistics| <= 1e-4 + e_ref, where e_ref = |reference float value - double value| measured on "
                 "that very sample.  uMean / uVariance (UMath.h:419-432, 512-526) add ~10^5..10^6 floats sequentially: their own rounding error "
                 "(up to (n - 1) 2^-24 relative, observed 4e-5..2e-4) is not something a device that sums exactly can or should reproduce; "
                 "it is measured per sample and granted, nothing else is.  At <= 10^5 signatures e_ref stays below 1e-5 and the plain 1e-4 bound decides "
                 "(tests/test_gpu_bayes.py, the headline parity block).")
PMC_LIVE = {}          # kernel -> {"fetch_kb", "write_kb", "hbm_bytes_per_launch"}: measured by THIS run (measure_pmc), else the committed profile


def measure_pmc(extra_args=()):
    """HBM traffic per launch, measured by this run: two rocprofv3 passes (--pmc FETCH_SIZE, then --pmc WRITE_SIZE; kernel trace
    only, as MI355X_MICROARCH.md prescribes) over a short invocation of this same script, reduced like tools/make_pmc_json.py
    (rocprofv3 reports KB; gfx950 counts 64 B per 128-B read request: reads are doubled).  Fills PMC_LIVE; returns a note."""
    import collections
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return "rocprofv3 not found: traffic from the committed profile"
    base = tempfile.mkdtemp(prefix="lcd_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp", LCD_BENCH_INNER="1")
    inner = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-cpu-baseline", "--no-extras", "--steps", "30", "--warmup", "5"] + list(extra_args)
    sums = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(base, counter)
            r = subprocess.run(["rocprofv3", "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "pmc", "--"] + inner,
                               cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
            files = glob.glob(d + "/**/*counter_collection.csv", recursive=True)
            if r.returncode != 0 or not files:
                return "rocprofv3 --pmc %s failed (%d): traffic from the committed profile" % (counter, r.returncode)
            agg = collections.defaultdict(lambda: [0, 0.0])
            for row in csv.DictReader(open(files[0])):
                if row["Counter_Name"] != counter:
                    continue
                k = row["Kernel_Name"].replace("(anonymous namespace)::", "").replace("lcd::", "").replace("void ", "").split("(")[0].split("<")[0]
                agg[k][0] += 1
                agg[k][1] += float(row["Counter_Value"])
            sums[counter] = {k: v[1] / v[0] for k, v in agg.items()}
        for k, fe in sums["FETCH_SIZE"].items():
            w = sums["WRITE_SIZE"].get(k, 0.0)
            PMC_LIVE[k] = {"fetch_kb": fe, "write_kb": w, "hbm_bytes_per_launch": (2.0 * fe + w) * 1024.0}
        return "measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE passes over `bench.py --full --no-cpu-baseline --no-extras --steps 30 --warmup 5%s`" % \
               ("".join(" " + x for x in extra_args))
    except Exception as e:  # noqa: BLE001
        return "PMC measurement failed (%s): traffic from the committed profile" % type(e).__name__
    finally:
        shutil.rmtree(base, ignore_errors=True)


N_SIG_RUN = N_SIG       # --signatures of this run (the committed PMC summary is only valid for the headline's 49 000 words x 100 000 signatures)


def pmc_source(name, note=""):
    """Where pmc_traffic(name) comes from: "live" (this run's passes), "committed" (the headline configuration's summary), or None."""
    key = name.split(" ")[0].split("<")[0]
    if key in PMC_LIVE:
        return "live: " + note if note else "live"
    if N_WORDS != 49000 or N_SIG_RUN != N_SIG:
        return None
    return "committed summary of the headline command (%s)%s" % (os.path.relpath(PMC_PROFILE, ROOT), "; " + note if note else "")


def pmc_traffic(name):
    """HBM traffic per launch of a kernel in GB: from this run's own rocprofv3 --pmc passes (measure_pmc) when they ran, else from the
    committed summary of the SAME configuration (the headline's words AND signatures: PMC_PROFILE); null otherwise -- a figure measured
    on another memory size is not this run's traffic."""
    key = name.split(" ")[0].split("<")[0]
    if key in PMC_LIVE:
        return PMC_LIVE[key]["hbm_bytes_per_launch"] / 1e9
    if N_WORDS != 49000 or N_SIG_RUN != N_SIG:
        return None                                      # the committed summary is the headline configuration's
    try:
        pmc = json.load(open(PMC_PROFILE))
        return pmc[key]["hbm_bytes_per_launch"] / 1e9 if key in pmc else None
    except Exception:
        return None


def rooflines(eng, n_rows_rank, n_sig, shard, knn=None, knn_timed=None):
    """Both big kernels, from the HIP events the engine recorded around their launches (knn: the 2-NN series read earlier; knn_timed: the
    samples taken INSIDE the timed region, averaged with the series the engine holds now -- every bracketed launch costs the stream ~12 us
    of gaps (profiles/r06_dispatch_timeline.txt), so the timed region carries few of them and the steps right behind it the rest)."""
    sc_ms, sc_n, sc_name = eng.profile_read_likelihood()
    kern_ms, kern_n, kern_name = eng.profile_read() if knn is None else knn
    if knn_timed is not None and knn_timed[1] > 0:
        t_ms, t_n, t_name = knn_timed
        kern_ms = (kern_ms * kern_n + t_ms * t_n) / (kern_n + t_n)
        kern_n += t_n
        kern_name = kern_name or t_name
    flops = 2.0 * Q * n_rows_rank * DIM           # ALGORITHMIC work per launch: GEMM-equivalent 2*Q*N*D
    achieved = flops / (kern_ms * 1e-3) / 1e12 if kern_ms > 0 else 0.0
    f16 = "fp16" in kern_name
    bf16 = "bf16" in kern_name or f16              # (the dense fp16 and bf16 matrix peaks are the same figure)
    peak = PEAK_BF16_TFLOPS if bf16 else PEAK_F32_TFLOPS
    roof_knn = {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                "traffic": pmc_traffic(kern_name), "traffic_source": pmc_source(kern_name), "traffic_unit": "GB per launch (PMC: 2 x FETCH_SIZE + WRITE_SIZE)", "kernel": kern_name,
                "ms": kern_ms, "samples": kern_n, "mfma_dtype": ("fp16 (1 product per fp32 product, fp32 accumulate)" if f16 else "bf16 (3 products per fp32 product, fp32 accumulate)") if bf16 else "f32",
                "executed_tflops": (3.0 if (bf16 and not f16) else 1.0) * achieved, "frac_of_f32_mfma_peak": achieved / PEAK_F32_TFLOPS,
                "algorithmic_gbps": (n_rows_rank * DIM * 4 + Q * DIM * 4 + Q * 16) / (kern_ms * 1e-3) / 1e9 if kern_ms > 0 else 0.0}
    roof_score = None
    if sc_ms > 0:
        # ALGORITHMIC bytes of the scoring launch, counted by the engine for the last frame's words (lcd_profile_score_work):
        # dense count rows read (256 B per dense word and bucket) + 4 B per sparse posting + 8 B per entry of the open bucket's log
        # + ni read and likelihood write (8 B per signature).  `postings` = what SURVEY.md 8d counts (P of the frame's words).
        work = eng.profile_score_work()
        sc_bytes = work["dense_row_bytes"] + 4.0 * work["sparse_postings"] + 8.0 * work["open_log_entries"] + 8.0 * n_sig
        gbps = sc_bytes / (sc_ms * 1e-3) / 1e9
        roof_score = {"bound": "hbm", "achieved": gbps, "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": gbps / PEAK_HBM_GBPS,
                      "traffic": pmc_traffic(sc_name), "traffic_source": pmc_source(sc_name), "traffic_unit": "GB per launch (PMC: 2 x FETCH_SIZE + WRITE_SIZE)", "kernel": sc_name,
                      "ms": sc_ms, "samples": sc_n, "algorithmic_bytes_per_launch": sc_bytes, "work": work,
                      "frac_if_4B_per_posting": (4.0 * work["postings"] + 8.0 * n_sig) / (sc_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS}
    return roof_knn, roof_score


# ----------------------------------------------------------------------------------------------------------------- CPU side
def build_oracle(vocab, words):
    import oracle as O
    t0 = time.time()
    m = O.OracleMemory(strategy=O.kNNBruteForce, nndr=NNDR)
    for w in range(1, N_WORDS + 1):
        m.vwd.add_word(w, vocab[w - 1])
    m.vwd.update()
    m.add_signatures_bulk(words)
    log("[bench] oracle memory (%d signatures) built in %.1fs" % (words.shape[0], time.time() - t0))
    return m


def parity_block(torch, vocab, words, frames_np, m, n_frames=3):
    """SURVEY.md 8d 'parity checks run with every bench': frames of THIS configuration through a fresh engine -- the timed entry
    point: lcd_frame_dev with registration + retirement + update()'s append on the device, on a pipelined handle, the frames enqueued
    back to back exactly as the timed loop does, so the fused launches are what is checked -- and through the oracle's Memory::update
    (preUpdate: cleanUnusedWords + VWDictionary::update(), then addNewWords) -> computeLikelihood."""
    import rtabmap_amd
    n_sig = words.shape[0]
    eng = rtabmap_amd.Engine("f32", DIM, vocab_capacity=N_WORDS + 4096, sig_capacity=n_sig + 64, pipeline=1, knn_mode=KNN_MODE)
    load_engine(eng, vocab, words)
    cap = n_sig + 16
    d_desc = [torch.from_numpy(frames_np[t]).cuda() for t in range(n_frames)]
    d_words = torch.zeros((n_frames, Q), dtype=torch.int32, device="cuda")
    d_like = torch.zeros((n_frames, cap), dtype=torch.float32, device="cuda")
    d_first = torch.zeros(n_frames, dtype=torch.int32, device="cuda")
    eng.set_option("next_word_id", N_WORDS + 1)                    # VWDictionary::_lastWordId + 1
    torch.cuda.synchronize()
    for t in range(n_frames):      # nothing is read back in between: the device numbers the new words as ++_lastWordId does (VWDictionary.cpp:1188)
        eng.frame_dev(d_desc[t].data_ptr(), Q, n_sig + 1 + t, float(n_sig + 1), d_words[t].data_ptr(), d_like[t].data_ptr(), cap,
                      first_new_word_id=LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
        eng.sig_remove(t + 1)
    eng.synchronize()
    got_all, like_all, first_all = d_words.cpu().numpy(), d_like.cpu().numpy(), d_first.cpu().numpy()
    ids_equal, argmax_equal, max_rel, n_cmp = True, True, 0.0, 0
    t_knn = t_lik = 0.0
    for t in range(n_frames):
        t1 = time.perf_counter()
        sid, exp = m.update(frames_np[t])                      # exact linear 2-NN + addNewWords, 1 thread
        t2 = time.perf_counter()
        got = got_all[t]
        ids_h = np.where(got < 0, int(first_all[t]) - got - 1, got).tolist()
        ids_equal &= bool(ids_h == list(exp))                  # the reference's integers: no renumbering in between
        live = np.array(m.signature_ids(), np.int32)
        t3 = time.perf_counter()
        oi, Lo = m.compute_likelihood(np.array(exp, np.int32), live)
        t4 = time.perf_counter()
        t_knn += t2 - t1
        t_lik += t4 - t3
        Lh = like_all[t][: n_sig + t + 1][oi - 1]             # signature id s sits in slot s - 1
        err = np.abs(Lh - Lo) / np.maximum(np.abs(Lo), 1e-7 / 1e-4)      # relative, with the 1e-7 absolute floor of the 1e-4 bound
        max_rel = max(max_rel, float(err.max()))
        n_cmp += int(Lo.size)
        argmax_equal &= bool(int(np.argmax(Lh[:-1])) == int(np.argmax(Lo[:-1])))
        m.forget(t + 1)
    rows, live_rows = eng.vocab_count()
    eng.close()
    return ({"frames": n_frames, "word_ids_equal": ids_equal, "new_word_ids": "numbered on the device as ++_lastWordId does (LCD_NEW_WORD_IDS_AUTO); compared as they are",
             "likelihood_max_rel": max_rel, "likelihood_values_compared": n_cmp,
             "argmax_equal": argmax_equal, "bound": "1e-4 relative (abs floor 1e-7)", "signatures": n_sig,
             "vocabulary_rows_after": int(rows), "oracle_words_after": len(m.vwd.word_ids()),
             "path": "lcd_frame_dev (registration + retirement + update()'s append on the device + TF-IDF, pipelined handle, frames enqueued "
                     "back to back) vs oracle Memory::update (cleanUnusedWords + update() + addNewWords) + computeLikelihood"},
            t_knn / n_frames, t_lik / n_frames)


def timed_engine_parity(m, step, frames_np, like_last, n_sig):
    """Parity ON THE ENGINE THAT WAS TIMED: the oracle replays what that engine registered -- every frame's word ids as the device
    decided them (the words a frame created get their descriptor; none is ever indexed, as in the timed loop), the retirement of the
    oldest signature after every frame -- and its restated Memory::computeLikelihood of the LAST frame is compared with the likelihood
    the timed engine left for that frame: the inverted index after hundreds of registrations, retirements, reserved and recycled
    postings keys, pipelined launches.  (Word assignment itself is checked by parity_block on a fresh engine: the oracle's exact
    2-NN of hundreds of frames would take minutes.)"""
    T = min(step.n_calls, step.d_words_log.shape[0])
    got = step.d_words_log[:T].cpu().numpy()
    first_new_log = step.d_first_log[:T].cpu().numpy().tolist() if step.auto_ids else [N_WORDS + 1 + i * Q for i in range(T)]
    nf = len(frames_np)
    t0 = time.perf_counter()
    for i in range(T):
        codes = got[i]
        ids = np.where(codes < 0, first_new_log[i] - codes - 1, codes).astype(np.int32)
        seen = set()
        for j in np.flatnonzero(codes < 0).tolist():
            if codes[j] not in seen:                                   # the first descriptor with the code created the word
                seen.add(int(codes[j]))
                m.vwd.add_word(int(ids[j]), frames_np[i % nf][j])
        sid = m.add_signature_with_id(n_sig + 1 + i, ids)
        assert sid == n_sig + 1 + i
        if i < T - 1:
            m.forget(1 + i)
    live = np.array(m.signature_ids(), np.int32)
    oi, Lo = m.compute_likelihood(ids, live)
    slots = np.where(oi <= n_sig, oi - 1, oi - 1)                      # signature id s sits in slot s - 1 (bulk ids 1..n_sig, then the frames)
    Lh = like_last[slots]
    err = np.abs(Lh - Lo) / np.maximum(np.abs(Lo), 1e-7 / 1e-4)
    dead = np.ones(n_sig + T, bool)
    dead[slots] = False
    return {"frames_replayed": T, "likelihood_max_rel": float(err.max()), "likelihood_values_compared": int(Lo.size),
            "argmax_equal": bool(int(np.argmax(Lh[:-1])) == int(np.argmax(Lo[:-1]))), "retired_slots_all_zero": bool(not like_last[: n_sig + T][dead].any()),
            "replay_s": time.perf_counter() - t0,
            "path": "the timed engine's own last frame (after %d pipelined frames with registration + retirement) vs the oracle's "
                    "Memory::computeLikelihood on the replayed memory" % T}


def flat_tfidf_ms(words, frame_words, n_sig, thread_counts):
    """The TF-IDF leg a CPU implementation could reach if it gave up the reference's std::map containers: flat word-major postings of the
    frame's words (built outside the timed region, as an index would hold them) scored with OpenMP over the words (oracle.flat_tfidf --
    a baseline, never a parity reference).  Returns {threads: ms}."""
    import oracle as O
    flat = words.reshape(-1)
    qw = np.unique(frame_words[frame_words > 0])
    sel = np.nonzero(np.isin(flat, qw))[0]
    key = flat[sel].astype(np.int64) * n_sig + (sel // words.shape[1])
    uk, cnt = np.unique(key, return_counts=True)
    pw, ps = uk // n_sig, (uk % n_sig).astype(np.int32)
    off = np.append(np.searchsorted(pw, qw, side="left"), len(pw)).astype(np.int64)
    ni = np.full(n_sig, words.shape[1], np.int32)
    out = {}
    for th in thread_counts:
        O.flat_tfidf(off, ps, cnt.astype(np.int32), ni, float(n_sig), th)                # warm (thread pool start-up)
        t0 = time.perf_counter()
        for _ in range(3):
            O.flat_tfidf(off, ps, cnt.astype(np.int32), ni, float(n_sig), th)
        out[th] = 1e3 * (time.perf_counter() - t0) / 3
    return out


def cpu_baselines(vocab, frames_np, t_linear_port, t_lik_full, n_sig, words=None, frame_words=None):
    """(i) the reference default -- rtflann kd-tree (4 trees, 32 checks), 1 thread; (ii) the exact configuration --
    rtflann LINEAR, 1 thread; (iii) generous -- the same rtflann code with OpenMP over the queries, at the thread count that is
    FASTEST on this box (500 queries do not feed every core: all cores is slower than one).  The TF-IDF leg of (i)-(iii) is the
    restated std::map Memory::computeLikelihood over the FULL signature memory (single-threaded in the reference); (iv) replaces it
    with flat postings + OpenMP (flat_tfidf_ms) next to the best 2-NN time: what `best_cpu_value` means."""
    import oracle as O
    cores = os.cpu_count() or 1
    counts = sorted(set(c for c in (1, 2, 4, 8, 16, 32, 64, cores) if c <= cores))
    out = {}

    def rate(t_knn, t_lik=t_lik_full):
        return n_sig / (t_knn + t_lik)
    t_kd = {}
    t_lin = {}
    if O.have_ref():
        kd = O.RefIndex(vocab, algo=O.ALGO_KDTREE, trees=4)
        lin = O.RefIndex(vocab, algo=O.ALGO_LINEAR)
        def timeit(f, n):
            f(frames_np[0])
            t0 = time.perf_counter()
            for i in range(n):
                f(frames_np[i % len(frames_np)])
            return (time.perf_counter() - t0) / n
        for c in counts:
            t_kd[c] = timeit(lambda d: kd.knn(d, k=2, checks=32, cores=c), 10 if c == 1 else 5)
        for c in (1, 8, 32, cores):
            if c <= cores:
                t_lin[c] = timeit(lambda d: lin.knn(d, k=2, checks=32, cores=c), 1 if c == 1 else 3)
        kind = "reference"
    else:
        t_lin[1] = t_linear_port
        t0 = time.perf_counter()
        O.knn2_linear(vocab, frames_np[0], threads=cores)
        t_lin[cores] = time.perf_counter() - t0
        kind = "port"
    variants = {}
    if t_kd:
        cb = min(t_kd, key=t_kd.get)
        variants["i_kdtree_1core"] = {"value": rate(t_kd[1]), "knn_ms": 1e3 * t_kd[1], "cores": 1}
        variants["iii_kdtree_best_threads"] = {"value": rate(t_kd[cb]), "knn_ms": 1e3 * t_kd[cb], "cores": cb,
                                               "knn_ms_by_threads": {str(c): 1e3 * t for c, t in t_kd.items()}}
    lb = min(t_lin, key=t_lin.get)
    variants["ii_linear_1core"] = {"value": rate(t_lin[1]), "knn_ms": 1e3 * t_lin[1], "cores": 1}
    variants["iii_linear_best_threads"] = {"value": rate(t_lin[lb]), "knn_ms": 1e3 * t_lin[lb], "cores": lb,
                                           "knn_ms_by_threads": {str(c): 1e3 * t for c, t in t_lin.items()}}
    if words is not None and frame_words is not None:
        ft = flat_tfidf_ms(words, frame_words, n_sig, [c for c in (1, 8, 32, cores) if c <= cores])
        fb = min(ft, key=ft.get)
        t_knn_best = min(list(t_kd.values()) + list(t_lin.values()))
        variants["iv_best_knn_flat_tfidf"] = {"value": rate(t_knn_best, 1e-3 * ft[fb]), "knn_ms": 1e3 * t_knn_best, "tfidf_ms": ft[fb], "tfidf_threads": fb,
                                              "tfidf_ms_by_threads": {str(c): t for c, t in ft.items()},
                                              "note": "not the reference's algorithm: flat word-major postings + OpenMP instead of std::map per word"}
    head = variants.get("i_kdtree_1core", variants["ii_linear_1core"])
    out = {"value": head["value"], "unit": "candidates/s", "cores": 1, "kind": kind,
           "sample": "2-NN of %d-descriptor frames over the full vocabulary with the reference's own rtflann (%s) + restated std::map "
                     "Memory::computeLikelihood over the full %d-signature memory (%.0f ms/frame, 3 frames); variants i-iii use the "
                     "same TF-IDF time, iv a flat threaded one" % (Q, "kd-tree 4 trees / 32 checks" if t_kd else "exact linear port", n_sig, 1e3 * t_lik_full),
           "tfidf_ms": 1e3 * t_lik_full, "variants": variants,
           "best_cpu_value": max(v["value"] for v in variants.values())}
    return out


# ----------------------------------------------------------------------------------------------------------------- extras (N = 1)
def host_path_ms(torch, eng, frames_np, n_sig, steps=20):
    """What a cv::Mat caller of VWDictionary::addNewWords / Memory::computeLikelihood gets: host pointers in, host pointers out
    (lcd_quantize + lcd_sig_add + lcd_likelihood + lcd_sig_remove), PCIe and synchronisation included."""
    sig_ids = np.arange(2000, 2000 + n_sig, dtype=np.int32)         # live ids do not matter for the cost: score whatever is live
    next_sig, oldest = 5_000_000, 4000
    t0 = None
    for i in range(steps + 3):
        if i == 3:
            t0 = time.perf_counter()
        w, _ = eng.quantize(frames_np[i % len(frames_np)], incremental=True, new_words_compared=True, nndr=NNDR)
        eng.sig_add(next_sig, np.where(w > 0, w, 0).astype(np.int32))
        eng.likelihood(w, sig_ids, float(n_sig + 1))
        eng.sig_remove(oldest)
        next_sig += 1
        oldest += 1
    return 1e3 * (time.perf_counter() - t0) / steps


def with_update_ms(torch, eng, stepper, steps=256, lag=8, rebuild_every=128):
    """The step with the WHOLE of Memory::preUpdate in it, every frame, nothing completed in between (Memory.cpp:1004-1016 runs
    cleanUnusedWords + VWDictionary::update() before every addNewWords of an incremental dictionary): the frame's new words become
    vocabulary rows behind its decision loop (append_new_words, as in the headline step); the signature registered `lag` frames earlier is
    retired as well (a short-lived node, like a WM -> LTM transfer: the words only it referenced become unused); cleanUnusedWords is ONE
    kernel enqueued behind the frames in flight (lcd_vocab_remove_unused_async: tombstones, logged for the host); every
    `rebuild_every`-th frame the vocabulary is compacted (lcd_vocab_rebuild, the full-rebuild branch VWDictionary.cpp:610-690 -- the only
    call of the loop that completes the pipeline).  Returns (ms per step, rows, live rows at the end)."""
    t0 = None
    for i in range(steps + 16):
        if i == 12:
            eng.vocab_rebuild()                          # (the first compaction allocates its second set of vocabulary buffers: not timed)
        if i == 16:
            eng.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        sid = stepper.next_sig
        stepper(i)
        if i >= lag:
            eng.sig_remove(sid - lag)
        eng.vocab_remove_unused_async()
        if i % rebuild_every == rebuild_every - 1:
            eng.vocab_rebuild()
    eng.synchronize()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    rows, live = eng.vocab_count()
    with_update_ms.divergent_refs = int(eng.stats().get("clean_divergent_refs", 0))   # (see run_replay_growing: async_clean_divergence)
    return ms, rows, live


def frame_latency_ms(torch, eng, stepper, stream, base_i, n=48):
    """What a caller waits for: lcd_frame_dev(t) called -> the event recorded behind frame t (lcd_record_event: behind every stage the
    frame still owes, i.e. its likelihood is readable) has fired.
      (a) paced: the caller keeps lcd_pipeline_depth() + 1 frames in flight (it waits for frame t - 3 before it submits frame t + 1): the
          latency of the pipeline itself, four frame periods;
      (b) saturated: frames submitted as fast as the call returns -- the queue in front of the device adds to it (the call itself holds the
          caller when the device is more than 8 frames behind);
      (c) a single frame followed by lcd_synchronize (the owed stages run as three stand-alone launch pairs).
    Host and device clocks are aligned once per series (an event + a synchronisation: a few microseconds of error)."""
    def series(paced):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        for e in evs:
            e.record(stream)
        eng.synchronize()
        torch.cuda.synchronize()
        eng.record_event(evs[0].cuda_event)
        torch.cuda.synchronize()
        t_base = time.perf_counter()                     # ~ the moment evs[0] fired (the stream was idle behind it)
        sub = []
        for i in range(n):
            if paced and i >= 4:
                evs[i - 3].synchronize()                  # frame i - 4 is complete: four in flight with this one
            sub.append(time.perf_counter() - t_base)
            stepper(base_i + i)
            eng.record_event(evs[i + 1].cuda_event)
        eng.synchronize()
        torch.cuda.synchronize()
        lat = np.array([evs[0].elapsed_time(evs[i + 1]) - 1e3 * sub[i] for i in range(n)])
        return lat[8:]                                    # the first frames meet an empty pipeline
    paced = series(True)
    sat = series(False)
    single = []
    for i in range(12):
        t0 = time.perf_counter()
        stepper(base_i + i)
        eng.synchronize()
        single.append(1e3 * (time.perf_counter() - t0))
    return {"paced_median": float(np.median(paced)), "paced_p95": float(np.percentile(paced, 95)),
            "saturated_median": float(np.median(sat)), "saturated_p95": float(np.percentile(sat, 95)),
            "single_frame_then_synchronize_median": float(np.median(single[2:]))}


def cpp_interface_ms(vocab, words, frames_np, n_sig, steps=12):
    """What a caller of the reference's own interface gets, at the headline's memory size: C++ MemoryHip::update (-> VWDictionaryHip::
    addNewWordsAndScore -> ONE lcd_frame_host call: quantisation, references, update()'s append, likelihood) + Memory::computeLikelihood of
    the new signature against every signature + forget of the oldest, in a C++ loop inside liblcd_host.so (cv::Mat-like host matrices in,
    the host mirror's std::map bookkeeping included).  Three ways to take the likelihood: the reference's std::map by value, a
    caller-owned std::map updated in place, flat vectors; and the call-by-call path of rounds 1-4 on the same memory.
    (The mirror's containers are filled by Memory::addSignature in C++ -- 50 M std::map insertions at 100 000 signatures -- and the
    device by one bulk registration.)"""
    from rtabmap_amd import vwdictionary as V
    mem = V.MemoryHip(strategy=V.kNNBruteForceHIP, incremental=True, nndr=NNDR, new_words_compared_together=True)
    vw = mem.vwd
    for w in range(1, vocab.shape[0] + 1):
        vw.add_word(w, vocab[w - 1])
    vw.update()
    t0 = time.perf_counter()
    mem.add_signatures_bulk(words[:n_sig])
    load_s = time.perf_counter() - t0
    fr = np.stack(frames_np[: min(len(frames_np), 16)])
    out = {"signatures": n_sig, "load_s": load_s}
    out["map_by_value"] = mem.time_loop_modes(fr, steps, 0)
    out["map_in_place"] = mem.time_loop_modes(fr, steps, 1)
    out["flat"] = mem.time_loop_modes(fr, steps, 2)
    out["update_ms_inside_lcd_frame_host"] = mem.fast_frame_device_ms()      # copies + launches + the one synchronisation; the rest of `update` is std::map bookkeeping
    mem.set_device_frames(False)
    out["call_by_call_map_by_value"] = mem.time_loop_modes(fr, max(3, steps // 3), 0)
    mem.close()
    return out


# ----------------------------------------------------------------------------------------------------------------- ORB stream
def leg_parity(torch, vocab, words, frame):
    """ONE frame of parity for a secondary leg: lcd_frame_dev (registration + update()'s append + TF-IDF, pipelined handle) against the oracle's
    addNewWords over the same dictionary (exact linear 2-NN, C++) and Memory::computeLikelihood -- the C++ std::map oracle up to 200 000
    signatures, its numpy restatement (oracle/tfidf_np.py, pinned to the C++ oracle by tests/test_oracle_golden.py) beyond."""
    import oracle as O
    import rtabmap_amd
    n_sig = words.shape[0]
    eng = rtabmap_amd.Engine("f32", DIM, vocab_capacity=N_WORDS + 4096, sig_capacity=n_sig + 64, pipeline=1, knn_mode=KNN_MODE)
    load_engine(eng, vocab, words)
    cap = n_sig + 16
    d_desc = torch.from_numpy(frame).cuda()
    d_words = torch.zeros(Q, dtype=torch.int32, device="cuda")
    d_like = torch.zeros(cap, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.frame_dev(d_desc.data_ptr(), Q, n_sig + 1, float(n_sig + 1), d_words.data_ptr(), d_like.data_ptr(), cap, first_new_word_id=N_WORDS + 1, append_new_words=True)
    eng.synchronize()
    got, Lh = d_words.cpu().numpy(), d_like.cpu().numpy()[: n_sig + 1]
    eng.close()
    t0 = time.perf_counter()
    o = O.OracleVWDictionary(strategy=O.kNNBruteForce, incremental=True, nndr=NNDR, new_words_compared_together=True)
    for w in range(1, N_WORDS + 1):
        o.add_word(w, vocab[w - 1])
    o.update()
    exp = o.add_new_words(frame, n_sig + 1)
    t_knn = time.perf_counter() - t0
    ids_h = np.where(got < 0, N_WORDS - got, got)                   # the frame's k-th new word: code -(k + 1) -> id N_WORDS + 1 + k (the oracle's ++_lastWordId)
    ids_equal = bool(ids_h.tolist() == list(exp))
    o.close()
    t1 = time.perf_counter()
    if n_sig < 200_000:
        m = build_oracle(vocab, words)
        sid, exp2 = m.update(frame)
        oi, Lo = m.compute_likelihood(np.array(exp2, np.int32), np.array(m.signature_ids(), np.int32))
        how = "C++ std::map oracle"
        m.close()
    else:
        from oracle import tfidf_np
        allw = np.concatenate([words, np.asarray(exp, np.int32)[None, :]], axis=0)
        Lo = tfidf_np.compute_likelihood_dense(allw, np.asarray(exp, np.int32))
        how = "numpy restatement (oracle/tfidf_np.py)"
    t_lik = time.perf_counter() - t1
    err = np.abs(Lh - Lo) / np.maximum(np.abs(Lo), 1e-7 / 1e-4)
    return {"frames": 1, "word_ids_equal": ids_equal, "likelihood_max_rel": float(err.max()), "likelihood_values_compared": int(Lo.size),
            "argmax_equal": bool(int(np.argmax(Lh[:-1])) == int(np.argmax(Lo[:-1]))), "bound": "1e-4 relative (abs floor 1e-7)", "signatures": int(n_sig),
            "likelihood_by": how, "oracle_seconds": {"addNewWords": t_knn, "computeLikelihood": t_lik}}


def p2p_exchange_leg():
    """The sharded frame's two exchanges through liblcd_p2p.so (include/lcd_p2p.h) between TWO processes sharing this GPU -- the only
    multi-rank configuration a one-GPU box has: the arenas are mapped through hipIpc exactly as between two GPUs, the wire is local HBM
    instead of xGMI.  Microseconds per exchange, enqueued back to back (tools/p2p_bench.py); ~10 s."""
    import subprocess
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "p2p_bench.py"), "--iters", "200"], cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL, timeout=90.0, text=True)
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": "exit code %d" % r.returncode}
        d = json.loads(lines[-1])
        d["command"] = "python tools/p2p_bench.py --iters 200"
        d["wall_s"] = time.perf_counter() - t0
        return d
    except Exception as e:                                        # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, e)}


def secondary_legs(budget_s=165.0):
    """The other configurations as short runs of this same script, so that what profiles/ claims for them is observed by whoever runs the
    command with --full (the previous review's item 8): config 3 on 300 ORB frames, 125 000 words (one GPU's share of config 4) for 50 steps,
    10^6 signatures for 30 steps -- each with its own roofline and one frame of parity.  A leg that would not fit the time budget is skipped
    and says so; a leg that fails reports its error instead of costing the line."""
    import subprocess
    # (expected seconds on the MI355X box of round 6: 8 / 27 / 52 -- drawing 5 x 10^8 Zipf words and the numpy restatement of ONE likelihood over them
    # take most of the last one; a slower host skips it and says so; LCD_BENCH_LEGS=all lifts the budget)
    legs = [("orb_stream_300_frames", ["--full", "--config", "orb_stream", "--steps", "300"], 15.0),
            ("words_125k", ["--full", "--words", "125000", "--steps", "50", "--warmup", "5", "--leg"], 35.0),
            ("signatures_1m", ["--full", "--signatures", "1000000", "--steps", "30", "--warmup", "5", "--leg"], 70.0),
            # the config-5 stand-in whose dictionary grows from empty (update -> addNewWords -> computeLikelihood -> adjustLikelihood every frame, a clean every
            # frame, retirements, rebuilds), 50 000 frames of the 10^6 of profiles/r06_bench_replay_growing_1m.json
            ("replay_growing_50k_frames", ["--full", "--config", "replay_growing", "--signatures", "50000"], 30.0)]
    if os.environ.get("LCD_BENCH_LEGS", "") == "all":
        budget_s = 1200.0
    out = {"note": "short runs of `python bench.py <args>` by this run; the full-size lines are profiles/r06_bench_*.json"}
    out["p2p_exchange_two_ranks_one_gpu"] = p2p_exchange_leg()
    t_start = time.perf_counter()
    for name, extra, expect in legs:
        left = budget_s - (time.perf_counter() - t_start)
        if left < 0.6 * expect:
            out[name] = {"skipped": "time budget of the --full command (%.0f s left, the leg needs ~%.0f s)" % (left, expect)}
            continue
        t0 = time.perf_counter()
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, cwd=ROOT, env=dict(os.environ, LCD_BENCH_INNER="1"),
                               stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=max(left, 30.0) + 30.0, text=True)
            lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:
                out[name] = {"error": "exit code %d" % r.returncode}
                continue
            d = json.loads(lines[-1])
            keep = {k: d.get(k) for k in ("metric", "value", "unit", "steps", "ms_per_step", "roofline", "roofline_score", "roofline_knn", "parity")}
            if d.get("recall") is not None:
                keep["recall"] = d.get("recall")
            keep["command"] = "python bench.py " + " ".join(extra)
            keep["workload"] = d.get("config", {}).get("workload")
            keep["wall_s"] = time.perf_counter() - t0
            out[name] = keep
        except Exception as e:                                    # noqa: BLE001
            out[name] = {"error": "%s: %s" % (type(e).__name__, e)}
    return out


def run_orb_stream(args):
    """BASELINE.json config 3 as SURVEY.md 8d specifies it: 2 000 frames of 500 ORB descriptors against an initially EMPTY incremental
    dictionary (NNDR 0.8) grown to ~200k words, every frame also removing the references of frame t - 1000, TF-IDF against the working
    memory, and -- as Memory::preUpdate does -- cleanUnusedWords before EVERY frame (lcd_vocab_remove_unused_async: one enqueued kernel).
    Device-pointer path: lcd_frame_dev on a plain handle (the exact Hamming scan has no matrix-core stage to pipeline behind),
    VWDictionary::update()'s append on the device (append_new_words), descriptors resident in HBM.  Parity at BOTH ends of the stream: the
    first frames against an oracle that starts empty, and the LAST frames -- the dictionary beyond 200k words, after a thousand
    retirements and two thousand device-side cleans -- against an oracle memory rebuilt from the engine's own state (its live rows in row
    order, the working memory's signatures from the device's word log), frame by frame: word ids and likelihood.  The Hamming scan's
    HIP-event time at the final vocabulary gives the roofline (integer VALU: SURVEY.md 8d Q2 counts 8 xor + 8 bit-count-adds per
    descriptor pair); the CPU baseline is the reference's rtflann Hamming scan (exact linear, the strategy the oracle pins) over the
    final vocabulary + the restated TF-IDF, on a bounded sample."""
    import torch
    import rtabmap_amd
    from rtabmap_amd import synth
    import oracle as O
    n_frames, q, W, n_check, n_tail = (args.steps if args.steps is not None else 2000), 500, 1000, 60, 20
    base = synth.vocab_orb(200000)
    # Queries-ORB of SURVEY.md 8d, a fresh draw per frame: 90 % noisy copies (each bit flipped w.p. 0.1) of rows of the hidden 200k-row
    # Vocab-ORB -- they come back in later frames and keep their words alive --, 10 % uniform random descriptors: words that die when their
    # frame leaves the working memory (the churn cleanUnusedWords is there for).  The dictionary settles near 200k words.
    frames = [synth.queries_orb(base, q, seed=501 + t, frac_known=0.9, flip=0.1) for t in range(n_frames)]
    d_frames = torch.from_numpy(np.stack(frames)).cuda()                                        # 2 000 x 16 KB resident in HBM
    stream = torch.cuda.Stream()
    eng = rtabmap_amd.Engine("u8", 32, vocab_capacity=262144, sig_capacity=n_frames + 64, stream=stream.cuda_stream)
    cap = n_frames + 64
    d_words = torch.zeros((n_frames, q), dtype=torch.int32, device="cuda")
    d_like = torch.zeros(cap, dtype=torch.float32, device="cuda")
    d_first = torch.zeros(n_frames, dtype=torch.int32, device="cuda")     # the id of every frame's first new word, as the device numbered it
    torch.cuda.synchronize()
    base_ptr, words_ptr, first_ptr = d_frames.data_ptr(), d_words.data_ptr(), d_first.data_ptr()
    a = eng.frame_args(q=q, flags=3, nndr_ratio=NNDR, d_likelihood=d_like.data_ptr(), likelihood_capacity=cap, append_new_words=1)
    n_prof = 40
    T0 = max(n_frames - n_tail, 0)                                 # the frames from T0 on run one by one next to the oracle

    def one(t):
        a.d_descriptors = base_ptr + t * q * 32
        a.d_word_ids = words_ptr + t * q * 4
        a.sig_id = t + 1
        a.first_new_word_id = LCD_NEW_WORD_IDS_AUTO          # nothing is read back: the device numbers the words as ++_lastWordId does (VWDictionary.cpp:1188)
        a.d_first_new_word_id = first_ptr + t * 4
        a.N = float(min(t + 1, W + 1))                      # Memory::getSignatures().size() with the new signature in it (Memory.cpp:2248)
        eng.frame_dev_args(a)
        if t + 1 > W:
            eng.sig_remove(t + 1 - W)
        eng.vocab_remove_unused_async()                      # Memory::cleanUnusedWords, in front of the next frame's update()

    def run(t0, t1):
        for t in range(t0, t1):
            one(t)
            if t % compact_every == compact_every - 1 and t + 1 > W:
                rows_now, live_now = eng.vocab_count()       # (completes the owed work) compaction when a quarter of the rows is dead
                if rows_now - live_now > rows_now // 4:
                    eng.vocab_rebuild()
    compact_every = 100
    t_start = time.perf_counter()
    run(0, max(T0 - n_prof, 0))
    eng.synchronize()
    eng.profile_begin(n_prof)                                    # HIP events around the scan kernel of the last timed frames (largest vocabulary)
    run(max(T0 - n_prof, 0), T0)
    eng.synchronize()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t_start
    n_timed = max(T0, 1)
    scan_ms, scan_n, scan_name = eng.profile_read()
    rows, live = eng.vocab_count()
    got = d_words.cpu().numpy()
    first = d_first.cpu().numpy()

    def eng_ids(t, codes):
        return np.where(codes < 0, int(first[t]) - codes - 1, codes)
    # ---- parity, head of the stream: the first frames against an oracle that starts empty (it assigns consecutive ids: compare the
    # canonical form -- every word replaced by the position of its first occurrence in the stream)
    o = O.OracleMemory(strategy=O.kNNBruteForce, nndr=NNDR, new_words_compared_together=True)
    canon_o, canon_h, first_o, first_h, exp_lists = [], [], {}, {}, []
    ids_identical = True                                          # ... and, the words being numbered on the device, the very integers
    for t in range(min(n_check, T0)):
        so, ido = o.update(frames[t])
        exp_lists.append(ido)
        ids_h = eng_ids(t, got[t]).tolist()
        ids_identical &= bool(ids_h == list(ido))
        for k, (wo, wh) in enumerate(zip(ido, ids_h)):
            canon_o.append(first_o.setdefault(wo, len(first_o)))
            canon_h.append(first_h.setdefault(wh, len(first_h)))
    ids_equal = canon_o == canon_h
    # ---- parity, tail of the stream: an oracle memory with the engine's own state at frame T0, then frame by frame
    vr, vi = eng.vocab_read(0, rows)
    keep = vi != 0
    o2 = O.OracleMemory(strategy=O.kNNBruteForce, nndr=NNDR, new_words_compared_together=True)
    for wid, r in zip(vi[keep].tolist(), vr[keep]):
        o2.vwd.add_word(int(wid), r)
    o2.vwd.update()
    live_sigs = list(range(max(T0 - W, 0) + 1, T0 + 1))
    known = set(vi[keep].tolist())
    tail_state_ok = True
    for sid in live_sigs:
        w = eng_ids(sid - 1, got[sid - 1]).astype(np.int32)
        tail_state_ok &= bool(set(w.tolist()) <= known)           # a live signature's words are rows of the vocabulary
        assert o2.add_signature_with_id(sid, w) == sid
    tail_state_ok &= not o2.vwd.get_unused_word_ids()            # the device-side cleans left no live row without a reference
    tail_ids_equal, tail_max_rel, tail_n, eng2orc, t_knn_tail, tail_identical = True, 0.0, 0, {}, 0.0, True
    for t in range(T0, n_frames):
        one(t)
        eng.synchronize()
        codes = d_words[t].cpu().numpy()
        first[t] = int(d_first[t].item())
        t1 = time.perf_counter()
        so, ido = o2.update(frames[t])
        t_knn_tail += time.perf_counter() - t1
        ids_h = eng_ids(t, codes).tolist()
        tail_identical &= bool(ids_h == list(ido))
        for j in np.flatnonzero(codes < 0).tolist():
            eng2orc.setdefault(ids_h[j], ido[j])
        tail_ids_equal &= bool(so == t + 1 and [eng2orc.get(w, w) for w in ids_h] == list(ido))
        live_sigs.append(t + 1)
        oi, Lo = o2.compute_likelihood(np.array(ido, np.int32), np.array(live_sigs, np.int32))
        Lh = d_like[: t + 1].cpu().numpy()[oi - 1]
        err = np.abs(Lh - Lo) / np.maximum(np.abs(Lo), 1e-7 / 1e-4)
        tail_max_rel = max(tail_max_rel, float(err.max()))
        tail_n += int(Lo.size)
        if t + 1 > W:
            o2.forget(t + 1 - W)
            live_sigs.remove(t + 1 - W)
    rows_end, live_end = eng.vocab_count()
    div_refs = int(eng.stats().get("clean_divergent_refs", 0))
    # ---- CPU baseline on a bounded sample: the reference's rtflann Hamming scan over the FINAL vocabulary, 1 core, + the restated TF-IDF
    if O.have_ref():
        lin = O.RefIndex(vr, algo=O.ALGO_LINEAR)
        knn = lambda d: lin.knn(d, k=2, checks=32, cores=1)       # noqa: E731
    else:
        knn = lambda d: O.knn2_linear(vr, d)                       # noqa: E731
    t1 = time.perf_counter()
    for t in range(2):
        knn(frames[n_frames - 1 - t])
    t_knn = (time.perf_counter() - t1) / 2
    live_o = np.array(o2.signature_ids(), np.int32)
    t2 = time.perf_counter()
    for t in range(3):
        o2.compute_likelihood(eng_ids(n_frames - 1 - t, got[n_frames - 1 - t] if n_frames - 1 - t < T0 else d_words[n_frames - 1 - t].cpu().numpy()).astype(np.int32), live_o)
    t_lik = (time.perf_counter() - t2) / 3 * (min(W, n_frames) / max(len(live_o), 1))   # scaled to the full working memory
    cand = min(W, n_frames)
    pairs = float(q) * rows
    lane_ops = pairs * 16.0                                       # 8 x (32-bit xor + 32-bit bit-count-add) per pair
    achieved = lane_ops / (scan_ms * 1e-3) / 1e12 if scan_ms > 0 else 0.0
    PEAK_INT = 39.3                                               # T lane-ops/s: 256 CUs x 64 lanes x 2.4 GHz
    out = {"metric": "loop-closure candidates/sec (ORB 256-bit, incremental dictionary from empty, W=1000)", "unit": "candidates/s",
           "value": n_timed * cand / wall, "n_gpus": 1, "steps": n_timed, "warmup": 0, "ms_per_step": 1e3 * wall / n_timed,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
           "config": {"workload": "config 3: %d ORB frames x %d descriptors, incremental dictionary grown from empty to %d words (%d rows), "
                                  "update() appends on the device, cleanUnusedWords enqueued every frame, W=%d retirement, device-pointer path "
                                  "(lcd_frame_dev, plain handle); %d timed frames, then %d frames one by one next to the oracle" % (n_frames, q, live, rows, W, n_timed, n_frames - T0),
                      "dictionary_words": int(live), "dictionary_words_at_the_end": int(live_end), "frames_per_s": n_timed / wall,
                      "async_clean_divergent_refs": {"references": div_refs, "frames": int(n_frames), "per_10000_frames": 1e4 * div_refs / max(int(n_frames), 1),
                                                     "note": "a plain handle completes every frame before the enqueued clean runs: 0 by construction (the counter is lcd_stats.clean_divergent_refs)"}},
           "roofline": {"bound": "valu-int", "achieved": achieved, "peak": PEAK_INT, "unit": "T lane-ops/s", "frac": achieved / PEAK_INT, "traffic": None,
                        "kernel": scan_name, "ms": scan_ms, "samples": scan_n, "rows_scanned": int(rows),
                        "algorithmic": "%d x %d descriptor pairs x 16 lane-ops (8 x (xor + bit-count-add))" % (q, rows),
                        "algorithmic_gbps": (rows * 32.0 + q * 32.0) / (scan_ms * 1e-3) / 1e9 if scan_ms > 0 else 0.0},
           "cpu_baseline": {"value": cand / (t_knn + t_lik), "unit": "candidates/s", "cores": 1, "kind": "reference" if O.have_ref() else "port",
                            "sample": "2 frames x exact Hamming 2-NN over the final %d-row vocabulary (%.0f ms/frame) + restated std::map TF-IDF "
                                      "scaled to %d signatures (%.1f ms/frame)" % (rows, 1e3 * t_knn, cand, 1e3 * t_lik)},
           "parity": {"frames_checked": list(range(min(n_check, T0))) [:3] + ["...", min(n_check, T0) - 1] + list(range(T0, n_frames)),
                      "new_word_ids": "numbered on the device as ++_lastWordId does (LCD_NEW_WORD_IDS_AUTO); word_ids_identical_integers compares them as they are",
                      "head": {"frames": [0, min(n_check, T0) - 1], "word_ids_equal": bool(ids_equal), "word_ids_identical_integers": bool(ids_identical)},
                      "tail": {"frames": [T0, n_frames - 1], "dictionary_words": int(live), "retirements_before": max(T0 - W, 0),
                               "state_consistent": bool(tail_state_ok), "word_ids_equal": bool(tail_ids_equal), "word_ids_identical_integers": bool(tail_identical),
                               "likelihood_max_rel": tail_max_rel, "likelihood_values_compared": tail_n,
                               "oracle_ms_per_frame": 1e3 * t_knn_tail / max(n_frames - T0, 1)},
                      "word_ids_equal": bool(ids_equal and tail_ids_equal and tail_state_ok),
                      "path": "lcd_frame_dev(u8, append_new_words) + lcd_vocab_remove_unused_async vs oracle Memory::update (cleanUnusedWords + "
                              "update() + addNewWords) + computeLikelihood; head: canonical word numbering from an empty dictionary; tail: the "
                              "oracle's memory rebuilt from the engine's rows and word log at frame %d" % T0}}
    print(json.dumps(out), flush=True)
    eng.close()


# ----------------------------------------------------------------------------------------------------------------- replay (config 5 stand-in)
def adjusted_exact(L, value):
    """Rtabmap::adjustLikelihood's value for one entry with the statistics evaluated in double precision (the same formula, Rtabmap.cpp:
    5691-5745): the reference's uMean / uVariance accumulate in FLOAT, in signature order -- over ~10^6 positive likelihoods that sum
    alone is off by up to ~1e-3 relative, which is the reference's rounding, not a property a device sum should reproduce (the device
    sums in double).  Used beside the oracle's float-sequential value, never instead of it."""
    v = np.asarray(L, np.float64)
    v = v[v > 0]
    if v.size == 0:
        return 1.0
    mean = float(np.float32(v.sum() / v.size))
    var = float(((v - mean) ** 2).sum() / (v.size - 1)) if v.size > 1 else 0.0
    std = float(np.float32(np.sqrt(np.float32(max(var, 0.0)))))
    value = float(value)
    if value > mean + std and mean != 0.0:
        return float(np.float32((value - (std - 0.0001)) / mean))
    return 1.0


def run_replay(args):
    """BASELINE.json config 5 cannot run here (KITTI images, OpenCV/PCL: SURVEY.md 8d); its prescribed stand-in does: a descriptor-stream
    replay with revisits through the loop-closure path of Rtabmap::process, EVERY frame: Memory::update (cleanUnusedWords is a no-op here:
    nothing is retired; VWDictionary::update() appends the previous frame's new words; addNewWords against the INCREMENTAL dictionary that
    starts as the 49k-word one, Memory.cpp:5941-6059) -> references -> Memory::computeLikelihood against EVERY signature in memory ->
    Rtabmap::adjustLikelihood + the best candidate (Rtabmap.cpp:2117-2131), with the memory grown through lcd_frame_dev, frame by frame,
    from empty to --signatures (1 000 000 asked for: nothing is retired, as the reference's WM cannot hold that many either, the point is
    the frame path at that size).  Trajectory: 2 048 places visited round robin, two noisy views per place alternating lap by lap: from
    the second lap on every frame revisits a place, and the loop-closure RECALL is counted like the reference's harness does
    (tools/ConsoleApp/main.cpp:383-506 compares the detected id with the ground truth): a frame counts when its best candidate (outside
    the newest 30 signatures) shows the same place.
    Parity on frames SAMPLED ACROSS THE WHOLE RUN (every frame's word ids stay on the device, the sampled frames' likelihood vectors too):
    word ids against the C++ oracle's VWDictionary::addNewWords over the dictionary as the engine had it at that frame (base words + the
    words the device's log says earlier frames created, exact linear 2-NN); likelihood and adjustLikelihood's record against the
    restated Memory::computeLikelihood on the memory replayed from the device's word log -- the C++ std::map oracle while the memory
    fits it (<= 120 000 signatures), its numpy restatement (oracle/tfidf_np.py, pinned to the C++ one) beyond."""
    import torch
    import rtabmap_amd
    from rtabmap_amd import synth
    import oracle as O
    from oracle import tfidf_np
    n_total = args.signatures if args.signatures != N_SIG else 1_000_000
    globals()["N_SIG_RUN"] = n_total
    P, V, q, stm, n_samples = 2048, 2, Q, 30, 14
    vocab = synth.vocab_surf(N_WORDS)
    place_words = synth.zipf_words(P, q, N_WORDS, seed=5)
    pool = np.stack([synth.frame_from_signature(vocab, place_words[p], seed=9000 + v * P + p, resample=0.0, sigma=0.03)
                     for v in range(V) for p in range(P)])                         # [V * P, q, 64]: view v of place p at v * P + p
    d_pool = torch.from_numpy(pool).cuda()
    stream = torch.cuda.Stream()
    eng = rtabmap_amd.Engine("f32", DIM, vocab_capacity=N_WORDS + V * P * q // 2, sig_capacity=n_total + 4096, stream=stream.cuda_stream, pipeline=1, knn_mode=KNN_MODE)
    eng.vocab_append(vocab, np.arange(1, N_WORDS + 1, dtype=np.int32))
    cap = n_total + 64
    depth = eng.pipeline_depth() + 1
    # sampled frames: spread over the run (the first laps -- where the dictionary still grows -- included), the last frame among them
    sample_t = sorted(set([3, P // 2, P + 7, 2 * P + 11, 3 * P + 5] + np.linspace(4 * P, n_total - 1, n_samples - 5).astype(np.int64).tolist()))
    sample_t = [t for t in sample_t if 0 <= t < n_total]
    sample_slot = {t: k for k, t in enumerate(sample_t)}
    d_words = torch.zeros((n_total, q), dtype=torch.int32, device="cuda")           # the word log: 2 KB per frame stays in HBM
    d_like = torch.zeros((depth, cap), dtype=torch.float32, device="cuda")
    d_like_s = [torch.zeros(t + 2, dtype=torch.float32, device="cuda") for t in sample_t]
    d_hyp = torch.zeros((n_total, 8), dtype=torch.int32, device="cuda")             # adjustLikelihood's record of EVERY frame (32 B)
    d_first = torch.zeros(n_total, dtype=torch.int32, device="cuda")                # the id of every frame's first new word, as the device numbered it
    torch.cuda.synchronize()
    a = eng.frame_args(q=q, flags=3, nndr_ratio=NNDR, exclude_recent=stm, append_new_words=1)
    pool_ptr, wp, lp, hp, fp = d_pool.data_ptr(), d_words.data_ptr(), d_like.data_ptr(), d_hyp.data_ptr(), d_first.data_ptr()
    eng.set_option("next_word_id", N_WORDS + 1)                                     # VWDictionary::_lastWordId + 1
    n_prof = 40

    def frame_index(t):
        return ((t // P) % V) * P + (t % P)
    # word ids: numbered on the device as ++_lastWordId numbers them (LCD_NEW_WORD_IDS_AUTO; VWDictionary.cpp:1188) -- nothing is read back between frames
    t_start = time.perf_counter()
    marks = {}
    for t in range(n_total):
        if t == n_total - n_prof:
            eng.synchronize()
            eng.profile_begin(n_prof)
        a.d_descriptors = pool_ptr + frame_index(t) * q * DIM * 4
        a.sig_id = t + 1
        a.N = float(t + 1)
        a.first_new_word_id = LCD_NEW_WORD_IDS_AUTO
        a.d_first_new_word_id = fp + t * 4
        a.d_word_ids = wp + t * q * 4
        k = sample_slot.get(t)
        if k is not None:
            a.d_likelihood = d_like_s[k].data_ptr()
            a.likelihood_capacity = t + 2
        else:
            a.d_likelihood = lp + (t % depth) * cap * 4
            a.likelihood_capacity = cap
        a.d_hypothesis = hp + t * 32
        eng.frame_dev_args(a)
        if t + 1 in (100_000, 500_000):
            eng.synchronize()
            marks[t + 1] = time.perf_counter() - t_start
    eng.synchronize()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t_start
    rows, live = eng.vocab_count()
    roof_knn, roof_score = rooflines(eng, rows, n_total, False)
    for r in (roof_knn, roof_score):
        if r:
            r["traffic"] = None                                    # (the committed PMC summary is the headline configuration's)
            r["traffic_note"] = "not measured for this configuration"
            r["measured_in"] = "HIP events attached to the launches of the last %d frames (memory at its final size)" % n_prof
    # ---- recall, over EVERY frame that revisits a place
    hyp = d_hyp.cpu().numpy()
    ts = np.arange(n_total)
    valid = ts >= P + stm
    best_sig = hyp[:, 0]
    hit = valid & (best_sig > 0) & (((best_sig - 1) % P) == (ts % P))
    recall = float(hit.sum()) / max(int(valid.sum()), 1)
    adjusted = hyp[:, 3].view(np.float32)
    # ---- parity on the sampled frames
    t_par = time.perf_counter()
    log = d_words.cpu().numpy()                                                    # [n_total, q] codes: > 0 word id, < 0 the frame's -(k+1)-th new word
    first_new = d_first.cpu().numpy().astype(np.int64)
    n_new_frame = np.where((log < 0).any(axis=1), -log.min(axis=1), 0)
    ids_consecutive = bool(first_new[0] == N_WORDS + 1 and np.array_equal(first_new[1:], first_new[:-1] + n_new_frame[:-1]))   # ++_lastWordId over the whole replay
    ids_log = np.where(log < 0, first_new[:, None] - log - 1, log).astype(np.int32)
    created_by = np.flatnonzero((log < 0).any(axis=1))                             # frames that created words (the first laps)
    o = O.OracleVWDictionary(strategy=O.kNNBruteForce, incremental=True, nndr=NNDR, new_words_compared_together=True)
    for w in range(1, N_WORDS + 1):
        o.add_word(w, vocab[w - 1])
    added_upto = 0                                                                  # frames whose created words the oracle dictionary holds
    known = set()
    mem = None                                                                      # the C++ oracle memory, while the replay fits it
    mem_upto = 0
    ids_equal, max_rel, n_cmp, hyp_ok, checked = True, 0.0, 0, True, []
    hyp_same = hyp_near = 0
    adj_rel_ref = adj_rel_exact = adj_ref_own = 0.0
    adj_ok = True
    knn_s = lik_s = 0.0
    for t in sample_t:
        # the dictionary as update() leaves it in front of frame t: every word a frame < t created, in id order
        for f in created_by[(created_by >= added_upto) & (created_by < t)].tolist():
            codes = log[f]
            for j in np.flatnonzero(codes < 0).tolist():
                wid = int(ids_log[f, j])
                if wid not in known:                                                # the first descriptor with the code created the word
                    known.add(wid)
                    o.add_word(wid, pool[frame_index(f)][j])
        added_upto = max(added_upto, t)
        o.update()
        last_before = o.last_word_id
        t1 = time.perf_counter()
        exp = o.add_new_words(pool[frame_index(t)], t + 1)
        knn_s += time.perf_counter() - t1
        # the oracle numbers the new words of frame t consecutively from ITS last id (++_lastWordId): compare by rank within the frame,
        # the form the device reports (-(k + 1) for the frame's k-th new word)
        canon_o = [-(w - last_before) if w > last_before else w for w in exp]
        ids_equal &= bool(canon_o == log[t].tolist())
        # the oracle's own new words of this frame were only needed for the comparison: drop them again (the replayed dictionary takes
        # the device's ids for them when a later sample needs them)
        new_o = sorted(set(w for w in exp if w > last_before))
        for w in set(exp):
            o.remove_all_word_ref(int(w), t + 1)
        if new_o:
            o.remove_words(new_o)
        # likelihood: Memory::computeLikelihood of frame t's words against signatures 1 .. t + 1 (frame t itself included)
        t2 = time.perf_counter()
        if t + 1 <= 120_000:
            if mem is None:
                mem = O.OracleMemory(strategy=O.kNNBruteForce, nndr=NNDR)
                for w in range(1, N_WORDS + 1):
                    mem.vwd.add_word(w, vocab[w - 1])
            for f in range(mem_upto, t + 1):
                for wid in set(ids_log[f][log[f] < 0].tolist()):
                    if mem.vwd.word_refs(int(wid)) is None:
                        mem.vwd.add_word(int(wid), vocab[0])                      # (the descriptor plays no part in the likelihood)
                assert mem.add_signature_with_id(f + 1, ids_log[f]) == f + 1
            mem_upto = t + 1
            oi, Lo = mem.compute_likelihood(ids_log[t], np.arange(1, t + 2, dtype=np.int32))
            how = "C++ oracle"
        else:
            Lo = tfidf_np.compute_likelihood_dense(ids_log[: t + 1], ids_log[t])
            how = "numpy restatement"
        lik_s += time.perf_counter() - t2
        Lh = d_like_s[sample_slot[t]][: t + 1].cpu().numpy()
        err = np.abs(Lh - Lo) / np.maximum(np.abs(Lo), 1e-7 / 1e-4)
        max_rel = max(max_rel, float(err.max()))
        n_cmp += int(Lo.size)
        # adjustLikelihood + best candidate over the signatures outside the newest `stm` (Rtabmap.cpp:2046-2131)
        n_cons = t + 1 - stm
        if n_cons > 0:
            adj = O.adjust_likelihood(np.concatenate([[0.0], Lo[:n_cons]]).astype(np.float32), 0.0)
            best = int(np.argmax(Lo[:n_cons]))
            # the best candidate: the same signature, or -- a place seen hundreds of times leaves hundreds of signatures with the same words,
            # whose likelihoods differ by rounding only (the device sums exactly, the reference in float) -- one whose reference
            # likelihood lies within the parity bound of the reference's maximum
            dev = int(hyp[t, 0]) - 1
            same = dev == best
            near = 0 <= dev < n_cons and float(Lo[dev]) >= float(Lo[best]) * (1.0 - 1e-4)
            hyp_same += int(same); hyp_near += int(near and not same)
            hyp_ok &= bool(same or near)
            pick = dev if near else best
            ref_adj = float(adj[1 + pick])
            got_adj = float(hyp[t, 3:4].view(np.float32)[0])
            adj_rel_ref = max(adj_rel_ref, abs(got_adj - ref_adj) / max(abs(ref_adj), 1e-3))
            ex_adj = adjusted_exact(Lo[:n_cons], Lo[pick])
            adj_rel_exact = max(adj_rel_exact, abs(got_adj - ex_adj) / max(abs(ex_adj), 1e-3))
            # the gate (ADJ_GATE_NOTE): within 1e-4 of the reference's formula, and of the reference's float-accumulated value up to what
            # that accumulation itself lost on THIS sample (|float statistics - double statistics|, measured here, not a constant)
            ref_own = abs(ref_adj - ex_adj) / max(abs(ex_adj), 1e-3)
            adj_ref_own = max(adj_ref_own, ref_own)
            adj_ok &= bool(abs(got_adj - ex_adj) / max(abs(ex_adj), 1e-3) <= 1e-4 and
                           abs(got_adj - ref_adj) / max(abs(ref_adj), 1e-3) <= 1e-4 + ref_own)
        checked.append({"frame": int(t), "signatures": int(t + 1), "likelihood_by": how})
    par_s = time.perf_counter() - t_par
    # ---- CPU baseline on a bounded sample: the reference's kd-tree / exact scan over the FINAL dictionary + the restated std::map TF-IDF
    # on the largest memory the C++ oracle held, scaled linearly to n_total signatures (the reference's loop is linear in the postings)
    vr, _ = eng.vocab_read(0, rows)
    if O.have_ref():
        kd = O.RefIndex(vr, algo=O.ALGO_KDTREE, trees=4)
        t1 = time.perf_counter()
        for i in range(5):
            kd.knn(pool[i], k=2, checks=32, cores=1)
        t_knn_cpu = (time.perf_counter() - t1) / 5
        knn_what = "rtflann kd-tree (4 trees, 32 checks), 1 core, %d rows" % rows
        kind = "reference"
    else:
        t1 = time.perf_counter()
        O.knn2_linear(vr, pool[0])
        t_knn_cpu = time.perf_counter() - t1
        knn_what = "exact linear port, 1 core, %d rows" % rows
        kind = "port"
    t_lik_cpu, lik_what = None, "not measured"
    if mem is not None and mem_upto >= 1000:
        t1 = time.perf_counter()
        for i in range(3):
            mem.compute_likelihood(ids_log[mem_upto - 1 - i], np.arange(1, mem_upto + 1, dtype=np.int32))
        t_lik_cpu = (time.perf_counter() - t1) / 3 * (n_total / float(mem_upto))
        lik_what = "restated std::map Memory::computeLikelihood on %d signatures, scaled x%.1f to %d" % (mem_upto, n_total / float(mem_upto), n_total)
    eng.close()
    cand_total = n_total * (n_total + 1) / 2.0
    out = {"metric": "loop-closure candidates/sec (descriptor-stream replay with revisits, memory grown to %d signatures)" % n_total,
           "unit": "candidates/s", "value": cand_total / wall, "n_gpus": 1, "steps": n_total, "warmup": 0, "ms_per_step": 1e3 * wall / n_total,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "config 5 stand-in (SURVEY.md 8d): %d frames x %d SURF descriptors through Memory::update -> addNewWords (incremental "
                                  "dictionary from %d words, update()'s append on the device) -> references -> computeLikelihood against every signature "
                                  "-> adjustLikelihood + best candidate, EVERY frame; %d places x %d views round robin, memory 0 -> %d signatures; "
                                  "pipelined lcd_frame_dev" % (n_total, q, N_WORDS, P, V, n_total),
                      "dictionary_rows_at_the_end": int(rows), "frames_that_created_words": int(created_by.size),
                      "frames_per_s": n_total / wall, "wall_s": wall, "wall_s_at_signatures": {str(k): v for k, v in marks.items()},
                      "ms_per_frame_last_half": 1e3 * (wall - marks.get(500_000, 0.0)) / (n_total - 500_000) if 500_000 in marks and n_total > 500_000 else None,
                      "parity_host_seconds": par_s},
           "roofline": roof_score if roof_score is not None else roof_knn, "roofline_score": roof_score, "roofline_knn": roof_knn,
           "recall": {"frames_counted": int(valid.sum()), "loop_closures_found": int(hit.sum()), "recall": recall,
                      "mean_adjusted_likelihood_of_hits": float(adjusted[hit].mean()) if hit.any() else None,
                      "rule": "every frame from the second lap on: the best raw-likelihood candidate outside the newest %d signatures shows the frame's place" % stm},
           "parity": {"frames_checked": checked, "word_ids_equal": bool(ids_equal),
                      "new_word_ids_consecutive_over_the_whole_replay": ids_consecutive,     # numbered on the device (LCD_NEW_WORD_IDS_AUTO) exactly as ++_lastWordId would: every frame's first id = the one before + the words that frame created
                      "likelihood_max_rel": max_rel, "likelihood_values_compared": n_cmp,
                      "adjust_likelihood_and_best_candidate_ok": bool(hyp_ok and adj_ok), "best_candidate_equal_or_a_rounding_tie": bool(hyp_ok), "adjusted_value_ok": bool(adj_ok), "best_candidate_identical": hyp_same,
                      "best_candidate_a_rounding_tie": hyp_near, "bound": "1e-4 relative (abs floor 1e-7)",
                      "adjusted_value_max_rel_vs_reference_float_statistics": adj_rel_ref,
                      "adjusted_value_max_rel_vs_the_same_formula_with_double_statistics": adj_rel_exact,
                      "adjusted_value_within_1e-4_of_the_reference": bool(adj_rel_ref <= 1e-4), "reference_float_statistics_own_error_max_rel": adj_ref_own, "adjusted_value_gate": ADJ_GATE_NOTE,
                      "adjusted_value_note": "Rtabmap::adjustLikelihood divides by uMean and subtracts sqrt(uVariance), which the reference accumulates in FLOAT over "
                                             "every positive likelihood in signature order (UMath.h:419-432, 512-526; restated that way by the oracle); the device sums "
                                             "in double.  Over ~10^6 values the float sum itself deviates from the exact one by more than the parity bound, so the first "
                                             "figure measures the reference's accumulation error, the second the device against the same formula without it",
                      "oracle_seconds": {"addNewWords": knn_s, "computeLikelihood": lik_s},
                      "path": "sampled frames of the replay: word ids vs the C++ oracle's addNewWords over the dictionary replayed from the device's word "
                              "log; likelihood + adjustLikelihood vs Memory::computeLikelihood on the memory replayed from that log (C++ std::map oracle up "
                              "to 120 000 signatures, its numpy restatement oracle/tfidf_np.py beyond)"}}
    if t_lik_cpu is not None:
        out["cpu_baseline"] = {"value": n_total / (t_knn_cpu + t_lik_cpu), "unit": "candidates/s (at the final memory size)", "cores": 1, "kind": kind,
                               "sample": "5 frames x %s (%.1f ms/frame) + 3 frames x %s (%.0f ms/frame)" % (knn_what, 1e3 * t_knn_cpu, lik_what, 1e3 * t_lik_cpu),
                               "gpu_at_the_final_size": n_total / (1e-3 * (out["config"]["ms_per_frame_last_half"] or out["ms_per_step"]))}
    print(json.dumps(out), flush=True)


def run_replay_growing(args):
    """Config 5's stand-in with what config 5 is about (Memory.cpp:5941-6059, Rtabmap.cpp:2117): a replay whose INCREMENTAL dictionary starts
    EMPTY and keeps growing, with the whole of Memory::preUpdate live.  Trajectory: every other frame is the first visit of a NEW place
    (n/2 places over n frames), the frames in between revisit a place seen before (uniform over the places so far).  A place = q - 1
    descriptors near words (N(0, 0.015^2) noise) of a 49 000-word Zipf world (the robot's environment: these become dictionary words as they are first seen) +
    one descriptor of its own (a word only this place has); a revisit = the place's descriptors + N(0, 0.015^2) noise, renormalised
    (two sightings of a world word are 2 sigma^2 D apart: at sigma = 0.03 the ratio test starts rejecting them against the world's closest
    pairs, and a word with two entries is rejected at every later sighting -- the dictionary then doubles every few thousand frames).  So
    the dictionary covers the world's used words within the first thousands of frames and then grows by about one word per new place
    (> 500 000 words at 10^6 frames), > 50 % of the frames create words.  Every frame: cleanUnusedWords (lcd_vocab_remove_unused_async)
    -> update() (the previous frame's words became rows on the device) -> addNewWords -> references -> computeLikelihood against every
    live signature -> adjustLikelihood + best candidate; every 8th frame the oldest signature is retired (its words lose a reference;
    a word without references is removed by the next clean); lcd_vocab_rebuild every 8192 frames (the only draining call) compacts the
    tombstones.  Descriptors are generated ON the device (torch, seeded) in batches; nothing but the per-frame arguments crosses PCIe.
    Recall: a revisit counts when the best candidate outside the newest 30 signatures shows its place (over the revisits whose place
    still has its first signature in memory).  Parity on frames sampled across the run: the pipeline is completed in front of a sampled
    frame and the device's vocabulary read back -- the frame's word ids must be VWDictionary::addNewWords' (C++ oracle) over exactly
    that dictionary in row order; likelihood and adjustLikelihood's record against the numpy restatement of Memory::computeLikelihood
    (pinned to the C++ oracle) on the live signatures replayed from the device's word log."""
    import torch
    import rtabmap_amd
    from rtabmap_amd import synth
    import oracle as O
    from oracle import tfidf_np
    n = args.signatures if args.signatures != N_SIG else 1_000_000
    globals()["N_SIG_RUN"] = n
    q, stm, retire_every, rebuild_every, B, sigma = Q, 30, 8, 8192, 512, 0.015
    n_places = n // 2 + 1
    stream = torch.cuda.Stream()
    vocab = synth.vocab_surf(N_WORDS)
    t_gen = time.perf_counter()
    with torch.cuda.stream(stream):
        g = torch.Generator(device="cuda")
        g.manual_seed(20260922)
        d_world = torch.from_numpy(vocab).cuda()
        ranks = torch.arange(1, N_WORDS + 1, dtype=torch.float64, device="cuda")
        probs = (1.0 / ranks)
        probs = (probs / probs.sum()).float()
        perm = torch.randperm(N_WORDS, generator=g, device="cuda")
        pool = torch.empty((n_places, q, DIM), dtype=torch.float32, device="cuda")     # view 0 of every place: 128 KB each, resident in HBM
        CH = 2048
        for c0 in range(0, n_places, CH):
            ch = min(CH, n_places - c0)
            idx = perm[torch.multinomial(probs.expand(ch, -1), q - 1, True, generator=g)]
            known = d_world[idx] + sigma * torch.randn((ch, q - 1, DIM), generator=g, device="cuda")
            own = torch.randn((ch, 1, DIM), generator=g, device="cuda")
            blk = torch.cat([known, own], dim=1)
            pool[c0:c0 + ch] = blk / blk.norm(dim=2, keepdim=True)
        del idx, known, own, blk
    stream.synchronize()
    gen_s = time.perf_counter() - t_gen
    # trajectory (host): even frames first visits, odd frames revisits
    ts = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(77)
    place = np.where(ts % 2 == 0, ts // 2, (rng.random(n) * (ts // 2 + 1)).astype(np.int64))
    place = np.minimum(place, ts // 2)
    d_place = torch.from_numpy(place).cuda()
    revisit = torch.from_numpy((ts % 2 == 1)).cuda()
    # word ids: numbered on the device as ++_lastWordId numbers them (LCD_NEW_WORD_IDS_AUTO; VWDictionary.cpp:1188) -- nothing is read back between frames
    eng = rtabmap_amd.Engine("f32", DIM, vocab_capacity=max(1 << 16, min(2 * n, 1_400_000)), sig_capacity=n + 4096, stream=stream.cuda_stream, pipeline=1, knn_mode=KNN_MODE)
    cap = n + 64
    depth = eng.pipeline_depth() + 1
    want = [1001, 5000, 20001, n // 8 + 1, n // 4, n // 2 + 1, (3 * n) // 4, n - 2]
    sample_t = sorted(set(t for t in want if 64 <= t < n))
    if n > 300_000:
        sample_t = sample_t[:3] + sample_t[-3:]                                         # the C++ oracle scans the whole dictionary per sample
    sample_slot = {t: k for k, t in enumerate(sample_t)}
    d_words = torch.zeros((n, q), dtype=torch.int32, device="cuda")
    d_like = torch.zeros((depth, cap), dtype=torch.float32, device="cuda")
    d_like_s = [torch.zeros(t + 2, dtype=torch.float32, device="cuda") for t in sample_t]
    d_hyp = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    d_first = torch.zeros(n, dtype=torch.int32, device="cuda")                      # the id of every frame's first new word, as the device numbered it
    bufs = [torch.empty((B, q, DIM), dtype=torch.float32, device="cuda") for _ in range(2)]
    snap = {}
    torch.cuda.synchronize()
    a = eng.frame_args(q=q, flags=3, nndr_ratio=NNDR, exclude_recent=stm, append_new_words=1)
    wp, lp, hp, fp = d_words.data_ptr(), d_like.data_ptr(), d_hyp.data_ptr(), d_first.data_ptr()
    n_prof = 40
    retired = 0
    paused = 0.0
    marks = {}
    t_start = time.perf_counter()
    for t in range(n):
        b = (t // B) & 1
        if t % B == 0:
            with torch.cuda.stream(stream):                                             # the batch's descriptors, on the engine's stream
                sl = slice(t, min(t + B, n))
                x = pool[d_place[sl]]
                x = x + (sigma * revisit[sl].float()).view(-1, 1, 1) * torch.randn(x.shape, generator=g, device="cuda")
                bufs[b][: x.shape[0]] = x / x.norm(dim=2, keepdim=True)
        if t in sample_slot:
            t0 = time.perf_counter()
            eng.synchronize()
            rows_t, live_t = eng.vocab_count()
            vr, vi = eng.vocab_read(0, rows_t) if rows_t else (np.zeros((0, DIM), np.float32), np.zeros(0, np.int32))
            snap[t] = (vr[vi != 0].copy(), vi[vi != 0].copy(), bufs[b][t % B].cpu().numpy(), retired)
            paused += time.perf_counter() - t0
        if t == n - n_prof:
            eng.synchronize()
            eng.profile_begin(n_prof)
        a.d_descriptors = bufs[b].data_ptr() + (t % B) * q * DIM * 4
        a.sig_id = t + 1
        a.N = float(t + 1 - retired)
        a.first_new_word_id = LCD_NEW_WORD_IDS_AUTO
        a.d_first_new_word_id = fp + t * 4
        a.d_word_ids = wp + t * q * 4
        k = sample_slot.get(t)
        if k is not None:
            a.d_likelihood = d_like_s[k].data_ptr()
            a.likelihood_capacity = t + 2
        else:
            a.d_likelihood = lp + (t % depth) * cap * 4
            a.likelihood_capacity = cap
        a.d_hypothesis = hp + t * 32
        eng.frame_dev_args(a)
        if t % retire_every == retire_every - 1:
            retired += 1
            eng.sig_remove(retired)
        eng.vocab_remove_unused_async()
        if t % rebuild_every == rebuild_every - 1:
            eng.vocab_rebuild()
        if t + 1 in (100_000, 500_000):
            eng.synchronize()
            marks[t + 1] = time.perf_counter() - t_start - paused
    eng.synchronize()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t_start - paused
    rows, live = eng.vocab_count()
    roof_knn, roof_score = rooflines(eng, rows, n - retired, False)
    for r in (roof_knn, roof_score):
        if r:
            r["traffic"] = None                                    # (the committed PMC summary is the headline configuration's)
            r["traffic_source"] = None
            r["traffic_note"] = "not measured for this configuration"
            r["measured_in"] = "HIP events attached to the launches of the last %d frames (dictionary and memory at their final size)" % n_prof
    # ---- recall
    hyp = d_hyp.cpu().numpy()
    best_sig = hyp[:, 0].astype(np.int64)
    retired_at = ts // retire_every                                                     # signatures 1 .. retired_at[t] are gone when frame t is scored (its own call's retirement comes after)
    first_sig = 2 * place + 1                                                           # the place's first visit is signature 2 * place + 1
    counted = (ts % 2 == 1) & (first_sig > retired_at) & (first_sig <= ts - stm)
    hit = counted & (best_sig > 0) & (place[np.clip(best_sig - 1, 0, n - 1)] == place)
    recall = float(hit.sum()) / max(int(counted.sum()), 1)
    # ---- the word log
    log = d_words.cpu().numpy()
    n_new_frame = np.where((log < 0).any(axis=1), -log.min(axis=1), 0)
    first_new = d_first.cpu().numpy().astype(np.int64)
    ids_consecutive = bool(first_new[0] == 1 and np.array_equal(first_new[1:], first_new[:-1] + n_new_frame[:-1]))   # ++_lastWordId over the whole replay: cleans, rebuilds, retirements included
    ids_log = np.where(log < 0, first_new[:, None] - log - 1, log).astype(np.int32)
    created = int(n_new_frame.sum())
    # ---- parity on the sampled frames
    t_par = time.perf_counter()
    ids_equal, max_rel, n_cmp, hyp_ok, checked = True, 0.0, 0, True, []
    hyp_same = hyp_near = 0
    adj_rel_ref = adj_rel_exact = adj_ref_own = 0.0
    adj_ok = True
    knn_s = lik_s = 0.0
    for t in sample_t:
        vr, vi, desc, ret_t = snap[t]
        o = O.OracleVWDictionary(strategy=O.kNNBruteForce, incremental=True, nndr=NNDR, new_words_compared_together=True)
        for w, r in zip(vi.tolist(), vr):
            o.add_word(int(w), r)
        rows_ascending = bool((np.diff(vi) > 0).all())                                 # the oracle's update() indexes in ascending id: the device's row order must be that
        o.update()
        last_before = o.last_word_id
        t1 = time.perf_counter()
        exp = o.add_new_words(desc, t + 1)
        knn_s += time.perf_counter() - t1
        canon_o = [-(w - last_before) if w > last_before else w for w in exp]
        ok = bool(canon_o == log[t].tolist())
        ids_equal &= ok
        o.close()
        t2 = time.perf_counter()
        Lo = tfidf_np.compute_likelihood_dense(ids_log[ret_t: t + 1], ids_log[t])
        lik_s += time.perf_counter() - t2
        Lh = d_like_s[sample_slot[t]][ret_t: t + 1].cpu().numpy()
        err = np.abs(Lh - Lo) / np.maximum(np.abs(Lo), 1e-7 / 1e-4)
        max_rel = max(max_rel, float(err.max()))
        n_cmp += int(Lo.size)
        dead = d_like_s[sample_slot[t]][:ret_t].cpu().numpy()
        hyp_ok &= bool(not dead.any())                                                  # retired signatures score 0
        n_cons = t + 1 - stm - ret_t
        if n_cons > 0:
            adj = O.adjust_likelihood(np.concatenate([[0.0], Lo[:n_cons]]).astype(np.float32), 0.0)
            best = int(np.argmax(Lo[:n_cons]))
            dev = int(hyp[t, 0]) - 1 - ret_t
            same = dev == best
            near = 0 <= dev < n_cons and float(Lo[dev]) >= float(Lo[best]) * (1.0 - 1e-4)
            hyp_same += int(same); hyp_near += int(near and not same)
            hyp_ok &= bool(same or near)
            pick = dev if near else best
            ref_adj = float(adj[1 + pick])
            got_adj = float(hyp[t, 3:4].view(np.float32)[0])
            adj_rel_ref = max(adj_rel_ref, abs(got_adj - ref_adj) / max(abs(ref_adj), 1e-3))
            ex_adj = adjusted_exact(Lo[:n_cons], Lo[pick])
            adj_rel_exact = max(adj_rel_exact, abs(got_adj - ex_adj) / max(abs(ex_adj), 1e-3))
            ref_own = abs(ref_adj - ex_adj) / max(abs(ex_adj), 1e-3)                    # (ADJ_GATE_NOTE)
            adj_ref_own = max(adj_ref_own, ref_own)
            adj_ok &= bool(abs(got_adj - ex_adj) / max(abs(ex_adj), 1e-3) <= 1e-4 and
                           abs(got_adj - ref_adj) / max(abs(ref_adj), 1e-3) <= 1e-4 + ref_own)
        checked.append({"frame": int(t), "live_signatures": int(t + 1 - ret_t), "dictionary_words": int(vi.size), "rows_ascending": rows_ascending,
                        "word_ids_equal": ok})
    par_s = time.perf_counter() - t_par
    # ---- CPU baseline on a bounded sample: the reference's kd-tree over the FINAL dictionary + the restated std::map TF-IDF on a
    # 20 000-signature window of the log, scaled linearly to the final memory (the reference's loop is linear in the postings)
    vr, vi = eng.vocab_read(0, rows)
    vr = vr[vi != 0]
    sample_desc = bufs[((n - 1) // B) & 1][: 5].cpu().numpy()
    if O.have_ref():
        kd = O.RefIndex(vr, algo=O.ALGO_KDTREE, trees=4)
        t1 = time.perf_counter()
        for i in range(5):
            kd.knn(sample_desc[i], k=2, checks=32, cores=1)
        t_knn_cpu = (time.perf_counter() - t1) / 5
        knn_what, kind = "rtflann kd-tree (4 trees, 32 checks), 1 core, %d words" % vr.shape[0], "reference"
    else:
        t1 = time.perf_counter()
        O.knn2_linear(vr, sample_desc[0])
        t_knn_cpu = time.perf_counter() - t1
        knn_what, kind = "exact linear port, 1 core, %d words" % vr.shape[0], "port"
    win = min(20000, n - retired)
    mem = O.OracleMemory(strategy=O.kNNBruteForce, nndr=NNDR)
    lo = n - win
    for wid in np.unique(ids_log[lo:]).tolist():
        if wid > 0:
            mem.vwd.add_word(int(wid), vocab[0])
    for f in range(lo, n):
        mem.add_signature_with_id(f + 1, ids_log[f])
    t1 = time.perf_counter()
    for i in range(3):
        mem.compute_likelihood(ids_log[n - 1 - i], np.arange(lo + 1, n + 1, dtype=np.int32))
    t_lik_cpu = (time.perf_counter() - t1) / 3 * ((n - retired) / float(win))
    lik_what = "restated std::map Memory::computeLikelihood on the newest %d signatures, scaled x%.1f to %d" % (win, (n - retired) / float(win), n - retired)
    mem.close()
    div_refs = int(eng.stats().get("clean_divergent_refs", 0))
    eng.close()
    live_total = float(np.sum(ts + 1 - retired_at))
    out = {"metric": "loop-closure candidates/sec (descriptor-stream replay, growing dictionary, memory grown to %d signatures)" % (n - retired),
           "unit": "candidates/s", "value": live_total / wall, "n_gpus": 1, "steps": n, "warmup": 0, "ms_per_step": 1e3 * wall / n,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic (generated on the device)",
           "config": {"workload": "config 5 stand-in with a GROWING incremental dictionary (SURVEY.md 8d; Memory.cpp:5941-6059, Rtabmap.cpp:2117): %d frames x %d SURF "
                                  "descriptors, dictionary from EMPTY, every other frame a new place (one word of its own + words of a 49k-word Zipf world), "
                                  "the others revisits with noise; per frame cleanUnusedWords (enqueued) -> update() on the device -> addNewWords -> references -> "
                                  "computeLikelihood against every live signature -> adjustLikelihood + best candidate; the oldest signature retired every %dth "
                                  "frame, lcd_vocab_rebuild every %d frames; pipelined lcd_frame_dev" % (n, q, retire_every, rebuild_every),
                      "dictionary_rows_at_the_end": int(rows), "dictionary_words_at_the_end": int(live), "words_created": created,
                      "frames_that_created_words": int((n_new_frame > 0).sum()), "frames_that_created_words_frac": float((n_new_frame > 0).mean()),
                      "signatures_live_at_the_end": int(n - retired), "signatures_retired": int(retired),
                      "async_clean_divergence": {"references_to_words_the_enqueued_clean_had_tombstoned": div_refs, "frames": int(n),
                                                 "per_10000_frames": 1e4 * div_refs / max(int(n), 1),
                                                 "meaning": "a frame in flight matched a word whose last OTHER reference was retired before the enqueued cleanUnusedWords ran: "
                                                            "the device tombstones the word (the frame keeps its reference, the word is never matched again) where the reference's "
                                                            "clean, which runs behind that frame's addNewWords (Memory.cpp:6899-6920), keeps it -- counted on the device at registration "
                                                            "(lcd_stats.clean_divergent_refs)"},
                      "frames_per_s": n / wall, "wall_s": wall, "wall_s_at_frames": {str(k): v for k, v in marks.items()},
                      "ms_per_frame_last_half": 1e3 * (wall - marks.get(500_000, 0.0)) / (n - 500_000) if 500_000 in marks and n > 500_000 else None,
                      "descriptor_pool_generated_on_device_s": gen_s, "parity_host_seconds": par_s, "paused_for_snapshots_s": paused},
           "roofline": roof_score if (roof_score is not None and roof_knn is not None and roof_score["ms"] > roof_knn["ms"]) else (roof_knn or roof_score),
           "roofline_score": roof_score, "roofline_knn": roof_knn,
           "recall": {"revisits_counted": int(counted.sum()), "loop_closures_found": int(hit.sum()), "recall": recall,
                      "rule": "revisit frames whose place still has its first signature in memory, older than the newest %d: the best raw-likelihood candidate shows the frame's place" % stm},
           "parity": {"frames_checked": checked, "word_ids_equal": bool(ids_equal),
                      "new_word_ids_consecutive_over_the_whole_replay": ids_consecutive,     # numbered on the device (LCD_NEW_WORD_IDS_AUTO) exactly as ++_lastWordId would: every frame's first id = the one before + the words that frame created
                      "likelihood_max_rel": max_rel, "likelihood_values_compared": n_cmp,
                      "adjust_likelihood_and_best_candidate_ok": bool(hyp_ok and adj_ok), "best_candidate_equal_or_a_rounding_tie_and_retired_slots_zero": bool(hyp_ok), "adjusted_value_ok": bool(adj_ok), "best_candidate_identical": hyp_same, "best_candidate_a_rounding_tie": hyp_near,
                      "adjusted_value_max_rel_vs_reference_float_statistics": adj_rel_ref,
                      "adjusted_value_max_rel_vs_the_same_formula_with_double_statistics": adj_rel_exact,
                      "adjusted_value_within_1e-4_of_the_reference": bool(adj_rel_ref <= 1e-4), "reference_float_statistics_own_error_max_rel": adj_ref_own, "adjusted_value_gate": ADJ_GATE_NOTE,
                      "adjusted_value_note": "the reference accumulates uMean / uVariance in FLOAT over every positive likelihood (UMath.h:419-432, 512-526; the oracle "
                                             "restates that), the device in double: over ~10^6 values the first figure is dominated by the reference's own accumulation error",
                      "bound": "1e-4 relative (abs floor 1e-7)", "oracle_seconds": {"addNewWords": knn_s, "computeLikelihood": lik_s},
                      "path": "sampled frames: the pipeline is completed and the device's dictionary read back in front of the frame; word ids vs the C++ oracle's "
                              "VWDictionary::addNewWords over that dictionary; likelihood + adjustLikelihood vs the numpy restatement of Memory::computeLikelihood "
                              "(oracle/tfidf_np.py, pinned to the C++ oracle) on the live signatures replayed from the device's word log"},
           "cpu_baseline": {"value": (n - retired) / (t_knn_cpu + t_lik_cpu), "unit": "candidates/s (at the final dictionary and memory size)", "cores": 1, "kind": kind,
                            "sample": "5 frames x %s (%.1f ms/frame) + 3 frames x %s (%.0f ms/frame)" % (knn_what, 1e3 * t_knn_cpu, lik_what, 1e3 * t_lik_cpu)}}
    out["cpu_baseline"]["gpu_at_the_final_size"] = (n - retired) / (1e-3 * (out["config"]["ms_per_frame_last_half"] or out["ms_per_step"]))
    print(json.dumps(out), flush=True)


# ----------------------------------------------------------------------------------------------------------------- main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 200; --config orb_stream: frames of the stream, default 2000; "
                    "the replays run one frame per signature, --signatures)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--signatures", type=int, default=N_SIG)
    ap.add_argument("--words", type=int, default=N_WORDS, help="vocabulary size (the headline is 49 000; 125 000 = one GPU's share of config 4, "
                    "1 000 000 = config 4's whole vocabulary on one GPU)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU legs (oracle build, parity block, CPU baselines)")
    ap.add_argument("--pmc", action="store_true", help="measure HBM traffic with rocprofv3 even with --no-cpu-baseline")
    ap.add_argument("--no-pmc", action="store_true", help="do not measure HBM traffic with rocprofv3 (two extra short runs of this script)")
    ap.add_argument("--no-extras", action="store_true", help="skip the secondary measurements (unpipelined, host path, with update)")
    ap.add_argument("--leg", action="store_true", help="this run is a secondary leg of another bench.py run (`secondary` of its line): the timed region, the "
                    "rooflines and ONE frame of parity (word ids + likelihood against the oracle / the numpy restatement at >= 200 000 signatures); "
                    "no extras, no CPU baselines, no counter passes, no further legs")
    ap.add_argument("--no-legs", action="store_true", help="do not run the secondary legs (config 3 on 300 frames, 125 000 words, 10^6 signatures)")
    ap.add_argument("--pipeline", type=int, default=1, help="1: software-pipelined frames (the launches of frame t carry the filter, decision loop, "
                    "registration and scoring of the three frames before it); 0: four launches per frame, nothing overlapped")
    ap.add_argument("--parallelism", choices=["auto", "shard", "replicas"], default="auto",
                    help="N > 1: ONE frame stream with the vocabulary sharded by word-id range + all-gather / all-reduce per frame (the "
                         "north star's layout for vocabularies that want several GPUs; strong scaling), or independent frame streams per "
                         "GPU (weak scaling, no data-path collective).  auto: the shard from 100 000 words per GPU up (config 4: 1M words "
                         "over 8 GPUs), replicas below (a 49k-word vocabulary is 12.5 MB: sharding it only adds two exchanges per frame); "
                         "the other one is measured in the same run as a secondary key")
    ap.add_argument("--exchange", choices=["rccl", "p2p", "p2p-f32"], default="rccl",
                    help="the two per-frame exchanges of the sharded frame (N > 1): RCCL calls on the process group, or liblcd_p2p.so's one-shot "
                         "peer-to-peer kernels over hipIpc-mapped arenas (include/lcd_p2p.h; p2p-f32: the all-reduce moves 32-bit floats)")
    ap.add_argument("--config", choices=["headline", "orb_stream", "replay", "replay_growing"], default="headline")
    ap.add_argument("--score-block", type=int, default=0, help="experiment: threads per workgroup of the scoring kernel (256/512/1024)")
    ap.add_argument("--knn-mode", default=None, choices=["bf16", "f16", "mfma32", "valu"],
                    help="the 2-NN filter of every SURF engine of the run (default: f16 = the one-product fp16 matrix-core filter, LCD_KNN_F16; "
                         "bf16 = the library's default, three bf16 products per fp32 product)")
    ap.add_argument("--diag", default="", help="diagnostics only (not the benchmark): comma list of no-new (new words get no references), "
                    "no-retire (the oldest signature is not retired), bound-ids (the caller numbers new words with an upper bound per frame instead of "
                    "the device numbering them as ++_lastWordId does)")
    ap.add_argument("--full", action="store_true", help="everything besides the headline: rooflines, the step distribution and steady state, the "
                    "secondary measurements, HBM counter passes, parity against the oracle, CPU baselines, the secondary legs and (N > 1) the "
                    "other parallelism; the --no-* options above trim it.  Without it a run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed as DIR/<name>.npy: "
                    "word_ids (the frame's word ids as lcd_frame_dev returns them: -(k+1) = the frame's k-th new word) and likelihood (every "
                    "signature slot); float32 / float64, at most 64 MB")
    args = ap.parse_args()

    if args.leg:
        args.full = True
        args.no_extras = True; args.no_pmc = True; args.no_legs = True
    if args.pmc and not args.full:
        ap.error("--pmc needs --full")
    if args.dump_outputs and args.config != "headline":
        ap.error("--dump-outputs: the headline configuration only")
    if not args.full:
        args.no_extras = True; args.no_pmc = True; args.no_legs = True; args.no_cpu_baseline = True
    DIAG.update(x for x in args.diag.split(",") if x)
    if args.knn_mode:
        globals()["KNN_MODE"] = args.knn_mode
    if args.words != N_WORDS:
        globals()["N_WORDS"] = args.words
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args.gpus, sys.argv[1:])
        return

    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the engine has no CPU fallback")
    if args.config == "orb_stream":
        return run_orb_stream(args)
    if args.steps is None:
        args.steps = 200
    if args.config == "replay":
        return run_replay(args)
    if args.config == "replay_growing":
        return run_replay_growing(args)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()
    torch.cuda.set_device(local)
    backend = "none"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("LCD_BENCH_BACKEND", "nccl" if torch.cuda.device_count() >= world else "gloo")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            log("[bench] rank %d: %d ranks on %d GPU(s): collectives over %s (functional run, not a measurement of xGMI)"
                % (rank, world, torch.cuda.device_count(), backend))
            dist.init_process_group(backend, rank=rank, world_size=world)

    import rtabmap_amd
    from rtabmap_amd import synth
    stream = torch.cuda.Stream()
    n_sig = args.signatures
    globals()["N_SIG_RUN"] = n_sig
    shard = world > 1 and (args.parallelism == "shard" or (args.parallelism == "auto" and N_WORDS // world >= 100000))
    vocab, words = make_state(n_sig)
    cap = n_sig + args.steps + args.warmup + 4096

    # frames resident in HBM: revisits of earlier places (70 % of the descriptors quantise back to that place's words).
    n_frames = min(64, max(8, args.steps))

    def make_frames(stream_id):
        rng = np.random.default_rng(7 + stream_id)
        src = rng.integers(0, n_sig, n_frames)
        fr = [synth.frame_from_signature(vocab, words[s], seed=1000 * stream_id + i) for i, s in enumerate(src)]
        return src, fr

    def run_shard(force_path=False):
        """ONE frame stream, the vocabulary sharded by word-id range over the ranks: all-gather of the top-2 records + int64 all-reduce
        of the partial likelihood per frame.  Returns (timed_loop result, rooflines, last likelihood, build seconds, frame sources).
        force_path (one rank): the sharded stages themselves instead of the fused single-GPU frame a world of one would take."""
        from rtabmap_amd.sharded import ShardedLoopClosure
        src, frames_np = make_frames(0)                    # all ranks see the same frames
        d_frames = [torch.from_numpy(f).cuda() for f in frames_np]
        sh = ShardedLoopClosure("f32", DIM, rank=rank, world=world, device=local, stream=stream, vocab_capacity=N_WORDS + 65536,
                                sig_capacity=n_sig + 8192, knn_mode=KNN_MODE)
        sh.force_sharded_path = bool(force_path)
        if world > 1 and args.exchange != "rccl":
            sh.enable_p2p(Q, n_sig + 8192, wire="f32" if args.exchange == "p2p-f32" else "i64")
        t0 = time.perf_counter()
        sh.load_vocabulary(vocab, np.arange(1, N_WORDS + 1, dtype=np.int32))
        w = words.reshape(-1)
        sh.add_signatures_bulk(np.arange(1, n_sig + 1, dtype=np.int32), np.arange(0, (n_sig + 1) * Q, Q, dtype=np.int64), w,
                               owned_mask=(w > sh.lo) & (w <= sh.hi))
        build_s = time.perf_counter() - t0
        sh.enable_device_append(N_WORDS + 1, 16)          # the step includes update(): each rank appends the new words it owns, on the device
        state = {"next": n_sig + 1, "old": 1, "like": None, "first_new": N_WORDS + 1}

        def step(i):
            # the all-reduce of frame i runs under the nearest-neighbour search of frame i + 1; its likelihood comes back one call later
            sh.frame(d_frames[i % n_frames], state["next"], float(n_sig + 1), incremental=True, new_words_compared=True,
                     nndr=NNDR, first_new_word_id=state["first_new"], defer=True)
            sh.retire(state["old"])
            state["next"] += 1
            state["old"] += 1
            state["first_new"] += Q
        res = timed_loop(torch, dist, world, stream, step, args.steps, args.warmup, profile_eng=sh.eng if args.full else None)
        roofs = rooflines(sh.eng, sh.hi - sh.lo, n_sig, True) if args.full else (None, None)
        like = sh.flush().cpu().numpy()                    # the last frame's (every timed step finalised its predecessor's); flush waits for the engine stream
        sh.close()
        return res, roofs, like, build_s, src

    def run_shard_native_world1():
        """The same sharded stages driven by the C++ driver of include/lcd_shard.h (liblcd_shard.so: lcd_shard_frame_deferred +
        lcd_shard_sig_remove per step, update()'s append on the device), ONE rank, no exchange: what a C++ caller's rank pays without the
        wire and without this script's Python between the stages."""
        from rtabmap_amd.sharded import NativeShardComm
        _, frames_np = make_frames(0)
        d_frames = [torch.from_numpy(f).cuda() for f in frames_np]
        e = rtabmap_amd.Engine("f32", DIM, device=local, vocab_capacity=N_WORDS + 65536, sig_capacity=n_sig + 8192, stream=stream.cuda_stream,
                               knn_mode=KNN_MODE)
        load_engine(e, vocab, words)
        comm = NativeShardComm(e, 0, 1)
        comm.set_growth(N_WORDS + 1, 16)
        comm.set_append(True)
        capl = n_sig + 8192
        d_w = torch.zeros(Q, dtype=torch.int32, device="cuda")
        d_l = [torch.zeros(capl, dtype=torch.float32, device="cuda") for _ in range(2)]
        st = {"next": n_sig + 1, "old": 1, "first_new": N_WORDS + 1, "k": 0}

        def step(i):
            comm.frame(d_frames[i % n_frames].data_ptr(), Q, st["next"], float(n_sig + 1), N_WORDS, d_w.data_ptr(), d_l[st["k"] & 1].data_ptr(), capl,
                       nndr=NNDR, first_new_word_id=st["first_new"], defer=True)
            comm.sig_remove(st["old"])
            st["next"] += 1; st["old"] += 1; st["first_new"] += Q; st["k"] += 1
        res = timed_loop(torch, dist, 1, stream, step, args.steps, args.warmup)
        comm.flush()
        e.synchronize()
        comm.close()
        e.close()
        return res

    results = {}
    # ---- primary measurement
    if shard:
        res, (roof_knn, roof_score), like, build_s, src = run_shard()
        last_words = None                                  # (the sharded frame's word ids stay inside ShardedLoopClosure)
        frames_total = args.steps
    else:
        src, frames_np = make_frames(rank)                 # replicas: every rank has its own stream of frames
        d_frames = [torch.from_numpy(f).cuda() for f in frames_np]
        eng = rtabmap_amd.Engine("f32", DIM, device=local, vocab_capacity=N_WORDS + 65536, sig_capacity=n_sig + 8192,
                                 stream=stream.cuda_stream, pipeline=args.pipeline, knn_mode=KNN_MODE)
        if args.score_block:
            eng.set_option("score_block", args.score_block)
        for kv in filter(None, os.environ.get("LCD_BENCH_OPTS", "").split(",")):      # timing experiments: key=value engine options
            eng.set_option(kv.split("=")[0], int(kv.split("=")[1]))
        build_s = load_engine(eng, vocab, words)
        log("[bench] rank %d: %d signatures bulk-loaded in %.2fs" % (rank, n_sig, build_s))
        log_frames = (args.warmup + args.steps) if (world == 1 and not args.no_cpu_baseline and args.warmup + args.steps <= 4096) else 0
        step = Stepper(eng, torch, d_frames, n_sig, cap, log_frames=log_frames)
        if args.full:
            eng.set_option("profile_likelihood", 0)       # the timed region brackets launch A only (the dominant kernel)
            try:
                eng.set_option("profile_skip", args.steps // 2 if args.steps >= 10 else 0)   # ... of the steps in the middle of the region, not of the first launches behind an idle queue
            except Exception:                             # (an older variant library of an A/B run: it samples the first launches)
                pass
        res = timed_loop(torch, dist, world, stream, step, args.steps, args.warmup, profile_eng=eng if args.full else None, eng=eng,
                         per_step_events=False, prof_n=max(1, args.steps // 20))
        knn_series = eng.profile_read() if args.full else None
        st = eng.stats()                                  # (drains the engine's thread)
        like = step.d_like[: n_sig + args.steps + args.warmup].cpu().numpy()
        last_words = step.last_word_ids().cpu().numpy() if args.dump_outputs else None
        roof_knn = roof_score = None
        if args.full:
            eng.set_option("profile_likelihood", 1)       # launch B: bracketed in 24 further steps that do not count for `value`
            eng.profile_begin(10)
            for i in range(24):
                step(args.warmup + args.steps + i)
            roof_knn, roof_score = rooflines(eng, N_WORDS, n_sig, False, knn_timed=knn_series)
            roof_knn["measured_in"] = ("%d launch(es) of the timed region (steps from its middle on) + %d of the 24 steps right behind it (HIP events attached to the dispatch); "
                                       "in the timed region alone: %.4f ms" % (knn_series[1], roof_knn["samples"] - knn_series[1], knn_series[0]))
            if roof_score:
                roof_score["measured_in"] = "24 steps after the timed region (HIP events around launch B of 10 of them)"
        frames_total = world * args.steps
        host_in_c = 1e-6 * st["frame_host_ns"] / max(st["frame_calls"], 1)
    wall = res["wall"]
    value = frames_total * n_sig / wall
    last = (args.warmup + args.steps - 1) % n_frames

    config = {"workload": "SURF-64 fp32 brute-force 2-NN (" + ("49k" if N_WORDS == 49000 else str(N_WORDS)) + " words) + NNDR + TF-IDF likelihood (%d signatures x 500 words, Zipf), "
                          "500 desc/frame, 1 frame/step" % n_sig,
              "frames_per_s": frames_total / wall, "device_ms_per_step": res["dev_ms"] / args.steps,
              "host_enqueue_ms_per_step": 1e3 * res["host_enqueue"] / args.steps,
              "host_ms_inside_lcd_frame_dev": None,
              "step_ms_median": float(np.median(res["per_step_ms"])) if res["per_step_ms"].size else None,
              "step_ms_p95": float(np.percentile(res["per_step_ms"], 95)) if res["per_step_ms"].size else None,
              "world_size_observed": world, "collective_backend": backend, "signatures_bulk_load_s": build_s,
              "knn_filter": {"f16": "fp16 matrix-core filter, one product per fp32 product (LCD_KNN_F16) + exact fp32 re-rank + certificate",
                             "bf16": "bf16 matrix-core filter, three products per fp32 product (LCD_KNN_BF16X3) + exact fp32 re-rank + certificate"}.get(KNN_MODE, KNN_MODE),
              "pipeline": "software-pipelined frames, four in flight: 2 launches per frame (A: query pre-split of frame t + filter of t-1 + decision loop "
                          "of t-2 + registration of t-3; B: re-rank of frame t-1 + scoring of t-3), one stream; the step includes VWDictionary::update()'s append branch on the device (append_new_words): the vocabulary "
                          "grows by the frame's new words before the next frame is searched" if (args.pipeline and not shard) else "4 launches per frame, one stream",
              "parallelism": ("vocabulary sharded by word-id range over %d GPUs (all-gather top-2 + int64 all-reduce per frame, the all-reduce "
                              "overlapped with the next frame's search; exchanges: %s)" % (world, {"rccl": "RCCL", "p2p": "liblcd_p2p.so, 64-bit integer wire",
                                                                                                  "p2p-f32": "liblcd_p2p.so, 32-bit float wire"}[args.exchange])) if shard
              else ("%d independent replicas (one frame stream per GPU, no data-path collective)" % world if world > 1 else "1 GPU")}

    if not shard:
        config["host_ms_inside_lcd_frame_dev"] = host_in_c
    if rank == 0 and args.dump_outputs:
        outputs = {"likelihood": like}
        if last_words is not None:
            outputs["word_ids"] = last_words
        dump_outputs(args.dump_outputs, outputs)
    # ---- the distribution needs >= 50 frames: extra, untimed-for-`value` steps when the driver asked for fewer
    if not shard and args.full:
        extra = timed_loop(torch, dist, world, stream, step, max(64, min(args.steps, 256)), 0, eng=eng)
        config["step_ms_median"] = float(np.median(extra["per_step_ms"]))
        config["step_ms_p95"] = float(np.percentile(extra["per_step_ms"], 95))
        config["distribution_from"] = "%d extra steps after the timed region, one event per step (the timed region itself carries none: an " \
                                      "event costs stream time); their mean %.4f ms" % (extra["per_step_ms"].size, float(extra["per_step_ms"].mean()))

    # ---- the same step over >= 200 further frames without any event in the stream: what the 20-step figure converges to once its
    # pipeline fill / drain (3 of 23 launch pairs) and the box-to-box noise of a 0.8 ms region stop mattering (the previous review's item 8)
    if not shard and world == 1 and args.full:
        n_steady = max(200, args.steps)
        steady = timed_loop(torch, dist, world, stream, step, n_steady, 0, eng=eng, per_step_events=False)
        config["steady_ms_per_step"] = 1e3 * steady["wall"] / n_steady
        config["steady_note"] = "%d further steps, no event in the stream, one synchronisation at the end; the bench cycles through %d distinct frames, so " \
                                "these are mostly revisits (few new words per frame) where the driver's %d steps are first visits (~150 new words each)" % (n_steady, n_frames, args.steps)

    def primary_line():
        out = {
            "metric": "loop-closure candidates/sec (49k vocab, 100k signatures, 500 desc/frame)" if N_WORDS == 49000 and n_sig == N_SIG else
                      "loop-closure candidates/sec (%d-word vocab, %d signatures, 500 desc/frame)" % (N_WORDS, n_sig),
            "value": value, "unit": "candidates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * wall / args.steps, "higher_is_better": True, "scaling": "strong" if shard else "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic", "config": config,
        }
        if roof_knn is not None:
            if roof_score is not None and roof_score["ms"] > roof_knn["ms"]:
                out["roofline"] = roof_score
            else:
                out["roofline"] = roof_knn
            out["roofline_score"] = roof_score
            out["roofline_knn"] = roof_knn
        if rank == 0:
            exp_top = int(src[last]) + 1
            got_top = int(np.argmax(like[:n_sig])) + 1
            config["last_frame_top_candidate_ok"] = bool(got_top == exp_top or exp_top < (1 + args.warmup + args.steps))
        return out

    # ---- N > 1: the other parallelism, same run, secondary key (an error there is reported, it does not cost the line -- and neither
    # does a collective that never completes: a watchdog thread prints the primary line and ends the rank)
    if world > 1 and not args.no_extras:
        import threading
        secondary_done = threading.Event()

        def bail():
            if secondary_done.wait(float(os.environ.get("LCD_BENCH_SECONDARY_TIMEOUT", "240"))):
                return
            config["secondary_parallelism_error"] = "timed out: the run ended without the secondary measurement"
            if rank == 0:
                print(json.dumps(primary_line()), flush=True)
            os._exit(0)
        threading.Thread(target=bail, daemon=True).start()
        try:
            if shard:
                src2, fr2 = make_frames(rank)
                d_fr2 = [torch.from_numpy(f).cuda() for f in fr2]
                eng2 = rtabmap_amd.Engine("f32", DIM, device=local, vocab_capacity=N_WORDS + 1024, sig_capacity=n_sig + 8192,
                                          stream=stream.cuda_stream, pipeline=args.pipeline, knn_mode=KNN_MODE)
                load_engine(eng2, vocab, words)
                st2 = Stepper(eng2, torch, d_fr2, n_sig, cap)
                r2 = timed_loop(torch, dist, world, stream, st2, args.steps, args.warmup, eng=eng2)
                config["replicas_value"] = world * args.steps * n_sig / r2["wall"]
                config["replicas_ms_per_step"] = 1e3 * r2["wall"] / args.steps
                eng2.close()
            else:
                r2 = run_shard()[0]
                config["shard_value"] = args.steps * n_sig / r2["wall"]
                config["shard_ms_per_step"] = 1e3 * r2["wall"] / args.steps
                config["shard_note"] = ("ONE frame stream with the vocabulary sharded by word-id range over %d GPUs (all-gather of the top-2 records + "
                                        "int64 all-reduce per frame; strong scaling): what `--parallelism shard` reports as `value`" % world)
        except Exception as e:                                # noqa: BLE001
            config["secondary_parallelism_error"] = "%s: %s" % (type(e).__name__, e)
        finally:
            secondary_done.set()

    out = primary_line()

    # ---- N = 1: secondary measurements, parity, CPU baselines
    if world == 1 and rank == 0:
        if not args.no_extras:
            engu = rtabmap_amd.Engine("f32", DIM, device=local, vocab_capacity=N_WORDS + 4096, sig_capacity=n_sig + 8192,
                                      stream=stream.cuda_stream, pipeline=0 if args.pipeline else 1, knn_mode=KNN_MODE)
            if args.score_block:
                engu.set_option("score_block", args.score_block)
            load_engine(engu, vocab, words)
            stu = Stepper(engu, torch, d_frames, n_sig, cap)
            ru = timed_loop(torch, dist, 1, stream, stu, max(50, min(args.steps, 200)), 10, profile_eng=engu, eng=engu)
            ku, su = rooflines(engu, N_WORDS, n_sig, False)
            key = "unpipelined" if args.pipeline else "pipelined"
            config[key + "_ms_per_step"] = 1e3 * ru["wall"] / max(50, min(args.steps, 200))
            config[key + "_kernel_ms"] = {"knn": ku["ms"], "score": su["ms"] if su else None}
            if args.pipeline:
                # the same two kernels launched on their own (not fused with the other frame's stages): their own rooflines
                out["roofline_knn_standalone"] = ku
                out["roofline_score_standalone"] = su
            config["host_path_ms_per_step"] = host_path_ms(torch, engu, frames_np, n_sig)
            engw = rtabmap_amd.Engine("f32", DIM, device=local, vocab_capacity=N_WORDS + 65536, sig_capacity=n_sig + 8192,
                                      stream=stream.cuda_stream, pipeline=args.pipeline, knn_mode=KNN_MODE)
            load_engine(engw, vocab, words)
            stw = Stepper(engw, torch, d_frames, n_sig, cap)
            wu, wrows, wlive = with_update_ms(torch, engw, stw)
            config["with_update_ms_per_step"] = wu
            config["with_update_async_clean_divergent_refs"] = {"references": getattr(with_update_ms, "divergent_refs", None), "frames": 272}
            config["with_update_note"] = "the headline step + the rest of Memory::preUpdate EVERY frame, nothing completed in between: the signature " \
                                         "registered 8 frames earlier retired too, cleanUnusedWords as one enqueued kernel " \
                                         "(lcd_vocab_remove_unused_async), lcd_vocab_rebuild every 128th frame (the only draining call; ~20 %% of the rows are tombstones by then); 256 steps; " \
                                         "vocabulary at the end: %d rows, %d live" % (wrows, wlive)
            engw.close()
            engn = rtabmap_amd.Engine("f32", DIM, device=local, vocab_capacity=N_WORDS + 4096, sig_capacity=n_sig + 8192,
                                      stream=stream.cuda_stream, pipeline=args.pipeline, knn_mode=KNN_MODE)
            load_engine(engn, vocab, words)
            stn = Stepper(engn, torch, d_frames, n_sig, cap, append=False)
            rn = timed_loop(torch, dist, 1, stream, stn, args.steps, args.warmup, eng=engn, per_step_events=False)
            config["no_append_ms_per_step"] = 1e3 * rn["wall"] / args.steps
            config["no_append_note"] = "the step as rounds 1-3 timed it: the frame's new words get postings but never become vocabulary rows (same command)"
            engn.close()
            lat = frame_latency_ms(torch, eng, step, stream, args.warmup + args.steps + 400)
            lat["note"] = "ms from the lcd_frame_dev call of a frame until its likelihood is readable (event behind every stage it owes): paced = the " \
                          "caller keeps four frames in flight (three further calls carry a frame's stages); saturated = calls back to back, the queue " \
                          "in front of the device included; single = one frame then lcd_synchronize (its stages run stand-alone)"
            config["frame_latency_ms"] = lat
            try:
                ci = cpp_interface_ms(vocab, words, frames_np, n_sig)
                config["cpp_interface_ms_per_step"] = ci["map_by_value"]["step"]
                config["cpp_interface_inplace_map_ms_per_step"] = ci["map_in_place"]["step"]
                config["cpp_interface_flat_ms_per_step"] = ci["flat"]["step"]
                config["cpp_interface_call_by_call_ms_per_step"] = ci["call_by_call_map_by_value"]["step"]
                config["cpp_interface_detail"] = ci
                config["cpp_interface_note"] = "C++ loop in liblcd_host.so through the reference's interface at %d signatures: MemoryHip::update (ONE lcd_frame_host call: " \
                                               "quantisation + references + update()'s append + likelihood; host matrices in, the mirror's std::map bookkeeping included) + " \
                                               "Memory::computeLikelihood(signature, ids) against every signature + forget(oldest).  ms_per_step = the reference's own signature " \
                                               "(std::map by value: ~10^5 node allocations per frame); inplace_map = a caller-owned std::map updated in place; flat = two vectors; " \
                                               "call_by_call = rounds 1-4's path (lcd_quantize, lcd_sig_add, lcd_likelihood) on the same memory.  detail = ms of " \
                                               "{step, update, likelihood, forget}; mirror filled in %.1f s" % (ci["signatures"], ci["load_s"])
            except Exception as e:                                # noqa: BLE001
                config["cpp_interface_error"] = "%s: %s" % (type(e).__name__, e)
            config["host_path_note"] = "lcd_quantize + lcd_sig_add + lcd_likelihood + lcd_sig_remove from host pointers (PCIe + syncs included)"
            try:
                rs = run_shard(force_path=True)[0]
                config["shard_stages_world1_ms_per_step"] = 1e3 * rs["wall"] / args.steps
                config["shard_stages_world1_note"] = "ONE rank running the SHARDED stages (what each of N ranks runs, without the wire): local search -> " \
                                                     "candidate records -> merge + decision loop (replicated) -> update()'s append of the owned new words on the " \
                                                     "device (shard_append, beside the registration in one launch) -> integer scoring -> conversion: nine launches per frame, no " \
                                                     "synchronisation; to be read against ms_per_step (the fused, pipelined single-GPU frame)"
            except Exception as e:                                # noqa: BLE001
                config["shard_stages_world1_error"] = "%s: %s" % (type(e).__name__, e)
            try:
                rn = run_shard_native_world1()
                config["shard_stages_world1_native_ms_per_step"] = 1e3 * rn["wall"] / args.steps
                config["shard_stages_world1_native_note"] = "the same stages through liblcd_shard.so (lcd_shard_frame_deferred + lcd_shard_sig_remove per step): the C++ " \
                                                            "driver a multi-GPU caller links, one rank, no exchange; shard_stages_world1_ms_per_step drives them from " \
                                                            "Python (torch stream contexts and events between the stages) and is bound by that host code"
            except Exception as e:                                # noqa: BLE001
                config["shard_stages_world1_native_error"] = "%s: %s" % (type(e).__name__, e)
            engu.close()
            engb = rtabmap_amd.Engine("f32", DIM, device=local, vocab_capacity=N_WORDS + 4096, sig_capacity=n_sig + 8192,
                                      stream=stream.cuda_stream, pipeline=args.pipeline, knn_mode=KNN_MODE)
            load_engine(engb, vocab, words)
            stb = BayesStepper(engb, torch, d_frames, n_sig, cap)
            rb = timed_loop(torch, dist, 1, stream, stb, max(50, min(args.steps, 200)), 10, eng=engb, per_step_events=False)
            config["with_bayes_ms_per_step"] = 1e3 * rb["wall"] / max(50, min(args.steps, 200))
            config["with_bayes_note"] = "step + adjustLikelihood + Bayes filter update over the working memory (chain graph, default Bayes/PredictionLC, " \
                                        "STM %d) + highest hypothesis on the device; the new signature's neighbour list handed over per frame; " \
                                        "%d lists loaded in %.2f s" % (STM, n_sig, stb.lists_load_s)
            res = np.frombuffer(stb.d_res.cpu().numpy().tobytes(), dtype=np.int32)
            config["with_bayes_last_hypothesis"] = {"sig_id": int(res[0]), "n_considered": int(res[5])}
            engb.close()
        if (not args.no_cpu_baseline or args.pmc) and not args.no_pmc and not os.environ.get("LCD_BENCH_INNER"):
            # HBM traffic of the big kernels, measured by this run (two short rocprofv3 passes over this script) instead of read
            # from the committed profile
            note = measure_pmc((["--words", str(args.words)] if args.words != 49000 else []) +
                               (["--signatures", str(args.signatures)] if args.signatures != N_SIG else []))
            for k in ("roofline", "roofline_score", "roofline_knn", "roofline_knn_standalone", "roofline_score_standalone"):
                if out.get(k):
                    out[k]["traffic"] = pmc_traffic(out[k]["kernel"])
                    out[k]["traffic_source"] = pmc_source(out[k]["kernel"], note)
        if args.leg and not args.no_cpu_baseline:
            out["parity"] = leg_parity(torch, vocab, words, frames_np[0])
        elif not args.no_cpu_baseline:
            m = build_oracle(vocab, words)
            par, t_lin_port, t_lik = parity_block(torch, vocab, words, frames_np, m)
            out["parity"] = par
            if step.d_words_log is not None and step.n_calls:
                m.close()
                m = build_oracle(vocab, words)                       # a fresh memory: the replay starts where the timed engine started
                out["parity"]["timed_engine"] = timed_engine_parity(m, step, frames_np, like, n_sig)
            out["cpu_baseline"] = cpu_baselines(vocab, frames_np, t_lin_port, t_lik, n_sig, words=words, frame_words=words[17])
            out["cpu_baseline"]["gpu_over_best_cpu"] = value / out["cpu_baseline"]["best_cpu_value"]
    if rank == 0 and world == 1 and not args.no_legs and not args.no_extras and not os.environ.get("LCD_BENCH_INNER") and \
            N_WORDS == 49000 and n_sig == N_SIG and args.config == "headline":
        eng.synchronize()
        out["secondary"] = secondary_legs()
    if rank == 0:
        print(json.dumps(out), flush=True)
    if not shard:
        eng.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
