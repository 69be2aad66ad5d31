"""The re-rank role of launch B (knn_mfma_rerank_body with two queries per workgroup) on every path its source takes, against the
unpipelined handle on the same inputs, in both matrix-core modes (bf16x3 and fp16 operands).

Compared bit for bit between the two handles: every frame's word ids, the id the device gave its first new word, the vocabulary the stream built
(rows and ids) -- and the 2-NN stage itself, read back through lcd_debug_last_frame_knn: rows, words and distances of every frame.  On the
pipelined handle the read-back right behind lcd_frame_dev(t) is what launch B's re-rank wrote for frame t - 1, before that frame's decision loop
(and the exact redo that rides with it) has run, together with the number of queries its certificate rejected: a frame without rejected queries
must equal the plain handle's final neighbours there and then, and the last frame is compared once more behind lcd_synchronize, redo included.
The stand-alone search of both handles (the same body, one query per workgroup) is checked against the reference's arithmetic restated in numpy.

Sizes come from the launch plan (lcd_debug_frame_plan: strips x 2 kept keys per query).  Which route the launches B took comes from
lcd_debug_launch_b_routes (host-side counts of the launches with shadow scores, writer workgroups, cross-frame tiles, staged pending rows, rows
written by the re-rank workgroups; the re-rank and writer workgroups of the latest launch), and every case asserts its own."""
import ctypes as C

import numpy as np
import pytest
import torch

from rtabmap_amd import capi, synth

pytestmark = pytest.mark.gpu
MODES = ["bf16", "f16"]
BF_KEEP = 2                                                            # keys the filter keeps per (strip, query)


def _keys_per_query(q, n_rows):
    lib = capi.load()
    out = (C.c_int * 5)()
    assert lib.lcd_debug_frame_plan(q, n_rows, 1, out) == 0
    assert out[2] == 0, "one workgroup per strip (the persistent filter keeps other records)"
    return out[1] * BF_KEEP


_VOCABS = {}


def _vocab(n_words):
    """(computed once per size, shared by the cases and never written to)"""
    if n_words not in _VOCABS:
        v = synth.vocab_surf(n_words, seed=1000 + n_words)
        v.setflags(write=False)
        _VOCABS[n_words] = v
    return _VOCABS[n_words]


def _growth_frames(base, q, n_frames, seed, fresh_frac=0.3):
    rng = np.random.default_rng(seed)
    history = [base[rng.integers(0, base.shape[0], q)] for _ in range(2)]
    frames = []
    for _ in range(n_frames):
        frames.append(synth.revisit_surf(rng, history, q, fresh_frac=fresh_frac))
        history.append(frames[-1])
    return frames


def _revisit_frames(base, q, n_frames, seed):
    """slightly noisy copies of vocabulary rows only: every descriptor matches its word, no frame creates one"""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(n_frames):
        f = base[rng.integers(0, base.shape[0], q)] + rng.standard_normal((q, 64)).astype(np.float32) * np.float32(0.002)
        frames.append(np.ascontiguousarray(f / np.linalg.norm(f, axis=1, keepdims=True), dtype=np.float32))
    return frames


def _frame_knn(eng, q):
    """lcd_debug_last_frame_knn: (rows, words, distances) [q x 2] of the latest frame's 2-NN stage as it stands, its descriptor count, its rejected queries"""
    lib = capi.load()
    row, word, dist = np.zeros((q, 2), np.int32), np.zeros((q, 2), np.int32), np.zeros((q, 2), np.float32)
    nq, rej = C.c_int(0), C.c_int(0)
    rc = lib.lcd_debug_last_frame_knn(eng.h, row.ctypes.data_as(C.c_void_p), word.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p), q, C.byref(nq), C.byref(rej))
    assert rc == 0
    return (row[: nq.value], word[: nq.value], dist[: nq.value]), nq.value, rej.value


def _routes(reset=False):
    out = (C.c_longlong * 8)()
    assert capi.load().lcd_debug_launch_b_routes(out, 1 if reset else 0) == 0
    return dict(zip(["rerank", "shadow", "writers", "cross", "staged", "rerank_writes", "n_wr", "n_rerank"], [int(v) for v in out]))


def _run(pipeline, knn_mode, base, frames, options=None, probe=None):
    """the stream on one handle: word ids per frame, first new word id per frame, rows created per frame, the vocabulary behind the base rows, every
    frame's 2-NN stage (pipelined: as launch B left it, with the rejected count; plain: final), the last frame's final 2-NN, the routes of the
    launches B, and the stand-alone 2-NN of `probe` with its count of exact redos"""
    import rtabmap_amd
    n_words, T = base.shape[0], len(frames)
    qmax = max(f.shape[0] for f in frames)
    eng = rtabmap_amd.Engine("f32", 64, sig_capacity=T + 8, pipeline=pipeline, knn_mode=knn_mode)
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    eng.vocab_append(base, np.arange(1, n_words + 1, dtype=np.int32))
    eng.set_option("next_word_id", n_words + 1)
    d_desc = [torch.from_numpy(f).cuda() for f in frames]
    d_w = torch.zeros((T, qmax), dtype=torch.int32, device="cuda")
    d_l = torch.zeros((T, T + 8), dtype=torch.float32, device="cuda")
    d_first = torch.zeros(T, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _routes(reset=True)
    stage, rejected = {}, {}
    for t, f in enumerate(frames):
        eng.frame_dev(d_desc[t].data_ptr(), f.shape[0], t + 1, float(t + 1), d_w[t].data_ptr(), d_l[t].data_ptr(), T + 8,
                      first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
        of = t - 1 if pipeline else t                                  # (the frame whose 2-NN stage has run when the call returns)
        if of >= 0:
            stage[of], nq, rejected[of] = _frame_knn(eng, qmax)
            assert nq == frames[of].shape[0]
    eng.synchronize()
    routes = _routes()
    final, nq, _ = _frame_knn(eng, qmax)                               # the last frame, its exact redo included
    assert nq == frames[-1].shape[0]
    words, first = d_w.cpu().numpy(), d_first.cpu().numpy()
    created = [len(set(w for w in words[t, : frames[t].shape[0]].tolist() if w < 0)) for t in range(T)]
    rows, live = eng.vocab_count()
    assert rows == live == n_words + sum(created)
    vr, vi = eng.vocab_read(n_words, rows - n_words) if rows > n_words else (np.zeros((0, 64), np.float32), np.zeros(0, np.int32))
    knn = eng.knn2(probe) if probe is not None else None
    st = eng.stats()                                                   # (knn_last_fallback_queries: of the stand-alone search just made)
    eng.close()
    return dict(words=words, first=first, created=created, vocab=(vr, vi), fallback=st["knn_last_fallback_queries"], frames=st["frame_calls"], knn=knn,
                stage=stage, rejected=rejected, final=final, routes=routes)


def _same_knn(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what + ": rows")
    np.testing.assert_array_equal(a[1], b[1], err_msg=what + ": words")
    np.testing.assert_array_equal(a[2].view(np.uint32), b[2].view(np.uint32), err_msg=what + ": distances")


def _both(knn_mode, base, frames, options=None, probe=None):
    plain = _run(False, knn_mode, base, frames, None, probe)
    piped = _run(True, knn_mode, base, frames, options, probe)
    print("routes of the pipelined handle's launches B:", piped["routes"], "rejected per frame:", piped["rejected"])
    np.testing.assert_array_equal(piped["words"], plain["words"])
    np.testing.assert_array_equal(piped["first"], plain["first"])
    np.testing.assert_array_equal(piped["vocab"][1], plain["vocab"][1])
    np.testing.assert_array_equal(piped["vocab"][0].view(np.uint32), plain["vocab"][0].view(np.uint32))
    assert piped["frames"] == plain["frames"] == len(frames)
    assert piped["routes"]["rerank"] == len(frames), "every frame's re-rank ran in a launch B"
    for t in sorted(piped["stage"]):                                   # the re-rank's own output, frame by frame
        if piped["rejected"][t] == 0:
            _same_knn(piped["stage"][t], plain["stage"][t], "frame %d behind launch B" % t)
    _same_knn(piped["final"], plain["final"], "last frame, complete")
    if probe is not None:
        assert piped["fallback"] == plain["fallback"], "queries of the stand-alone search re-done exactly"
        np.testing.assert_array_equal(piped["knn"][0], plain["knn"][0])
        np.testing.assert_array_equal(piped["knn"][1].view(np.uint32), plain["knn"][1].view(np.uint32))
    return piped


def _reference_2nn(rows, ids, queries):
    """rtflann's L2 (dist.h:150-177) in numpy float32, every operation rounded on its own: per 4 floats ((d0 d0 + d1 d1) + d2 d2) + d3 d3, the sixteen
    terms added in order; the two nearest rows, ties to the lower row"""
    out_id, out_d = np.zeros((queries.shape[0], 2), np.int32), np.zeros((queries.shape[0], 2), np.float32)
    for i, qv in enumerate(queries):
        d = rows - qv
        s = d * d
        t = ((s[:, 0::4] + s[:, 1::4]) + s[:, 2::4]) + s[:, 3::4]
        res = np.zeros(rows.shape[0], np.float32)
        for c in range(16):
            res = res + t[:, c]
        order = np.lexsort((np.arange(rows.shape[0]), res))[:2]
        out_id[i], out_d[i] = ids[order], res[order]
    return out_id, out_d


# ---- key counts: no second key per thread (<= 256 keys per query), a second, a third, and the loop behind the third
@pytest.mark.parametrize("knn_mode", MODES)
@pytest.mark.parametrize("n_words,q,lo,hi", [(3000, 96, 1, 256), (6000, 96, 257, 512), (72000, 500, 513, 768), (72000, 96, 769, 1 << 20)])
def test_keys_per_query_in_every_range_of_the_key_loops(knn_mode, n_words, q, lo, hi):
    base = _vocab(n_words)
    frames = _growth_frames(base, q, 4, seed=7 + n_words + q)
    probe = np.ascontiguousarray(frames[-1][:24])
    keys = _keys_per_query(q, n_words)
    assert lo <= keys <= hi, "the plan of %d rows x %d queries keeps %d keys per query" % (n_words, q, keys)
    got = _both(knn_mode, base, frames, probe=probe)
    assert lo <= _keys_per_query(q, n_words + sum(got["created"])) <= hi          # ... and still does over the rows the stream added
    # the stand-alone search of the handle (the same body, one query per workgroup) over base rows + created rows
    rows = np.concatenate([base, got["vocab"][0]])
    ids = np.concatenate([np.arange(1, n_words + 1, dtype=np.int32), got["vocab"][1]])
    rid, rd = _reference_2nn(rows, ids, probe)
    np.testing.assert_array_equal(got["knn"][0], rid)
    np.testing.assert_array_equal(got["knn"][1].view(np.uint32), rd.view(np.uint32))


# ---- query counts: the odd query out (its half of the workgroup walks the last query again and writes nothing), one workgroup, several
@pytest.mark.parametrize("knn_mode", MODES)
@pytest.mark.parametrize("q", [1, 2, 3, 129, 500])
def test_frames_of_odd_and_even_descriptor_counts(knn_mode, q):
    base = _vocab(3000)
    frames = _growth_frames(base, q, 5, seed=100 + q, fresh_frac=0.4)
    got = _both(knn_mode, base, frames)
    assert got["frames"] == 5 and all(f.shape[0] == q for f in frames)
    # two queries per workgroup, padded to the eight XCDs: q odd leaves the last working workgroup a half without a query, and its neighbours were compared above
    assert got["routes"]["n_rerank"] == ((q + 1) // 2 + 7) // 8 * 8
    if q >= 3:
        assert sum(got["created"]) > 0


# ---- growth frames: every frame creates words -- shadow scores, pending rows and the sixteen row-writer workgroups; the staged paths the options keep
@pytest.mark.parametrize("knn_mode", MODES)
@pytest.mark.parametrize("options", [{"shadow_rows": 2}, {}, {"shadow_rows": 0}, {"shadow_rows": 0, "row_writer_wgs": 0}, {"cross_frame_tiles": 1}])
def test_frames_that_each_create_words(knn_mode, options):
    base = _vocab(3000)
    frames = _growth_frames(base, 200, 8, seed=211, fresh_frac=0.35)
    got = _both(knn_mode, base, frames, options=options)
    assert min(got["created"]) > 20, "every frame creates words: %r" % (got["created"],)
    ro, T = got["routes"], len(frames)
    if options.get("cross_frame_tiles"):
        assert ro["cross"] >= T - 2 and ro["shadow"] == 0
    elif options.get("shadow_rows", 1) == 0:
        assert ro["shadow"] == 0 and ro["cross"] == 0 and ro["staged"] >= T - 2, "every re-rank workgroup stages and scans the pending rows"
        if options.get("row_writer_wgs", 16) == 0:
            assert ro["writers"] == 0 and ro["rerank_writes"] >= T - 2, "the re-rank workgroups write the rows they staged"
        else:
            assert ro["writers"] >= T - 2 and ro["n_wr"] == 16 and ro["rerank_writes"] == 0
    else:
        need = T - 2 if options.get("shadow_rows") == 2 else 1       # (the built-in waits until the stream has shown that it creates words)
        assert ro["shadow"] >= need and ro["writers"] >= ro["shadow"] and ro["n_wr"] == 16 and ro["cross"] == 0
    # words a frame created are matched by the frames that revisit it: positive ids beyond the base vocabulary
    assert (got["words"] > 3000).sum() > 10


# ---- revisit frames: nothing pending, no row written
@pytest.mark.parametrize("knn_mode", MODES)
def test_frames_that_only_revisit_existing_words(knn_mode):
    base = _vocab(3000)
    frames = _revisit_frames(base, 200, 6, seed=311)
    got = _both(knn_mode, base, frames)
    assert got["created"] == [0] * 6 and (got["words"] > 0).all()
    ro = got["routes"]
    assert ro["shadow"] == 0 and ro["cross"] == 0 and ro["rerank_writes"] == 0 and ro["n_rerank"] == 104, "no launch B carried pending rows of any kind"
    assert all(r == 0 for r in got["rejected"].values())
    assert got["vocab"][1].shape[0] == 0


# ---- exact redo: more near-identical rows than the re-rank takes candidates (128) around a query -> its certificate fails
@pytest.mark.parametrize("knn_mode", MODES)
def test_a_query_the_certificate_sends_to_the_exact_redo(knn_mode):
    rng = np.random.default_rng(411)
    base = _vocab(3000).copy()
    centre = base[17].copy()
    cluster = centre + rng.standard_normal((400, 64)).astype(np.float32) * np.float32(1e-6)      # 400 rows within rounding of each other
    base[1000:1400] = cluster / np.linalg.norm(cluster, axis=1, keepdims=True)
    frames = _revisit_frames(base, 64, 3, seed=412)
    for f in frames:
        f[5] = base[1200]                                              # the last frame's query 5 sits in the cluster (as do 6 and 7, a little off)
        f[6] = centre
        f[7] = base[1001]
    got = _both(knn_mode, base, frames, probe=np.ascontiguousarray(frames[-1][:16]))
    assert got["fallback"] >= 3, "queries 5, 6 and 7 of the stand-alone search go to the exact redo: %d" % got["fallback"]
    # ... and so they do in the pipelined frames: the certificate of launch B's re-rank (two queries per workgroup) rejected them, frame by frame
    assert sorted(got["rejected"]) == [0, 1] and all(r >= 3 for r in got["rejected"].values()), got["rejected"]
    rid, rd = _reference_2nn(np.concatenate([base, got["vocab"][0]]), np.concatenate([np.arange(1, 3001, dtype=np.int32), got["vocab"][1]]), frames[-1][:16])
    np.testing.assert_array_equal(got["knn"][0], rid)
    np.testing.assert_array_equal(got["knn"][1].view(np.uint32), rd.view(np.uint32))
