"""The records a bf16 / fp16 matrix-core filter hands to its re-rank: one 16-byte StripRecord per (row block, query) -- two 32-bit keys whose
index bits carry tile, 4-row group and the half of the tile the key's lane held, and the block's bound -- widened to (score bits, vocabulary
row) on the reader's side; the 128- / 256-float filter keeps 64-bit keys (ShareRecords).  Every case compares word ids AND distance bits with
the exact scan (the `valu` mode of a plain handle) on the same inputs, through lcd_knn2 and through lcd_frame_dev, where the packing can go
wrong: row counts at tile and strip edges, a padded last tile, both neighbours in one 4-row group, in the two halves of a tile (rows r and
r + 4), in a strip's first and last tile, exact ties (the lower row wins), a query that IS a row (its score rounds slightly negative), frames
of 1, 2, 33, 500 and 513 descriptors, the one-strip, pre-split (pipelined) and persistent filters, and rows of 128 and 256 floats.

The pipelined cases run with lcd_set_option("strip_tiles", 8): strips of the built-in length S = 8 tiles (256 rows) at a few hundred rows
(the planner gives one tile per strip below 8 193 rows).  The stand-alone search gets strips of 2 and of 8 tiles from 9 000 and 57 400 rows.
The exact scan of a vocabulary and a query set is computed once and shared.

Equal results alone do not show that the records were read right: a wrong half bit, first tile or score mask makes the re-rank evaluate other
rows than the filter scored, its certificate (the measured error against eps, the bound) rejects the query, and the exact redo still returns
the exact scan's answer.  So every case also asserts WHICH path served it -- the filter kernel's name from the handle's profile for lcd_knn2,
a launch B with re-rank workgroups (lcd_debug_launch_b_routes) for a frame -- and bounds the queries that went to the exact redo
(knn_last_fallback_queries, the rejected count of lcd_debug_last_frame_knn) by a quarter of the frame, at least one: a broken half bit
sends the queries whose first or second key comes from the second half of a tile there (three in four), a broken first tile or mask nearly
all of them, while a working filter loses only queries whose second and third neighbours lie within eps of each other.

The engine gives a vocabulary of fewer than 256 rows to the exact scan on every handle (run_knn2_raw, goes_through_pipeline): the row
counts 1, 31, 32, 33 and 255 the issue names cannot reach the filter.  They are kept as what they are -- the hand-over at the engine's own
threshold, asserted to be served by the exact scan -- and the tile and strip edges are tested where the filter runs: 256 + {0, 1, 31, 32,
33}, 2 * 256 - 1, 2 * 256 + 1 and 600 rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from rtabmap_amd import capi, synth

pytestmark = pytest.mark.gpu
MODES = ["bf16", "f16"]
S_ROWS = 8 * 32                                                        # rows of a strip of the built-in length
Q_POOL = 513

_CACHE = {}


def _unit(x):
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), dtype=np.float32)


def _planted(n, dim=64):
    """n unit rows with exact duplicates planted: in one 4-row group, in the two halves of a tile (r, r + 4), in two tiles of a strip, in two strips
    (each pair only where both rows exist)"""
    key = ("vocab", n, dim)
    if key not in _CACHE:
        v = synth.vocab_surf(n, seed=4000 + n, dim=dim).copy()
        for a, b in _pairs(n):
            v[b] = v[a]
        v.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _pairs(n):
    """(lower row, its duplicate)"""
    want = [(8, 9), (16, 20), (40, 40 + 5 * 32 + 3), (70, 70 + S_ROWS), (S_ROWS - 1, S_ROWS), (n - 2, n - 1)]
    out, used = [], set()
    for a, b in want:
        if 0 <= a < b < n and not ({a, b} & used):
            out.append((a, b)); used |= {a, b}
    return out


def _pool(n, dim=64):
    """Q_POOL queries against _planted(n): [0] IS a row (distance 0, the filter's score rounds to either side of it), [1..] next to every planted pair
    (an exact tie: the lower row wins), then midpoints of rows r, r + 1 of one 4-row group and of rows r, r + 4 (the two halves of a tile) in a
    strip's first and last tile, the vocabulary's first and last row, and noisy copies of random rows"""
    key = ("pool", n, dim)
    if key not in _CACHE:
        v = _planted(n, dim)
        rng = np.random.default_rng(5000 + n + dim)
        qs = [v[min(3, n - 1)].copy()]
        for a, _ in _pairs(n):
            qs.append(v[a] + np.float32(0.01) * rng.standard_normal(dim).astype(np.float32))
        for s0 in range(0, n, S_ROWS):
            for t0 in (s0, s0 + S_ROWS - 32):                          # the strip's first and last tile
                for a, b in ((t0 + 12, t0 + 13), (t0 + 25, t0 + 29)):
                    if b < n:
                        qs.append(0.5 * (v[a] + v[b]) + np.float32(0.003) * rng.standard_normal(dim).astype(np.float32))
        qs.append(v[0] + np.float32(0.01) * rng.standard_normal(dim).astype(np.float32))
        qs.append(v[n - 1] + np.float32(0.01) * rng.standard_normal(dim).astype(np.float32))
        qs = np.stack(qs)[:Q_POOL]
        rest = v[rng.integers(0, n, Q_POOL - len(qs))] + np.float32(0.02) * rng.standard_normal((Q_POOL - len(qs), dim)).astype(np.float32)
        p = np.concatenate([qs[:1], _unit(np.concatenate([qs[1:], rest]))])     # ([0] stays the row's own bits)
        p = np.ascontiguousarray(p, dtype=np.float32)
        p.setflags(write=False)
        _CACHE[key] = p
    return _CACHE[key]


def _engine(mode, dim=64, pipeline=False, options=None, **kw):
    import rtabmap_amd
    eng = rtabmap_amd.Engine("f32", dim, knn_mode=mode, pipeline=pipeline, **kw)
    for k, val in (options or {}).items():
        eng.set_option(k, val)
    return eng


def _exact_knn2(n, q, dim=64):
    """the exact scan's (word ids, distances) of the first q pool queries, once per (n, q, dim)"""
    key = ("exact", n, q, dim)
    if key not in _CACHE:
        eng = _engine("valu", dim)
        eng.vocab_append(_planted(n, dim), np.arange(1, n + 1, dtype=np.int32))
        _CACHE[key] = eng.knn2(_pool(n, dim)[:q])
        eng.close()
    return _CACHE[key]


def _same(got, exp, what):
    np.testing.assert_array_equal(got[0], exp[0], err_msg=what + ": word ids")
    np.testing.assert_array_equal(got[1].view(np.uint32), exp[1].view(np.uint32), err_msg=what + ": distance bits")


def _check_ties(n, exp):
    """what the exact scan itself says about the planted inputs: the row's own query at distance 0, the lower row first in every tie"""
    ids, d = exp
    if n > 3:
        assert d[0, 0] == 0.0 and ids[0, 0] == 4
    for i, (a, b) in enumerate(_pairs(n)):
        if 1 + i < ids.shape[0]:
            assert (ids[1 + i, 0], ids[1 + i, 1]) == (a + 1, b + 1) and d[1 + i, 0] == d[1 + i, 1], (i, a, b, ids[1 + i], d[1 + i])


def _frame_knn(eng, q):
    """lcd_debug_last_frame_knn: (words, distances) [q x 2] of the latest frame's 2-NN stage as it stands, and the queries its certificate rejected"""
    lib = capi.load()
    row, word, dist = np.zeros((q, 2), np.int32), np.zeros((q, 2), np.int32), np.zeros((q, 2), np.float32)
    nq, rej = C.c_int(0), C.c_int(0)
    assert lib.lcd_debug_last_frame_knn(eng.h, row.ctypes.data_as(C.c_void_p), word.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p), q, C.byref(nq), C.byref(rej)) == 0
    assert nq.value == q
    return (word, dist), rej.value


def _rerank_launches(reset=False):
    """launches B with re-rank workgroups since the last reset (host-side count, lcd_debug_launch_b_routes)"""
    out = (C.c_longlong * 8)()
    assert capi.load().lcd_debug_launch_b_routes(out, 1 if reset else 0) == 0
    return int(out[0])


def _redo_cap(q):
    return max(q // 4, 1)


def _knn2(mode, n, q, options=None, dim=64):
    """lcd_knn2 of the first q pool queries on a fresh handle: (word ids, distances), the name of the kernel that searched, the queries re-done exactly"""
    eng = _engine(mode, dim, options=options)
    eng.vocab_append(_planted(n, dim), np.arange(1, n + 1, dtype=np.int32))
    eng.profile_begin(2)
    got = eng.knn2(_pool(n, dim)[:q])
    _, n_prof, name = eng.profile_read()
    redone = eng.stats()["knn_last_fallback_queries"]
    eng.close()
    assert n_prof >= 1, (n_prof, name)
    return got, name, redone


def _check_knn2(mode, n, q, kernel, options=None, dim=64):
    """... equal to the exact scan's, searched by `kernel`, and -- when that is a filter -- with at most _redo_cap(q) queries re-done exactly"""
    got, name, redone = _knn2(mode, n, q, options, dim)
    print("lcd_knn2 %s, %d rows x %d queries: %s, %d re-done exactly" % (mode, n, q, name, redone))
    assert name.split(" ")[0] == kernel, (name, kernel)
    _same(got, _exact_knn2(n, q, dim), "lcd_knn2, %d rows x %d queries" % (n, q))
    if kernel != "knn2_l2_kernel":
        assert redone <= _redo_cap(q), "the exact redo must not stand in for the filter: %d of %d queries" % (redone, q)


def _one_frame(mode, pipeline, n, q, options=None):
    """the first q pool queries as a frame through lcd_frame_dev (no word is appended): its word ids, its 2-NN stage (words, distances), the queries
    launch B's certificate rejected and the launches B with re-rank workgroups.  A pipelined handle gets the frame TWICE: the rejected count of a
    frame can be read behind the NEXT lcd_frame_dev only (its decision loop and redo, which clear it, have not run then); nothing is appended, so
    both frames search the same vocabulary."""
    eng = _engine(mode, pipeline=pipeline, options=options, sig_capacity=8)
    eng.vocab_append(_planted(n), np.arange(1, n + 1, dtype=np.int32))
    d_q = torch.from_numpy(_pool(n)[:q].copy()).cuda()
    d_w = torch.zeros((2, q), dtype=torch.int32, device="cuda")
    d_l = torch.zeros((2, 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _rerank_launches(reset=True)
    eng.frame_dev(d_q.data_ptr(), q, 1, 1.0, d_w[0].data_ptr(), d_l[0].data_ptr(), 16, first_new_word_id=n + 1)
    rejected = 0
    if pipeline:
        eng.frame_dev(d_q.data_ptr(), q, 2, 2.0, d_w[1].data_ptr(), d_l[1].data_ptr(), 16, first_new_word_id=n + 1 + q)
        if _rerank_launches() > 0:                                     # (frame 1's launch B has been enqueued: the stage read here is frame 0's)
            _, rejected = _frame_knn(eng, q)
    eng.synchronize()
    launches = _rerank_launches()
    knn, _ = _frame_knn(eng, q)                                        # the last frame, complete (the same descriptors over the same vocabulary)
    words = d_w[0].cpu().numpy()
    eng.close()
    return words, knn, rejected, launches


def _exact_frame(n, q):
    key = ("frame", n, q)
    if key not in _CACHE:
        _CACHE[key] = _one_frame("valu", False, n, q)[:2]
    return _CACHE[key]


def _check_frame(mode, n, q, options, filtered=True):
    """a pipelined frame against the exact handle's; filtered: it went through launch A's filter and launch B's re-rank, which rejected at most _redo_cap(q)"""
    words, knn, rejected, launches = _one_frame(mode, True, n, q, options)
    print("frame %s, %d rows x %d descriptors, %r: %d launches B with re-rank workgroups, %d rejected" % (mode, n, q, options, launches, rejected))
    ewords, eknn = _exact_frame(n, q)
    np.testing.assert_array_equal(words, ewords)
    _same(knn, eknn, "the frame's 2-NN stage")
    if n >= 2:                                                         # (a frame over fewer than two rows searches nothing, on either handle)
        _same(knn, _exact_knn2(n, q), "the frame's 2-NN stage against lcd_knn2's exact scan")
    if filtered:
        assert launches == 2, "both frames' re-ranks ran in a launch B: %d" % launches
        assert rejected <= _redo_cap(q), "the exact redo must not stand in for the filter: %d of %d queries" % (rejected, q)
    else:
        assert launches == 0, "a vocabulary below 256 rows is the exact scan's"


# ---- rows at tile and strip edges WHERE THE FILTER RUNS (256 rows and more; the last tile padded unless the count is a multiple of 32): a second strip
# whose only tile holds 1, 31, 32 rows, whose second tile holds 1 row (256 + 33), two full strips less one row, two strips plus one row.  Strips of the
# built-in length in the pipelined filter ("strip_tiles" = 8), one tile per strip in the stand-alone one.
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [S_ROWS, S_ROWS + 1, S_ROWS + 31, S_ROWS + 32, S_ROWS + 33, 2 * S_ROWS - 1, 2 * S_ROWS + 1])
def test_row_counts_at_tile_and_strip_edges(mode, n):
    q = 33
    _check_ties(n, _exact_knn2(n, q))
    _check_knn2(mode, n, q, "knn_bf16_filter_kernel")
    _check_frame(mode, n, q, {"strip_tiles": 8})


# ---- the row counts below the engine's threshold of 256 rows: NOT a test of the records -- the exact scan serves them on every handle, and that is
# what is asserted; kept for the hand-over at the threshold (255 here, 256 above)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 31, 32, 33, S_ROWS - 1])
def test_row_counts_below_the_filter_threshold_are_the_exact_scans(mode, n):
    q = 33
    _check_ties(n, _exact_knn2(n, q))
    _check_knn2(mode, n, q, "knn2_l2_kernel")
    _check_frame(mode, n, q, {"strip_tiles": 8}, filtered=False)


# ---- frames of 1, 2, 33, 500, 513 descriptors over three strips (600 rows: 256 + 256 + 88, the last tile holds 24 rows)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("q", [1, 2, 33, 500, 513])
def test_query_counts_over_three_strips(mode, q):
    n = 600
    _check_ties(n, _exact_knn2(n, q))
    _check_knn2(mode, n, q, "knn_bf16_filter_kernel")
    _check_frame(mode, n, q, {"strip_tiles": 8})
    if q == 33:                                                        # a strip length that is no power of two, and the planner's own (one tile per strip)
        _check_frame(mode, n, q, {"strip_tiles": 3})
        _check_frame(mode, n, q, None)


# ---- the stand-alone filter's own strips of 2 and of 8 tiles (one workgroup per strip), the last tile padded
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,tiles", [(9000, 2), (57400, 8)])
def test_stand_alone_search_with_strips_of_several_tiles(mode, n, tiles):
    q = 96
    out = (C.c_int * 5)()
    assert capi.load().lcd_debug_frame_plan(q, n, 0, out) == 0 and out[0] == tiles and out[2] == 0, list(out)   # (the pipelined plan without distance tiles is the stand-alone one)
    assert n % 32 != 0
    _check_ties(n, _exact_knn2(n, q))
    _check_knn2(mode, n, q, "knn_bf16_filter_kernel")
    _check_frame(mode, n, q, None)


# ---- the persistent filter: 33 000 rows x 513 queries is about the smallest shape with more strips than compute units (two query blocks x 207
# strips of 5 tiles against 256 units); with "filter_units" = 7 the strips are walked by 3 persistent workgroups per query block, 69 strips each,
# stand-alone (knn_bf16_filter_kernel_p) and in a pipelined frame's launch A
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pipeline", [False, True])
def test_persistent_filter(mode, pipeline):
    n, q = 33000, 513
    _check_ties(n, _exact_knn2(n, q))
    if pipeline:
        _check_frame(mode, n, q, {"filter_units": 7})
    else:
        _check_knn2(mode, n, q, "knn_bf16_filter_kernel_p", options={"filter_units": 7})


# ---- rows of 128 and 256 floats: the filter that keeps 64-bit keys (shares of up to four strips; "filter_units" = 8: several shares per workgroup)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dim", [128, 256])
@pytest.mark.parametrize("units", [None, 8])
def test_rows_of_128_and_256_floats(mode, dim, units):
    n, q = 3000 + 17, 65
    _check_ties(n, _exact_knn2(n, q, dim))
    _check_knn2(mode, n, q, "knn_wide_filter_kernel", options={"filter_units": units} if units else None, dim=dim)


# ---- a pipelined stream of a dozen frames that append their words on the device and number them there, against the unpipelined handle (exact scan).
# Every frame revisits the frames before it: the words frame t creates are the nearest neighbours of frame t + 1's descriptors (its shadow candidates
# and pending rows).
def _stream(mode, pipeline, options=None):
    n, q, T = 600, 200, 12
    base = _planted(n)
    key = ("frames", n, q, T)
    if key not in _CACHE:
        rng = np.random.default_rng(77)
        history = [base[rng.integers(0, n, q)] for _ in range(2)]
        frames = []
        for _ in range(T):
            frames.append(synth.revisit_surf(rng, history, q, fresh_frac=0.35))
            history.append(frames[-1])
        _CACHE[key] = frames
    frames = _CACHE[key]
    eng = _engine(mode, pipeline=pipeline, options=options, sig_capacity=T + 8)
    eng.vocab_append(base, np.arange(1, n + 1, dtype=np.int32))
    eng.set_option("next_word_id", n + 1)
    d_desc = [torch.from_numpy(f).cuda() for f in frames]
    d_w = torch.zeros((T, q), dtype=torch.int32, device="cuda")
    d_l = torch.zeros((T, T + 8), dtype=torch.float32, device="cuda")
    d_first = torch.zeros(T, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _rerank_launches(reset=True)
    rejected = []
    for t, f in enumerate(frames):
        eng.frame_dev(d_desc[t].data_ptr(), q, t + 1, float(t + 1), d_w[t].data_ptr(), d_l[t].data_ptr(), T + 8,
                      first_new_word_id=capi.LCD_NEW_WORD_IDS_AUTO, append_new_words=True, d_first_new_word_id_ptr=d_first[t:].data_ptr())
        if pipeline and t > 0:                                         # frame t - 1 as launch B's re-rank left it: the queries its certificate rejected
            rejected.append(_frame_knn(eng, q)[1])
    eng.synchronize()
    launches = _rerank_launches()
    knn, _ = _frame_knn(eng, q)
    rows, live = eng.vocab_count()
    vr, vi = eng.vocab_read(n, rows - n)
    out = dict(words=d_w.cpu().numpy(), first=d_first.cpu().numpy(), knn=knn, rows=rows, vocab=(vr, vi), rejected=rejected, launches=launches)
    eng.close()
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("options", [{"strip_tiles": 8}, {"strip_tiles": 8, "shadow_rows": 2}, {"strip_tiles": 8, "shadow_rows": 0}])
def test_a_dozen_appending_frames_against_the_unpipelined_handle(mode, options):
    if "stream" not in _CACHE:
        _CACHE["stream"] = _stream("valu", False)
    exp = _CACHE["stream"]
    got = _stream(mode, True, options)
    np.testing.assert_array_equal(got["words"], exp["words"])
    np.testing.assert_array_equal(got["first"], exp["first"])
    assert got["rows"] == exp["rows"] > 600 + 12 * 20, "every frame creates words"
    np.testing.assert_array_equal(got["vocab"][1], exp["vocab"][1])
    np.testing.assert_array_equal(got["vocab"][0].view(np.uint32), exp["vocab"][0].view(np.uint32))
    _same(got["knn"], exp["knn"], "the last frame's 2-NN stage")
    print("rejected per frame:", got["rejected"], "launches B with re-rank workgroups:", got["launches"])
    assert got["launches"] == 12, "every frame's re-rank ran in a launch B"
    assert len(got["rejected"]) == 11 and max(got["rejected"]) <= _redo_cap(200), "the exact redo must not stand in for the filter: %r" % (got["rejected"],)
    # (a property of the INPUT, the same on the exact handle: words a frame created win in the frames behind it -- positive ids beyond the base
    # vocabulary from the third frame on; the second frame draws most of its descriptors from the two base frames of the history)
    assert all((exp["words"][t] > 600).sum() > 10 for t in range(2, 12)), [int((exp["words"][t] > 600).sum()) for t in range(12)]
